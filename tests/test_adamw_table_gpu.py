"""sm_adamw_table (one launch over a device table of segments, each with its parameter group's
learning rate and weight decay) against sm_adamw called per segment -- bit for bit -- and
against torch.optim.AdamW; its non-finite skip and argument checks; optim.GroupedAdamW on
finetune.VideoClassifier."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

LENS = [0, 1, 3, 4, 5, 2047, 2048, 2049, 4099]
GROUPS = [0, 1, 0, 1, 0, 1, 0, 1, 0]
LR, WD, LR_MULT = (1e-3, 1e-4), (0.05, 0.0), 0.5
B1, B2, EPS = 0.9, 0.999, 1e-8
SENTINEL = -12345.5
STEPS = 5                      # 3 for the bit / reference checks, 2 more for the skip test


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_mae_amd import build
    build.build()


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _inputs():
    g = torch.Generator().manual_seed(1234)
    p0 = [torch.randn(n, generator=g) for n in LENS]
    grads = [[torch.randn(n, generator=g) * 0.01 for n in LENS] for _ in range(STEPS)]
    return p0, grads


def _lr_eff(group):
    return float(np.float32(LR[group]) * np.float32(LR_MULT))      # the fp32 product the call forms


@pytest.fixture(scope="module")
def yardstick():
    """sm_adamw per segment with that segment's hyperparameters: (p0, grads, states), states[t]
    the per-segment (p, m, v) CPU tensors after step t + 1.  Computed once, never modified."""
    from ssl_mae_amd import kernels as K
    p0, grads = _inputs()
    p = [t.clone().to(DEV) for t in p0]
    m = [torch.zeros(n, device=DEV) for n in LENS]
    v = [torch.zeros(n, device=DEV) for n in LENS]
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    states = []
    for t in range(STEPS):
        for s, n in enumerate(LENS):
            K.adamw(p[s], grads[t][s].to(DEV), m[s], v[s], _lr_eff(GROUPS[s]), B1, B2, EPS, WD[GROUPS[s]], None, step,
                    advance_step=(s == len(LENS) - 1))
        states.append([(p[s].cpu().clone(), m[s].cpu().clone(), v[s].cpu().clone()) for s in range(len(LENS))])
    assert step.item() == STEPS
    return p0, grads, states


def _misaligned(variant, s, role):
    if variant == "aligned":
        return False
    if variant == "unaligned":
        return True
    # mixed: every third segment fully aligned, one with a single role off, one with all four off
    return s % 3 == 2 or (s % 3 == 1 and role == s % 4)


class Packed:
    """One backing buffer per role (p, g, m, v); the segments separated by guard gaps of at least
    3 sentinel elements, each base 16-byte aligned or offset by one element."""

    def __init__(self, variant, p0):
        self.starts = []
        sizes = []
        for role in range(4):
            pos, st = 0, []
            for s, n in enumerate(LENS):
                pos = (pos + 3 + 3) // 4 * 4 + (1 if _misaligned(variant, s, role) else 0)
                st.append(pos)
                pos += n
            self.starts.append(st)
            sizes.append(pos + 3)
        self.bufs = [torch.full((sz,), SENTINEL, dtype=torch.float32, device=DEV) for sz in sizes]
        assert all(b.data_ptr() % 16 == 0 for b in self.bufs)
        for s, n in enumerate(LENS):
            self.seg(0, s).copy_(p0[s])
            self.seg(2, s).zero_()
            self.seg(3, s).zero_()
        self.found_inf = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.step = torch.zeros(1, dtype=torch.int64, device=DEV)
        from ssl_mae_amd import kernels as K
        addrs = [tuple(self.bufs[r].data_ptr() + 4 * self.starts[r][s] for r in range(4)) for s in range(len(LENS))]
        self.addrs = addrs
        self.table, self.S, self.C = K.adamw_table(addrs, LENS, GROUPS, torch.device(DEV))

    def seg(self, role, s):
        return self.bufs[role][self.starts[role][s]:self.starts[role][s] + LENS[s]]

    def set_grads(self, gs):
        for s in range(len(LENS)):
            self.seg(1, s).copy_(gs[s])

    def run(self, check_finite=True):
        from ssl_mae_amd import ops
        ops.adamw_table_step([self.bufs[0], self.bufs[2], self.bufs[3]], self.table, self.S, self.C, LR, WD, LR_MULT,
                             B1, B2, EPS, self.found_inf, self.step, check_finite)

    def guards_intact(self):
        for role in range(4):
            mask = torch.ones(self.bufs[role].numel(), dtype=torch.bool)
            for s, n in enumerate(LENS):
                mask[self.starts[role][s]:self.starts[role][s] + n] = False
            if not bool((self.bufs[role].cpu()[mask] == SENTINEL).all()):
                return False
        return True

    def matches(self, state):
        return all(torch.equal(self.seg(role, s).cpu(), state[s][i])
                   for s in range(len(LENS)) for i, role in enumerate((0, 2, 3)))


@pytest.mark.parametrize("variant", ["mixed", "aligned", "unaligned"])
def test_table_step_bits_equal_per_segment_adamw(yardstick, variant):
    p0, grads, states = yardstick
    pk = Packed(variant, p0)
    kinds = {all(a % 16 == 0 for a in row) for row, n in zip(pk.addrs, LENS) if n}
    assert kinds == {"mixed": {True, False}, "aligned": {True}, "unaligned": {False}}[variant]
    for t in range(3):
        pk.set_grads(grads[t])
        pk.run()
        assert pk.matches(states[t]), (variant, t)
        assert pk.guards_intact(), (variant, t)
        assert pk.found_inf.item() == 0
    assert pk.step.item() == 3


def test_table_step_matches_torch_adamw(yardstick):
    p0, grads, _ = yardstick
    ref = [t.clone().requires_grad_(True) for t in p0]
    opt = torch.optim.AdamW([{"params": [ref[s] for s in range(len(LENS)) if GROUPS[s] == g], "lr": LR[g] * LR_MULT,
                              "weight_decay": WD[g]} for g in (0, 1)], betas=(B1, B2), eps=EPS)
    pk = Packed("mixed", p0)
    for t in range(3):
        for s in range(len(LENS)):
            ref[s].grad = grads[t][s].clone()
        opt.step()
        pk.set_grads(grads[t])
        pk.run()
    got = torch.cat([pk.seg(0, s).cpu() for s in range(len(LENS))])
    want = torch.cat([r.detach() for r in ref])
    for s, n in enumerate(LENS):
        if n:
            print(f"segment {s} (len {n}, group {GROUPS[s]}): rel_err {rel_err(pk.seg(0, s), ref[s]):.3e}")
    err = rel_err(got, want)
    print(f"all {got.numel()} entries: rel_err {err:.3e}")
    assert err < 1e-6


def test_nonfinite_gradient_skips_the_step(yardstick):
    p0, grads, states = yardstick
    pk = Packed("mixed", p0)
    for t in range(3):
        pk.set_grads(grads[t])
        pk.run()
    assert pk.matches(states[2])
    before = [b.clone() for b in pk.bufs]
    pk.set_grads(grads[3])
    bad_seg = 7                                       # group index 1, the second group
    assert GROUPS[bad_seg] == 1
    pk.seg(1, bad_seg)[2048] = float("nan")           # the segment's last element: a scalar tail
    pk.run()
    for role in (0, 2, 3):
        assert torch.equal(pk.bufs[role].view(torch.int32), before[role].view(torch.int32)), role
    assert pk.step.item() == 3 and pk.found_inf.item() == 1
    # the next clean step proceeds, as step 4
    pk.set_grads(grads[3])
    pk.run()
    assert pk.found_inf.item() == 0 and pk.step.item() == 4
    assert pk.matches(states[3]) and pk.guards_intact()
    # check_finite = 0: the flag is neither read nor written
    pk.found_inf.fill_(1)
    pk.set_grads(grads[4])
    pk.run(check_finite=False)
    assert pk.found_inf.item() == 1 and pk.step.item() == 5
    assert pk.matches(states[4]) and pk.guards_intact()


def test_argument_checks_launch_nothing(yardstick):
    from ssl_mae_amd import _lib, kernels as K
    p0, grads, _ = yardstick
    pk = Packed("mixed", p0)
    pk.set_grads(grads[0])
    pk.found_inf.fill_(7)
    pk.step.fill_(11)
    before = [b.clone() for b in pk.bufs]
    lib = _lib.load()
    lr = (ctypes.c_float * 65)(*([1e-3] * 65))
    wd = (ctypes.c_float * 65)(*([0.05] * 65))

    def call(table=pk.table.data_ptr(), nbytes=pk.table.numel(), S=pk.S, C=pk.C, groups=2, lr_p=lr, wd_p=wd,
             flag=pk.found_inf.data_ptr(), step=pk.step.data_ptr(), check=1):
        def vp(x):
            return ctypes.c_void_p(x) if isinstance(x, int) else ctypes.cast(x, ctypes.c_void_p)
        return lib.sm_adamw_table(vp(table), nbytes, S, C, groups, vp(lr_p), vp(wd_p), LR_MULT, B1, B2, EPS, vp(flag),
                                  vp(step), check, _lib.stream())

    assert call(groups=0) == -2
    assert call(groups=K.ADAMW_MAX_GROUPS + 1) == -2
    assert call(table=0) == -2
    assert call(nbytes=pk.table.numel() - 16) == -2
    assert call(nbytes=pk.table.numel() + 16) == -2
    assert call(C=pk.C + 1) == -2                       # the counts no longer give table_bytes
    assert call(S=-1) == -2
    assert call(lr_p=0) == -2 and call(wd_p=0) == -2 and call(step=0) == -2 and call(flag=0) == -2
    empty = torch.from_numpy(K.adamw_table_layout([], [], []).copy()).to(DEV)
    assert call(table=empty.data_ptr(), nbytes=empty.numel(), S=0, C=0) == 0        # zero segments
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(pk.bufs, before))
    assert pk.found_inf.item() == 7 and pk.step.item() == 11
    assert call(groups=K.ADAMW_MAX_GROUPS) == 0         # the largest group count is accepted
    assert pk.step.item() == 12 and pk.found_inf.item() == 0


# ------------------------------------------------------------------ GroupedAdamW on VideoClassifier
NC, B, T, S = 4, 2, 2, 112


@pytest.fixture(scope="module")
def trained():
    """(model after one fp32 training step's backward, its parameters and gradients cloned)."""
    from ssl_mae_amd.finetune import VideoClassifier
    from ssl_mae_amd.init_rule import synthetic_clip
    torch.manual_seed(5)
    model = VideoClassifier(NC, img_size=S).to(DEV).train()
    clip = torch.from_numpy(synthetic_clip(B, T, S, seed=70)).to(DEV)
    label = torch.tensor([1, 3], device=DEV)
    loss = torch.nn.CrossEntropyLoss()(model(clip).float(), label)
    loss.backward()
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    return model, params, grads, (clip, label)


def _ft_cfg(**training):
    tr = {"learning_rate": 3e-4, "weight_decay": 0.05, "head_lr": 1e-3, "backbone_lr": 1e-4, "layer_decay": 1.0,
          "no_decay_1d": False}
    tr.update(training)
    return {"training": tr}


@pytest.mark.parametrize("layer_decay", [1.0, 0.75])
def test_grouped_adamw_matches_torch_on_video_classifier(trained, layer_decay):
    from ssl_mae_amd.finetune import param_groups
    from ssl_mae_amd.optim import GroupedAdamW
    model, params, grads, _ = trained
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(params[n])
    groups = param_groups(model, _ft_cfg(layer_decay=layer_decay, no_decay_1d=layer_decay != 1.0), "two_stage")
    assert len(groups) == (2 if layer_decay == 1.0 else len({(g["lr"], g["weight_decay"]) for g in groups}))
    assert len(groups) >= 2 and groups[0]["lr"] == 1e-3
    opt = GroupedAdamW(groups)
    opt.step()
    assert opt.table_builds == 1 and opt.step_count.item() == 1 and opt.found_inf.item() == 0
    ref = {n: params[n].cpu().clone().requires_grad_(True) for n in params}
    for n in ref:
        ref[n].grad = grads[n].cpu().clone()
    torch.optim.AdamW([{"params": [ref[n] for n in g["names"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
                       for g in groups]).step()
    worst = ("", 0.0)
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, grads[n]), n                 # both sides consumed identical gradients
        e = rel_err(p, ref[n])
        worst = max(worst, (n, e), key=lambda x: x[1])
        assert e < 1e-6, (n, e)
    print(f"layer_decay {layer_decay}: {len(groups)} groups, {len(opt.table_segments)} segments, worst rel_err "
          f"{worst[1]:.3e} ({worst[0]})")
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(params[n])


def test_grouped_adamw_frozen_backbone_cache_and_unfreeze(trained):
    from ssl_mae_amd.finetune import VideoClassifier, set_requires_grad
    from ssl_mae_amd.optim import GroupedAdamW
    _, _, _, (clip, label) = trained
    torch.manual_seed(6)
    model = VideoClassifier(NC, img_size=S).to(DEV)
    params = {n: p.detach().clone() for n, p in model.named_parameters()}
    set_requires_grad(model.backbone, False)
    head = list(model.classifier.parameters())
    opt = GroupedAdamW([{"params": head, "lr": 1e-3, "weight_decay": 0.05},
                        {"params": list(model.backbone.parameters()), "lr": 1e-4, "weight_decay": 0.05}])

    def train_step():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.CrossEntropyLoss()(model(clip).float(), label)
        loss.backward()
        opt.step()

    model.train()
    bn = next(m for m in model.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d))
    mean0 = bn.running_mean.clone()
    ptrs = []
    for _ in range(3):
        train_step()
        ptrs.append([p.grad.data_ptr() for p in head])
    flat = head[0].__dict__.get("_sm_flat")
    assert flat is None                                          # the head lives outside the flat buffer
    assert sorted(n for n, _ in opt.table_segments) == sorted(p.numel() for p in head)   # only the head
    assert opt.table_builds == 1 and ptrs[0] == ptrs[1] == ptrs[2]
    for n, p in model.backbone.named_parameters():
        assert torch.equal(p, params["backbone." + n]), n        # frozen: bit-unchanged
    assert not torch.equal(bn.running_mean, mean0)               # train-mode BN statistics did move
    assert not torch.equal(head[0], params["classifier.weight"])
    set_requires_grad(model.backbone, True)
    train_step()
    assert opt.table_builds == 2
    assert sum(n for n, _ in opt.table_segments) >= sum(p.numel() for p in model.parameters())
    train_step()
    assert opt.table_builds == 2                                 # exactly one rebuild
    name0, p_first = next(iter(model.backbone.named_parameters()))
    assert not torch.equal(p_first, params["backbone." + name0])
    assert opt.step_count.item() == 5

    # state_dict -> a new optimizer -> load_state_dict -> the next step gives identical bits
    sd = opt.state_dict()
    assert sd["step"] == 5 and len(sd["param_groups"]) == 2 and len(sd["state"]) == len(list(model.parameters()))
    saved = [p.detach().clone() for p in model.parameters()]
    opt.step()                                                   # the gradients of the last backward again
    after_a = [p.detach().clone() for p in model.parameters()]
    with torch.no_grad():
        for p, q in zip(model.parameters(), saved):
            p.copy_(q)
    opt2 = GroupedAdamW([{"params": head, "lr": 5.0, "weight_decay": 0.5},
                         {"params": list(model.backbone.parameters()), "lr": 5.0, "weight_decay": 0.5}])
    opt2.load_state_dict(sd)
    assert [g["lr"] for g in opt2.param_groups] == [1e-3, 1e-4]
    opt2.step()
    assert opt2.step_count.item() == 6
    for p, a in zip(model.parameters(), after_a):
        assert torch.equal(p, a)

"""sm_clip_mix and sm_soft_ce on the GPU against tests/mix_mirror.py, finetune.SoftCEFn and
driver.train_pass with a mixer and label smoothing.

Tolerances.  clip_mix: bit for bit (the mirror makes the kernel's fp32 operations in its order).
soft_ce: the ones test_privacy_gpu.py applies to sm_logits_metrics: the loss sum 1e-5 relative of
the fp64 value, |dlogits - want| / grad_scale <= 1e-5, counts exact; with eps == 0 and no partner
every output has sm_logits_metrics' bits."""
import numpy as np
import pytest
import torch

from mix_mirror import clip_mix_mirror, soft_ce_mirror

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _offset_view(t):
    """The same values 4 bytes past a 16-byte boundary: the scalar path."""
    base = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ------------------------------------------------------------------ clip_mix
def _boxes(H, W):
    return [(0, 0, 0, 0), (2, 2, 0, 3), (0, 0, H, W), (0, 2, 2, 3), (H - 2, 1, 2, 3), (1, 0, 3, 2), (1, W - 3, 2, 3),
            (1, 3, 2, 3)]            # empty twice, the frame, each edge, one that cuts a 4-vector on both sides


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("H,W", [(6, 8), (5, 7)])
def test_clip_mix_matches_the_mirror(B, H, W):
    from ssl_mae_amd import kernels as Kn
    rng = np.random.default_rng(B * 100 + W)
    x_np = (rng.standard_normal((B, 6, H, W)) * 2).astype(np.float32)
    x = torch.from_numpy(x_np).to(DEV)
    P = B // 2
    boxes = _boxes(H, W)
    for i, bx in enumerate(boxes):
        for lam in (0.0, 0.3, 1.0):
            box_np = np.array([boxes[(i + 3 * p) % len(boxes)] for p in range(P)], dtype=np.int32).reshape(P, 4)
            lam_np = np.array([lam, 0.75][:P], dtype=np.float32)
            want = clip_mix_mirror(x_np, lam_np, box_np)
            lam_t, box_t = torch.from_numpy(lam_np), torch.from_numpy(box_np)
            got = Kn.clip_mix(x, lam_t, box_t)                              # host table: checked, one upload
            assert np.array_equal(_bits(got), want.view(np.int32)), (bx, lam)
            # a device table, the scalar path (x and out 4 bytes off), and in place: the same bits
            assert torch.equal(Kn.clip_mix(x, lam_t.to(DEV), box_t.to(DEV)), got)
            xo = _offset_view(x)
            assert torch.equal(Kn.clip_mix(xo, lam_t, box_t, out=_offset_view(torch.zeros_like(x))), got)
            for src in (x.clone(), xo):
                assert Kn.clip_mix(src, lam_t, box_t, out=src) is src and torch.equal(src, got)
    if B == 1:
        assert torch.equal(Kn.clip_mix(x, torch.empty(0), torch.empty(0, 4, dtype=torch.int32)), x)


def test_clip_mix_5d_clip_and_more_than_one_block():
    """[B,3,T,H,W] with 3 * T * H * W = 6144 elements per clip: 6 blocks of vectors, 24 of scalars."""
    from ssl_mae_amd import ops
    rng = np.random.default_rng(1)
    x_np = rng.standard_normal((4, 3, 2, 32, 32)).astype(np.float32)
    lam_np = np.array([0.4, 1.0], dtype=np.float32)
    box_np = np.array([[0, 0, 0, 0], [5, 6, 20, 9]], dtype=np.int32)
    want = clip_mix_mirror(x_np, lam_np, box_np)
    x = torch.from_numpy(x_np).to(DEV)
    got = ops.clip_mix(x, torch.from_numpy(lam_np).to(DEV), torch.from_numpy(box_np).to(DEV))
    assert np.array_equal(_bits(got), want.view(np.int32))
    got = ops.clip_mix(_offset_view(x), torch.from_numpy(lam_np), torch.from_numpy(box_np))
    assert np.array_equal(_bits(got), want.view(np.int32))
    # every frame of a clip carries the same box: the mix is clip-consistent
    assert torch.equal(got[1][:, :, 5:25, 6:15], x[2][:, :, 5:25, 6:15])


def test_clip_mix_non_finite_partner_stays_out():
    from ssl_mae_amd import kernels as Kn
    x = torch.ones(2, 6, 6, 8, device=DEV)
    x[1, :, 0, 0], x[1, :, 5, 7], x[1, :, 2, 4] = float("nan"), float("inf"), 7.0
    box = torch.tensor([[2, 3, 2, 3]], dtype=torch.int32)
    for v in (x, _offset_view(x)):
        got = Kn.clip_mix(v, torch.ones(1), box)
        want = torch.ones(6, 6, 8, device=DEV)
        want[:, 2, 4] = 7.0
        assert torch.equal(got[0], want)
        assert torch.isnan(got[1, 0, 0, 0]) and torch.isinf(got[1, 0, 5, 7])     # the partner keeps its own


def test_clip_mix_refuses_bad_arguments():
    from ssl_mae_amd import _lib
    from ssl_mae_amd import kernels as Kn
    x = torch.zeros(4, 6, 6, 8, device=DEV)
    lam, box = torch.ones(2), torch.zeros(2, 4, dtype=torch.int32)
    Kn.clip_mix(x, lam, box)
    for bad_box in ([0, 0, 7, 1], [5, 0, 2, 1], [0, 6, 1, 3], [-1, 0, 1, 1], [0, 0, 1, -1]):
        b = box.clone()
        b[1] = torch.tensor(bad_box, dtype=torch.int32)
        with pytest.raises(_lib.KernelError):
            Kn.clip_mix(x, lam, b)
    for args in ((x, lam.double(), box), (x, lam, box.long()), (x, torch.ones(3), box),
                 (x, lam, torch.zeros(1, 4, dtype=torch.int32)), (x, lam.to(DEV), box), (x.double(), lam, box),
                 (x[:, :, :, ::2], lam, box), (x.cpu(), lam, box)):
        with pytest.raises(_lib.KernelError):
            Kn.clip_mix(*args)
    for out in (torch.zeros(4, 6, 6, 8, device=DEV, dtype=torch.float64), torch.zeros(4, 6, 8, 6, device=DEV),
                torch.zeros(4, 6, 6, 16, device=DEV)[..., ::2]):
        with pytest.raises(_lib.KernelError):
            Kn.clip_mix(x, lam, box, out=out)
    big = torch.zeros(2 * x.numel(), device=DEV)
    with pytest.raises(_lib.KernelError):                    # overlaps x without being x
        Kn.clip_mix(big[:x.numel()].view(x.shape), lam, box, out=big[16:16 + x.numel()].view(x.shape))


def test_clip_mixer_on_the_device():
    """ClipMixer's launch equals the mirror of its own draws; labels and weights line up."""
    from ssl_mae_amd.mae_loader import ClipMixer
    g = torch.Generator().manual_seed(0)
    clip = torch.randn(5, 3, 2, 8, 8, generator=g).to(DEV)
    label = torch.tensor([3, 1, 4, 1, 5], device=DEV)
    m = ClipMixer(seed=11)
    for _ in range(4):
        mixed, la, lb, lam = m(clip, label)
        last = m.last
        lam_px = [last["lam"][p] if last["kind"][p] == "mixup" else 1.0 for p in range(2)]
        want = clip_mix_mirror(clip.cpu().numpy(), lam_px, last["box"])
        assert np.array_equal(_bits(mixed), want.view(np.int32))
        assert la is label and torch.equal(lb, label.flip(0))
        w = last["weight"]
        assert lam.dtype == torch.float32 and lam.cpu().tolist() == [w[0], w[1], 1.0, w[1], w[0]]
    assert mixed.data_ptr() != clip.data_ptr()


# ------------------------------------------------------------------ soft_ce
def _soft_case(N, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, C, generator=g) * 3
    ya, yb = torch.randint(0, C, (N,), generator=g), torch.randint(0, C, (N,), generator=g)
    lam = torch.rand(N, generator=g)
    lam[0] = 0.0
    if N > 2:
        lam[1], yb[2] = 1.0, ya[2]
    return logits, ya, yb, lam


@pytest.mark.parametrize("C", [3, 101, 260, 1000, 2047, 4095, 4096])
def test_soft_ce_matches_the_mirror(C):
    from ssl_mae_amd import kernels as Kn
    for N in (1, 5, 37):
        logits, ya, yb, lam = _soft_case(N, C, 1000 * N + C)
        lg, ya_, yb_, lam_ = logits.to(DEV), ya.to(DEV), yb.to(DEV), lam.to(DEV)
        scale = 1.0 / N
        for eps in (0.0, 0.1):
            for b, w in ((yb_, lam_), (None, None)):
                loss, dwant, hits = soft_ce_mirror(logits.numpy(), ya.numpy(), None if b is None else yb.numpy(),
                                                   None if w is None else lam.numpy(), eps, scale)
                dl = torch.empty_like(lg)
                out = Kn.soft_ce(lg, ya_, b, w, eps, dl, scale)
                assert out.shape == (2,) and out.dtype == torch.float64
                o = out.cpu().numpy()
                e_loss = abs(o[0] - loss.sum()) / abs(loss.sum())
                e_dl = float(np.abs(dl.cpu().numpy().astype(np.float64) - dwant).max() / scale)
                print(f"N={N} C={C} eps={eps} mixed={b is not None}: loss err {e_loss:.3e}, dlogits err {e_dl:.3e}")
                assert e_loss <= 1e-5 and e_dl <= 1e-5
                assert o[1] == hits
                # the scalar path: same bits
                dl2 = _offset_view(torch.zeros_like(dl))
                out2 = Kn.soft_ce(_offset_view(lg), ya_, b, w, eps, dl2, scale)
                assert torch.equal(out2, out) and torch.equal(dl2, dl)
                assert torch.equal(Kn.soft_ce(lg, ya_, b, w, eps), out)           # no gradient wanted


@pytest.mark.parametrize("C", [3, 101, 260, 1000, 4096])
def test_soft_ce_with_a_hard_target_has_logits_metrics_bits(C):
    from ssl_mae_amd import kernels as Kn
    for N in (1, 5, 37, 300):
        logits, ya, yb, lam = _soft_case(N, C, 7 * N + C)
        logits, ya = logits.to(DEV), ya.to(DEV)
        for x in (logits, _offset_view(logits)):
            d_h, d_s = torch.empty_like(logits), torch.empty_like(logits)
            hard = Kn.logits_metrics(x, ya, 1, 1, d_h, 1.0 / N)
            soft = Kn.soft_ce(x, ya, None, None, 0.0, d_s, 1.0 / N)
            assert soft[0].item() == hard[0, 0].item() and soft[1].item() == hard[0, 2].item()
            assert torch.equal(_as_int(d_s), _as_int(d_h))
            # lam == 1 with a partner is the same one-hot target
            mixed = Kn.soft_ce(x, ya, yb.to(DEV), torch.ones(N, device=DEV), 0.0, d_s, 1.0 / N)
            assert torch.equal(mixed, soft) and torch.equal(_as_int(d_s), _as_int(d_h))


def _as_int(t):
    return t.contiguous().view(torch.int32)


def test_soft_ce_large_logits_bad_labels_and_limits():
    from ssl_mae_amd import _lib
    from ssl_mae_amd import kernels as Kn
    logits, ya, yb, lam = _soft_case(5, 101, 5)
    args = (ya.to(DEV), yb.to(DEV), lam.to(DEV), 0.1)
    base = Kn.soft_ce(logits.to(DEV), *args).cpu().numpy()
    dl = torch.empty(5, 101, device=DEV)
    far = Kn.soft_ce((logits + 1e4).to(DEV), *args, dl, 1.0).cpu().numpy()
    want, _, want_hits = soft_ce_mirror((logits + 1e4).numpy(), ya.numpy(), yb.numpy(), lam.numpy(), 0.1)
    want = want.sum()
    print(f"loss {base[0]!r}; logits + 1e4: {far[0]!r}, fp64 of the shifted fp32 logits {want!r}")
    assert np.isfinite(far[0]) and bool(torch.isfinite(dl).all()) and far[1] == want_hits
    # fp32 values near 1e4 are 2^-10 apart: each of the 5 row losses carries the rounding of logsumexp
    # (half of that) and nothing else of that size; twice that is allowed
    assert abs(far[0] - want) <= 5 * 2.0 ** -10
    for bad_a, bad_b in ((101, 0), (-1, 0), (0, 101), (0, -1)):
        a, b = ya.clone(), yb.clone()
        a[3] = bad_a if bad_a else a[3]
        b[3] = bad_b if bad_b else b[3]
        out = Kn.soft_ce(logits.to(DEV), a.to(DEV), b.to(DEV), lam.to(DEV), 0.1).cpu().numpy()
        assert np.isnan(out[0]), (bad_a, bad_b)
    for bad in (float("nan"), float("inf")):
        l2 = logits.clone()
        l2[2, 7] = bad
        assert np.isnan(Kn.soft_ce(l2.to(DEV), *args).cpu().numpy()[0])
    # -inf is an ordinary value: a column without target weight adds nothing, one with weight (every
    # column once the labels are smoothed) makes the loss +inf, as -t log(0) is
    l2 = logits.clone()
    col = next(c for c in range(101) if c not in (int(ya[2]), int(yb[2])))
    l2[2, col] = float("-inf")
    assert np.isfinite(Kn.soft_ce(l2.to(DEV), *args[:3], 0.0).cpu().numpy()[0])
    assert Kn.soft_ce(l2.to(DEV), *args).cpu().numpy()[0] == np.inf
    z = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.KernelError):
        Kn.soft_ce(torch.zeros(2, 4097, device=DEV), z)
    for eps in (1.0, -0.1, float("nan")):
        with pytest.raises(_lib.KernelError):
            Kn.soft_ce(torch.zeros(2, 8, device=DEV), z, eps=eps)
    for kw in ({"labels_b": z}, {"lam": torch.ones(2, device=DEV)}, {"labels_b": z, "lam": torch.ones(3, device=DEV)},
               {"labels_b": z.int(), "lam": torch.ones(2, device=DEV)}):
        with pytest.raises(_lib.KernelError):
            Kn.soft_ce(torch.zeros(2, 8, device=DEV), z, **kw)


def test_soft_ce_ties_go_to_the_lower_index():
    from ssl_mae_amd import kernels as Kn
    logits = torch.zeros(3, 6, device=DEV)
    logits[:, 2] = logits[:, 4] = 1.0
    ya = torch.tensor([2, 4, 0], device=DEV)
    assert Kn.soft_ce(logits, ya, eps=0.1)[1].item() == 1.0


def test_soft_ce_fn_autograd():
    from ssl_mae_amd import kernels as Kn
    from ssl_mae_amd.finetune import SoftCEFn
    logits, ya, yb, lam = (t.to(DEV) for t in _soft_case(5, 101, 9))
    dl = torch.empty_like(logits)
    out = Kn.soft_ce(logits, ya, yb, lam, 0.1, dl, 1.0 / 5)
    x = logits.clone().requires_grad_()
    loss = SoftCEFn.apply(x, ya, yb, lam, 0.1)
    assert loss.dtype == torch.float32 and loss.item() == (out[0] / 5).float().item()
    (loss * 3.0).backward()
    assert torch.equal(x.grad, dl * 3.0)
    x.grad = None
    SoftCEFn.apply(x, ya, None, None, 0.1).backward()
    Kn.soft_ce(logits, ya, None, None, 0.1, dl, 1.0 / 5)
    assert torch.equal(x.grad, dl)


# ------------------------------------------------------------------ train_pass
class _Stub(torch.nn.Module):
    def __init__(self, nc):
        super().__init__()
        self.head = torch.nn.Linear(3, nc)

    def forward(self, clip):
        return self.head(clip.float().mean(dim=(2, 3, 4)))


def _batches(steps, B, nc, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 3, 2, 8, 8, generator=g).to(DEV), torch.randint(0, nc, (B,), generator=g).to(DEV))
            for _ in range(steps)]


def test_train_pass_with_mixer_and_smoothing():
    from ssl_mae_amd import driver
    from ssl_mae_amd.mae_loader import ClipMixer
    nc, eps = 5, 0.1
    torch.manual_seed(0)
    model = _Stub(nc).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    mixer = ClipMixer(seed=4)
    batches = _batches(3, 4, nc, 1)
    seen, infos = [], []

    def on_step(step, loss, logits, label):
        seen.append((step, loss.item(), logits.cpu().numpy(), label.cpu().numpy()))

    def on_mix(step, labels_b, lam):
        infos.append((step, labels_b.cpu().numpy(), lam.cpu().numpy(), dict(mixer.last)))

    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    steps, samples = driver.train_pass(model, batches, opt, DEV, False, sums, None, on_step, mixer=mixer,
                                       label_smoothing=eps, on_mix=on_mix)
    assert (steps, samples) == (3, 12) and len(seen) == len(infos) == 3
    total = 0.0
    for (s, loss, logits, label), (s2, lb, lam, last), (_, y) in zip(seen, infos, batches):
        assert s == s2 and np.array_equal(label, y.cpu().numpy())              # on_step: the batch's own labels
        assert np.array_equal(lb, label[::-1])
        w = last["weight"]
        assert lam.tolist() == [w[0], w[1], w[1], w[0]]
        want = soft_ce_mirror(logits, label, lb, lam, eps)[0].mean()
        print(f"step {s}: loss {loss!r}, fp64 soft loss {want!r}, draws {last['kind']}")
        assert abs(loss - want) <= 1e-5 * abs(want)
        total += loss
    assert abs(sums[0].item() - total) <= 1e-12 * abs(total) and abs(sums[1].item() - 4 * total) <= 1e-12 * abs(total)
    # label smoothing alone: no mixer, the soft loss of the smoothed labels
    seen.clear()
    driver.train_pass(model, batches[:1], opt, DEV, False, sums, None, on_step, label_smoothing=eps)
    _, loss, logits, label = seen[0]
    want = soft_ce_mirror(logits, label, None, None, eps)[0].mean()
    assert abs(loss - want) <= 1e-5 * abs(want)


def test_train_pass_defaults_are_the_unchanged_path():
    from ssl_mae_amd import driver
    from ssl_mae_amd.finetune import TopCEFn
    nc = 5
    batches = _batches(3, 4, nc, 2)
    losses = {}
    for name in ("pass", "plain"):
        torch.manual_seed(0)
        model = _Stub(nc).to(DEV)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        got = []
        if name == "pass":
            sums = torch.zeros(2, dtype=torch.float64, device=DEV)
            driver.train_pass(model, batches, opt, DEV, False, sums, None, lambda s, loss, lg, y: got.append(loss.item()))
        else:
            for clip, label in batches:                   # the step as it was before the new arguments
                opt.zero_grad(set_to_none=True)
                loss = TopCEFn.apply(model(clip), label)
                loss.backward()
                opt.step()
                got.append(loss.item())
        losses[name] = got
    assert losses["pass"] == losses["plain"]

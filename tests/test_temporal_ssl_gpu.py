"""Temporal SSL pretraining on the GPU: the csrc/temporal.hip kernels against the fp64 mirror
(tests/temporal_mirror.py), and the model / step against the fixture the reference recorded
(tests/golden/temporal_ssl.npz, tests/golden/make_golden_temporal.py).

Tolerances.  Loss kernels: the project's 1e-5 (relative on the losses, relative to the largest
|dpred| on the gradient).  EMA: 2^-23 (|m e| + |(1 - m) p|), three roundings.  Clip: norm 1e-6
relative, scaled values 2^-23 relative of g coef.  Fixture (a) (fp32, head only): 1e-5 of each
quantity's scale; (b) (fp32 end to end): the project's fp32 parity 1e-3 in the form of the
fine-tune row's ft_ssl test; bf16: 3e-2 on the losses.
A parameter whose gradient is analytically zero (a bias in front of a train-mode BatchNorm, the
attention key bias) holds rounding noise on both sides, and AdamW turns noise g into a step
lr g / (|g| + 1e-8) of either sign: for those (reference gradient L2 below 1e-5 of the largest)
only sizes are checked -- the gradient stays noise, the values move by at most lr.  The same
holds for single elements whose gradient is below the gradient tolerance; fixture (a) compares
the after-step values element by element with that allowance on exactly those elements
(temporal_mirror.adam_step_slack), fixture (b) through per-parameter summaries."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import temporal_mirror as TM
from ssl_mae_amd import temporal_ssl as TS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_mae_amd import build
    build.build()


def KK():
    from ssl_mae_amd import ops
    return ops


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "temporal_ssl.npz"))


# ------------------------------------------------------------------ masked-frame loss
MFM_CASES = [(8, 576, 6), (15, 37, 11), (4, 64, 1), (400, 96, 300)]     # (R, D, N); 300 rows = 10 partitions of 32
# the final kernel's 256 strided sums over N rows and D columns see fewer than 256, and more than 256, of each
# (N = 33: two row partitions); D = 4 and 100 take the scalar form in bf16 (no multiple of 8)
MFM_CASES += [(N + 3, D, N) for N in (1, 33, 257) for D in (4, 100, 576)]
W_MFM, W_VAR, EPS, UP = 1.0, 25.0, 1e-4, 0.7
_mfm_ref = {}


def _mfm_case(R, D, N, dtype):
    """Inputs and the mirror's answers, computed once per case."""
    key = (R, D, N, dtype)
    if key not in _mfm_ref:
        g = torch.Generator().manual_seed(R * 1000 + D * 7 + N)
        pred = (torch.randn(R, D, generator=g) * torch.linspace(0.2, 3.0, D)).to(dtype)
        teacher = torch.randn(R, D, generator=g)
        idx = torch.sort(torch.randperm(R, generator=g)[:N]).values            # scattered, ascending
        sigma = TM.mfm_terms(pred, teacher, idx, 1.0, EPS)[2]
        target = TM.midpoint_target(sigma) if N > 1 else 1.0
        losses, dpred, sigma = TM.mfm_loss_and_grad(pred, teacher, idx, W_MFM, W_VAR, target, EPS, UP)
        _mfm_ref[key] = (pred, teacher, idx, target, losses, dpred, sigma)
    return _mfm_ref[key]


def _run_mfm(pred, teacher, idx, target, out_dtype=torch.float32):
    K = KK()
    out, stats = K.mfm_loss_fwd(pred, teacher, idx, W_MFM, W_VAR, target, EPS)
    gout = torch.tensor([UP], dtype=torch.float32, device=DEV)
    return out, K.mfm_loss_bwd(pred, teacher, idx, stats, gout, W_MFM, W_VAR, out_dtype=out_dtype)


def _offset_view(t):
    """The same values in a view that starts one element into its storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R,D,N", MFM_CASES)
def test_mfm_loss_against_mirror(R, D, N, dtype):
    pred, teacher, idx, target, losses, dref, sigma = _mfm_case(R, D, N, dtype)
    if N > 1:        # the hinge is active for some columns and not for others, none at the kink
        below, above = int((sigma < target).sum()), int((sigma > target).sum())
        assert below >= D // 4 and above >= D // 4, (below, above)
        assert float(((sigma - target).abs() / target).min()) > 1e-3
    else:
        assert float((sigma - math.sqrt(EPS)).abs().max()) < 1e-12       # a single row: sigma = sqrt(eps)
    p, t, i32 = pred.to(DEV), teacher.to(DEV), idx.to(torch.int32).to(DEV)
    out, dp = _run_mfm(p, t, i32, target)
    got = out.double().cpu()
    print("losses", got.tolist(), losses.tolist())
    for k in range(3):
        assert abs(float(got[k]) - float(losses[k])) <= 1e-5 * abs(float(losses[k])), (k, got, losses)
    err = float((dp.double().cpu() - dref).abs().max())
    print("dpred err", err, "of", float(dref.abs().max()))
    assert err <= 1e-5 * float(dref.abs().max())
    unmasked = torch.ones(R, dtype=torch.bool)
    unmasked[idx] = False
    assert bool((dp.cpu()[unmasked].view(torch.int32) == 0).all())          # exactly +0
    # run to run
    out2, dp2 = _run_mfm(p, t, i32, target)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(dp.view(torch.int32),
                                                                                        dp2.view(torch.int32))
    # a view offset by one element takes the scalar form: same bits
    out3, dp3 = _run_mfm(_offset_view(p), t, i32, target)
    assert torch.equal(out.view(torch.int32), out3.view(torch.int32))
    assert torch.equal(dp.view(torch.int32), dp3.view(torch.int32))
    out4, dp4 = _run_mfm(p, _offset_view(t), i32, target)
    assert torch.equal(out.view(torch.int32), out4.view(torch.int32))
    assert torch.equal(dp.view(torch.int32), dp4.view(torch.int32))
    if dtype == torch.bfloat16:      # the default gradient dtype is pred's: the same values, rounded once
        _, dpb = _run_mfm(p, t, i32, target, out_dtype=None)
        assert dpb.dtype == torch.bfloat16 and torch.equal(dpb, dp.to(torch.bfloat16))


def test_mfm_loss_function_autograd():
    """MFMLossFn / cosine_loss / variance_loss: the gradient reaches pred through element 2 only."""
    pred, teacher, idx, target, losses, dref, _ = _mfm_case(8, 576, 6, torch.float32)
    p = pred.to(DEV).requires_grad_(True)
    out = TS.MFMLossFn.apply(p, teacher.to(DEV), idx.to(torch.int32).to(DEV), W_MFM, W_VAR, target, EPS)
    (out[2] * UP).backward()
    assert float((p.grad.double().cpu() - dref).abs().max()) <= 1e-5 * float(dref.abs().max())
    rows = pred[idx].to(DEV)
    z = teacher[idx].to(DEV)
    mfm, var, _ = TM.mfm_terms(pred[idx], teacher[idx], torch.arange(idx.numel()), 1.0, EPS)
    assert abs(float(TS.cosine_loss(rows, z)) - float(mfm)) <= 1e-5 * float(mfm)
    assert abs(float(TS.variance_loss(rows, 1.0, EPS)) - float(var)) <= 1e-5 * float(var)


# ------------------------------------------------------------------ EMA
@pytest.mark.parametrize("m", [0.0, 0.996, 1.0])
@pytest.mark.parametrize("offset", [0, 1])
def test_ema_update(m, offset):
    n = 100003                                               # not a multiple of 4
    g = torch.Generator().manual_seed(5)
    e = torch.randn(n + offset, generator=g)[offset:]
    p = torch.randn(n + offset, generator=g)[offset:]
    ref, bound = TM.ema_fp64(e, p, m)
    dst = torch.empty(n + offset, device=DEV)[offset:]
    dst.copy_(e)
    src = p.to(DEV)
    KK().ema_update(dst, src, m)
    got = dst.cpu()
    assert bool(((got.double() - ref).abs() <= bound).all())
    if m == 1.0:
        assert torch.equal(got.view(torch.int32), e.view(torch.int32))
    if m == 0.0:
        assert torch.equal(got.view(torch.int32), p.view(torch.int32))
    assert torch.equal(src.cpu(), p)


@pytest.mark.parametrize("offset", [0, 1])
def test_ema_update_past_the_grid_cap(offset):
    """n = 4 * 8192 * 256 + 5: the grid is capped at 8192 blocks, so the 16-byte form's grid-stride loop
    takes a second turn (one group) and a tail of one element; the scalar form (offset view) takes five."""
    n = 4 * 8192 * 256 + 5
    g = torch.Generator().manual_seed(6)
    e = torch.randn(n + offset, generator=g)[offset:]
    p = torch.randn(n + offset, generator=g)[offset:]
    ref, bound = TM.ema_fp64(e, p, 0.996)
    dst = torch.empty(n + offset, device=DEV)[offset:]
    dst.copy_(e)
    assert (dst.data_ptr() % 16 != 0) == bool(offset)
    KK().ema_update(dst, p.to(DEV), 0.996)
    assert bool(((dst.cpu().double() - ref).abs() <= bound).all())


def test_update_ema_over_the_flat_buffers():
    model = TS.TemporalSSL(64, 1, 2, 5, encoder=TM.StandInEncoder(64)).to(DEV)
    ema = copy.deepcopy(model)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.5)
    before = {n: p.detach().clone() for n, p in ema.named_parameters()}
    bufs = {n: b.detach().clone() for n, b in ema.named_buffers()}
    TS.update_ema(ema, model, 0.9)
    student = dict(model.named_parameters())
    for n, p in ema.named_parameters():
        ref, bound = TM.ema_fp64(before[n].cpu(), student[n].detach().cpu(), 0.9)
        assert bool(((p.detach().cpu().double() - ref).abs() <= bound).all()), n
    for n, b in ema.named_buffers():                           # parameters only
        assert torch.equal(b, bufs[n]), n


# ------------------------------------------------------------------ gradient clipping
def _clip_ref(g, ranges, max_norm, norm_out):
    sel = torch.cat([g[s:e] for s, e in ranges]).double()
    norm = float(sel.norm())
    coef = torch.tensor(max_norm, dtype=torch.float32) / (norm_out.cpu() + 1e-6)     # fp32, as torch forms it
    return norm, float(torch.clamp(coef, max=1.0))


@pytest.mark.parametrize("ranges", [[(8, 9000), (9016, 20000)], [(3, 10001)],
                                    [(i * 1000, i * 1000 + 400 + i) for i in range(20)],
                                    # 19 ranges, the first and the tenth empty: 17 non-empty ones in two groups
                                    # of at most 16, each of which must be taken exactly once
                                    [(i * 1000, i * 1000 + (0 if i in (0, 9) else 400 + i)) for i in range(19)]],
                         ids=["gap", "misaligned", "20ranges", "19ranges_2empty"])
def test_grad_clip(ranges):
    g = torch.randn(20500, generator=torch.Generator().manual_seed(9)) * 0.3
    d = g.to(DEV)
    norm_out = KK().grad_clip(d, ranges, 1.0)
    norm, coef = _clip_ref(g, ranges, 1.0, norm_out)
    print("norm", float(norm_out), norm, "coef", coef)
    assert abs(float(norm_out) - norm) <= 1e-6 * norm and coef < 1.0
    got = d.cpu()
    inside = torch.zeros(g.numel(), dtype=torch.bool)
    for s, e in ranges:
        inside[s:e] = True
    assert torch.equal(got[~inside].view(torch.int32), g[~inside].view(torch.int32))   # the gaps are not touched
    want = g[inside].double() * coef
    assert bool(((got[inside].double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
    # a second buffer with the same values: bit-identical
    d2 = g.to(DEV)
    n2 = KK().grad_clip(d2, ranges, 1.0)
    assert torch.equal(d2.view(torch.int32), d.view(torch.int32)) and torch.equal(n2, norm_out)


_CLIP_EDGE_N = 256 * 8192 + 1


@pytest.fixture(scope="module")
def clip_edge_grad():
    return torch.randn(_CLIP_EDGE_N + 8, generator=torch.Generator().manual_seed(12)) * 0.3


@pytest.mark.parametrize("start", [0, 3], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("length", [1, 8192, 8192 + 1, 256 * 8192, _CLIP_EDGE_N])
def test_grad_clip_chunk_counts(clip_edge_grad, length, start):
    """One range of 1, 256 and 257 chunks (the second level's 256 strided sums see fewer than 256,
    exactly 256 and 257 partials), and chunks of one element and of 8192 + 1 (a block whose last
    three waves, or all but one lane, add nothing)."""
    g = clip_edge_grad
    ranges = [(start, start + length)]
    max_norm = 0.01                                          # below |g[0]| = 0.04 and |g[3]| = 0.14: every case clips
    d = g.to(DEV)
    norm_out = KK().grad_clip(d, ranges, max_norm)
    norm, coef = _clip_ref(g, ranges, max_norm, norm_out)
    print("length", length, "norm", float(norm_out), norm, "coef", coef)
    assert abs(float(norm_out) - norm) <= 1e-6 * norm and coef < 1.0
    got = d.cpu()
    inside = torch.zeros(g.numel(), dtype=torch.bool)
    inside[start:start + length] = True
    assert torch.equal(got[~inside].view(torch.int32), g[~inside].view(torch.int32))
    want = g[inside].double() * coef
    assert bool(((got[inside].double() - want).abs() <= 2.0 ** -23 * want.abs()).all())


def test_grad_clip_below_max_norm_leaves_the_buffer():
    g = torch.randn(30000, generator=torch.Generator().manual_seed(10)) * 1e-3
    d = g.to(DEV)
    norm_out = KK().grad_clip(d, [(0, 12345), (12352, 30000)], 1.0)
    assert float(norm_out) < 1.0
    assert torch.equal(d.cpu().view(torch.int32), g.view(torch.int32))


def test_grad_clip_nan_then_adamw_skips():
    from ssl_mae_amd.mae_vit_adapter import make_flat
    from ssl_mae_amd.optim import FusedAdamW
    lin = nn.Sequential(nn.Linear(24, 40), nn.Linear(40, 8)).to(DEV)
    flat = make_flat(lin, torch.device(DEV))
    opt = FusedAdamW(lin.parameters(), lr=1e-2)
    flat.grad.copy_(torch.randn(flat.total, generator=torch.Generator().manual_seed(3)))
    flat.grad[17] = float("nan")
    flat.touch(*lin.parameters())
    before = flat.data.clone()
    norm = KK().grad_clip(flat.grad, flat.touched_ranges(), 1.0)
    assert not math.isfinite(float(norm))
    assert not bool(torch.isfinite(flat.grad).all())
    opt.step()
    assert torch.equal(flat.data, before) and int(opt._state["step"]) == 0
    # the same with finite gradients: the step is taken
    flat.grad.copy_(torch.randn(flat.total, generator=torch.Generator().manual_seed(4)))
    assert math.isfinite(float(KK().grad_clip(flat.grad, flat.touched_ranges(), 1.0)))
    opt.step()
    assert not torch.equal(flat.data, before) and int(opt._state["step"]) == 1


# ------------------------------------------------------------------ ReLU + dropout
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_relu_dropout_p0_is_relu(dtype):
    x = torch.randn(67, 520, generator=torch.Generator().manual_seed(2)).to(dtype).to(DEV)
    y = KK().relu_dropout_fwd(x, 0.0, 99)
    assert torch.equal(y, torch.relu(x))
    dy = torch.randn(67, 520, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    for ref in (x, y):                                       # the forward's input or its output
        assert torch.equal(KK().relu_dropout_bwd(ref, dy, 0.0, 99), torch.where(x > 0, dy, torch.zeros_like(dy)))


def _dropout_run():
    x = (torch.rand(1024, 1024, generator=torch.Generator().manual_seed(4)) + 0.5).to(DEV)     # all positive
    seed = 0x9E3779B97F4A7C15
    y = KK().relu_dropout_fwd(x, 0.1, seed)
    return x, y, seed


def test_relu_dropout_mask_scale_and_backward():
    x, y, seed = _dropout_run()
    scale, thr = TM.drop_scale(0.1)
    kept = y != 0
    frac = float(kept.double().mean())
    n = x.numel()
    rate = (65536 - thr) / 65536.0                           # the 16-bit threshold's keep rate, 58982 / 65536
    assert thr == 6554 and abs(scale * rate - 1.0) < 1e-15   # unbiased: the scale is the rate's inverse
    print("kept fraction", frac, "quantised rate", rate)
    assert abs(frac - rate) <= 4 * math.sqrt(rate * (1 - rate) / n)
    assert torch.equal(y[kept], (x * torch.tensor(scale, dtype=torch.float32, device=DEV))[kept])
    dy = torch.ones_like(x)
    for ref in (x, y):
        dx = KK().relu_dropout_bwd(ref, dy, 0.1, seed)
        assert torch.equal(dx != 0, kept)                    # the backward regenerates the forward's mask
        assert torch.equal(dx[kept], torch.full_like(dx[kept], scale))
    y2 = KK().relu_dropout_fwd(x, 0.1, seed + 1)
    assert not torch.equal(y2 != 0, kept)


def test_relu_dropout_kept_fraction_within_4_sigma_of_0p9():
    """At p = 0.1 the kept fraction is within 4 sigma of 0.9 over 2^20 elements (sigma = 2.93e-4).
    The counter hash's 8-bit threshold (230 / 256 = 0.8984 at p = 0.1, the attention / GELU
    dropout's convention) lies 5.3 sigma from 0.9 and measured 6.6 sigma away, so this kernel takes
    the hash's 16-bit threshold: 58982 / 65536 = 0.899994, with the inverse of that rate as scale."""
    x, y, _ = _dropout_run()
    frac = float((y != 0).double().mean())
    sigma = math.sqrt(0.9 * 0.1 / x.numel())
    print("kept fraction", frac, "sigma", sigma, "distance / sigma", (frac - 0.9) / sigma)
    assert abs(frac - 0.9) <= 4 * sigma


def test_block_relu_flag_against_torch():
    """BlockFn with st.relu on an fp32 stream (eval: no dropout) against nn.TransformerEncoderLayer's
    own forward and autograd in fp32 on the host, at L = T = 5."""
    torch.manual_seed(0)
    B, T, D, H = 3, 5, 64, 2
    model = TS.TemporalSSL(D, 1, H, T, encoder=TM.StandInEncoder(D)).to(DEV).eval()
    layer = copy.deepcopy(model.temporal.layers[0]).cpu().train()
    for m in layer.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    layer.self_attn.dropout = 0.0
    x = torch.randn(B, T, D)
    xr = x.clone().requires_grad_(True)
    yr = layer(xr)
    w = torch.randn(B, T, D)
    (yr * w).sum().backward()
    from ssl_mae_amd.functions import BlockFn, Mode
    from ssl_mae_amd.mae_vit_adapter import _St, ensure_flat
    mode = Mode(False, 1)
    ensure_flat(model, mode)
    lay = model.temporal.layers[0]
    sa = lay.self_attn
    st = _St(mode=mode, N=B, L=T, heads=H, head_dim=D // H, eps=lay.norm1.eps, relu=True, attn_drop=0.0, seed_attn=0,
             drop1=0.0, seed1=0, drop_ff=0.0, seed_ff=0, drop2=0.0, seed2=0, dp1=None, dp2=None)
    xd = x.reshape(B * T, D).to(DEV).requires_grad_(True)
    y = BlockFn.apply(xd, st, lay.norm1.weight, lay.norm1.bias, sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight,
                      sa.out_proj.bias, lay.norm2.weight, lay.norm2.bias, lay.linear1.weight, lay.linear1.bias,
                      lay.linear2.weight, lay.linear2.bias)
    (y * w.reshape(B * T, D).to(DEV)).sum().backward()
    assert float((y.detach().cpu() - yr.detach().reshape(B * T, D)).abs().max()) < 1e-4
    assert float((xd.grad.cpu() - xr.grad.reshape(B * T, D)).abs().max()) < 1e-4
    ref = dict(layer.named_parameters())
    for n, p in lay.named_parameters():
        scale = float(ref[n].grad.abs().max()) + 1e-6
        assert float((p._sm_grad.cpu() - ref[n].grad).abs().max()) < 1e-4 * max(scale, 1.0), n


# ------------------------------------------------------------------ attention at L = T
@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 3e-2)], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", [4, 5, 16])
@pytest.mark.parametrize("D", [32, 64])
def test_attention_at_temporal_lengths(L, D, dtype, tol):
    """The attention kernels at the temporal layers' sequence lengths against fp32 torch math."""
    N, H = 3, 2
    g = torch.Generator().manual_seed(L * 100 + D)
    qkv = torch.randn(N * L, 3 * H * D, generator=g).to(dtype)
    do = torch.randn(N * L, H * D, generator=g).to(dtype)
    r = qkv.float().view(N, L, 3, H, D).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)     # [3,N,H,L,D]
    p = torch.softmax(r[0] @ r[1].transpose(-1, -2) / math.sqrt(D), dim=-1)
    o_ref = (p @ r[2]).permute(0, 2, 1, 3).reshape(N * L, H * D)
    (o_ref * do.float()).sum().backward()
    dqkv_ref = r.grad.permute(1, 3, 0, 2, 4).reshape(N * L, 3 * H * D)
    K = KK()
    o, lse = K.attn_fwd(qkv.to(DEV), N, L, H, D, 0.0, 0)
    dqkv = K.attn_bwd(qkv.to(DEV), o, do.to(DEV), lse, N, L, H, D, 0.0, 0)
    assert float((o.float().cpu() - o_ref.detach()).abs().max()) < tol * max(1.0, float(o_ref.abs().max()))
    assert float((dqkv.float().cpu() - dqkv_ref).abs().max()) < tol * max(1.0, float(dqkv_ref.abs().max()))


# ------------------------------------------------------------------ fixtures
CFG = {"training": {"amp": False, "clip_grad_norm": 1.0, "log_interval": 1000, "learning_rate": 5e-4,
                    "weight_decay": 0.05},
       "ssl_objectives": {"mask_ratio": 0.75, "mfm_weight": 1.0, "ema_momentum": 0.996, "var_weight": 25.0,
                          "var_eps": 1e-4, "var_target_std": 1.0, "top_weight": 1.0, "top_start_epoch": 1,
                          "top_every": 1, "top_subsample": 1.0, "top_detach_backbone": False}}


def _cfg(top_subsample):
    cfg = copy.deepcopy(CFG)
    cfg["ssl_objectives"]["top_subsample"] = top_subsample
    return cfg


def _parity(model):
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, nn.MultiheadAttention):
            m.dropout = 0.0
        if hasattr(m, "drop_prob"):
            m.drop_prob = 0.0


def _step(gold, tag, model, top_subsample, amp=False, teacher_amp=None):
    from ssl_mae_amd.init_rule import apply_rule, synthetic_clip
    from ssl_mae_amd.optim import FusedAdamW
    B, T, S = int(gold[tag + "B"]), int(gold[tag + "T"]), int(gold[tag + "S"])
    model = model.to(DEV)
    apply_rule(model)
    _parity(model)
    ema = copy.deepcopy(model)
    for p in ema.parameters():
        p.requires_grad_(False)
    model.train()
    ema.eval()
    opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    clip = torch.from_numpy(synthetic_clip(B, T, S, seed=int(gold[tag + "clip_seed"]))).to(DEV)
    torch.manual_seed(int(gold[tag + "seed"]))
    cfg = _cfg(top_subsample)
    if teacher_amp is not None:
        cfg["training"]["teacher_amp"] = teacher_amp
    r = TS.ssl_step(model, ema, clip, cfg, 1, 1, opt=opt, amp=amp)
    assert np.array_equal(r["mask"].numpy(), gold[tag + "mask"])
    assert np.array_equal(r["labels"].numpy(), gold[tag + "labels"])
    return model, ema, r


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _summary_ok(t, row, tol, step=None):
    """t against a fixture row (sum, L2, first 8): L2 relative, sum and head relative plus `tol`
    of the tensor's RMS scale (cancellation), as the fine-tune row's ft_ssl test.  `step` = (sum,
    L2, first 8) of how far an optimizer step may have moved the elements (see _check_params)."""
    s, l2, head = TM.summary(t)
    n = t.numel()
    rms = float(row[1]) / max(1, n) ** 0.5
    step = np.zeros(10) if step is None else step
    bad = []
    if abs(l2 - row[1]) > tol * row[1] + 1e-12 + step[1]:
        bad.append(("l2", l2, float(row[1])))
    if abs(s - row[0]) > tol * abs(row[0]) + tol * rms * n ** 0.5 + step[0]:
        bad.append(("sum", s, float(row[0])))
    ref_h = row[2:2 + head.size]
    if np.any(np.abs(head - ref_h) > tol * np.abs(ref_h) + tol * rms + step[2:2 + head.size]):
        bad.append(("head", float(np.max(np.abs(head - ref_h))), rms))
    return bad


def _check_params(gold, tag, model, ema, tol, lr=5e-4, m=0.996):
    """Clipped gradient, student after AdamW and teacher after the EMA update against the fixture.
    AdamW's first step is lr g / (|g| + 1e-8): where |g| is below the gradient tolerance the step
    is a full lr of either sign whatever the arithmetic, so the fixture's `cond` row holds, per
    parameter, how far (in lr) a gradient error of tol max|g| can move the elements -- zero to
    rounding for every element well above the tolerance (make_golden_temporal.py record()).  A
    parameter whose whole gradient is rounding noise gets the bound of a full step per element."""
    names = [str(n) for n in gold[tag + "names"]]
    params, teacher = dict(model.named_parameters()), dict(ema.named_parameters())
    assert set(names) == {n for n, p in params.items()}
    top = float(gold[tag + "g"][:, 1].max())
    bad = []
    for i, n in enumerate(names):
        g = params[n]._sm_grad
        numel = g.numel()
        if float(gold[tag + "g"][i, 1]) < 1e-5 * top:
            if float(g.double().norm()) > 1e-4 * top:
                bad.append((n, "noise", float(g.double().norm())))
            step = lr * np.concatenate([[2.0 * numel, 2.0 * numel ** 0.5], np.full(8, 2.0)])
        else:
            bad += [(n, "g") + b for b in _summary_ok(g, gold[tag + "g"][i], tol)]
            step = lr * gold[tag + "cond"][i]
        bad += [(n, "after") + b for b in _summary_ok(params[n], gold[tag + "after"][i], tol, step)]
        bad += [(n, "ema") + b for b in _summary_ok(teacher[n], gold[tag + "ema"][i], tol, (1.0 - m) * step)]
    return bad


def test_fixture_a_head_only(gold):
    """The reference's step through the real TemporalSSL head with the stand-in encoder, fp32:
    every recorded quantity, element by element, within 1e-5 of its scale.  One allowance on top,
    for the values after AdamW / EMA only: an element whose gradient is below the 1e-5 gradient
    tolerance takes a first Adam step lr g / (|g| + 1e-8) of either sign in any arithmetic, the
    reference's included, so such elements (counted and printed) get up to 2 lr."""
    model = TS.TemporalSSL(int(gold["a/D"]), 1, 2, int(gold["a/T"]), encoder=TM.StandInEncoder(int(gold["a/D"])))
    model, ema, r = _step(gold, "a/", model, 0.7)
    figures = {k: (float(r[k]), float(gold["a/" + k])) for k in ("mfm", "var", "top", "norm")}
    print(figures)
    for k in ("ctx", "ctx_t", "pred"):
        ref = torch.from_numpy(gold["a/" + k]).reshape(-1)
        err = float((r[k].float().cpu().reshape(-1) - ref).abs().max())
        print(k, err, float(ref.abs().max()))
        assert err <= 1e-5 * float(ref.abs().max()), k
    for k, (got, ref) in figures.items():
        assert abs(got - ref) <= 1e-5 * abs(ref), (k, got, ref)
    # gradients in full, per parameter relative to its largest entry
    names = [str(n) for n in gold["a/names"]]
    params = dict(model.named_parameters())
    top = float(gold["a/g"][:, 1].max())
    off = 0
    bad = []
    for i, n in enumerate(names):
        p = params[n]
        ref = torch.from_numpy(gold["a/grads"][off:off + p.numel()]).reshape(p.shape)
        off += p.numel()
        if float(gold["a/g"][i, 1]) < 1e-5 * top:
            continue                                          # analytically zero: checked by size below
        err = float((p._sm_grad.cpu() - ref).abs().max())
        if err > 1e-5 * float(ref.abs().max()):
            bad.append((n, err, float(ref.abs().max())))
    assert off == gold["a/grads"].size and not bad, bad
    # the student after AdamW and the teacher after the EMA update, every element: 1e-5 of the
    # parameter's largest value, plus what one AdamW step can move an element whose gradient is
    # below the gradient tolerance (TM.adam_step_slack, nothing elsewhere; x (1 - m) for the teacher)
    teacher = dict(ema.named_parameters())
    lr, m = 5e-4, 0.996
    off, loose = 0, 0
    for i, n in enumerate(names):
        p = params[n]
        k = p.numel()
        noise = float(gold["a/g"][i, 1]) < 1e-5 * top
        if noise and float(p._sm_grad.double().norm()) > 1e-4 * top:
            bad.append((n, "noise gradient", float(p._sm_grad.double().norm())))
        slack = lr * TM.adam_step_slack(torch.from_numpy(gold["a/grads"][off:off + k]), 1e-5, whole_noise=noise)
        loose += int((slack > 1e-9).sum())
        for key, t, f in (("after_full", p, 1.0), ("ema_full", teacher[n], 1.0 - m)):
            ref = torch.from_numpy(gold["a/" + key][off:off + k]).double()
            err = (t.detach().double().reshape(-1).cpu() - ref).abs()
            if bool((err > 1e-5 * float(ref.abs().max()) + f * slack).any()):
                bad.append((n, key, float(err.max()), float(ref.abs().max())))
        off += k
    print("elements with an AdamW allowance:", loose, "of", off)
    assert off == gold["a/after_full"].size == gold["a/ema_full"].size and not bad, bad[:10]
    bn = model.predictor_bn1
    for k in ("running_mean", "running_var"):
        ref = torch.from_numpy(gold["a/buf/predictor_bn1." + k])
        assert float((getattr(bn, k).cpu() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), k
    assert int(bn.num_batches_tracked) == int(gold["a/buf/predictor_bn1.num_batches_tracked"]) == 1
    assert int(ema.predictor_bn1.num_batches_tracked) == 0    # the teacher's buffers stay as constructed


@pytest.fixture(scope="module")
def step_b(gold):
    model = TS.TemporalSSL(576, 2, 9, int(gold["b/T"]))
    return _step(gold, "b/", model, 1.0)


def test_fixture_b_one_real_step(gold, step_b):
    """One fp32 step with the TinyViT encoder end to end: losses, the pre-clip norm, every
    parameter's clipped gradient, the student after AdamW, the teacher after the EMA update and
    the BatchNorm buffers within the project's fp32 parity of 1e-3."""
    model, ema, r = step_b
    figures = {k: (float(r[k]), float(gold["b/" + k])) for k in ("mfm", "var", "top", "norm")}
    print(figures)
    for k, (got, ref) in figures.items():
        assert abs(got - ref) <= 1e-3 * abs(ref), (k, got, ref)
    bad = _check_params(gold, "b/", model, ema, 1e-3)
    assert not bad, bad[:10]
    bufs = dict(model.named_buffers())
    for i, n in enumerate(str(n) for n in gold["b/bufnames"]):
        v = bufs[n].double().reshape(-1)
        ref = gold["b/bufstats"][i]
        assert abs(float(v.sum()) - ref[0]) <= 1e-3 * abs(ref[0]) + 1e-3 * ref[1] and \
            abs(float(v.norm()) - ref[1]) <= 1e-3 * ref[1] + 1e-9, (n, float(v.sum()), float(v.norm()), ref)
    for k in ("running_mean", "running_var"):
        ref = torch.from_numpy(gold["b/buf/predictor_bn1." + k])
        assert float((getattr(model.predictor_bn1, k).cpu() - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
    tracked = [int(b) for n, b in ema.named_buffers() if n.endswith("num_batches_tracked")]
    assert max(tracked) == int(gold["b/ema_bn_tracked_max"]) == 0


def test_fixture_b_bf16_autocast(gold):
    model = TS.TemporalSSL(576, 2, 9, int(gold["b/T"]))
    _, _, r = _step(gold, "b/", model, 1.0, amp=True)
    figures = {k: (float(r[k]), float(gold["b/" + k])) for k in ("mfm", "var", "top")}
    print(figures)
    for k, (got, ref) in figures.items():
        assert abs(got - ref) <= 3e-2 * abs(ref), (k, got, ref)
    assert r["pred"].dtype == torch.bfloat16 and r["ctx"].dtype == torch.float32


def test_teacher_amp_false_is_the_fp32_teacher(gold, step_b):
    """training.teacher_amp: false under bf16 autocast gives the teacher tokens of the fp32 step
    bit for bit (same weights, same clip, the fp32 path), the student staying bf16."""
    model = TS.TemporalSSL(576, 2, 9, int(gold["b/T"]))
    _, _, r = _step(gold, "b/", model, 1.0, amp=True, teacher_amp=False)
    assert torch.equal(r["ctx_t"], step_b[2]["ctx_t"]) and r["pred"].dtype == torch.bfloat16
    _, _, r2 = _step(gold, "b/", TS.TemporalSSL(576, 2, 9, int(gold["b/T"])), 1.0, amp=True)
    assert not torch.equal(r2["ctx_t"], step_b[2]["ctx_t"])            # the default: the student's precision
    for k in ("mfm", "var", "top"):
        assert abs(float(r[k]) - float(gold["b/" + k])) <= 3e-2 * abs(float(gold["b/" + k])), k


def test_top_detach_backbone_trains_the_head_only(gold):
    from ssl_mae_amd.init_rule import apply_rule, synthetic_clip
    model = TS.TemporalSSL(64, 1, 2, 5, encoder=TM.StandInEncoder(64)).to(DEV)
    apply_rule(model)
    ema = copy.deepcopy(model).eval()
    model.train()
    cfg = _cfg(1.0)
    cfg["ssl_objectives"].update(mfm_weight=0.0, var_weight=0.0, top_detach_backbone=True)
    clip = torch.from_numpy(synthetic_clip(3, 5, 32, seed=1)).to(DEV)
    TS.ssl_step(model, ema, clip, cfg, 1, 1, opt=None)
    assert float(model.top_head.weight._sm_grad.abs().max()) > 0
    assert float(model.temporal.layers[0].linear1.weight._sm_grad.abs().max()) == 0
    cfg["ssl_objectives"]["top_start_epoch"] = 6                 # TOP off before its start epoch
    assert TS.ssl_step(model, ema, clip, cfg, 1, 1, opt=None)["top"] is None
    cfg["ssl_objectives"].update(top_start_epoch=1, top_every=2)
    assert TS.ssl_step(model, ema, clip, cfg, 1, 1, opt=None)["top"] is None
    assert TS.ssl_step(model, ema, clip, cfg, 1, 2, opt=None)["top"] is not None


def test_permute_frames_4way_is_index_arithmetic():
    clip = torch.randn(4, 3, 8, 16, 16, generator=torch.Generator().manual_seed(8)).to(DEV)
    torch.manual_seed(11)
    top, labels = TS.permute_frames_4way(clip)
    torch.manual_seed(11)
    want = torch.randint(0, 4, (4,))
    assert torch.equal(labels.cpu(), want) and top.shape == clip.shape
    for b in range(4):
        idx = TS._perm_index_4way(8, int(want[b])).to(DEV)
        assert torch.equal(top[b], clip[b][:, idx])


def test_driver_runs_an_epoch_and_the_checkpoint_loads(tmp_path):
    import yaml
    from conftest import ROOT
    from ssl_mae_amd.finetune import VideoClassifier, load_pretrained_ssl
    from ssl_mae_amd.utils import load_config
    cfg = load_config(os.path.join(ROOT, "configs", "ssl_train.yaml"))
    cfg["dataset"].update(clip_len=4, synthetic_steps=2, train_split=None)
    cfg["training"].update(log_interval=1)
    cfg["model"].update(temporal_layers=1)
    cfg["ssl_objectives"].update(top_start_epoch=1)
    path = tmp_path / "ssl.yaml"
    path.write_text(yaml.safe_dump(cfg))
    TS.main(["--config", str(path), "--epochs", "1", "--save_every", "1", "--batch_size", "2",
             "--save_dir", str(tmp_path / "out")])
    ck = tmp_path / "out" / "ssl_ep1.pth"
    state = torch.load(str(ck), map_location="cpu", weights_only=True)
    assert list(state) == ["epoch", "student", "ema", "opt"] and state["opt"]["step"] == 2
    assert all(bool(torch.isfinite(v).all()) for v in state["student"].values())
    moved = sum(not torch.equal(state["student"][k], state["ema"][k]) for k in state["student"]
                if k.endswith("weight"))
    assert moved > 100                                         # the student trained, the teacher trails it
    clf = VideoClassifier(5)
    assert load_pretrained_ssl(clf, str(ck))
    for k, v in clf.backbone.state_dict().items():
        assert torch.equal(v, state["student"]["encoder." + k]), k

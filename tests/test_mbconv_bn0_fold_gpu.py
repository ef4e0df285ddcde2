"""BN0's backward dx map folded into the MBConv expand conv's gradient GEMMs (csrc/mbfold.hip,
sm_dwconv_bn_bwd_dz, sm_linear_dx2; functions.BN0_FOLD).

The folded path never writes da1 = gamma rho (dz - k0 - xhat k1): with a1 = x W^T the map goes
into the weights of da1's two consumers,
    dX  = dz W' - x T + r0,                  W' = diag(omega) W, T = W^T diag(delta) W, r0 = c^T W
    dW += diag(omega) P - diag(delta) W G + c s^T,    P = dz^T x, G = x^T x, s = sum_m x.
Reference: fp32 torch autograd of conv2d(gelu(batch_norm(x W^T)), groups=mid) from the same bf16
inputs; bounds: the project's for the same quantities (test_kernels_gpu.py
test_dwconv_bn_bwd_vs_fp32, test_c2_bf16_gpu.py): dX 2e-2 (max-norm relative) against the
reference and against the two-pass path, dW_exp 1e-2 against the reference."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_mae_amd import _lib
    _lib.load()


def KK():
    from ssl_mae_amd import kernels
    return kernels


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _xbn(Cin, seed):
    """BatchNorm (mean, rstd, weight, bias) of a stored block input (the stem's folded BN2)."""
    return ((rnd(Cin, seed=seed, scale=0.3) + 0.1).to(DEV), (torch.rand(Cin, generator=torch.Generator().manual_seed(seed + 1)) + 0.5).to(DEV),
            (rnd(Cin, seed=seed + 2, scale=0.2) + 1.0).to(DEV), (rnd(Cin, seed=seed + 3, scale=0.2) + 0.3).to(DEV))


# ------------------------------------------------------------------ 1. kernel level
@pytest.mark.parametrize("Fr,H,Cin,mid,s,bnin", [(4, 19, 16, 64, 1, False), (4, 19, 16, 64, 2, False),
                                                 (4, 20, 16, 64, 2, False), (2, 16, 96, 384, 1, False),
                                                 (2, 14, 192, 768, 2, False), (2, 24, 32, 128, 1, True)])
def test_folded_expand_gradients_vs_fp32_and_two_pass(Fr, H, Cin, mid, s, bnin):
    """The folded sequence as MBConvFn.backward runs it (first pass without the dx pass, prep,
    P / G / s, combine, two-segment data gradient) against fp32 autograd and the two-pass path:
    ragged strips and M = 1444 (no multiple of an m-tile), the stride-2 odd / even sizes, the
    real channel widths (K segments 384 + 96, 768 + 192), and a BatchNorm-folded block input."""
    kk = KK()
    W_ = H
    Ho = (H - 1) // s + 1
    M = Fr * H * W_
    wexp = rnd(mid, Cin, seed=301, scale=1.5 / Cin ** 0.5).to(torch.bfloat16).to(DEV)
    if bnin:
        xs = (rnd(M, Cin, seed=300, scale=1.0) + 0.2).to(torch.bfloat16).to(DEV)
        xbn = _xbn(Cin, 310)
        x = kk.bn_apply(xs, *xbn, gelu=False)                       # bf16(BN(xs)), what every read forms
        a1 = kk.linear_bnin(xs, xbn + (False,), wexp)
        assert torch.equal(a1, kk.linear(x, wexp))
    else:
        xs, xbn = None, None
        x = (rnd(M, Cin, seed=300, scale=1.0) + 0.2).to(torch.bfloat16).to(DEV)
        a1 = kk.linear(x, wexp)
    g0 = (rnd(mid, seed=302, scale=0.2) + 1.0).to(DEV)
    b0 = rnd(mid, seed=303, scale=0.2).to(DEV)
    wdw = rnd(mid, 9, seed=304, scale=0.3).to(DEV)
    m0, r0 = kk.bn_stats(a1)
    act0 = (m0, r0, g0, b0, True)
    da2 = rnd(Fr * Ho * Ho, mid, dtype=torch.bfloat16, seed=305, scale=1e-2).to(DEV)

    # two-pass path (today's): da1 stored, plain GEMMs
    dw_o = torch.zeros(mid, 9, device=DEV)
    dg_o, db_o = torch.zeros(mid, device=DEV), torch.zeros(mid, device=DEV)
    da1 = kk.dwconv_bn_bwd(da2, a1, act0, wdw, dw_o, dg_o, db_o, Fr, H, W_, mid, stride=s)
    dX_o = kk.linear_dx(da1, wexp)
    dW_o = kk.linear_dw(da1, x, torch.zeros(mid, Cin, device=DEV))

    # folded path
    dw_f = torch.zeros(mid, 9, device=DEV)
    dg_f, db_f = torch.zeros(mid, device=DEV), torch.zeros(mid, device=DEV)
    dz, coef = kk.dwconv_bn_bwd_dz(da2, a1, act0, wdw, dw_f, dg_f, db_f, Fr, H, W_, mid, stride=s)
    wst, r0f, vec = kk.mbconv_fold_prep(coef, m0, r0, g0, wexp, xbn)
    P = torch.empty(mid, Cin, device=DEV)
    xin = xs if bnin else x
    if bnin:
        kk.linear_dw_se(dz, xs, xbn + (False,), None, 0, P, accumulate=False)
    else:
        kk.linear_dw(dz, x, P, accumulate=False)
    gram, xsum = torch.zeros(Cin, Cin, device=DEV), torch.zeros(Cin, device=DEV)
    kk.linear_dw_bias(xin, xin, gram, xsum)
    dW_f = kk.mbconv_fold_dw(vec, wexp, P, gram, xsum, M, torch.zeros(mid, Cin, device=DEV), xbn)
    dX_f = kk.linear_dx2(dz, xin, wst, bias=r0f)

    # fp32 autograd reference from the same bf16 inputs
    tx = x.float().clone().requires_grad_(True)
    tW = wexp.float().clone().requires_grad_(True)
    tg, tb, tw = g0.clone().requires_grad_(True), b0.clone().requires_grad_(True), wdw.clone().requires_grad_(True)
    t4 = (tx @ tW.t()).view(Fr, H, W_, mid).permute(0, 3, 1, 2)
    y = F.conv2d(F.gelu(F.batch_norm(t4, None, None, tg, tb, True, 0.0, 1e-5)), tw.view(mid, 1, 3, 3), None, s, 1, 1,
                 mid)
    y.backward(da2.float().view(Fr, Ho, Ho, mid).permute(0, 3, 1, 2))
    torch.cuda.synchronize()

    figs = {"dX/ref": rel_err(dX_f, tx.grad), "dX/old": rel_err(dX_f, dX_o), "dW/ref": rel_err(dW_f, tW.grad),
            "old dX/ref": rel_err(dX_o, tx.grad), "old dW/ref": rel_err(dW_o, tW.grad)}
    print("bn0 fold", (Fr, H, Cin, mid, s, bnin), {k: f"{v:.2e}" for k, v in figs.items()})
    assert figs["dX/ref"] < 2e-2 and figs["dX/old"] < 2e-2
    assert figs["dW/ref"] < 1e-2
    # same first-pass kernels, same inputs: bit for bit
    assert torch.equal(dw_f, dw_o) and torch.equal(dg_f, dg_o) and torch.equal(db_f, db_o)
    assert rel_err(dw_f, tw.grad) < 1e-2 and rel_err(dg_f, tg.grad) < 2e-2 and rel_err(db_f, tb.grad) < 2e-2
    # the stored dz is the two-pass path's before its dx pass: its dx map applied to (dz, coef)
    # gives that path's da1 (fp32 formula, one bf16 rounding; the kernel's fused multiply-adds
    # may move a value across one rounding boundary: at most one bf16 ulp, on few elements)
    wr = g0 * r0
    ref_da1 = (wr * (dz.float() - coef[0] - (a1.float() - m0) * r0 * coef[1])).to(torch.bfloat16)
    diff = (ref_da1.float() - da1.float()).abs()
    assert (diff <= 2.0 ** -7 * da1.float().abs() + 1e-30).all()
    assert (diff == 0).float().mean().item() > 0.99


@pytest.mark.parametrize("Cin", [16, 264])
def test_fold_dw_vs_torch_formula(Cin):
    """sm_mbconv_fold_dw with a BatchNorm-folded input against the fp64 torch formula, fp32 output
    within 1e-5 (max-norm relative, as the prep kernel's): Cin = 16 leaves 240 of the block's 256
    partial sums of a1 / a2 empty, Cin = 264 gives threads 0..7 two terms each."""
    kk = KK()
    mid, M = 8, 1000
    w = rnd(mid, Cin, seed=340, scale=1.5 / Cin ** 0.5).to(torch.bfloat16).to(DEV)
    vec = torch.stack([rnd(mid, seed=341, scale=0.2) + 1.0, rnd(mid, seed=342, scale=1e-3),
                       rnd(mid, seed=343, scale=1e-3)]).to(DEV)
    P = rnd(mid, Cin, seed=344).to(DEV)
    xs = rnd(M, Cin, seed=345).double() + 0.2
    G, s = (xs.t() @ xs).float().to(DEV), xs.sum(0).float().to(DEV)
    xbn = _xbn(Cin, 350)
    sink0 = rnd(mid, Cin, seed=346).to(DEV)
    got = kk.mbconv_fold_dw(vec, w, P, G, s, M, sink0.clone(), xbn)
    torch.cuda.synchronize()
    sc = (xbn[1] * xbn[2]).double()
    sh = xbn[3].double() - xbn[0].double() * sc
    Wd, om, dl, cc = w.double(), vec[0].double(), vec[1].double(), vec[2].double()
    wa = (w.float() * (xbn[1] * xbn[2])).double()                    # W sc, rounded to fp32 as the kernel stores it
    a1, a2 = wa @ s.double(), Wd @ sh
    sj = sc * s.double() + M * sh
    wg = sc * (wa @ G.double()) + a1[:, None] * sh + a2[:, None] * sj
    ref = sink0.double() + om[:, None] * P.double() + cc[:, None] * sj - dl[:, None] * wg
    err = rel_err(got, ref)
    print(f"fold_dw Cin={Cin}: err {err:.3e}")
    assert err < 1e-5


# ------------------------------------------------------------------ 2. prep kernel
@pytest.mark.parametrize("mid,Cin,bnin", [(64, 16, False), (384, 96, False), (64, 16, True), (384, 96, True)])
def test_fold_prep_vs_torch_formula(mid, Cin, bnin):
    """W', -T, r0, omega, delta, c against the fp64 torch formula.  bf16 outputs within one bf16
    ulp (2^-7 relative) plus, for -T, the fp32 summation's worst-case error mid 2^-24 sum_c |term|;
    fp32 outputs within 1e-5 (max-norm relative)."""
    kk = KK()
    w = rnd(mid, Cin, seed=320, scale=1.5 / Cin ** 0.5).to(torch.bfloat16).to(DEV)
    coef = torch.stack([rnd(mid, seed=321, scale=1e-3), rnd(mid, seed=322, scale=1e-3)]).to(DEV)
    mean = (rnd(mid, seed=323, scale=0.5) + 0.2).to(DEV)
    rstd = (torch.rand(mid, generator=torch.Generator().manual_seed(324)) + 0.5).to(DEV)
    gamma = (rnd(mid, seed=325, scale=0.2) + 1.0).to(DEV)
    xbn = _xbn(Cin, 330) if bnin else None
    wst, r0, vec = kk.mbconv_fold_prep(coef, mean, rstd, gamma, w, xbn)
    torch.cuda.synchronize()
    Wd, k0, k1, mu, rho, ga = (t.double() for t in (w, coef[0], coef[1], mean, rstd, gamma))
    om = ga * rho
    dl = om * rho * k1
    cc = om * (rho * k1 * mu - k0)
    T = Wd.t() @ (dl[:, None] * Wd)
    Tabs = Wd.abs().t() @ (dl.abs()[:, None] * Wd.abs())
    r0_ref = cc @ Wd
    if bnin:
        sc = (xbn[1] * xbn[2]).double()
        sh = xbn[3].double() - xbn[0].double() * sc
        r0_ref = r0_ref - sh @ T
        T, Tabs = sc[:, None] * T, sc.abs()[:, None] * Tabs
    for got, ref, nm in ((vec[0], om, "omega"), (vec[1], dl, "delta"), (vec[2], cc, "c"), (r0, r0_ref, "r0")):
        assert rel_err(got, ref) < 1e-5, nm
    wp_ref = om[:, None] * Wd
    assert ((wst[:mid].double() - wp_ref).abs() <= 2.0 ** -7 * wp_ref.abs()).all()
    assert ((wst[mid:].double() + T).abs() <= 2.0 ** -7 * T.abs() + mid * 2.0 ** -24 * Tabs).all()


# ------------------------------------------------------------------ 3. two-segment GEMM
@pytest.mark.parametrize("M", [256 * 3 + 77, 100])
@pytest.mark.parametrize("K1,K2", [(64, 16), (384, 96), (64, 96), (384, 16)])
@pytest.mark.parametrize("extras", [False, True])
def test_linear_dx2_bit_identical_to_concatenation(M, K1, K2, extras):
    """A = [dz | x] from two buffers against the same kernel on a materialised concatenation
    (both segments views of one [M][K1 + K2] buffer): bit-identical, with and without bias and
    residual; M = 845 (256-row tiles, ragged last one) and M = 100 (the 128-row tile); the
    second segment ends inside a K-step (K2 = 16, 96)."""
    kk = KK()
    N = K2
    dz = rnd(M, K1, dtype=torch.bfloat16, seed=340, scale=1e-2).to(DEV)
    x = (rnd(M, K2, seed=341) + 0.2).to(torch.bfloat16).to(DEV)
    w = rnd(K1 + K2, N, dtype=torch.bfloat16, seed=342, scale=0.2).to(DEV)
    bias = rnd(N, seed=343, scale=1e-2).to(DEV) if extras else None
    res = rnd(M, N, dtype=torch.bfloat16, seed=344, scale=1e-2).to(DEV) if extras else None
    got = kk.linear_dx2(dz, x, w, bias=bias, residual=res)
    cat = torch.cat([dz, x], 1).contiguous()
    same = kk.linear_dx2(cat[:, :K1], cat[:, K1:], w, bias=bias, residual=res)
    torch.cuda.synchronize()
    assert torch.equal(got, same)
    ref = cat.float() @ w.float()
    if extras:
        ref = ref + bias + res.float()
    assert rel_err(got, ref) < 2e-2


def test_linear_dx2_refuses_a_first_segment_off_the_k_step():
    """K1 % 64 != 0: a K-step would straddle the two buffers -- status -2 before any launch."""
    from ssl_mae_amd import _lib
    lib = _lib.load()
    M, K1, K2 = 128, 96, 24
    dz = torch.zeros(M, K1, dtype=torch.bfloat16, device=DEV)
    x = torch.zeros(M, K2, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(K1 + K2, K2, dtype=torch.bfloat16, device=DEV)
    out = torch.full((M, K2), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib.sm_linear_dx2(M, K2, K1, K2, _lib.ptr(dz), K1, _lib.ptr(x), K2, _lib.ptr(w), None, None, _lib.ptr(out),
                           _lib.stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((out == 7.0).all())
    with pytest.raises(_lib.KernelError):
        KK().linear_dx2(dz, x, w)


# ------------------------------------------------------------------ 4 / 5. MBConvFn level
PARAMS = ("w_exp", "bn0.w", "bn0.b", "w_dw", "bn2.w", "bn2.b", "se.fc0", "se.fc2", "w_proj", "bn5.w", "bn5.b")


def _mbconv(Cin, Cout, stride, drop_path):
    from ssl_mae_amd import tiny_vit as TV
    torch.manual_seed(7)
    m = TV.MBConv(Cin, Cout, 4, stride, drop_path)
    with torch.no_grad():
        for i in (0, 2, 5):
            m.conv[i].bn.weight.copy_(torch.rand_like(m.conv[i].bn.weight) * 0.4 + 0.8)
            m.conv[i].bn.bias.copy_(torch.randn_like(m.conv[i].bn.bias) * 0.2)
    return m.train()


def _run_mbconv(proto, x, dout, fold, resident, x_bn):
    """One forward + backward of a fresh copy of `proto` with functions.BN0_FOLD = fold."""
    from ssl_mae_amd import functions as Fn
    from ssl_mae_amd.optim import FlatParams
    m = copy.deepcopy(proto).to(DEV)
    flat = FlatParams(list(m.named_parameters()), DEV)
    flat.begin_forward(True)
    xin = x.clone().requires_grad_(True)
    prev = Fn.BN0_FOLD
    Fn.BN0_FOLD = fold
    try:
        out = m.run(xin, Fn.Mode(True, seed_base=123), resident=resident, x_bn=x_bn)
        out.backward(dout)
    finally:
        Fn.BN0_FOLD = prev
    torch.cuda.synchronize()
    c = m.conv
    ps = (c[0].c.weight, c[0].bn.weight, c[0].bn.bias, c[2].c.weight, c[2].bn.weight, c[2].bn.bias, c[4].fc[0].weight,
          c[4].fc[2].weight, c[5].c.weight, c[5].bn.weight, c[5].bn.bias)
    return out.detach().clone(), xin.grad.clone(), {n: p._sm_grad.detach().clone() for n, p in zip(PARAMS, ps)}


def _mbconv_case(Cin, stride, resident, bnin, drop_path=0.0):
    Fr, H = 4, 20
    Cout = Cin if stride == 1 else 2 * Cin
    Ho = (H - 1) // stride + 1
    proto = _mbconv(Cin, Cout, stride, drop_path)
    x = (rnd(Fr, H, H, Cin, seed=360) + 0.2).to(torch.bfloat16).to(DEV)
    dout = rnd(Fr, Ho, Ho, Cout, dtype=torch.bfloat16, seed=361, scale=1e-2).to(DEV)
    x_bn = _xbn(Cin, 370) if bnin else None
    on = _run_mbconv(proto, x, dout, True, resident, x_bn)
    off = _run_mbconv(proto, x, dout, False, resident, x_bn)
    return on, off


@pytest.mark.parametrize("stride,resident,bnin", [(1, False, False), (1, False, True), (1, True, False),
                                                  (1, "lite", True), (2, False, False), (2, False, True),
                                                  (2, "lite", False)])
def test_mbconvfn_fold_on_vs_off(stride, resident, bnin):
    """MBConvFn with the switch on against off in one process, mid = 64: stride 1 with the
    residual and a DropPath row scale, stride 2 without the residual, with and without a
    BatchNorm-folded input, a1 resident / recomputed (recompute_a1) / a1 and a2 recomputed
    (recompute_a2).  dx and the expand weight gradient within the kernel-level bounds; every
    gradient the fold does not touch bit-identical."""
    (out_on, dx_on, g_on), (out_off, dx_off, g_off) = _mbconv_case(16, stride, resident, bnin,
                                                                   drop_path=0.25 if stride == 1 else 0.0)
    assert torch.equal(out_on, out_off)
    figs = {"dx": rel_err(dx_on, dx_off), "w_exp": rel_err(g_on["w_exp"], g_off["w_exp"])}
    print("mbconv fold on/off", (stride, resident, bnin), {k: f"{v:.2e}" for k, v in figs.items()})
    assert dx_off.abs().max() > 0 and g_off["w_exp"].abs().max() > 0
    assert figs["dx"] < 2e-2 and figs["w_exp"] < 1e-2
    for n in PARAMS[1:]:
        assert torch.equal(g_on[n], g_off[n]), n


def test_mbconvfn_ineligible_width_takes_the_two_pass_path():
    """mid = 96 (96 % 64 != 0): the switch changes nothing, bit for bit."""
    (out_on, dx_on, g_on), (out_off, dx_off, g_off) = _mbconv_case(24, 1, False, False)
    assert torch.equal(out_on, out_off) and torch.equal(dx_on, dx_off)
    for n in PARAMS:
        assert torch.equal(g_on[n], g_off[n]), n

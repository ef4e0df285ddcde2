"""The reduction terms of the normalisation backwards on the GPU: sm_layernorm_bwd(_branch),
sm_bn_bwd, sm_dwconv_bn_bwd(_dz) and sm_se_bn_bwd against the fp64 references of
tests/norm_grad_cases.py, with gradients whose per-row / per-channel means are as large as the
gradient (null-space gradients a + b xhat, the same plus a quarter of noise, and their images
through the depthwise conv's transpose and the SE backward).  Errors are err_S, relative to the
size dx would have without its correction terms; the tolerances are the table of
tests/norm_grad_cases.py, and tests/test_norm_grad_cases_cpu.py shows for every case here that a
10 % (null space: 1 %) error in either term moves the reference by twice (four times) as much."""
import pytest
import torch

import norm_grad_cases as N

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ssl_mae_amd import _lib as L
    L.load()


def KK():
    from ssl_mae_amd import kernels
    return kernels


def dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------ LayerNorm
def _ln_run(p, branch=False):
    kk = KK()
    x, gamma, dy = dev(p["x"]), dev(p["gamma"]), dev(p["dy"])
    _, mean, rstd = kk.layernorm(x, gamma, dev(p["beta"]), out_dtype=p["dy"].dtype)
    dg, db = dev(p["dgamma0"]).clone(), dev(p["dbeta0"]).clone()
    if branch:
        dx, dxb = kk.layernorm_bwd_branch(dy, x, mean, rstd, gamma, dg, db, dres=dev(p["dres"]))
        return dx, dg, db, dxb
    return kk.layernorm_bwd(dy, x, mean, rstd, gamma, dg, db, dres=dev(p["dres"])), dg, db


@pytest.mark.parametrize("case", N.LN_CASES, ids=N.ids(N.LN_CASES))
def test_layernorm_bwd_terms(case):
    """C = 4 / 100 / 576 / 1024: the generic kernel's first chunk alone, a partly filled pass, three
    chunks and all four; 192 / 384: the 16- and 32-lane forms.  M = 1, 15 (one short of the 16 rows
    in flight), 777 (13 blocks, the last with 9 rows).  With and without dres, into non-zero sinks."""
    p = N.ln_build(case)
    ref = N.ln_ref(p)
    dx, dg, db = _ln_run(p)
    e = N.err_S(dx, ref.dx, ref.S)
    eg = N.rel_max(dg.cpu().double() - p["dgamma0"].double(), ref.dgamma)
    eb = N.rel_max(db.cpu().double() - p["dbeta0"].double(), ref.dbeta)
    print("%s: err_S %.3e (tol %.0e) dgamma %.2e dbeta %.2e" % (case.id, e, N.tol_of(case), eg, eb))
    assert dx.dtype == case.xd
    assert e < N.tol_of(case)
    assert eg < N.TOL_PARAM and eb < N.TOL_PARAM


@pytest.mark.parametrize("case", N.LN_BRANCH_CASES, ids=N.ids(N.LN_BRANCH_CASES))
def test_layernorm_bwd_branch_terms(case):
    """sm_layernorm_bwd_branch with a null-space gradient: dx and the sinks bit-identical to
    sm_layernorm_bwd, the bf16 copy (p = 0, no row scale) the cast of that dx."""
    kk = KK()
    p = N.ln_build(case)
    dx1, dg1, db1 = _ln_run(p)
    dx2, dg2, db2, dxb = _ln_run(p, branch=True)
    assert torch.equal(dx1, dx2) and torch.equal(dg1, dg2) and torch.equal(db1, db2)
    want = dx1 if case.xd == torch.bfloat16 else kk.cast(dx1, torch.bfloat16)
    assert dxb.dtype == torch.bfloat16 and torch.equal(dxb, want)


# ------------------------------------------------------------------ BatchNorm
@pytest.mark.parametrize("case", N.BN_CASES, ids=N.ids(N.BN_CASES))
def test_bn_bwd_terms(case):
    """C <= 128: the single-row tail of bn_bwd_dx_kernel alone; C >= 384: its two-row loop; C = 1536:
    two channel slices through one coef workspace.  M = 5, 527, 3000.  The rpg cases: a DropPath-like
    row scale (zeros and 1 / (1 - p)) per row and per ragged group of 37 rows."""
    kk = KK()
    p = N.bn_build(case)
    ref = N.bn_ref(p)
    x, w, b = dev(p["x"]), dev(p["w"]), dev(p["b"])
    mean, rstd = kk.bn_stats(x)
    dw, db = dev(p["dw0"]).clone(), dev(p["db0"]).clone()
    dx = kk.bn_bwd(dev(p["dy"]), x, mean, rstd, w, b, p["gelu"], dw, db, row_scale=dev(p["row_scale"]),
                   rows_per_group=p["rpg"])
    e = N.err_S(dx, ref.dx, ref.S)
    ew = N.rel_max(dw.cpu().double() - p["dw0"].double(), ref.dw)
    eb = N.rel_max(db.cpu().double() - p["db0"].double(), ref.db)
    print("%s: err_S %.3e (tol %.0e) dw %.2e db %.2e" % (case.id, e, N.tol_of(case), ew, eb))
    assert dx.dtype == case.dt
    assert e < N.tol_of(case)
    assert ew < N.TOL_PARAM and eb < N.TOL_PARAM


# ------------------------------------------------------------------ fused depthwise + BN0
def _chan_err(got, ref, scale):
    """max over channels of |got - ref| / scale, scale per channel."""
    return ((got.detach().double().cpu() - ref.double()).abs() / scale).max().item()


def _dw_run(p, dz_form):
    kk = KK()
    c = p["case"]
    x, w, b = dev(p["x"]), dev(p["w"]), dev(p["b"])
    mean, rstd = kk.bn_stats(x)
    act = (mean, rstd, w, b, True)
    dwdw = torch.zeros(c.C, 9, device=DEV)
    dg, db = dev(p["dg0"]).clone(), dev(p["db0"]).clone()
    fn = kk.dwconv_bn_bwd_dz if dz_form else kk.dwconv_bn_bwd
    out = fn(dev(p["dy"]), x, act, dev(p["wdw"]), dwdw, dg, db, c.Fr, c.H, c.H, c.C, stride=c.s)
    return out, dwdw, dg.cpu().double() - p["dg0"].double(), db.cpu().double() - p["db0"].double()


def _dw_sums_check(case, ref, dwdw, dg, db):
    M = ref.dz.shape[0]
    zmax = ref.dz.abs().amax(0)
    eg, eb = _chan_err(dg, ref.dgamma, M * zmax), _chan_err(db, ref.dbeta, M * zmax)
    ew = N.rel_max(dwdw, ref.dwdw)
    print("%s: dgamma %.2e dbeta %.2e (tol %.1e, per channel) dw %.2e" % (case.id, eg, eb, N.TOL_COEF, ew))
    assert eg < N.TOL_COEF and eb < N.TOL_COEF
    assert ew < N.TOL_DWDW


@pytest.mark.parametrize("case", N.DW_CASES, ids=N.ids(N.DW_CASES))
def test_dwconv_bn_bwd_terms(case):
    """sm_dwconv_bn_bwd against fp64 autograd of conv2d(GELU(batch_norm(x))) from the same bf16
    inputs, BN0's k0 and k1 as large as the gradient that reaches it."""
    p = N.dw_build(case)
    ref = N.dwconv_bn_ref(p)
    da1, dwdw, dg, db = _dw_run(p, False)
    e = N.err_S(da1, ref.dx, ref.S)
    print("%s: err_S %.3e (tol %.0e)" % (case.id, e, N.tol_of(case)))
    assert e < N.tol_of(case)
    _dw_sums_check(case, ref, dwdw, dg, db)


@pytest.mark.parametrize("case", N.DW_CASES, ids=N.ids(N.DW_CASES))
def test_dwconv_bn_bwd_dz_terms(case):
    """sm_dwconv_bn_bwd_dz: dz, and coef = mean(dz), mean(dz xhat) per channel against the
    reference's own, each channel relative to its own max |dz|."""
    p = N.dw_build(case)
    ref = N.dwconv_bn_ref(p)
    (dz, coef), dwdw, dg, db = _dw_run(p, True)
    zmax = ref.dz.abs().amax(0)
    ez = N.rel_max(dz, ref.dz)
    e0, e1 = _chan_err(coef[0], ref.k0, zmax), _chan_err(coef[1], ref.k1, zmax)
    print("%s: dz %.2e coef0 %.2e coef1 %.2e (tol %.1e, per channel)" % (case.id, ez, e0, e1, N.TOL_COEF))
    assert dz.dtype == torch.bfloat16 and ez < N.TOL_DZ
    assert e0 < N.TOL_COEF and e1 < N.TOL_COEF
    _dw_sums_check(case, ref, dwdw, dg, db)


# ------------------------------------------------------------------ fused SE + BN2
@pytest.mark.parametrize("case", N.SE_CASES, ids=N.ids(N.SE_CASES))
def test_se_bn_bwd_terms(case):
    """sm_se_bn_bwd against fp64 autograd of SE(GELU(batch_norm(x))) from the same bf16 inputs.  The
    kernel's SE input is h2 at its stored precision, bf16: the gate gradient's sums over dy h2 (dz2,
    and dz1 behind it) carry that rounding, 2^-9 per summand, and get the same bound as the
    per-channel sums."""
    kk = KK()
    p = N.se_build(case)
    ref = N.se_bn_ref(p)
    Fn, HW, C = case.Fn, case.HW, case.C
    x, w1, w2 = dev(p["x"]), dev(p["w1"]), dev(p["w2"])
    mean, rstd = kk.bn_stats(x)
    act = (mean, rstd, dev(p["w"]), dev(p["b"]), True)
    _, _, h1, s = kk.se_fwd(x, Fn, HW, C, w1, w2, act=act, want_y=False)
    dw, db = dev(p["dw0"]).clone(), dev(p["db0"]).clone()
    dx, dz2, dz1 = kk.se_bn_bwd(dev(p["dy"]), x, Fn, HW, C, w1, w2, s, h1, act, dw, db)
    e = N.err_S(dx, ref.dx, ref.S)
    M = Fn * HW
    ew = _chan_err(dw.cpu().double() - p["dw0"].double(), ref.dw, M * ref.dz.abs().amax(0))
    eb = _chan_err(db.cpu().double() - p["db0"].double(), ref.db, M * ref.dz.abs().amax(0))
    e2, e1 = N.rel_max(dz2, ref.dz2), N.rel_max(dz1, ref.dz1)
    print("%s: err_S %.3e (tol %.0e) dw %.2e db %.2e (tol %.1e, per channel) dz2 %.2e dz1 %.2e" %
          (case.id, e, N.tol_of(case), ew, eb, N.TOL_COEF, e2, e1))
    assert e < N.tol_of(case)
    assert ew < N.TOL_COEF and eb < N.TOL_COEF
    assert e2 < N.TOL_COEF and e1 < N.TOL_COEF

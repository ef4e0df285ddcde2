"""The inputs of tests/test_norm_grad_terms_gpu.py, judged without a GPU: for every case of that
file (same builder, shape, dtype and seed, from tests/norm_grad_cases.py)

  * sensitivity: the fp64 reference with either reduction term scaled by 0.9 moves by at least twice
    the case's GPU tolerance in err_S (null-space cases: scaled by 0.99, four times), so an error of
    that size in the kernel's term cannot pass;
  * headroom (ln_bwd, bn_bwd): the same formula evaluated plainly in fp32, inputs and the stored dx
    rounded to the kernel's dtypes, stays below half the tolerance (a sixteenth for null-space cases,
    whose table entries are 16 x this figure rounded up to a power of ten);
  * the table: null-space entries are powers of ten, at most 1e-3, and not a decade looser than
    16 x the worst figure measured here.

Also the references themselves against torch autograd in fp64."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import norm_grad_cases as N


def _sens(case, p, ref, base, knobs):
    """err_S of the reference with each term scaled (0.9; null space 0.99), and the least the case's
    tolerance demands of it (twice; null space four times)."""
    scale, factor = (0.99, 4.0) if case.kind == "null" else (0.9, 2.0)
    return [N.err_S(ref(p, **{k: scale}).dx, base.dx, base.S) for k in knobs], factor * N.tol_of(case)


@functools.lru_cache(maxsize=None)
def _figures(case):
    """(err_S of term 1 scaled, of term 2 scaled, demanded minimum, fp32 evaluation's err_S or None)."""
    fam = case.family
    build, ref, knobs = {"ln": (N.ln_build, N.ln_ref, ("s1_scale", "s2_scale")),
                         "bn": (N.bn_build, N.bn_ref, ("k0_scale", "k1_scale")),
                         "dw": (N.dw_build, N.dwconv_bn_ref, ("k0_scale", "k1_scale")),
                         "se": (N.se_build, N.se_bn_ref, ("k0_scale", "k1_scale"))}[fam]
    p = build(case)
    base = ref(p)
    (e1, e2), need = _sens(case, p, ref, base, knobs)
    emu = None
    if fam in ("ln", "bn"):
        stored = p["x"].dtype if fam == "ln" else p["dy"].dtype
        emu = N.err_S(ref(p, dtype=torch.float32).dx.to(stored), base.dx, base.S)
    return e1, e2, need, emu


def _check(case):
    e1, e2, need, emu = _figures(case)
    tol = N.tol_of(case)
    print("%s tol %.0e: term1 %.3e term2 %.3e (need %.1e) fp32 %s" %
          (case.id, tol, e1, e2, need, "-" if emu is None else "%.3e" % emu))
    assert e1 >= need and e2 >= need, (case.id, e1, e2, need)
    if emu is not None:
        assert emu < tol / (16.0 if case.kind == "null" else 2.0), (case.id, emu, tol)


@pytest.mark.parametrize("case", N.LN_CASES, ids=N.ids(N.LN_CASES))
def test_ln_case(case):
    _check(case)


@pytest.mark.parametrize("case", N.BN_CASES, ids=N.ids(N.BN_CASES))
def test_bn_case(case):
    _check(case)


@pytest.mark.parametrize("case", N.DW_CASES, ids=N.ids(N.DW_CASES))
def test_dw_case(case):
    _check(case)


@pytest.mark.parametrize("case", N.SE_CASES, ids=N.ids(N.SE_CASES))
def test_se_case(case):
    _check(case)


def test_tolerance_table():
    """Null-space entries: a power of ten <= 1e-3, and the power of ten just above 16 x the worst
    fp32-evaluation figure of the row's cases."""
    worst = {}
    for case in N.LN_CASES + N.BN_CASES:
        if case.kind == "null":
            key = (case.family, "null", case.tol_dtype)
            worst[key] = max(worst.get(key, 0.0), _figures(case)[3])
    assert set(worst) == {k for k in N.TOL if k[1] == "null"}
    for key, m in sorted(worst.items()):
        tol = N.TOL[key]
        print(key, "measured %.2e, x16 = %.2e, table %.0e" % (m, 16 * m, tol))
        assert tol <= 1e-3
        assert abs(math.log10(tol) - round(math.log10(tol))) < 1e-9
        assert 16 * m <= tol < 160 * m, (key, m, tol)
    assert N.TOL[("ln", "mixed", "f32")] == N.TOL[("bn", "mixed", "f32")] == 1e-4
    assert N.TOL[("ln", "mixed", "bf16")] == N.TOL[("bn", "mixed", "bf16")] == N.TOL[("se", "fused", "bf16")] == 2e-2
    assert N.TOL[("dw", "fused", "bf16")] == 3e-2


def test_case_lists_cover_the_shapes():
    ln = {(c.C, c.M, c.xd, c.yd, c.kind, c.dres) for c in N.LN_CASES}
    assert len(ln) == len(N.LN_CASES) == 6 * 3 * 3 * 2 * 2
    assert {c.C for c in N.LN_CASES} == {4, 100, 192, 384, 576, 1024} and {c.M for c in N.LN_CASES} == {1, 15, 777}
    assert {c.C for c in N.BN_CASES} == {8, 48, 96, 384, 768, 1536} and {c.M for c in N.BN_CASES} == {5, 527, 3000}
    assert {c.rpg for c in N.BN_CASES} == {0, 1, 37}
    # the GELU with ordinary parameters at every shape in fp32, the row-scale shapes included
    plain = {(c.C, c.M, c.rpg) for c in N.BN_CASES if c.act == "plain" and c.dt == N.F32 and c.kind == "mixed"}
    assert plain == {(C, M, 0) for C, M in N.BN_SHAPES} | {(C, M, r) for C, M in N.BN_RS_SHAPES for r in (1, 37)}
    for act in ("none", "neutral"):
        for dt in (N.F32, N.BF16):
            assert {(c.C, c.M) for c in N.BN_CASES if c.act == act and c.dt == dt and not c.rpg} == set(N.BN_SHAPES)
    assert len({c.id for c in N.LN_CASES + N.BN_CASES}) == len(N.LN_CASES) + len(N.BN_CASES)
    assert len({c.seed for c in N.LN_CASES + N.BN_CASES + N.DW_CASES + N.SE_CASES}) == \
        len(N.LN_CASES) + len(N.BN_CASES) + len(N.DW_CASES) + len(N.SE_CASES)
    assert N.LN_BRANCH_CASES and all(c in N.LN_CASES for c in N.LN_BRANCH_CASES)


def test_builders_are_deterministic_and_as_described():
    p, q = N.bn_build(N.BN_CASES[5]), N.bn_build(N.BN_CASES[5])
    assert torch.equal(p["dy"], q["dy"]) and torch.equal(p["x"], q["x"])
    p = N.ln_build(N.LN_CASES[40])
    g = p["gamma"]
    assert (g > 0).any() and (g < 0).any() and g.abs().min() >= 0.5 and g.abs().max() <= 1.5
    w, b = N.bn_params(torch.Generator().manual_seed(1), 64, "neutral")
    assert (w > 0).any() and (w < 0).any() and w.abs().min() >= 0.1 and w.abs().max() <= 0.2
    z = torch.linspace(-5, 5, 1001, dtype=torch.float64)[:, None] * w.double() + b.double()
    assert (N.gelu_grad(z) - 1).abs().max() < 1e-9            # the neutralised GELU, |xhat| <= 5
    rs = N.droppath_like(torch.Generator().manual_seed(2), 15)
    vals = set(rs.tolist())
    assert len(vals) == 2 and 0.0 in vals and abs(max(vals) - 1 / 0.9) < 1e-6
    d = N.dw_build(N.DW_CASES[0])
    assert torch.equal(d["dy"].float().to(torch.bfloat16), d["dy"])
    # the per-channel constant of the fused gradients is a bf16 number
    a, _ = N._bf16_exact_coeffs(torch.Generator().manual_seed(3), torch.ones(32), torch.rand(32).double() + 0.5)
    assert torch.equal(a.to(torch.bfloat16).double(), a)


def test_null_space_is_null():
    """In fp64, from unrounded gradients, the dx of a + b xhat is zero but for eps: mean(xhat^2) is
    var / (var + eps), which leaves b xhat eps / (var + eps), about 1e-5 / 4 of S here."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(50, 24, generator=g).double() * 2 + 0.5
    _, _, xhat = N._bn_stats(x)
    a, b = N._unit_coeffs(g, xhat.abs().amax(0))
    w = torch.randn(24, generator=g).double()
    r = N.bn_bwd_ref(a + b * xhat, x, w, torch.zeros(24), False)
    assert r.dx.abs().max() / r.S < 1e-5
    xr = x.t().contiguous()
    mean = xr.mean(1, keepdim=True)
    xh = (xr - mean) * ((xr - mean).square().mean(1, keepdim=True) + N.EPS).rsqrt()
    a, b = N._unit_coeffs(g, xh.abs().amax(1))
    gamma = (N._signs(g, 50) * (0.5 + torch.rand(50, generator=g))).double()
    r = N.ln_bwd_ref((a[:, None] + b[:, None] * xh) / gamma, xr, gamma)
    assert r.dx.abs().max() / r.S < 1e-5


# ------------------------------------------------------------------ the references against autograd
def test_ln_ref_matches_autograd():
    p = N.ln_build(N.LnCase(100, 15, N.F32, N.F32, "mixed", True, 11))
    x = p["x"].double().requires_grad_(True)
    gm, bt = p["gamma"].double().requires_grad_(True), p["beta"].double().requires_grad_(True)
    F.layer_norm(x, (100,), gm, bt, N.EPS).backward(p["dy"].double())
    r = N.ln_ref(p)
    assert N.rel_max(r.dx, x.grad + p["dres"].double()) < 1e-12
    assert N.rel_max(r.dgamma, gm.grad) < 1e-12 and N.rel_max(r.dbeta, bt.grad) < 1e-12


@pytest.mark.parametrize("act,rpg", [("none", 0), ("plain", 0), ("neutral", 7)])
def test_bn_ref_matches_autograd(act, rpg):
    p = N.bn_build(N.BnCase(24, 50, N.F32, "mixed", act, rpg, 12))
    x = p["x"].double().requires_grad_(True)
    w, b = p["w"].double().requires_grad_(True), p["b"].double().requires_grad_(True)
    y = F.batch_norm(x, None, None, w, b, True, 0.0, N.EPS)
    if p["gelu"]:
        y = F.gelu(y)
    dy = p["dy"].double()
    if rpg:
        dy = dy * p["row_scale"].double()[torch.arange(50) // rpg][:, None]
    y.backward(dy)
    r = N.bn_ref(p)
    assert N.rel_max(r.dx, x.grad) < 1e-11
    assert N.rel_max(r.dw, w.grad) < 1e-11 and N.rel_max(r.db, b.grad) < 1e-11
    assert N.rel_max(r.k0 * 50, r.db) < 1e-14 and N.rel_max(r.k1 * 50, r.dw) < 1e-14


def test_fused_refs_match_full_autograd():
    """dz by autograd + BatchNorm's closed-form dx map == autograd through the statistics."""
    for build, ref, case in ((N.dw_build, N.dwconv_bn_ref, N.DW_CASES[1]), (N.se_build, N.se_bn_ref, N.SE_CASES[1])):
        p = build(case)
        assert N.rel_max(ref(p).dx, ref(p, full_autograd=True)) < 1e-11


@pytest.mark.parametrize("case", N.DW_CASES + N.SE_CASES, ids=N.ids(N.DW_CASES + N.SE_CASES))
def test_per_channel_bound_is_sensitive(case):
    """TOL_COEF (the fused kernels' coef, dgamma and dbeta, per channel, of the channel's max |dz|)
    comes from the rounding of bf16, not from a measurement.  What it lets through: a relative error r
    in a channel's k0 (k1) shows there as r |k0| / max |dz|.  Where k0 leads (the even channels) max |dz|
    is little more than |k0|, so r above 2^-8 (1 + the minor share) shows: 1 % must, in the median such
    channel.  Where k1 leads (the odd ones) max |dz| is about |k1| max |xhat|, 2.5 to 3 times |k1|: 2 %
    must.  (dx, at 2e-2 or 3e-2 of S, sees 10 %: test_dw_case, test_se_case.)"""
    build, ref = (N.dw_build, N.dwconv_bn_ref) if case.family == "dw" else (N.se_build, N.se_bn_ref)
    r = ref(build(case))
    zmax = r.dz.abs().amax(0)
    even = torch.arange(case.C) % 2 == 0
    for name, k, lead, must in (("k0", r.k0, even, 1e-2), ("k1", r.k1, ~even, 2e-2)):
        least = N.TOL_COEF * zmax / k.abs()          # the least relative error the bound catches, per channel
        print("%s %s: least relative error caught: %.2e in the best channel, %.2e in the median leading one"
              % (case.id, name, least.min(), least[lead].median()))
        assert least[lead].median() < must

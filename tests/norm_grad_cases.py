"""Inputs, fp64 references and tolerances for the normalisation backward tests
(tests/test_norm_grad_cases_cpu.py, tests/test_norm_grad_terms_gpu.py).  torch CPU code only.

Both norm backwards subtract two reduction terms from the incoming gradient,
    LayerNorm:  dx = rstd (gy - s1 - xhat s2),      gy = gamma dy, s1 = mean_row(gy), s2 = mean_row(gy xhat)
    BatchNorm:  dx = w rstd (g - k0 - xhat k1),     g = dy row_scale GELU', k0 = mean_ch(g), k1 = mean_ch(g xhat)
and with an i.i.d. gradient the terms are 1 / sqrt(n) of the gradient: dropping one outright stays
inside a bf16 tolerance.  The gradients built here are a + b xhat (a, b constant along the reduced
axis: the null space of the dx map, the correct output is rounding residue) with or without a
quarter of i.i.d. noise, so that the terms are as large as the gradient itself.

Every error is err_S: max |got - ref| / S, S = max |w rstd g| (max |rstd gamma dy| for LayerNorm),
the size dx would have without its correction terms; never the output's own maximum, which is
near zero here.

The units of a case (rows for LayerNorm, channels for BatchNorm) alternate between a-heavy and
b-heavy ones (the other coefficient a quarter as large) and b is divided by the unit's max |xhat|.
|a| and max |b xhat| of one unit add up in S, so with both at full size in every unit neither term
could pass half of S, and a 10 % error in one term could not reach twice a 2e-2 tolerance."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

F32, BF16 = torch.float32, torch.bfloat16
F64 = torch.float64
EPS = 1e-5
_NAME = {F32: "f32", BF16: "bf16"}

# ------------------------------------------------------------------ tolerances (err_S)
# Null-space cases: 16 x the worst error of the fp32 evaluation against the fp64 reference over the
# cases of that row (test_norm_grad_cases_cpu.py::test_tolerance_table prints and checks it, `measured` below),
# rounded up to a power of ten, never above 1e-3.  Mixed and fused cases: the project's tolerances,
# 1e-4 (fp32), 2e-2 (bf16), 3e-2 (the depthwise kernel's da1 behind two bf16-stored gradients).
# Key: (family, kind, dtype of the stored dx).
TOL = {
    ("ln", "null", "f32"): 1e-5,     # measured 4.52e-7 (x 16 = 7.2e-6), fp32 x with fp32 or bf16 dy
    ("ln", "null", "bf16"): 1e-3,    # measured 1.97e-5 (x 16 = 3.2e-4): the bf16 rounding of the stored residue
    ("ln", "mixed", "f32"): 1e-4,    # fp32 x and dx; dy fp32 or bf16 (the reference starts from the same rounded dy)
    ("ln", "mixed", "bf16"): 2e-2,   # bf16 x, dres and dx
    ("bn", "null", "f32"): 1e-4,     # measured 7.53e-7 (x 16 = 1.2e-5)
    ("bn", "null", "bf16"): 1e-3,    # measured 1.26e-5 (x 16 = 2.0e-4): the bf16 rounding of the stored residue
    ("bn", "mixed", "f32"): 1e-4,
    ("bn", "mixed", "bf16"): 2e-2,
    ("dw", "fused", "bf16"): 3e-2,
    ("se", "fused", "bf16"): 2e-2,
}
# dgamma / dbeta, dw / db: fp32 (fp64 for BatchNorm) sums of the same rounded inputs, of their maximum
TOL_PARAM = 1e-4
# The fused kernels' per-channel sums (coef = mean(dz), mean(dz xhat); dgamma, dbeta = M coef), per
# channel and relative to that channel's max |dz|.  The gradient and x are the reference's bf16 values,
# so each summand is within one bf16 rounding of dz, 2^-9 |dz|, of the reference's, whether the kernel
# sums dz before or after it stores it; the mean of M such errors is below 2^-9 max |dz| (times
# mean |xhat| <= 1 for the second sum).  Twice that.
TOL_COEF = 2.0 ** -8
# The rest of what the fused kernels return, of its maximum: dz as stored (bf16), the depthwise weight
# gradient (as tests/test_kernels_gpu.py::test_dwconv_bn_bwd_vs_fp32)
TOL_DZ = 2e-2
TOL_DWDW = 1e-2


def tol_of(case):
    return TOL[(case.family, "null" if case.kind == "null" else "fused" if case.kind == "fused" else "mixed",
                case.tol_dtype)]


def err_S(got, ref, S):
    """max |got - ref| / S in fp64."""
    return ((got.detach().double().cpu() - ref.double()).abs().max() / S).item()


def rel_max(got, ref):
    ref = ref.double()
    return ((got.detach().double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _signs(g, n):
    """+-1 with both signs present (n >= 2)."""
    s = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    if n >= 2:
        s[0], s[1] = 1.0, -1.0
    return s


def _unit_coeffs(g, xmax, amp=3.0, minor=0.25):
    """a, b per unit (fp64): |a| and |b| max|xhat| about `amp` in the units where they lead and
    `minor` of that in the others; a single unit carries both in full."""
    n = xmax.numel()
    a = _signs(g, n).double() * amp * (1 + 0.15 * _randn(g, n).double().clamp(-2, 2))
    b = _signs(g, n).double() * amp * (1 + 0.15 * _randn(g, n).double().clamp(-2, 2)) / xmax.double()
    if n > 1:
        lead_a = torch.arange(n) % 2 == 0
        a = torch.where(lead_a, a, a * minor)
        b = torch.where(lead_a, b * minor, b)
    return a, b


def _level(unit_scale):
    """The factor each unit's gradient is divided by, so that w rstd g (rstd gamma dy) has the same
    size in every unit: S is a maximum over all units, and one unit with a large rstd (LayerNorm
    rows at C = 4) or |w| (0.1 to 0.2 in the neutralised GELU) would otherwise set it alone."""
    return unit_scale / unit_scale.median()


def gelu_grad(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


# ------------------------------------------------------------------ references
LnRef = namedtuple("LnRef", "dx dgamma dbeta s1 s2 S")
BnRef = namedtuple("BnRef", "dx dw db k0 k1 S")


def ln_bwd_ref(dy, x, gamma, dres=None, s1_scale=1.0, s2_scale=1.0, dtype=F64):
    """LayerNorm backward from the kernel's rounded inputs, statistics recomputed, in `dtype`
    (fp64: the reference; fp32: the plain evaluation the headroom check measures)."""
    xd, gy = x.to(dtype), dy.to(dtype) * gamma.to(dtype)
    mean = xd.mean(1, keepdim=True)
    rstd = ((xd - mean).square().mean(1, keepdim=True) + EPS).rsqrt()
    xhat = (xd - mean) * rstd
    s1 = gy.mean(1, keepdim=True)
    s2 = (gy * xhat).mean(1, keepdim=True)
    dx = rstd * (gy - s1_scale * s1 - xhat * (s2_scale * s2))
    if dres is not None:
        dx = dx + dres.to(dtype)
    dyd = dy.to(dtype)
    return LnRef(dx, (dyd * xhat).sum(0), dyd.sum(0), s1[:, 0], s2[:, 0], (rstd * gy).abs().max().item())


def _bn_stats(xd):
    mean = xd.mean(0)
    rstd = ((xd - mean).square().mean(0) + EPS).rsqrt()
    return mean, rstd, (xd - mean) * rstd


def _bn_dx(g, xhat, w, rstd, k0_scale=1.0, k1_scale=1.0):
    """BatchNorm's dx map of the gradient g at the affine output, [M][C]."""
    k0 = g.mean(0)
    k1 = (g * xhat).mean(0)
    wr = w * rstd
    dx = wr * (g - k0_scale * k0 - xhat * (k1_scale * k1))
    return BnRef(dx, (g * xhat).sum(0), g.sum(0), k0, k1, (wr * g).abs().max().item())


def bn_bwd_ref(g, x, w, b, gelu, row_scale=None, rows_per_group=1, k0_scale=1.0, k1_scale=1.0, dtype=F64):
    """BatchNorm (+ GELU) backward of the gradient g [M][C] from the kernel's rounded inputs."""
    _, rstd, xhat = _bn_stats(x.to(dtype))
    w, b = w.to(dtype), b.to(dtype)
    gg = g.to(dtype)
    if row_scale is not None:
        gg = gg * row_scale.to(dtype)[torch.arange(x.shape[0]) // rows_per_group][:, None]
    if gelu:
        gg = gg * gelu_grad(xhat * w + b)
    return _bn_dx(gg, xhat, w, rstd, k0_scale, k1_scale)


DwRef = namedtuple("DwRef", "dx dz dwdw dgamma dbeta k0 k1 S xhat")
SeRef = namedtuple("SeRef", "dx dz dz2 dz1 dw db k0 k1 S xhat")


def dwconv_bn_ref(p, k0_scale=1.0, k1_scale=1.0, full_autograd=False):
    """fp64 autograd of conv2d(GELU(batch_norm(x)), groups=C) from the bf16 inputs: dz at the
    BatchNorm's affine output and the depthwise weight gradient by autograd, BatchNorm's dx map
    in closed form (full_autograd: dx by autograd through the statistics too)."""
    c = p["case"]
    Fr, H, C, s = c.Fr, c.H, c.C, c.s
    Ho = (H - 1) // s + 1
    x = p["x"].double().requires_grad_(full_autograd)
    w, b = p["w"].double(), p["b"].double()
    _, rstd, xhat = _bn_stats(x)
    z = xhat * w + b
    if not full_autograd:
        z = z.detach().requires_grad_(True)
    tw = p["wdw"].double().requires_grad_(True)
    y = F.conv2d(F.gelu(z).view(Fr, H, H, C).permute(0, 3, 1, 2), tw.view(C, 1, 3, 3), None, s, 1, 1, C)
    dy = p["dy"].double().view(Fr, Ho, Ho, C).permute(0, 3, 1, 2)
    if full_autograd:
        return torch.autograd.grad(y, x, dy)[0]
    dz, dwdw = torch.autograd.grad(y, (z, tw), dy)
    r = _bn_dx(dz, xhat.detach(), w, rstd.detach(), k0_scale, k1_scale)
    return DwRef(r.dx, dz, dwdw, r.dw, r.db, r.k0, r.k1, r.S, xhat.detach())


def se_bn_ref(p, k0_scale=1.0, k1_scale=1.0, full_autograd=False):
    """fp64 autograd of SE(GELU(batch_norm(x))), y = h sigmoid(relu(mean_hw(h) w1^T) w2^T)."""
    c = p["case"]
    Fn, HW, C = c.Fn, c.HW, c.C
    x = p["x"].double().requires_grad_(full_autograd)
    w, b = p["w"].double(), p["b"].double()
    _, rstd, xhat = _bn_stats(x)
    z = xhat * w + b
    if not full_autograd:
        z = z.detach().requires_grad_(True)
    h = F.gelu(z).view(Fn, HW, C)
    z1 = h.mean(1) @ p["w1"].double().t()
    z2 = torch.relu(z1) @ p["w2"].double().t()
    y = (h * torch.sigmoid(z2)[:, None, :]).reshape(Fn * HW, C)
    dy = p["dy"].double()
    if full_autograd:
        return torch.autograd.grad(y, x, dy)[0]
    dz, dz1, dz2 = torch.autograd.grad(y, (z, z1, z2), dy)
    r = _bn_dx(dz, xhat.detach(), w, rstd.detach(), k0_scale, k1_scale)
    return SeRef(r.dx, dz, dz2, dz1, r.dw, r.db, r.k0, r.k1, r.S, xhat.detach())


# ------------------------------------------------------------------ cases
class LnCase(namedtuple("LnCase", "C M xd yd kind dres seed")):
    family = "ln"

    @property
    def tol_dtype(self):
        return _NAME[self.xd]              # the dtype of x, dres and the stored dx

    @property
    def id(self):
        return "ln-C%d-M%d-%s_%s-%s-%s" % (self.C, self.M, _NAME[self.xd], _NAME[self.yd], self.kind,
                                           "dres" if self.dres else "nodres")


class BnCase(namedtuple("BnCase", "C M dt kind act rpg seed")):
    """act: 'none' (no GELU), 'neutral' (GELU, b = 8 and |w| in [0.1, 0.2]: GELU' = 1), 'plain' (GELU,
    ordinary parameters); rpg: rows per group of a row scale, 0 without one."""
    family = "bn"

    @property
    def tol_dtype(self):
        return _NAME[self.dt]

    @property
    def id(self):
        return "bn-C%d-M%d-%s-%s-%s%s" % (self.C, self.M, _NAME[self.dt], self.kind, self.act,
                                          "-rpg%d" % self.rpg if self.rpg else "")


class DwCase(namedtuple("DwCase", "Fr H C s seed")):
    family, kind, tol_dtype = "dw", "fused", "bf16"

    @property
    def id(self):
        return "dw-F%d-H%d-C%d-s%d" % (self.Fr, self.H, self.C, self.s)


class SeCase(namedtuple("SeCase", "Fn HW C seed")):
    family, kind, tol_dtype = "se", "fused", "bf16"

    @property
    def id(self):
        return "se-F%d-HW%d-C%d" % (self.Fn, self.HW, self.C)


LN_DTYPES = [(F32, F32), (BF16, BF16), (F32, BF16)]   # (x and dx, dy) as tests/test_kernels_gpu.py::test_layernorm


def _ln_cases():
    out = []
    for C in (4, 100, 192, 384, 576, 1024):
        for M in (1, 15, 777):
            for xd, yd in LN_DTYPES:
                for kind in ("null", "mixed"):
                    for dres in (True, False):
                        out.append(LnCase(C, M, xd, yd, kind, dres, 1000 + len(out)))
    return out


# A mixed gradient through an active GELU (ordinary parameters, w = 1 + 0.1 randn, b = 0.1 randn) meets
# the sensitivity condition in fp32 (k0 x 0.9 moves the reference by 3.6e-2 of S or more, k1 x 0.9 by
# 6e-2, against the 2e-4 that the 1e-4 tolerance demands) and not in bf16, where 4e-2 is demanded: GELU'
# gates half of every channel, so k0 is about a / 2 where S is about 1.13 a (the maximum of GELU'), and
# 0.1 x 0.5 / 1.13 = 4.4e-2 is all a 10 % error can move before the noise takes its share; a twice as
# large, or the other coefficient at a tenth, leaves the worst of the grid between 3.6e-2 and 4.06e-2.
# So the fp32 cases run the GELU with ordinary parameters as well as neutralised, the bf16 cases
# neutralised only; GELU' in bf16 stays with test_batchnorm_train.
BN_KINDS = [("null", "none"), ("mixed", "none"), ("null", "neutral"), ("mixed", "neutral")]
BN_SHAPES = [(C, M) for C in (8, 48, 96, 384, 768, 1536) for M in (5, 527, 3000)]
BN_RS_SHAPES = [(48, 527), (384, 3000), (1536, 527)]


def _bn_cases():
    out = []

    def add(C, M, dt, kind, act, rpg):
        out.append(BnCase(C, M, dt, kind, act, rpg, 2000 + len(out)))

    for C, M in BN_SHAPES:
        for dt in (F32, BF16):
            for kind, act in BN_KINDS:
                add(C, M, dt, kind, act, 0)
    # DropPath row scale (zeros and 1 / (1 - p)), one row per group and ragged groups of 37
    for C, M in BN_RS_SHAPES:
        for dt in (F32, BF16):
            for rpg in (1, 37):
                for act in ("none", "neutral"):
                    add(C, M, dt, "mixed", act, rpg)
    # the GELU with ordinary parameters (fp32: see above), without and with the row scale
    for C, M in BN_SHAPES:
        add(C, M, F32, "mixed", "plain", 0)
    for C, M in BN_RS_SHAPES:
        for rpg in (1, 37):
            add(C, M, F32, "mixed", "plain", rpg)
    return out


LN_CASES = _ln_cases()
BN_CASES = _bn_cases()
# layernorm_bwd_branch exists at C = 192 and 384: the null-space cases with a residual
LN_BRANCH_CASES = [c for c in LN_CASES if c.C in (192, 384) and c.kind == "null" and c.dres]
DW_CASES = [DwCase(2, 9, 32, 1, 3000), DwCase(2, 9, 32, 2, 3001), DwCase(2, 8, 64, 2, 3002)]
SE_CASES = [SeCase(3, 49, 96, 3100), SeCase(2, 64, 64, 3101)]


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------ input builders
def ln_build(case):
    """x, gamma, beta, dy, dres, and the values dgamma / dbeta hold before the call."""
    g = _gen(case.seed)
    M, C = case.M, case.C
    x = (_randn(g, M, C) * 3 + 1).to(case.xd)
    gamma = _signs(g, C) * (0.5 + torch.rand(C, generator=g))
    beta = _randn(g, C) * 0.1
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = ((xd - mean).square().mean(1, keepdim=True) + EPS).rsqrt()
    xhat = (xd - mean) * rstd
    a, b = _unit_coeffs(g, xhat.abs().amax(1))
    dy = (a[:, None] + b[:, None] * xhat) / gamma.double()
    noise = _randn(g, M, C).double()
    if case.kind == "mixed":
        dy = dy + 0.25 * noise
    dy = dy / _level(rstd)
    # a null-space dx is residue: a residual of full size would put its own bf16 rounding, 2^-9 |dres|,
    # above the 1e-3 the null-space tolerance may not pass; at 2^-9 randn it is as large as the residue
    # of a bf16 gradient, and leaving it out an error of several times that tolerance
    dres = (_randn(g, M, C) * (1.0 if case.kind == "mixed" else 2.0 ** -9)).to(case.xd) if case.dres else None
    return dict(case=case, x=x, gamma=gamma, beta=beta, dy=dy.to(case.yd), dres=dres,
                dgamma0=_randn(g, C) * 0.5, dbeta0=_randn(g, C) * 0.5)


def ln_ref(p, **kw):
    return ln_bwd_ref(p["dy"], p["x"], p["gamma"], p["dres"], **kw)


def bn_params(g, C, act):
    if act == "neutral":
        return _signs(g, C) * (0.1 + 0.1 * torch.rand(C, generator=g)), torch.full((C,), 8.0)
    return _randn(g, C) * 0.1 + 1, _randn(g, C) * 0.1


def droppath_like(g, n, p=0.1):
    rs = torch.where(torch.rand(n, generator=g) < p, 0.0, 1.0 / (1.0 - p)).float()
    rs[0] = 1.0 / (1.0 - p)
    if n > 1:
        rs[n // 2] = 0.0
    return rs


def bn_build(case):
    g = _gen(case.seed)
    M, C = case.M, case.C
    x = (_randn(g, M, C) * 2 + 0.5).to(case.dt)
    w, b = bn_params(g, C, case.act)
    _, rstd, xhat = _bn_stats(x.double())
    a, bc = _unit_coeffs(g, xhat.abs().amax(0))
    dy = a + bc * xhat
    noise = _randn(g, M, C).double()
    if case.kind == "mixed":
        dy = dy + 0.25 * noise
    dy = dy / _level(w.double().abs() * rstd)
    row_scale = droppath_like(g, (M + case.rpg - 1) // case.rpg) if case.rpg else None
    return dict(case=case, x=x, w=w, b=b, dy=dy.to(case.dt), gelu=case.act != "none", row_scale=row_scale,
                rpg=max(case.rpg, 1), dw0=_randn(g, C) * 0.5, db0=_randn(g, C) * 0.5)


def bn_ref(p, **kw):
    return bn_bwd_ref(p["dy"], p["x"], p["w"], p["b"], p["gelu"], p["row_scale"], p["rpg"], **kw)


def _bf16_exact_coeffs(g, xmax, level, minor=0.125):
    """_unit_coeffs for the fused kernels, levelled: |a| in [2, 4] (an eighth of that where b leads)
    over the channel's level, rounded to bf16 so that the constant is exact in the bf16 gradient."""
    n = xmax.numel()
    a = _signs(g, n).double() * (2 + 2 * torch.rand(n, generator=g).double())
    b = _signs(g, n).double() * (2 + 2 * torch.rand(n, generator=g).double()) / xmax.double()
    lead_a = torch.arange(n) % 2 == 0
    a = (torch.where(lead_a, a, a * minor) / level).to(BF16).double()
    return a, torch.where(lead_a, b * minor, b) / level


def dw_build(case):
    """Depthwise 3x3 (stride s) on GELU(BN0(x)) with the GELU neutralised.  The gradient at the conv
    output is a_c + b_c xhat(output position) + noise; the conv's transpose carries it to BN0 as
    about W(p) (a_c + b_c xhat(p)), W(p) the sum of the taps that reach input position p, when x is
    smooth in space and W(p) is flat: x is a bilinear field plus a little noise and the taps are
    (1 2 1) x (1 2 1) (which sums to the same at every stride-2 phase) with 10 % jitter and a sign."""
    g = _gen(case.seed)
    Fr, H, C, s = case.Fr, case.H, case.C, case.s
    coarse = _randn(g, Fr, C, 3, 3)
    xs = F.interpolate(coarse, size=(H, H), mode="bilinear", align_corners=True) * 1.5 + 0.2
    x = (xs.permute(0, 2, 3, 1) + 0.05 * _randn(g, Fr, H, H, C)).reshape(-1, C).to(BF16)
    w, b = bn_params(g, C, "neutral")
    k = torch.tensor([1.0, 2.0, 1.0])
    wdw = (_signs(g, C)[:, None] * 0.1 * torch.outer(k, k).reshape(1, 9)) * (1 + 0.1 * _randn(g, C, 9))
    _, rstd, xhat = _bn_stats(x.double())
    a, bc = _bf16_exact_coeffs(g, xhat.abs().amax(0), _level(w.double().abs() * rstd))
    xo = xhat.view(Fr, H, H, C)[:, ::s, ::s, :]
    dy = (a + bc * xo + 0.05 * _randn(g, *xo.shape).double()).reshape(-1, C).to(BF16)
    return dict(case=case, x=x, w=w, b=b, wdw=wdw, dy=dy, dg0=_randn(g, C) * 0.5, db0=_randn(g, C) * 0.5)


def se_build(case):
    """SE on GELU(BN2(x)), GELU neutralised; small fc weights keep the gate near 1/2 in every frame,
    so the gradient at BN2 stays about gate (a_c + b_c xhat)."""
    g = _gen(case.seed)
    Fn, HW, C = case.Fn, case.HW, case.C
    R = C // 4
    x = (_randn(g, Fn * HW, C) * 2).to(BF16)
    w, b = bn_params(g, C, "neutral")
    w1 = _randn(g, R, C) * 0.02
    w2 = _randn(g, C, R) * 0.2
    _, rstd, xhat = _bn_stats(x.double())
    a, bc = _bf16_exact_coeffs(g, xhat.abs().amax(0), _level(w.double().abs() * rstd))
    dy = (a + bc * xhat + 0.05 * _randn(g, Fn * HW, C).double()).to(BF16)
    return dict(case=case, x=x, w=w, b=b, w1=w1, w2=w2, dy=dy, dw0=_randn(g, C) * 0.5, db0=_randn(g, C) * 0.5)

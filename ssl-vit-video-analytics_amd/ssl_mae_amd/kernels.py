"""Thin tensor-level wrappers over the C ABI (include/sm_api.h).

Each function allocates its outputs (torch caching allocator, current device),
launches on the current stream and returns tensors.  No CPU path exists: a
missing library or a non-CUDA tensor raises.
"""
import math

import torch

from . import _lib
from ._lib import call, dt, ptr, query, stream


def _chk(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.KernelError("ssl_mae_amd kernels need device tensors (no CPU fallback)")


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------ GEMM
def gemm(A, B, C, M, N, K, a_layout, b_layout, lda, ldb, ldc, bias=None, alpha=1.0, beta=0.0,
         gelu=False, aux=None, R=None, round_branch=False, drop_p=0.0, seed=0, row_scale=None, rows_per_group=1,
         gelu_bwd=False):
    _chk(A, B, C)
    ab = dt(A)
    if dt(B) != ab:
        raise _lib.KernelError("GEMM operands must share a dtype")
    nbytes = query("sm_gemm_workspace_bytes", ab, M, N, K)
    ws = _ws(nbytes, A.device) if nbytes else None
    epi = (1 if gelu else 0) | (2 if round_branch else 0) | (4 if gelu_bwd else 0)
    call("sm_gemm", ab, dt(C), a_layout, b_layout, M, N, K, ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(bias),
         float(alpha), float(beta), epi, ptr(aux), ptr(R), float(drop_p), int(seed) & ((1 << 64) - 1), ptr(row_scale),
         int(rows_per_group), ptr(ws), nbytes, stream())
    return C


def gemm_persistent(mode=-1):
    """Select the persistent (1) or one-tile-per-block (0) form of the plain bf16 forward /
    data-gradient GEMMs (bit-identical outputs); mode < 0 queries.  Returns the previous mode."""
    return int(query("sm_gemm_persistent", int(mode)))


GEMM_TUNING_KEYS = ("pp", "pp_min_n", "pp_max_k", "pp_rounds", "pp_rounds_small_k", "pp_rounds_mid_k", "mf16_min_k",
                    "dw384", "dw384_notr")


def gemm_tuning(key, value=None, reset=False):
    """A/B knob of the GEMM dispatch (sm_gemm_tuning; scripts/ only, the product path never
    sets one): returns the current value of `key` (GEMM_TUNING_KEYS), then stores `value`
    (or the default with reset=True)."""
    import ctypes
    k = GEMM_TUNING_KEYS.index(key)
    prev = ctypes.c_int(0)
    call("sm_gemm_tuning", k, -1 if reset else (1 if value is not None else 0), int(value or 0),
         ctypes.addressof(prev))
    return prev.value


_GEMM_TUNING_DEFAULTS = {"pp": 1, "pp_min_n": 128, "pp_max_k": 384, "pp_rounds": -1,
                         "pp_rounds_small_k": 8, "pp_rounds_mid_k": 2, "mf16_min_k": 1 << 30,
                         "dw384": 1, "dw384_notr": 1}


def gemm_tuning_nondefault():
    """{key: value} of every GEMM knob not at its default (reported in bench.py's config)."""
    out = {}
    for k, d in _GEMM_TUNING_DEFAULTS.items():
        v = gemm_tuning(k)
        if v != d:
            out[k] = v
    return out


def calibrate_mfma(shape=32, iters=20000, blocks=None, device=None):
    """Bare bf16 MFMA loop on random register data (csrc/calib.hip), the box calibration of
    bench.py: shape 32 = v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16; `blocks`
    workgroups of 4 waves (default 2 per CU).  Returns (TFLOP/s, median in-kernel clock MHz,
    ms) over one timed launch after a warm-up launch."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if blocks is None:
        blocks = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    stamps = torch.zeros(blocks, 2, dtype=torch.int64, device=dev)
    sink = torch.zeros(blocks * 256, dtype=torch.float32, device=dev)
    call("sm_calibrate_mfma", int(shape), max(1, int(iters) // 10), int(blocks), ptr(stamps), ptr(sink), stream())   # warm-up
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    call("sm_calibrate_mfma", int(shape), int(iters), int(blocks), ptr(stamps), ptr(sink), stream())
    e.record()
    e.synchronize()
    ms = s.elapsed_time(e)
    flop = 2.0 * 32 * 32 * 16 * 8 * iters * 4 * blocks    # 8 MFMAs (32x32x16 or 2x 16x16x32 pairs) per iter
    st = stamps.cpu()
    mem, real = st[:, 0].double(), st[:, 1].double()
    ok = real > 0
    mhz = float((mem[ok] / real[ok] * 100.0).median()) if ok.any() else None
    return flop / (ms * 1e-3) / 1e12, mhz, ms


def linear(x, w, bias=None, out_dtype=None, gelu=False, residual=None, round_branch=False, drop_p=0.0, seed=0,
           row_scale=None, rows_per_group=1):
    """y = residual + rs[row] * drop(act(x @ w^T + bias)); returns (y, pre-activation) with GELU."""
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=out_dtype or x.dtype, device=x.device)
    pre = torch.empty_like(out) if gelu else None
    gemm(x, w, out, M, N, K, 0, 0, K, K, N, bias=bias, gelu=gelu, aux=pre,
         beta=1.0 if residual is not None else 0.0, R=residual, round_branch=round_branch, drop_p=drop_p,
         seed=seed, row_scale=row_scale, rows_per_group=rows_per_group)
    return (out, pre) if gelu else out


def linear_dx(dy, w, out_dtype=None, residual=None, gelu_pre=None, drop_p=0.0, seed=0):
    """dx = dy @ w (+ residual);  dy [M,N], w [N,K].  gelu_pre: the input of a GELU (with
    dropout drop_p / seed on its output) that produced this Linear's input: returns the
    gradient w.r.t. that pre-activation, dx * keep * 256/(256-round(256p)) * GELU'(gelu_pre), in the
    epilogue (no dh round trip, no separate gelu_bwd pass)."""
    M, N = dy.shape
    K = w.shape[1]
    out = torch.empty((M, K), dtype=out_dtype or dy.dtype, device=dy.device)
    if gelu_pre is not None:
        if gelu_pre.shape != out.shape or gelu_pre.dtype != out.dtype or residual is not None:
            raise _lib.KernelError("linear_dx: gelu_pre must match dx's shape/dtype (no residual)")
        gemm(dy, w, out, M, K, N, 0, 1, N, K, K, aux=gelu_pre.contiguous(), gelu_bwd=True, drop_p=drop_p, seed=seed)
        return out
    gemm(dy, w, out, M, K, N, 0, 1, N, K, K, beta=1.0 if residual is not None else 0.0, R=residual)
    return out


def linear_dx_gelu(dy, w, pre, drop_p=0.0, seed=0):
    """(dL/dpre, h) of y = dropout(GELU(pre)) @ w^T: dL/dpre = linear_dx(dy, w, gelu_pre=pre)
    and h = gelu(pre, drop_p, seed) (the fc2 weight gradient's operand) from one GEMM
    epilogue (sm_linear_dx_gelu): pre is read once, no recompute pass.  bf16 only."""
    _chk(dy, w, pre)
    M, N = dy.shape
    K = w.shape[1]
    if (dy.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or pre.dtype != torch.bfloat16
            or tuple(pre.shape) != (M, K) or w.shape[0] != N):
        raise _lib.KernelError("linear_dx_gelu: bf16 dy [M,N], w [N,K], pre [M,K]")
    dx = torch.empty((M, K), dtype=torch.bfloat16, device=dy.device)
    h = torch.empty_like(dx)
    call("sm_linear_dx_gelu", M, N, K, ptr(dy), ptr(w), ptr(pre), ptr(dx), ptr(h), float(drop_p), int(seed), stream())
    return dx, h


def linear_dw(dy, x, grad_sink, accumulate=True):
    """grad_sink[N,K] (+)= dy^T @ x   (fp32 sink; reduction over the M token rows)."""
    M, N = dy.shape
    K = x.shape[1]
    gemm(dy, x, grad_sink, N, K, M, 1, 1, N, K, K, beta=1.0 if accumulate else 0.0)
    return grad_sink


def linear_dw_bias(dy, x, grad_w, grad_b, gelu=None):
    """grad_w[N,K] += dy^T @ x' and grad_b[N] += sum over rows of dy.  bf16: one GEMM
    whose n0 == 0 blocks also sum dy (sm_linear_dw_bias); fp32 (parity): two ops.
    x' = x, or with gelu=(drop_p, seed) x' = dropout(GELU(x)) of the fc1 pre-activation
    x: formed in the GEMM's operand loads (sm_linear_dw_bias_gelu) when the weight
    gradient has one 256-row tile (N <= 256), else by the gelu kernel first (two
    m-tiles would activate every element twice; the recompute pass is cheaper)."""
    M, N = dy.shape
    K = x.shape[1]
    if gelu is not None:
        if (N <= 256 and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and N % 8 == 0 and K % 8 == 0):
            _chk(dy, x, grad_w, grad_b)
            nbytes = query("sm_linear_dw_bias_workspace_bytes", M, N, K)
            ws = _ws(nbytes, dy.device)
            call("sm_linear_dw_bias_gelu", M, N, K, ptr(dy), ptr(x), float(gelu[0]), int(gelu[1]), ptr(grad_w),
                 ptr(grad_b), 1, ptr(ws), nbytes, stream())
            return grad_w
        return linear_dw_bias(dy, gelu_fwd(x, gelu[0], gelu[1]), grad_w, grad_b)
    if dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and N % 8 == 0 and K % 8 == 0:
        _chk(dy, x, grad_w, grad_b)
        nbytes = query("sm_linear_dw_bias_workspace_bytes", M, N, K)
        ws = _ws(nbytes, dy.device)
        call("sm_linear_dw_bias", M, N, K, ptr(dy), ptr(x), ptr(grad_w), ptr(grad_b), 1, ptr(ws), nbytes, stream())
        return grad_w
    linear_dw(dy, x, grad_w)
    colsum(dy, grad_b)
    return grad_w


def linear_bn_stats(x, w, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, updates=1,
                    num_batches=None):
    """y = x @ w^T (bf16) and the train-mode BatchNorm statistics of y from the GEMM's
    epilogue (sm_linear_bn_stats; = linear + bn_stats without the read pass of y).
    Returns (y, mean, rstd)."""
    _chk(x, w)
    M, Kd = x.shape
    N = w.shape[0]
    if w.shape[1] != Kd or x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise _lib.KernelError("linear_bn_stats: bf16 x [M,K], w [N,K]")
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(N, dtype=torch.float32, device=x.device)
    rstd = torch.empty(N, dtype=torch.float32, device=x.device)
    nbytes = query("sm_linear_bn_stats_workspace_bytes", M, N)
    ws = _ws(nbytes, x.device)
    call("sm_linear_bn_stats", M, N, Kd, ptr(x), ptr(w), ptr(y), ptr(mean), ptr(rstd), ptr(running_mean),
         ptr(running_var), ptr(num_batches), float(momentum), float(eps), int(updates), ptr(ws), nbytes, stream())
    return y, mean, rstd


def linear_bnin(a, act, w, bn=None, updates=1):
    """y [M,N] bf16 = x @ w^T with x = bf16(BN(a)) (act = (mean, rstd, weight, bias), no GELU)
    formed in the GEMM's A-operand loads (sm_linear_bnin; bit-identical to bn_apply +
    linear).  bn: also the train-mode BatchNorm statistics of y (sm_linear_bnin_bn_stats,
    = linear_bn_stats); returns y, or (y, mean, rstd) with bn."""
    _chk(a, w, *act[:4])
    M, Kd = a.shape
    N = w.shape[0]
    if w.shape[1] != Kd or a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or act[4]:
        raise _lib.KernelError("linear_bnin: bf16 a [M,K], w [N,K], BatchNorm act without GELU")
    y = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    if bn is None:
        call("sm_linear_bnin", M, N, Kd, ptr(a), *[ptr(t) for t in act[:4]], ptr(w), ptr(y), stream())
        return y
    running_mean, running_var, momentum, eps, num_batches = bn
    mean = torch.empty(N, dtype=torch.float32, device=a.device)
    rstd = torch.empty(N, dtype=torch.float32, device=a.device)
    nbytes = query("sm_linear_bn_stats_workspace_bytes", M, N)
    ws = _ws(nbytes, a.device)
    call("sm_linear_bnin_bn_stats", M, N, Kd, ptr(a), *[ptr(t) for t in act[:4]], ptr(w), ptr(y), ptr(mean),
         ptr(rstd), ptr(running_mean), ptr(running_var), ptr(num_batches), float(momentum), float(eps), int(updates),
         ptr(ws), nbytes, stream())
    return y, mean, rstd


def linear_se(a2, w, act, gate, hw):
    """y [M,N] bf16 = h3 @ w^T with h3 = se_scale(a2, gate, act) formed in the GEMM's
    A-operand loads (sm_linear_se; bit-identical to se_fwd's h3 + linear).  a2 [M,C] bf16,
    w [N,C] bf16, gate [M/hw, C] fp32, hw % 128 == 0, C % 64 == 0."""
    _chk(a2, w, gate)
    M, C = a2.shape
    N = w.shape[0]
    if w.shape[1] != C or gate.shape != (M // hw, C) or M % hw:
        raise _lib.KernelError("linear_se: shape mismatch")
    y = torch.empty((M, N), dtype=torch.bfloat16, device=a2.device)
    call("sm_linear_se", M, N, C, ptr(a2), ptr(w), *_act_args(act), ptr(gate.contiguous()), int(hw), ptr(y),
         stream())
    return y


def linear_dw_se(dy, a2, act, gate, hw, grad_sink, accumulate=True):
    """grad_sink[N,C] (+)= dy^T @ h3 with h3 = se_scale(a2, gate, act) formed in the GEMM's
    operand loads (sm_linear_dw_se; bit-identical to se_scale + linear_dw).  dy [M,N],
    a2 [M,C] bf16, gate [M/hw, C] fp32, hw % 64 == 0."""
    _chk(dy, a2, grad_sink)
    M, N = dy.shape
    C = a2.shape[1]
    if gate is None:          # B = the BatchNorm output act(a2) itself (the stem's BN2, no gate)
        hw = 1
    elif gate.shape != (M // hw, C) or M % hw:
        raise _lib.KernelError("linear_dw_se: gate shape mismatch")
    if a2.shape[0] != M or grad_sink.shape != (N, C):
        raise _lib.KernelError("linear_dw_se: shape mismatch")
    nbytes = query("sm_linear_dw_se_workspace_bytes", M, N, C)
    ws = _ws(nbytes, dy.device)
    call("sm_linear_dw_se", M, N, C, ptr(dy), ptr(a2), *_act_args(act),
         ptr(None if gate is None else gate.contiguous()), int(hw), ptr(grad_sink), 1 if accumulate else 0,
         ptr(ws), nbytes, stream())
    return grad_sink


def colsum(x, out, accumulate=True):
    M, C = x.shape
    nbytes = query("sm_colsum_workspace_bytes", M, C)
    ws = _ws(nbytes, x.device)
    call("sm_colsum", dt(x), M, C, ptr(x), ptr(out), 1 if accumulate else 0, ptr(ws), nbytes, stream())
    return out


# ------------------------------------------------------------------ attention
def attn_tuning(D, shape=None, reset=False):
    """MFMA shape of the bf16 attention backward for head dim D (sm_attn_tuning): 32 =
    v_mfma_f32_32x32x16_bf16, 16 = v_mfma_f32_16x16x32_bf16.  Returns the current shape,
    then stores `shape` (or the default with reset=True).  Tests and A/B scripts only."""
    import ctypes
    prev = ctypes.c_int(0)
    call("sm_attn_tuning", 0 if D == 64 else 1, -1 if reset else (1 if shape is not None else 0), int(shape or 0),
         ctypes.addressof(prev))
    return prev.value


def attn_fwd(qkv, N, L, H, D, drop_p=0.0, seed=0):
    _chk(qkv)
    out = torch.empty((N * L, H * D), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((N, H, L), dtype=torch.float32, device=qkv.device)
    call("sm_attn_fwd", dt(qkv), N, L, H, D, ptr(qkv), ptr(out), ptr(lse), 1.0 / math.sqrt(D), float(drop_p),
         int(seed), stream())
    return out, lse


def attn_bwd(qkv, o, do, lse, N, L, H, D, drop_p=0.0, seed=0):
    _chk(qkv, o, do, lse)
    dqkv = torch.empty_like(qkv)
    ws = _ws(query("sm_attn_bwd_workspace_bytes", dt(qkv), N, L, H, D), qkv.device)   # Delta (+ scaled Q)
    call("sm_attn_bwd", dt(qkv), N, L, H, D, ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(ws), ptr(dqkv),
         1.0 / math.sqrt(D), float(drop_p), int(seed), stream())
    return dqkv


# ------------------------------------------------------------------ LayerNorm
def layernorm(x, gamma, beta, out_dtype=None, eps=1e-5):
    _chk(x)
    M, C = x.shape
    y = torch.empty((M, C), dtype=out_dtype or x.dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("sm_layernorm_fwd", dt(x), dt(y), M, C, ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
         float(eps), stream())
    return y, mean, rstd


def layernorm_recompute(x, gamma, beta, out_dtype, eps=1e-5):
    return layernorm(x, gamma, beta, out_dtype, eps)[0]


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None):
    M, C = x.shape
    dx = torch.empty_like(x)
    nbytes = query("sm_layernorm_bwd_workspace_bytes", M, C)
    ws = _ws(nbytes, x.device)
    call("sm_layernorm_bwd", dt(x), dt(dy), dt(dx), M, C, ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
         ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, stream())
    return dx


def layernorm_bwd_branch(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None, drop_p=0.0, seed=0, row_scale=None,
                         rows_per_group=1):
    """layernorm_bwd plus the branch copy dxb = bf16(bf16(dx) * row_scale * dropout keep)
    (sm_layernorm_bwd_branch; = cast + dropout_bwd of dx).  Returns (dx, dxb)."""
    M, C = x.shape
    dx = torch.empty_like(x)
    dxb = torch.empty((M, C), dtype=torch.bfloat16, device=x.device)
    nbytes = query("sm_layernorm_bwd_workspace_bytes", M, C)
    ws = _ws(nbytes, x.device)
    call("sm_layernorm_bwd_branch", dt(x), dt(dy), dt(dx), M, C, ptr(dy), ptr(x), ptr(mean), ptr(rstd), ptr(gamma),
         ptr(dx), ptr(dres), ptr(dgamma), ptr(dbeta), ptr(dxb), float(drop_p), int(seed), ptr(row_scale),
         int(rows_per_group), ptr(ws), nbytes, stream())
    return dx, dxb


# ------------------------------------------------------------------ BatchNorm (train)
def bn_stats(x2d, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, updates=1, num_batches=None):
    _chk(x2d)
    M, C = x2d.shape
    mean = torch.empty(C, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty(C, dtype=torch.float32, device=x2d.device)
    nbytes = query("sm_bn_workspace_bytes", M, C)
    ws = _ws(nbytes, x2d.device)
    call("sm_bn_stats", dt(x2d), M, C, ptr(x2d), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var),
         ptr(num_batches), float(momentum), float(eps), int(updates), ptr(ws), nbytes, stream())
    return mean, rstd


def bn_eval_params(bn):
    """(mean, rstd) of an eval-mode BatchNorm module from its running statistics."""
    C = bn.running_mean.numel()
    dev = bn.running_mean.device
    _chk(bn.running_mean)
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    call("sm_bn_eval_params", ptr(bn.running_mean), ptr(bn.running_var), C, float(bn.eps), ptr(mean), ptr(rstd),
         stream())
    return mean, rstd


def bn_apply(x2d, mean, rstd, w, b, gelu=False, out_dtype=None, residual=None, row_scale=None, rows_per_group=1,
             residual_bn=None):
    """residual_bn = (mean, rstd, weight, bias): the residual is stored before its own
    BatchNorm and enters as bf16(BN(residual)) (sm_bn_apply_res_bn)."""
    M, C = x2d.shape
    y = torch.empty((M, C), dtype=out_dtype or x2d.dtype, device=x2d.device)
    if residual_bn is not None:
        if residual is None:
            raise _lib.KernelError("bn_apply: residual_bn without a residual")
        call("sm_bn_apply_res_bn", dt(x2d), dt(y), M, C, ptr(x2d), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(y),
             1 if gelu else 0, ptr(residual), *[ptr(t) for t in residual_bn[:4]], ptr(row_scale), int(rows_per_group),
             stream())
        return y
    call("sm_bn_apply", dt(x2d), dt(y), M, C, ptr(x2d), ptr(mean), ptr(rstd), ptr(w), ptr(b), ptr(y),
         1 if gelu else 0, ptr(residual), ptr(row_scale), int(rows_per_group), stream())
    return y


def bn_bwd(dy, x2d, mean, rstd, w, b, gelu, dw_sink, db_sink, row_scale=None, rows_per_group=1):
    M, C = x2d.shape
    dx = torch.empty_like(dy)
    nbytes = query("sm_bn_workspace_bytes", M, C)
    ws = _ws(nbytes, x2d.device)
    call("sm_bn_bwd", dt(x2d), dt(dy), M, C, ptr(dy), ptr(x2d), ptr(mean), ptr(rstd), ptr(w), ptr(b),
         1 if gelu else 0, ptr(row_scale), int(rows_per_group), ptr(dx), ptr(dw_sink), ptr(db_sink), ptr(ws),
         nbytes, stream())
    return dx


# ------------------------------------------------------------------ elementwise
def gelu(x, drop_p=0.0, seed=0):
    return gelu_fwd(x, drop_p, seed)


def gelu_fwd(x, drop_p=0.0, seed=0):
    y = torch.empty_like(x)
    call("sm_gelu_fwd", dt(x), x.numel(), x.shape[-1], ptr(x), ptr(y), float(drop_p), int(seed), stream())
    return y


def gelu_bwd(pre, dy, drop_p=0.0, seed=0):
    dx = torch.empty_like(dy)
    call("sm_gelu_bwd", dt(pre), dt(dy), dy.numel(), dy.shape[-1], ptr(pre), ptr(dy), ptr(dx), float(drop_p),
         int(seed), stream())
    return dx


def dropout_bwd(dy, drop_p=0.0, seed=0, row_scale=None, rows_per_group=1):
    dx = torch.empty_like(dy)
    call("sm_dropout_bwd", dt(dy), dy.numel(), dy.shape[-1], ptr(dy), ptr(dx), float(drop_p), int(seed),
         ptr(row_scale), int(rows_per_group), stream())
    return dx


def cast_dropout_bwd(dy, drop_p=0.0, seed=0, row_scale=None, rows_per_group=1):
    """bf16(bf16(dy) * row_scale * dropout keep) of an fp32 dy in one pass (= cast + dropout_bwd)."""
    _chk(dy)
    if dy.dtype != torch.float32:
        raise _lib.KernelError("cast_dropout_bwd takes an fp32 gradient")
    dx = torch.empty(dy.shape, dtype=torch.bfloat16, device=dy.device)
    call("sm_cast_dropout_bwd", dy.numel(), dy.shape[-1], ptr(dy), ptr(dx), float(drop_p), int(seed), ptr(row_scale),
         int(rows_per_group), stream())
    return dx


def droppath_scale(n, p, seed, device):
    out = torch.empty(n, dtype=torch.float32, device=device)
    call("sm_droppath_scale", int(n), float(p), int(seed), ptr(out), stream())
    return out


def add(a, b, out_dtype=None):
    o = torch.empty(b.shape, dtype=out_dtype or b.dtype, device=b.device)
    if dt(b) != dt(o):
        raise _lib.KernelError("add: b and out must share dtype")
    call("sm_add", dt(a), dt(o), o.numel(), ptr(a), ptr(b), ptr(o), stream())
    return o


def cast(a, dtype, out=None):
    o = out if out is not None else torch.empty(a.shape, dtype=dtype, device=a.device)
    call("sm_cast", dt(a), dt(o), a.numel(), ptr(a), ptr(o), stream())
    return o


def fill_(t, v):
    call("sm_fill", ptr(t), t.numel(), float(v), stream())
    return t


# ------------------------------------------------------------------ convolutions
def _stem_geometry(clip):
    """B, T, H, W, the five element strides (sB, sC, sT, sH, sW) and the stride-2, pad-1 output
    size of a clip [B,3,T,H,W] or of frames [N,3,H,W] (T = 1, sT = 0)."""
    if clip.dim() == 5:
        B, _, T, H, W = clip.shape
        strides = clip.stride()
    else:
        B, _, H, W = clip.shape
        T = 1
        sB, sC, sH, sW = clip.stride()
        strides = (sB, sC, 0, sH, sW)
    return B, T, H, W, strides, (H + 1) // 2, (W + 1) // 2


def stem_im2col(clip, out_dtype, frames_view=None):
    """clip [B,3,T,H,W] (fp32, any strides) -> col [B*T*Ho*Wo, 32] (stride 2, pad 1)."""
    _chk(clip)
    if clip.dtype != torch.float32:
        clip = clip.float()
    B, T, H, W, strides, Ho, Wo = _stem_geometry(clip)
    col = torch.empty((B * T * Ho * Wo, 32), dtype=out_dtype, device=clip.device)
    call("sm_stem_im2col", dt(col), ptr(clip), B, T, H, W, *strides, 2, ptr(col), stream())
    return col, (B * T, Ho, Wo)


def stem_conv1_bn_stats(clip, wpack, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, updates=1,
                        num_batches=None):
    """PatchEmbed conv1 (3->48, 3x3, stride 2, pad 1) straight from the fp32 clip [B,3,T,H,W]
    (or frames [N,3,H,W]; any strides) with bf16 order-0 packed weights [48][32], plus the
    train-mode BatchNorm statistics of its bf16 output (sm_stem_conv1_bn_stats;
    = stem_im2col + linear_bn_stats with no im2col buffer).  Returns (y, mean, rstd, (F, Ho, Wo))."""
    _chk(clip, wpack)
    if clip.dtype != torch.float32:
        clip = clip.float()
    if wpack.dtype != torch.bfloat16 or tuple(wpack.shape) != (48, 32) or not wpack.is_contiguous():
        raise _lib.KernelError("stem_conv1_bn_stats: wpack is contiguous bf16 [48][32]")
    B, T, H, W, strides, Ho, Wo = _stem_geometry(clip)
    y = torch.empty((B * T * Ho * Wo, 48), dtype=torch.bfloat16, device=clip.device)
    mean = torch.empty(48, dtype=torch.float32, device=clip.device)
    rstd = torch.empty(48, dtype=torch.float32, device=clip.device)
    nbytes = query("sm_stem_conv1_workspace_bytes")
    ws = _ws(nbytes, clip.device)
    call("sm_stem_conv1_bn_stats", ptr(clip), B, T, H, W, *strides, ptr(wpack), ptr(y), ptr(mean), ptr(rstd),
         ptr(running_mean), ptr(running_var), ptr(num_batches), float(momentum), float(eps), int(updates),
         ptr(ws), nbytes, stream())
    return y, mean, rstd, (B * T, Ho, Wo)


def stem_conv2_bn_stats(a1, act, wpack, F, H, W, running_mean=None, running_var=None, momentum=0.1, eps=1e-5,
                        updates=1, num_batches=None):
    """PatchEmbed conv2 over h1 = act(a1) (act = (mean, rstd, weight, bias, gelu) of BN1)
    plus the train-mode BatchNorm statistics of its bf16 output (sm_stem_conv2_bn_stats;
    = bn_apply + conv3x3_fwd_bn_stats with h1 never written).  a1 [F*H*W, 48] bf16, wpack
    order-1 [96, 432] bf16.  Returns (y [F*H*W, 96], mean, rstd)."""
    _chk(a1, wpack)
    _conv_chk(a1, 48)
    _conv_chk(wpack, 432)
    m, r, g, b, gelu = act
    y = torch.empty((F * H * W, 96), dtype=torch.bfloat16, device=a1.device)
    mean = torch.empty(96, dtype=torch.float32, device=a1.device)
    rstd = torch.empty(96, dtype=torch.float32, device=a1.device)
    nbytes = query("sm_stem_conv2_workspace_bytes", F)
    ws = _ws(nbytes, a1.device)
    call("sm_stem_conv2_bn_stats", ptr(a1), F, H, W, ptr(m), ptr(r), ptr(g), ptr(b), int(bool(gelu)), ptr(wpack),
         ptr(y), ptr(mean), ptr(rstd), ptr(running_mean), ptr(running_var), ptr(num_batches), float(momentum),
         float(eps), int(updates), ptr(ws), nbytes, stream())
    return y, mean, rstd


def im2col3(x, F, H, W, C, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    col = torch.empty((F * Ho * Wo, 9 * C), dtype=x.dtype, device=x.device)
    call("sm_im2col3", dt(x), ptr(x), F, H, W, C, stride, ptr(col), stream())
    return col


def col2im3(dcol, F, H, W, C, stride):
    dx = torch.empty((F * H * W, C), dtype=dcol.dtype, device=dcol.device)
    call("sm_col2im3", dt(dcol), ptr(dcol), F, H, W, C, stride, ptr(dx), stream())
    return dx


def conv_wpack(w, Kpad, order, dtype):
    """w [Cout][Cin][3][3] fp32 -> packed [Cout][Kpad] (order 0 / 1) or [Cin][Kpad] (order 2)."""
    Cout, Cin = w.shape[0], w.shape[1]
    out = torch.empty((Cin if order == 2 else Cout, Kpad), dtype=dtype, device=w.device)
    call("sm_conv_wpack", dt(out), ptr(w), ptr(out), Cout, Cin, Kpad, order, stream())
    return out


def _conv_chk(t, C):
    if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.shape[-1] != C:
        raise _lib.KernelError(f"conv3x3 operands are contiguous bf16 channels-last [pixels][{C}]")


def conv3x3_fwd(x, wpack, F, H, W, Cin, Cout):
    """Stem conv2 (3x3, stride 1, pad 1) over channels-last bf16 x [F*H*W, Cin] with
    order-1 packed weights [Cout][9*Cin]: implicit-im2col GEMM -> y [F*H*W, Cout] bf16."""
    _chk(x, wpack)
    _conv_chk(x, Cin)
    _conv_chk(wpack, 9 * Cin)
    y = torch.empty((F * H * W, Cout), dtype=torch.bfloat16, device=x.device)
    call("sm_conv3x3_fwd", ptr(x), ptr(wpack), ptr(y), F, H, W, Cin, Cout, stream())
    return y


def conv3x3_fwd_bn_stats(x, wpack, F, H, W, Cin, Cout, running_mean=None, running_var=None, momentum=0.1,
                         eps=1e-5, updates=1, num_batches=None):
    """conv3x3_fwd plus the train-mode BatchNorm statistics of y from the GEMM epilogue
    (sm_conv3x3_fwd_bn_stats; = conv3x3_fwd + bn_stats without the read pass of y).
    Returns (y, mean, rstd)."""
    _chk(x, wpack)
    _conv_chk(x, Cin)
    _conv_chk(wpack, 9 * Cin)
    P = F * H * W
    y = torch.empty((P, Cout), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(Cout, dtype=torch.float32, device=x.device)
    rstd = torch.empty(Cout, dtype=torch.float32, device=x.device)
    nbytes = query("sm_linear_bn_stats_workspace_bytes", P, Cout)
    ws = _ws(nbytes, x.device)
    call("sm_conv3x3_fwd_bn_stats", ptr(x), ptr(wpack), ptr(y), F, H, W, Cin, Cout, ptr(mean), ptr(rstd),
         ptr(running_mean), ptr(running_var), ptr(num_batches), float(momentum), float(eps), int(updates), ptr(ws),
         nbytes, stream())
    return y, mean, rstd


def conv3x3_dgrad(dy, wpack_t, F, H, W, Cin, Cout):
    """dL/dx of conv3x3_fwd from dy [F*H*W, Cout] and order-2 packed weights [Cin][9*Cout]."""
    _chk(dy, wpack_t)
    _conv_chk(dy, Cout)
    _conv_chk(wpack_t, 9 * Cout)
    dx = torch.empty((F * H * W, Cin), dtype=torch.bfloat16, device=dy.device)
    call("sm_conv3x3_dgrad", ptr(dy), ptr(wpack_t), ptr(dx), F, H, W, Cin, Cout, stream())
    return dx


def conv3x3_wgrad(dy, x, dw_sink, F, H, W, Cin, Cout, accumulate=True):
    """dw_sink [Cout][9*Cin] fp32 (+)= weight gradient of conv3x3_fwd (order-1 layout)."""
    _chk(dy, x, dw_sink)
    _conv_chk(dy, Cout)
    _conv_chk(x, Cin)
    if dw_sink.dtype != torch.float32 or dw_sink.shape != (Cout, 9 * Cin) or not dw_sink.is_contiguous():
        raise _lib.KernelError("conv3x3_wgrad sink is contiguous fp32 [Cout][9*Cin]")
    nbytes = query("sm_conv3x3_wgrad_workspace_bytes", F, H, W, Cin, Cout)
    ws = _ws(nbytes, dy.device)
    call("sm_conv3x3_wgrad", ptr(dy), ptr(x), ptr(dw_sink), 1 if accumulate else 0, F, H, W, Cin, Cout, ptr(ws),
         nbytes, stream())
    return dw_sink


def conv_wunpack_add(packed, grad, order):
    Cout, Cin = grad.shape[0], grad.shape[1]
    call("sm_conv_wunpack_add", ptr(packed), ptr(grad), Cout, Cin, packed.shape[1], order, stream())


def dwconv(x, w, F, H, W, C, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((F * Ho * Wo, C), dtype=x.dtype, device=x.device)
    call("sm_dwconv_fwd", dt(x), ptr(x), ptr(w), ptr(y), F, H, W, C, stride, stream())
    return y


def dwconv_bwd(dy, x, w, dw_sink, F, H, W, C, stride, need_dx=True):
    dx = torch.empty_like(x) if need_dx else None
    nbytes = query("sm_dwconv_wgrad_workspace_bytes", F, H, W, C, stride)
    ws = _ws(nbytes, x.device)
    call("sm_dwconv_bwd", dt(x), ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw_sink), F, H, W, C, stride, ptr(ws),
         nbytes, stream())
    return dx


def _act_args(act):
    """act = None or (mean, rstd, weight, bias, gelu): the BN(+GELU) folded into loads."""
    if act is None:
        return [None, None, None, None, 0]
    mean, rstd, w, b, gelu = act
    return [ptr(mean), ptr(rstd), ptr(w), ptr(b), 1 if gelu else 0]


def dwconv_fused(x, act, w, F, H, W, C, stride, bn_out=None, bn_updates=1):
    """y = dwconv3x3(act(x)) (bf16); with bn_out (a BatchNorm2d module) also its
    train-mode statistics of y (running stats updated bn_updates times): returns
    (y, mean, rstd) (or y)."""
    _chk(x)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    dev = x.device
    y = torch.empty((F * Ho * Wo, C), dtype=x.dtype, device=dev)
    part = None
    if bn_out is not None:
        rows = query("sm_dwconv_fused_partial_rows", F, H, stride)
        part = torch.empty((rows, 2, C), dtype=torch.float32, device=dev)
    a = _act_args(act)
    call("sm_dwconv_fused_fwd", F, H, W, C, stride, ptr(x), a[0], a[1], a[2], a[3], a[4], ptr(w), ptr(y), ptr(part),
         stream())
    if bn_out is None:
        return y
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    rstd = torch.empty(C, dtype=torch.float32, device=dev)
    nbytes = query("sm_bn_partials_workspace_bytes", C)
    ws = _ws(nbytes, dev)
    call("sm_bn_stats_from_partials", ptr(part), part.shape[0], C, F * Ho * Wo, ptr(mean), ptr(rstd),
         ptr(bn_out.running_mean), ptr(bn_out.running_var), ptr(bn_out.num_batches_tracked),
         float(bn_out.momentum), float(bn_out.eps), int(bn_updates), ptr(ws), nbytes, stream())
    return y, mean, rstd


def dwconv_fused_bwd(dy, x, act, w, dw_sink, F, H, W, C, stride, need_dx=True):
    """dx = dL/d act(x), dw_sink += dL/dw for y = dwconv3x3(act(x)) (bf16)."""
    _chk(dy, x)
    dx = torch.empty_like(x) if need_dx else None
    nbytes = query("sm_dwconv_fused_bwd_workspace_bytes", F, H, W, C, stride)
    ws = _ws(nbytes, x.device)
    a = _act_args(act)
    call("sm_dwconv_fused_bwd", F, H, W, C, stride, ptr(dy), ptr(x), a[0], a[1], a[2], a[3], a[4], ptr(w), ptr(dx),
         ptr(dw_sink), ptr(ws), nbytes, stream())
    return dx


def dwconv_bn_bwd(dy, x, act, w, dw_sink, dg_sink, db_sink, F, H, W, C, stride=1):
    """y = dwconv3x3(act(x), stride 1 or 2), act = GELU(BN(x)) with batch statistics
    (act = (mean, rstd, gamma, beta, gelu)): returns dL/dx; dw_sink, dg_sink, db_sink
    += dL/dw, dL/dgamma, dL/dbeta (bf16).  F, H, W, C: the input's."""
    _chk(dy, x)
    dx = torch.empty_like(x)
    nbytes = query("sm_dwconv_bn_bwd_workspace_bytes", F, H, W, C)
    ws = _ws(nbytes, x.device)
    a = _act_args(act)
    call("sm_dwconv_bn_bwd", int(stride), F, H, W, C, ptr(dy), ptr(x), a[0], a[1], a[2], a[3], a[4], ptr(w), ptr(dx),
         ptr(dw_sink), ptr(dg_sink), ptr(db_sink), ptr(ws), nbytes, stream())
    return dx


def dwconv_bn_bwd_dz(dy, x, act, w, dw_sink, dg_sink, db_sink, F, H, W, C, stride=1):
    """dwconv_bn_bwd without its streaming dx pass (sm_dwconv_bn_bwd_dz): returns (dz, coef) with
    dz = g GELU'(BN(x)) [F*H*W, C] bf16 and coef [2, C] = mean(dz), mean(dz xhat); the sinks
    as dwconv_bn_bwd.  The BatchNorm's dx map is folded into the consumers (mbconv_fold_*)."""
    _chk(dy, x)
    dz = torch.empty_like(x)
    coef = torch.empty((2, C), dtype=torch.float32, device=x.device)
    nbytes = query("sm_dwconv_bn_bwd_workspace_bytes", F, H, W, C)
    ws = _ws(nbytes, x.device)
    a = _act_args(act)
    call("sm_dwconv_bn_bwd_dz", int(stride), F, H, W, C, ptr(dy), ptr(x), a[0], a[1], a[2], a[3], a[4], ptr(w),
         ptr(dz), ptr(dw_sink), ptr(dg_sink), ptr(db_sink), ptr(coef), ptr(ws), nbytes, stream())
    return dz, coef


def _xbn_args(xbn):
    return [None] * 4 if xbn is None else [ptr(t) for t in xbn[:4]]


def mbconv_fold_prep(coef, mean, rstd, gamma, w, xbn=None):
    """BN0's backward folded into the expand conv's gradient weights (sm_mbconv_fold_prep):
    returns (wst [mid + Cin, Cin] bf16 = [diag(omega) w; -w^T diag(delta) w], r0 [Cin] = c^T w,
    vec [3, mid] = omega, delta, c) from coef [2, mid], BN0's (mean, rstd, gamma) and the bf16
    expand weight w [mid, Cin].  xbn = (mean, rstd, weight, bias): the block input is the
    BatchNorm of a stored tensor; its affine goes into -T and r0 (the GEMM reads the stored one)."""
    _chk(coef, mean, rstd, gamma, w)
    mid, Cin = w.shape
    if w.dtype != torch.bfloat16 or not w.is_contiguous() or tuple(coef.shape) != (2, mid):
        raise _lib.KernelError("mbconv_fold_prep: contiguous bf16 w [mid, Cin], coef [2, mid]")
    wst = torch.empty((mid + Cin, Cin), dtype=torch.bfloat16, device=w.device)
    r0 = torch.empty(Cin, dtype=torch.float32, device=w.device)
    vec = torch.empty((3, mid), dtype=torch.float32, device=w.device)
    call("sm_mbconv_fold_prep", mid, Cin, ptr(coef), ptr(mean), ptr(rstd), ptr(gamma), ptr(w), *_xbn_args(xbn),
         ptr(wst), ptr(r0), ptr(vec), stream())
    return wst, r0, vec


def mbconv_fold_dw(vec, w, P, G, s, M, grad_sink, xbn=None):
    """grad_sink [mid, Cin] += diag(omega) P - diag(delta) (w G) + c s^T (sm_mbconv_fold_dw; fp64):
    the expand weight gradient from P = dz^T x, G = x^T x, s = column sums of x over M rows
    (xbn: G and s are the stored input's, P the BatchNorm output's)."""
    _chk(vec, w, P, G, s, grad_sink)
    mid, Cin = w.shape
    if (tuple(P.shape) != (mid, Cin) or tuple(G.shape) != (Cin, Cin) or s.numel() != Cin
            or tuple(grad_sink.shape) != (mid, Cin) or tuple(vec.shape) != (3, mid) or w.dtype != torch.bfloat16):
        raise _lib.KernelError("mbconv_fold_dw: shape mismatch")
    call("sm_mbconv_fold_dw", mid, Cin, int(M), ptr(vec), ptr(w), ptr(P), ptr(G), ptr(s), *_xbn_args(xbn),
         ptr(grad_sink), stream())
    return grad_sink


def linear_dx2(a1, a2, w, bias=None, residual=None):
    """dx [M, N] = [a1 | a2] @ w (+ bias) (+ residual) without the concatenation (sm_linear_dx2):
    a1 [M, K1], a2 [M, K2] bf16 with unit column stride (row strides free), w [K1 + K2, N];
    K1 % 64 == 0."""
    _chk(a1, a2, w, bias, residual)
    M, K1 = a1.shape
    K2 = a2.shape[1]
    N = w.shape[1]
    if (a2.shape[0] != M or w.shape[0] != K1 + K2 or a1.stride(1) != 1 or a2.stride(1) != 1 or not w.is_contiguous()
            or any(t.dtype != torch.bfloat16 for t in (a1, a2, w))
            or (residual is not None and (tuple(residual.shape) != (M, N) or residual.dtype != torch.bfloat16
                                          or not residual.is_contiguous()))):
        raise _lib.KernelError("linear_dx2: bf16 a1 [M,K1], a2 [M,K2], w [K1+K2,N], residual [M,N]")
    dx = torch.empty((M, N), dtype=torch.bfloat16, device=a1.device)
    call("sm_linear_dx2", M, N, K1, K2, ptr(a1), a1.stride(0), ptr(a2), a2.stride(0), ptr(w), ptr(bias),
         ptr(residual), ptr(dx), stream())
    return dx


def se_fwd(x, F, HW, C, w1, w2, act=None, want_y=True):
    """SELayer on h = act(x): returns (y = h * gate, pooled, relu(z1), gate)."""
    R = w1.shape[0]
    dev = x.device
    pooled = torch.empty((F, C), dtype=torch.float32, device=dev)
    h1 = torch.empty((F, R), dtype=torch.float32, device=dev)
    s = torch.empty((F, C), dtype=torch.float32, device=dev)
    y = torch.empty_like(x) if want_y else None
    nbytes = query("sm_se_workspace_bytes", F, HW, C)
    ws = _ws(nbytes, dev)
    call("sm_se_fwd", dt(x), ptr(x), *_act_args(act), F, HW, C, R, ptr(w1), ptr(w2), ptr(pooled), ptr(h1), ptr(s),
         ptr(y), ptr(ws), nbytes, stream())
    return y, pooled, h1, s


def se_scale(x, s, F, HW, C, act=None):
    y = torch.empty_like(x)
    call("sm_se_scale", dt(x), ptr(x), *_act_args(act), ptr(s), ptr(y), F, HW, C, stream())
    return y


def se_bwd(dy, x, F, HW, C, w1, w2, s, h1, act=None):
    R = w1.shape[0]
    dev = x.device
    dz2 = torch.empty((F, C), dtype=torch.float32, device=dev)
    dz1 = torch.empty((F, R), dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    nbytes = query("sm_se_workspace_bytes", F, HW, C)
    ws = _ws(nbytes, dev)
    call("sm_se_bwd", dt(x), ptr(dy), ptr(x), *_act_args(act), F, HW, C, R, ptr(w1), ptr(w2), ptr(s), ptr(h1),
         ptr(dz2), ptr(dz1), ptr(dx), ptr(ws), nbytes, stream())
    return dx, dz2, dz1


def se_bn_bwd(dy, x, F, HW, C, w1, w2, s, h1, act, dw_sink, db_sink):
    """Fused backward of y = SE(GELU(BN(x))) with BN's batch statistics act = (mean,
    rstd, w, b, gelu): returns (dx, dz2, dz1) as se_bwd followed by bn_bwd on its dx;
    dw_sink / db_sink accumulate BN's weight / bias gradients."""
    _chk(dy, x)
    R = w1.shape[0]
    dev = x.device
    dz2 = torch.empty((F, C), dtype=torch.float32, device=dev)
    dz1 = torch.empty((F, R), dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    nbytes = query("sm_se_bn_bwd_workspace_bytes", F, HW, C)
    ws = _ws(nbytes, dev)
    call("sm_se_bn_bwd", dt(x), ptr(dy), ptr(x), *_act_args(act), F, HW, C, R, ptr(w1), ptr(w2), ptr(s), ptr(h1),
         ptr(dz2), ptr(dz1), ptr(dx), ptr(dw_sink), ptr(db_sink), ptr(ws), nbytes, stream())
    return dx, dz2, dz1


# ------------------------------------------------------------------ MAE glue
def tube_mask(noise, T, n_mask, with_index=True):
    """noise [B,L] fp32 (device) -> mask uint8 [B,T,L], idx int32 [B*T*n_mask]."""
    _chk(noise)
    B, L = noise.shape
    mask = torch.empty((B, T, L), dtype=torch.uint8, device=noise.device)
    idx = torch.empty((B * T * n_mask,), dtype=torch.int32, device=noise.device) if with_index else None
    call("sm_tube_mask", ptr(noise), B, T, L, n_mask, ptr(mask), ptr(idx), stream())
    return mask, idx


def pos_blend(y, tpos, spos, tok, mask_u8, B, T, L, D, out_dtype):
    x = torch.empty((B * T * L, D), dtype=out_dtype, device=y.device)
    call("sm_pos_blend_fwd", dt(y), dt(x), ptr(y), ptr(tpos), ptr(spos), ptr(tok), ptr(mask_u8), ptr(x), B, T, L, D,
         stream())
    return x


def pos_blend_bwd(dx, mask_u8, y_dtype, dtpos, dspos, dtok, B, T, L, D):
    dy = torch.empty(dx.shape, dtype=y_dtype, device=dx.device)
    ws = torch.empty((2, B * T, D), dtype=torch.float32, device=dx.device)
    call("sm_pos_blend_bwd", dt(dx), dt(dy), ptr(dx), ptr(mask_u8), ptr(dy), ptr(dtpos), ptr(dspos), ptr(dtok),
         ptr(ws), B, T, L, D, stream())
    return dy


def _clip_args(clip):
    B, C, T, H, W = clip.shape
    return (B, T, H, W) + tuple(clip.stride())


def mae_loss_fwd(pred, clip, mask_u8, norm_pix=True):
    _chk(pred, clip, mask_u8)
    B, T, H, W, sB, sC, sT, sH, sW = _clip_args(clip)
    L = (H // 8) * (W // 8)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    denom = torch.empty((1,), dtype=torch.float32, device=pred.device)
    nbytes = query("sm_loss_workspace_bytes", B, T, L)
    ws = _ws(nbytes, pred.device)
    call("sm_mae_loss_fwd", dt(pred), ptr(pred), ptr(clip), sB, sC, sT, sH, sW, ptr(mask_u8), B, T, H, W,
         1 if norm_pix else 0, ptr(loss), ptr(denom), ptr(ws), nbytes, stream())
    return loss, denom


def mae_loss_bwd(pred, clip, mask_u8, norm_pix, grad_out, denom):
    B, T, H, W, sB, sC, sT, sH, sW = _clip_args(clip)
    dpred = torch.empty_like(pred)
    g = grad_out.reshape(1).float().contiguous()
    call("sm_mae_loss_bwd", dt(pred), ptr(pred), ptr(clip), sB, sC, sT, sH, sW, ptr(mask_u8), B, T, H, W,
         1 if norm_pix else 0, ptr(g), ptr(denom), ptr(dpred), stream())
    return dpred


def patchify(imgs, p=8):
    _chk(imgs)
    x = imgs if imgs.dtype == torch.float32 else imgs.float()
    B, C, T, H, W = x.shape
    out = torch.empty((B, T * (H // p) * (W // p), p * p * C), dtype=torch.float32, device=x.device)
    call("sm_patchify", ptr(x), B, C, T, H, W, *x.stride(), p, ptr(out), stream())
    return out


def unpatchify(tokens, C, T, H, W, p=8):
    _chk(tokens)
    t = tokens.contiguous().float()
    B = t.shape[0]
    out = torch.empty((B, C, T, H, W), dtype=torch.float32, device=t.device)
    call("sm_unpatchify", ptr(t), B, C, T, H, W, p, ptr(out), stream())
    return out


def scale_(t, a):
    call("sm_scale", ptr(t), t.numel(), float(a), stream())
    return t


def gather_rows(src2d, idx):
    out = torch.empty((idx.numel(), src2d.shape[1]), dtype=src2d.dtype, device=src2d.device)
    call("sm_gather_rows", dt(src2d), ptr(src2d), ptr(idx), idx.numel(), src2d.shape[1], ptr(out), stream())
    return out


def std(x):
    out = torch.empty((), dtype=torch.float32, device=x.device)
    nbytes = query("sm_std_workspace_bytes")
    ws = _ws(nbytes, x.device)
    call("sm_std", dt(x), ptr(x), x.numel(), ptr(out), ptr(ws), nbytes, stream())
    return out


# ------------------------------------------------------------------ fine-tune head pooling
def segment_mean(x, G, R, C):
    """x [G*R, C] (or [G, R, C]) -> fp32 [G, C], mean over the R rows of each segment."""
    _chk(x)
    if not x.is_contiguous() or x.numel() != G * R * C:
        raise _lib.KernelError("segment_mean needs a contiguous [G][R][C] tensor")
    out = torch.empty((G, C), dtype=torch.float32, device=x.device)
    call("sm_segment_mean", dt(x), ptr(x), G, R, C, ptr(out), stream())
    return out


def segment_mean_bwd(dy, G, R, C, dtype):
    _chk(dy)
    if dy.dtype != torch.float32 or not dy.is_contiguous():
        raise _lib.KernelError("segment_mean_bwd takes the fp32 [G][C] gradient of segment_mean")
    dx = torch.empty((G * R, C), dtype=dtype, device=dy.device)
    call("sm_segment_mean_bwd", dt(dx), ptr(dy), G, R, C, ptr(dx), stream())
    return dx


# ------------------------------------------------------------------ optimizer
def nonfinite(g, flag):
    call("sm_nonfinite", ptr(g), g.numel(), ptr(flag), stream())


def adamw(p, g, m, v, lr, b1, b2, eps, wd, found_inf, step, shadow=None, advance_step=True):
    call("sm_adamw", ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), p.numel(), float(lr), float(b1), float(b2),
         float(eps), float(wd), ptr(found_inf), ptr(step), 1 if advance_step else 0, stream())


ADAMW_MAX_GROUPS = 64                        # SM_ADAMW_MAX_GROUPS
ADAMW_CHUNK_ELEMS = 2048                     # SM_ADAMW_CHUNK_ELEMS
ADAMW_TABLE_MAGIC = 0x314254574D414441       # SM_ADAMW_TABLE_MAGIC


def adamw_table_bytes(num_segments, num_chunks):
    return (64 + 44 * num_segments + 12 * num_chunks + 15) // 16 * 16


def adamw_table_layout(addrs, lens, groups):
    """The bytes of sm_adamw_table's segment table (include/sm_api.h "AdamW segment table") as
    a uint8 NumPy array; pure host code.  addrs: per segment the (p, g, m, v) device addresses;
    lens: elements per segment; groups: the parameter group of each segment."""
    import numpy as np
    S = len(lens)
    if len(addrs) != S or len(groups) != S:
        raise _lib.KernelError(f"adamw_table_layout: {len(addrs)} address rows, {S} lengths, {len(groups)} groups")
    addr = np.array([tuple(int(x) for x in a) for a in addrs], dtype=np.uint64).reshape(S, 4)
    seg_len = np.array([int(n) for n in lens], dtype=np.int64).reshape(S)
    seg_group = np.array([int(g) for g in groups], dtype=np.int64).reshape(S)
    if (seg_len < 0).any():
        raise _lib.KernelError("adamw_table_layout: a segment length is negative")
    if (seg_group < 0).any() or (seg_group >= ADAMW_MAX_GROUPS).any():
        raise _lib.KernelError(f"adamw_table_layout: group indices are 0..{ADAMW_MAX_GROUPS - 1}")
    if (addr % 4 != 0).any() or (addr[seg_len > 0] == 0).any():
        raise _lib.KernelError("adamw_table_layout: every segment address is a non-null multiple of 4")
    n_chunks = (seg_len + ADAMW_CHUNK_ELEMS - 1) // ADAMW_CHUNK_ELEMS
    chunk_seg = np.repeat(np.arange(S, dtype=np.int32), n_chunks)
    first_chunk = np.cumsum(n_chunks) - n_chunks
    chunk_off = (np.arange(len(chunk_seg), dtype=np.int64) - np.repeat(first_chunk, n_chunks)) * ADAMW_CHUNK_ELEMS
    C = len(chunk_seg)
    total = adamw_table_bytes(S, C)
    header = np.array([ADAMW_TABLE_MAGIC, S, C, ADAMW_CHUNK_ELEMS, total, 0, 0, 0], dtype=np.int64)
    raw = b"".join(a.tobytes() for a in (header, np.ascontiguousarray(addr.T), seg_len, chunk_off.astype(np.int64),
                                         chunk_seg.astype(np.int32), seg_group.astype(np.int32)))
    raw += b"\0" * (total - len(raw))
    return np.frombuffer(raw, dtype=np.uint8)


def adamw_table_counts(layout):
    """(num_segments, num_chunks) of a table's bytes, after checking its header against the
    documented formula -- the validation the per-step call relies on."""
    import numpy as np
    raw = np.asarray(layout, dtype=np.uint8)
    if raw.size < 64:
        raise _lib.KernelError("adamw table: shorter than its header")
    magic, S, C, chunk, total = (int(x) for x in np.frombuffer(raw[:40].tobytes(), dtype=np.int64))
    if magic != ADAMW_TABLE_MAGIC or chunk != ADAMW_CHUNK_ELEMS or S < 0 or C < 0 \
            or total != adamw_table_bytes(S, C) or total != raw.size:
        raise _lib.KernelError("adamw table: the header does not describe these bytes")
    return S, C


def adamw_table(addrs, lens, groups, device):
    """Builds and uploads the segment table: (uint8 device tensor, num_segments, num_chunks)."""
    layout = adamw_table_layout(addrs, lens, groups)
    S, C = adamw_table_counts(layout)
    table = torch.from_numpy(layout.copy()).to(device)
    if table.data_ptr() % 16:
        raise _lib.KernelError("adamw_table: the device allocation is not 16-byte aligned")
    return table, S, C


def adamw_table_step(table, num_segments, num_chunks, lr, wd, lr_mult, b1, b2, eps, found_inf, step,
                     check_finite=True):
    """One optimizer step over every segment of the table: segment s with lr[group[s]] * lr_mult
    and wd[group[s]].  At most three stream operations, no host synchronisation."""
    import ctypes
    _chk(table, found_inf, step)
    if table.dtype != torch.uint8 or not table.is_contiguous():
        raise _lib.KernelError("adamw_table_step: the table is a contiguous uint8 device tensor (adamw_table)")
    if len(lr) != len(wd):
        raise _lib.KernelError(f"adamw_table_step: {len(lr)} learning rates but {len(wd)} weight decays")
    n = len(lr)
    lrs = (ctypes.c_float * max(1, n))(*[float(x) for x in lr])
    wds = (ctypes.c_float * max(1, n))(*[float(x) for x in wd])
    call("sm_adamw_table", ptr(table), table.numel(), int(num_segments), int(num_chunks), n,
         ctypes.cast(lrs, ctypes.c_void_p), ctypes.cast(wds, ctypes.c_void_p), float(lr_mult), float(b1), float(b2),
         float(eps), ptr(found_inf), ptr(step), 1 if check_finite else 0, stream())


# ------------------------------------------------------------------ federated averaging
def fedavg_weighted_sum(bufs, weights, out=None):
    """out = sum_j bufs[j] * weights[j] in client order (fed_loop.py:46-49), bit-exact.
    bufs: equal-length contiguous fp32 device tensors; weights: fp32-representable floats."""
    import ctypes
    if not bufs:
        raise _lib.KernelError("fedavg_weighted_sum needs at least one client buffer")
    _chk(*bufs)
    if len(weights) != len(bufs):
        raise _lib.KernelError(f"fedavg_weighted_sum: {len(bufs)} client buffers but {len(weights)} weights")
    n = bufs[0].numel()
    for b in bufs:
        if b.dtype != torch.float32 or b.numel() != n or not b.is_contiguous() or b.device != bufs[0].device:
            raise _lib.KernelError("fedavg client buffers must be contiguous fp32 of one length on one device")
    if out is None:
        out = torch.empty_like(bufs[0])
    k = len(bufs)
    ptrs = (ctypes.c_void_p * k)(*[b.data_ptr() for b in bufs])
    ws = (ctypes.c_float * k)(*[float(w) for w in weights])
    call("sm_fedavg_weighted_sum", k, ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(ws, ctypes.c_void_p), n,
         ptr(out), stream())
    return out


def fedavg_counters_max(bufs, out=None):
    """out = elementwise max over clients of int64 counters (fed_loop.py:52-55)."""
    import ctypes
    if not bufs:
        raise _lib.KernelError("fedavg_counters_max needs at least one client buffer")
    _chk(*bufs)
    n = bufs[0].numel()
    for b in bufs:
        if b.dtype != torch.int64 or b.numel() != n or not b.is_contiguous() or b.device != bufs[0].device:
            raise _lib.KernelError("fedavg counters must be contiguous int64 of one length on one device")
    if out is None:
        out = torch.empty_like(bufs[0])
    k = len(bufs)
    ptrs = (ctypes.c_void_p * k)(*[b.data_ptr() for b in bufs])
    call("sm_fedavg_counters_max", k, ctypes.cast(ptrs, ctypes.c_void_p), n, ptr(out), stream())
    return out


FEDAVG_MAX_CLIENTS = 32
FEDAVG_CHUNK_ELEMS = 2048                    # SM_FEDAVG_CHUNK_ELEMS
_FEDAVG_TABLE_MAGIC = 0x31424154444546      # SM_FEDAVG_TABLE_MAGIC


def fedavg_exchange_table(models, dtype):
    """The device table of sm_fedavg_exchange (dtype fp32) / sm_fedavg_exchange_counters (int64)
    for a cohort: `models` is P lists of S tensors, segment s laid out identically in every
    model.  Returns (uint8 device tensor, host list of the P*S addresses); the layout is
    documented in include/sm_api.h."""
    import numpy as np
    P = len(models)
    if P < 1 or P > FEDAVG_MAX_CLIENTS + 1:
        raise _lib.KernelError(f"fedavg_exchange_table: {P} models, 1..{FEDAVG_MAX_CLIENTS + 1} supported")
    S = len(models[0])
    if dtype not in (torch.float32, torch.int64):
        raise _lib.KernelError("fedavg_exchange_table: fp32 or int64 segments")
    first = next((t for m in models for t in m), None)
    device = first.device if first is not None else torch.device("cuda", torch.cuda.current_device())
    for m in models:
        if len(m) != S:
            raise _lib.KernelError("fedavg_exchange_table: every model needs the same segments")
        _chk(*m)
        for t, t0 in zip(m, models[0]):
            if t.dtype != dtype or t.shape != t0.shape or not t.is_contiguous() or t.device != device:
                raise _lib.KernelError("fedavg_exchange_table: a segment must be contiguous, of the table's dtype "
                                       "and of one shape on one device in every model")
    seg_len = np.array([t.numel() for t in models[0]], dtype=np.int64)
    n_chunks = (seg_len + FEDAVG_CHUNK_ELEMS - 1) // FEDAVG_CHUNK_ELEMS
    chunk_seg = np.repeat(np.arange(S, dtype=np.int32), n_chunks)
    first_chunk = np.cumsum(n_chunks) - n_chunks
    chunk_off = (np.arange(len(chunk_seg), dtype=np.int64) - np.repeat(first_chunk, n_chunks)) * FEDAVG_CHUNK_ELEMS
    addr = np.array([t.data_ptr() for m in models for t in m], dtype=np.uint64)
    C = len(chunk_seg)
    total = (64 + 8 * P * S + 8 * S + 12 * C + 15) // 16 * 16
    elem = 4 if dtype == torch.float32 else 8
    header = np.array([_FEDAVG_TABLE_MAGIC, P, S, C, elem, FEDAVG_CHUNK_ELEMS, total, 0], dtype=np.int64)
    raw = b"".join(a.tobytes() for a in (header, addr, seg_len, chunk_off.astype(np.int64), chunk_seg))
    raw += b"\0" * (total - len(raw))
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    return table, addr.tolist()


def _fedavg_exchange_call(name, src_models, weights, dst_models, table, extra, global_model=None):
    """What the exchange entry points share: the table check, the source / weight count check and
    the leading arguments (sources, weights if any, the global model if any, destinations, table);
    `extra` is the entry point's own trailing arguments."""
    import ctypes
    _chk(table)
    if table.dtype != torch.uint8 or not table.is_contiguous():
        raise _lib.KernelError(f"{name}: the table is a contiguous uint8 device tensor (fedavg_exchange_table)")
    if weights is not None and len(weights) != len(src_models):
        raise _lib.KernelError(f"{name}: {len(src_models)} sources but {len(weights)} weights")
    src = (ctypes.c_int32 * max(1, len(src_models)))(*[int(i) for i in src_models])
    dst = (ctypes.c_int32 * max(1, len(dst_models)))(*[int(i) for i in dst_models])
    args = [len(src_models), ctypes.cast(src, ctypes.c_void_p)]
    if weights is not None:
        ws = (ctypes.c_float * max(1, len(weights)))(*[float(w) for w in weights])
        args.append(ctypes.cast(ws, ctypes.c_void_p))
    if global_model is not None:
        args.append(int(global_model))
    args += [len(dst_models), ctypes.cast(dst, ctypes.c_void_p), ptr(table), table.numel()] + extra + [stream()]
    call("sm_" + name, *args)


def fedavg_exchange(src_models, weights, dst_models, table, copy_only=False):
    """One launch over an fp32 cohort table: the weighted sum of the source models' segments in
    source order (fedavg_weighted_sum's arithmetic, bit for bit) -- or, with copy_only, the one
    source's bits -- written into every destination model's segments, which may be sources too."""
    if copy_only:
        weights = [1.0] * len(src_models)
    _fedavg_exchange_call("fedavg_exchange", src_models, weights, dst_models, table, [1 if copy_only else 0])


def fedavg_exchange_counters(src_models, dst_models, table):
    """The int64 max over the source models' segments into every destination model's."""
    _fedavg_exchange_call("fedavg_exchange_counters", src_models, None, dst_models, table, [])


def fedavg_dp_exchange(src_models, weights, global_model, dst_models, table, num_chunks, seg_clip, clip_norm,
                       noise_std, seed, stats=None, ws=None):
    """DP-FedAvg over an fp32 cohort table (sm_fedavg_dp_exchange, include/sm_api.h): the sources'
    updates against model `global_model`, clipped to `clip_norm` over the segments whose `seg_clip`
    byte is 1, averaged with the normalised `weights` onto it, plus noise_std x the counter Gaussian
    of (seed, segment, element); segments with byte 0 get the plain weighted sum.  The result goes
    into every destination model.  `num_chunks` is the table's chunk count (it sizes the
    workspace); seg_clip is a uint8 device tensor with one byte per segment of the table.
    -> stats, fp32 [2 * sources] on the device: the update norms, then the clip scales."""
    _chk(table, seg_clip, stats, ws)
    if seg_clip is not None and (seg_clip.dtype != torch.uint8 or not seg_clip.is_contiguous()):
        raise _lib.KernelError("fedavg_dp_exchange: seg_clip is a contiguous uint8 device tensor")
    k = len(src_models)
    if stats is None:
        stats = torch.empty(2 * max(k, 1), dtype=torch.float32, device=table.device)
    elif stats.dtype != torch.float32 or stats.numel() != 2 * k or not stats.is_contiguous():
        raise _lib.KernelError("fedavg_dp_exchange: stats must be contiguous fp32 [2 * sources]")
    if ws is None:
        ws = _ws(max(query("sm_fedavg_dp_exchange_workspace_bytes", k, int(num_chunks)), 0), table.device)
    _fedavg_exchange_call("fedavg_dp_exchange", src_models, weights, dst_models, table,
                          [ptr(seg_clip), float(clip_norm), float(noise_std), int(seed) & ((1 << 64) - 1), ptr(stats),
                           ptr(ws), ws.numel()], global_model=global_model)
    return stats


FEDAVG_Q8_BLOCK = 256                        # SM_FEDAVG_Q8_BLOCK


def fedavg_q8_exchange(src_models, weights, global_model, dst_models, table, num_chunks, seg_mode, resid,
                       codes=None, scales=None, part=None):
    """Compressed FedAvg over an fp32 cohort table (sm_fedavg_q8_exchange, include/sm_api.h): over
    the segments whose `seg_mode` byte is 1 every source's update against model `global_model`, plus
    its residual row, is quantised to int8 with one fp32 scale per 256-element block, the
    dequantised updates are averaged with the normalised `weights` onto the global model and the
    quantisation errors go back into `resid` (fp32 [rows, num_chunks * 2048], row = model index - 1);
    segments with byte 0 get the plain weighted sum.  The result goes into every destination model.
    codes (int8 [sources, num_chunks, 2048]) and scales (fp32 [sources, num_chunks, 8]) receive what
    the clients upload when both are given.
    -> part, fp64 [sources, num_chunks, 2] on the device: per chunk, max |v| and the sum of squares
    of the new residual."""
    _chk(table, seg_mode, resid, codes, scales, part)
    name = "fedavg_q8_exchange"
    if seg_mode is not None and (seg_mode.dtype != torch.uint8 or not seg_mode.is_contiguous()):
        raise _lib.KernelError(f"{name}: seg_mode is a contiguous uint8 device tensor")
    k, C = len(src_models), int(num_chunks)
    rows = 0
    if resid is not None:
        if (resid.dtype != torch.float32 or resid.dim() != 2 or resid.shape[1] != C * FEDAVG_CHUNK_ELEMS
                or not resid.is_contiguous()):
            raise _lib.KernelError(f"{name}: resid must be contiguous fp32 [rows, {C * FEDAVG_CHUNK_ELEMS}]")
        rows = resid.shape[0]
    if codes is not None and (codes.dtype != torch.int8 or codes.numel() != k * C * FEDAVG_CHUNK_ELEMS
                              or not codes.is_contiguous()):
        raise _lib.KernelError(f"{name}: codes must be contiguous int8 [{k}, {C}, {FEDAVG_CHUNK_ELEMS}]")
    n_scales = k * C * (FEDAVG_CHUNK_ELEMS // FEDAVG_Q8_BLOCK)
    if scales is not None and (scales.dtype != torch.float32 or scales.numel() != n_scales
                               or not scales.is_contiguous()):
        raise _lib.KernelError(f"{name}: scales must be contiguous fp32 [{k}, {C}, "
                               f"{FEDAVG_CHUNK_ELEMS // FEDAVG_Q8_BLOCK}]")
    if part is None:
        part = torch.empty((max(k, 1), C, 2), dtype=torch.float64, device=table.device)
    elif part.dtype != torch.float64 or part.numel() != 2 * k * C or not part.is_contiguous():
        raise _lib.KernelError(f"{name}: part must be contiguous fp64 [{k}, {C}, 2]")
    _fedavg_exchange_call(name, src_models, weights, dst_models, table,
                          [ptr(seg_mode), ptr(resid), int(rows), ptr(codes), ptr(scales), ptr(part)],
                          global_model=global_model)
    return part


# ------------------------------------------------------------------ clip input pipeline
def frames_normalize(frames, mean, std, bgr_swap=True, valid=None, out=None):
    """uint8 [B,T,H,W,3] decoded frames -> fp32 [B,3,T,H,W] normalised clip
    (train_ssl_mae.py:137-141 transform + mae_loader.py:70-77 BGR swap / permute)."""
    import ctypes
    _chk(frames, valid)
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise _lib.KernelError("frames must be contiguous uint8 [B,T,H,W,3]")
    B, T, H, W, _ = frames.shape
    if valid is not None and (valid.dtype not in (torch.uint8, torch.bool) or valid.numel() != B):
        raise _lib.KernelError("valid must be uint8/bool [B]")
    if out is None:
        out = torch.empty((B, 3, T, H, W), dtype=torch.float32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s = (ctypes.c_float * 3)(*[float(x) for x in std])
    call("sm_frames_normalize", ptr(frames), ptr(valid), B, T, H, W, ctypes.cast(m, ctypes.c_void_p),
         ctypes.cast(s, ctypes.c_void_p), 1 if bgr_swap else 0, ptr(out), stream())
    return out


def _frames_resize(symbol, cols, packed, desc, T, out_hw, mean, std, bgr_swap, out):
    import ctypes
    name = symbol[3:]
    _chk(packed, desc)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.KernelError("packed must be a contiguous 1-D uint8 tensor")
    if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != cols or not desc.is_contiguous():
        raise _lib.KernelError(f"desc must be a contiguous int64 [B,{cols}] tensor")
    if desc.device != packed.device:
        raise _lib.KernelError("packed and desc must be on one device")
    B, T = desc.shape[0], int(T)
    Ho, Wo = (int(x) for x in out_hw)
    if T < 0 or not (0 <= Ho <= 4096 and 0 <= Wo <= 4096):
        raise _lib.KernelError(f"{name} needs T >= 0 and an output size within [0, 4096]")
    if out is None:
        out = torch.empty((B, 3, T, Ho, Wo), dtype=torch.float32, device=packed.device)
    else:
        _chk(out)
        if out.dtype != torch.float32 or tuple(out.shape) != (B, 3, T, Ho, Wo) or not out.is_contiguous():
            raise _lib.KernelError(f"out must be contiguous fp32 [{B},3,{T},{Ho},{Wo}]")
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s = (ctypes.c_float * 3)(*[float(x) for x in std])
    call(symbol, ptr(packed), ptr(desc), packed.numel(), B, T, Ho, Wo, ctypes.cast(m, ctypes.c_void_p),
         ctypes.cast(s, ctypes.c_void_p), 1 if bgr_swap else 0, ptr(out), stream())
    return out


def frames_resize_normalize(packed, desc, T, out_hw, mean, std, bgr_swap=True, out=None):
    """packed uint8 (1-D; clip b = [T,Hs_b,Ws_b,3] RGB at byte desc[b,0]) + desc int64 [B,4]
    {byte offset, Hs, Ws, flags (1 = flip, 2 = invalid)} -> fp32 [B,3,T,Ho,Wo]: bilinear resize
    (align_corners=False), clip-level horizontal flip and normalisation in one launch
    (mae_dataset.py:84-90, :129-133).  A clip whose range leaves `packed`, or whose size is
    outside [1, 8192], comes back as zeros."""
    return _frames_resize("sm_frames_resize_normalize", 4, packed, desc, T, out_hw, mean, std, bgr_swap, out)


def frames_crop_resize_normalize(packed, desc, T, out_hw, mean, std, bgr_swap=True, out=None):
    """frames_resize_normalize with a source window per clip: desc int64 [B,8] {byte offset, Hs,
    Ws, flags, y0, x0, Hc, Wc}.  The output is rows [y0, y0 + Hc) x columns [x0, x0 + Wc) of every
    frame resized to (Ho, Wo), bit for bit what frames_resize_normalize gives on a buffer that
    holds only the window; the flip is within the window.  A window that leaves its frame or is
    empty gives a zero clip, as every descriptor does that frames_resize_normalize rejects."""
    return _frames_resize("sm_frames_crop_resize_normalize", 8, packed, desc, T, out_hw, mean, std, bgr_swap, out)


# ------------------------------------------------------------------ Mixup / CutMix (csrc/mix.hip)
MIX_MAX_PAIRS = 65535     # one grid row per pair


def mix_boxes_check(boxes, H, W):
    """Host rows (y0, x0, h, w): every box must lie inside the H x W frame and have no negative
    side (an empty box, h == 0 or w == 0, is fine anywhere inside)."""
    for p, (y0, x0, h, w) in enumerate(boxes):
        if y0 < 0 or x0 < 0 or h < 0 or w < 0 or y0 + h > H or x0 + w > W:
            raise _lib.KernelError(f"clip_mix: pair {p}: box rows [{y0}, {y0 + h}) x columns [{x0}, {x0 + w}) has a "
                                   f"negative side or leaves the {H}x{W} frame")


def clip_mix(x, lam_px, box, out=None):
    """x fp32 [B, ..., H, W] (contiguous; a [B,3,T,H,W] clip batch) -> the batch mixed with its own
    flip, clip b with clip B-1-b, in one launch (sm_clip_mix, include/sm_api.h): inside pair p's box
    (y0, x0, h, w), on every plane, the partner's pixel; outside it the clip's own pixel when
    lam_px[p] == 1 and lam_px[p] * own + (1 - lam_px[p]) * partner otherwise.  lam_px fp32 [B//2],
    box int32 [B//2, 4].  Given as HOST tensors they are checked here (mix_boxes_check) and go up
    in one copy; given on the device they are used as they are, and the boxes are the CALLER's
    guarantee (they are not read back; mae_loader.ClipMixer checks its table before the upload).
    out=None allocates; out may be x itself (in place), no other overlap."""
    _chk(x, out)
    if x.dim() < 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.KernelError("clip_mix takes a contiguous fp32 [B, ..., H, W] tensor")
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    P = B // 2
    planes = x[0].numel() // max(H * W, 1) if B else 0
    if B and (H < 1 or W < 1 or planes < 1 or planes * H * W >= 2 ** 31 or P + B % 2 > MIX_MAX_PAIRS):
        raise _lib.KernelError(f"clip_mix: a clip needs 1 <= elements < 2^31 and the batch at most {MIX_MAX_PAIRS} pairs")
    if lam_px.dtype != torch.float32 or tuple(lam_px.shape) != (P,) or not lam_px.is_contiguous():
        raise _lib.KernelError(f"clip_mix: lam_px must be contiguous fp32 [{P}]")
    if box.dtype != torch.int32 or tuple(box.shape) != (P, 4) or not box.is_contiguous():
        raise _lib.KernelError(f"clip_mix: box must be contiguous int32 [{P},4]")
    if lam_px.device != box.device or (lam_px.is_cuda and lam_px.device != x.device):
        raise _lib.KernelError("clip_mix: lam_px and box must both be host tensors or both be on x's device")
    if not lam_px.is_cuda:
        mix_boxes_check(box.tolist(), H, W)
        table = torch.cat([box.reshape(-1), lam_px.view(torch.int32)]).to(x.device)     # one copy
        box, lam_px = table[:4 * P].view(P, 4), table[4 * P:].view(torch.float32)
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
        raise _lib.KernelError("clip_mix: out must be a contiguous fp32 tensor like x")
    elif out.data_ptr() != x.data_ptr() and abs(out.data_ptr() - x.data_ptr()) < 4 * x.numel():
        raise _lib.KernelError("clip_mix: out may be x itself, but must not overlap it otherwise")
    call("sm_clip_mix", ptr(x), B, planes, H, W, ptr(lam_px) if P else None, ptr(box) if P else None, ptr(out),
         stream())
    return out


# ------------------------------------------------------------------ visual privacy (csrc/anonymize.hip)
BOX_TILE_H, BOX_TILE_W = 32, 64      # SM_BOX_TILE_H / SM_BOX_TILE_W
BOX_MAX_SIDE = 8192
BOX_MAX_KSIZE = 63


def box_launch_max_frames(max_h, max_w):
    """The most frames one launch takes at these bounds: N x tiles <= 2^31 - 1 blocks."""
    tiles = -(-int(max_h) // BOX_TILE_H) * -(-int(max_w) // BOX_TILE_W)
    return (2 ** 31 - 1) // max(tiles, 1)


def _box_batch(name, bufs, desc, boxes, box_start, max_h, max_w):
    _chk(*bufs, desc, boxes, box_start)
    dev = bufs[0].device
    for t in bufs:
        if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous() or t.numel() != bufs[0].numel():
            raise _lib.KernelError(f"{name}: pixel buffers must be contiguous 1-D uint8 tensors of one length")
    if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 3 or not desc.is_contiguous():
        raise _lib.KernelError(f"{name}: desc must be a contiguous int64 [N,3] tensor")
    if boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 4 or not boxes.is_contiguous():
        raise _lib.KernelError(f"{name}: boxes must be a contiguous int32 [num_boxes,4] tensor")
    N = desc.shape[0]
    if box_start.dtype != torch.int32 or box_start.dim() != 1 or box_start.numel() != N + 1 \
            or not box_start.is_contiguous():
        raise _lib.KernelError(f"{name}: box_start must be a contiguous int32 [{N + 1}] tensor")
    if any(t.device != dev for t in (*bufs, desc, boxes, box_start)):
        raise _lib.KernelError(f"{name}: every tensor must be on one device")
    max_h, max_w = int(max_h), int(max_w)
    if not (1 <= max_h <= BOX_MAX_SIDE and 1 <= max_w <= BOX_MAX_SIDE):
        raise _lib.KernelError(f"{name}: max_h and max_w must lie in [1, {BOX_MAX_SIDE}]")
    if N > box_launch_max_frames(max_h, max_w):
        raise _lib.KernelError(f"{name}: {N} frames at {max_h}x{max_w} exceed one launch's "
                               f"{box_launch_max_frames(max_h, max_w)}")
    return N, max_h, max_w


def frames_box_blur(packed, desc, boxes, box_start, weights, max_h, max_w, out=None):
    """packed uint8 (1-D; frame n = [H_n,W_n,3] RGB at byte desc[n,0]) + desc int64 [N,3] {byte
    offset, H, W} + boxes int32 [num_boxes,4] {x, y, w, h} + box_start int32 [N+1] -> uint8 of the
    same layout: the pixels in the union of a frame's clipped boxes get the separable Gaussian
    `weights` (host floats, odd length in [3, 63]) of the original frame with reflect-101 edges,
    every other pixel keeps its bytes; one launch (include/sm_api.h).  A frame whose descriptor is
    out of range is not written (out=None: those bytes are zero)."""
    import ctypes
    name = "frames_box_blur"
    N, max_h, max_w = _box_batch(name, (packed,), desc, boxes, box_start, max_h, max_w)
    w = [float(x) for x in weights]
    if not (3 <= len(w) <= BOX_MAX_KSIZE) or len(w) % 2 == 0:
        raise _lib.KernelError(f"{name}: the kernel size must be odd and in [3, {BOX_MAX_KSIZE}], got {len(w)}")
    if out is None:
        out = torch.zeros_like(packed)
    else:
        _chk(out)
        if out.dtype != torch.uint8 or out.shape != packed.shape or not out.is_contiguous() \
                or out.device != packed.device:
            raise _lib.KernelError(f"{name}: out must be a contiguous uint8 tensor like packed")
        if abs(out.data_ptr() - packed.data_ptr()) < packed.numel():
            raise _lib.KernelError(f"{name}: out must not overlap packed (the blur reads the original frame)")
    wv = (ctypes.c_float * len(w))(*w)
    call("sm_frames_box_blur", ptr(packed), ptr(desc), packed.numel(), N, max_h, max_w, ptr(boxes), ptr(box_start),
         boxes.shape[0], ctypes.cast(wv, ctypes.c_void_p), len(w), ptr(out), stream())
    return out


def box_region_stats(a, b, desc, boxes, box_start, max_h, max_w, stats=None):
    """Two buffers of frames_box_blur's layout -> int64 [N,4] = {P, SSE, Ea, Eb} per frame over the
    union U of its clipped boxes: pixels in U, the sum of (a - b)^2 over U and the channels, and the
    squared right / down neighbour differences of a and of b at the pixels of U; exact integers,
    one memset and one launch (include/sm_api.h)."""
    name = "box_region_stats"
    N, max_h, max_w = _box_batch(name, (a, b), desc, boxes, box_start, max_h, max_w)
    if stats is None:
        stats = torch.zeros((N, 4), dtype=torch.int64, device=a.device)
    else:
        _chk(stats)
        if stats.dtype != torch.int64 or tuple(stats.shape) != (N, 4) or not stats.is_contiguous():
            raise _lib.KernelError(f"{name}: stats must be a contiguous int64 [{N},4] tensor")
    call("sm_box_region_stats", ptr(a), ptr(b), ptr(desc), a.numel(), N, max_h, max_w, ptr(boxes), ptr(box_start),
         boxes.shape[0], ptr(stats), stream())
    return stats


# ------------------------------------------------------------------ streaming dynamic inference
def _clip5(clip):
    _chk(clip)
    if clip.dim() != 5 or clip.dtype != torch.float32:
        raise _lib.KernelError("dynamic inference takes an fp32 [B,C,T,H,W] clip")
    return tuple(clip.shape) + tuple(clip.stride())


def _i32(t, n, what):
    if t is None:
        return
    _chk(t)
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
        raise _lib.KernelError(f"{what} must be a contiguous int32 tensor of at least {n} entries")


def motion_scores(clip):
    """clip fp32 [B,C,T,H,W] (any strides) -> fp32 [B,T] mean |frame t - frame t-1| (0 at t = 0)."""
    args = _clip5(clip)
    B, C, T, H, W = args[:5]
    scores = torch.empty((B, T), dtype=torch.float32, device=clip.device)
    nbytes = query("sm_motion_scores_workspace_bytes", B, C, T, H, W)
    ws = _ws(nbytes, clip.device)
    call("sm_motion_scores", ptr(clip), *args, ptr(scores), ptr(ws), nbytes, stream())
    return scores


def topk_frames(scores, k):
    """scores fp32 [B,T] -> int32 [B, min(k,T)]: the top-k frames in ascending frame order
    (ties: lower index first; NaN last)."""
    _chk(scores)
    if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
        raise _lib.KernelError("topk_frames takes contiguous fp32 [B,T] scores")
    B, T = scores.shape
    idx = torch.empty((B, min(int(k), T)), dtype=torch.int32, device=scores.device)
    call("sm_topk_frames", ptr(scores), B, T, int(k), ptr(idx), stream())
    return idx


def gather_frames(clip, b_idx, t_idx, n, rows_per_b=1, t_fixed=0):
    """-> dense fp32 [n,C,H,W], out[i] = clip[b_i, :, t_i]; b_i = b_idx[i] (int32) or
    i // rows_per_b when b_idx is None, t_i = t_idx[i] or t_fixed when t_idx is None."""
    args = _clip5(clip)
    n = int(n)
    _i32(b_idx, n, "b_idx")
    _i32(t_idx, n, "t_idx")
    C, H, W = args[1], args[3], args[4]
    out = torch.empty((n, C, H, W), dtype=torch.float32, device=clip.device)
    call("sm_gather_frames", ptr(clip), *args, ptr(b_idx), int(rows_per_b), ptr(t_idx), int(t_fixed), n, ptr(out),
         stream())
    return out


def exit_step(emb, active, n, w, bias, threshold, min_frames, final, sum_emb, cnt, decided, final_logits, used, conf):
    """One streaming early-exit update over the n samples active[:n] (state updated in place)."""
    _chk(active, w, bias, sum_emb, cnt, decided, final_logits, used, conf, emb)
    B, D = sum_emb.shape
    K = w.shape[0]
    n = int(n)
    _i32(active, n, "active")
    for t, dtype, shape, what in ((w, torch.float32, (K, D), "w"), (bias, torch.float32, (K,), "bias"),
                                  (sum_emb, torch.float32, (B, D), "sum"), (cnt, torch.int32, (B,), "cnt"),
                                  (decided, torch.uint8, (B,), "decided"),
                                  (final_logits, torch.float32, (B, K), "final_logits"),
                                  (used, torch.int32, (B,), "used"), (conf, torch.float32, (B,), "conf")):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.KernelError(f"exit_step: {what} must be contiguous {dtype} {shape}")
    if emb is not None and (emb.dtype != torch.float32 or not emb.is_contiguous() or tuple(emb.shape) != (n, D)):
        raise _lib.KernelError(f"exit_step: emb must be contiguous fp32 [{n},{D}]")
    call("sm_exit_step", ptr(emb), ptr(active), n, B, D, K, ptr(w), ptr(bias), float(threshold), int(min_frames),
         1 if final else 0, ptr(sum_emb), ptr(cnt), ptr(decided), ptr(final_logits), ptr(used), ptr(conf), stream())


def active_compact(decided, active, count):
    """active[:count] <- the ascending indices s with decided[s] == 0."""
    _chk(decided, active, count)
    B = decided.numel()
    _i32(active, B, "active")
    _i32(count, 1, "count")
    if decided.dtype != torch.uint8 or not decided.is_contiguous():
        raise _lib.KernelError("decided must be contiguous uint8 [B]")
    call("sm_active_compact", ptr(decided), B, ptr(active), ptr(count), stream())


# ------------------------------------------------------------------ feature-privacy evaluation
PRIVACY_MAX_CONFIGS = 64      # SM_PRIVACY_MAX_CONFIGS
LOGITS_MAX_CLASSES = 4096     # SM_LOGITS_MAX_CLASSES


def _f32_2d(t, what):
    _chk(t)
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.KernelError(f"{what} must be a contiguous fp32 matrix")


def privacy_perturb(z, sigmas, thresholds, seeds):
    """z fp32 [N,D] -> fp32 [G,N,D]: out[g] = (z + sigmas[g] * n_g) * keep_g, the draws a pure
    function of (seeds[g], row, col) (include/sm_api.h).  thresholds[g] in [0, 2^32]: an element
    is kept iff its 32-bit mask draw is >= the threshold."""
    import ctypes
    _f32_2d(z, "privacy_perturb: z")
    G = len(sigmas)
    if len(thresholds) != G or len(seeds) != G:
        raise _lib.KernelError("privacy_perturb: sigmas, thresholds and seeds must have one entry per configuration")
    N, D = z.shape
    out = torch.empty((G, N, D), dtype=torch.float32, device=z.device)
    sg = (ctypes.c_float * max(G, 1))(*[float(s) for s in sigmas])
    th = (ctypes.c_uint64 * max(G, 1))(*[int(t) for t in thresholds])
    sd = (ctypes.c_uint64 * max(G, 1))(*[int(s) & ((1 << 64) - 1) for s in seeds])
    call("sm_privacy_perturb", ptr(z), N, D, G, ctypes.cast(sg, ctypes.c_void_p), ctypes.cast(th, ctypes.c_void_p),
         ctypes.cast(sd, ctypes.c_void_p), ptr(out), stream())
    return out


def logits_metrics(logits, labels, k, segments=1, dlogits=None, grad_scale=1.0):
    """logits fp32 [S*N, C], labels int64 [N] -> fp64 [S,4]: per segment sum of the cross-entropy,
    sum of the entropy, top-1 hits, top-k hits.  dlogits (fp32, logits' shape, optional) receives
    (softmax - onehot) * grad_scale."""
    _f32_2d(logits, "logits_metrics: logits")
    _chk(labels, dlogits)
    rows, C = logits.shape
    S = int(segments)
    if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous():
        raise _lib.KernelError("logits_metrics: labels must be a contiguous int64 vector")
    N = labels.numel()
    if S < 1 or rows != S * N:
        raise _lib.KernelError(f"logits_metrics: {rows} rows are not {S} segments of {N} labels")
    if dlogits is not None and (dlogits.dtype != torch.float32 or dlogits.shape != logits.shape
                                or not dlogits.is_contiguous()):
        raise _lib.KernelError("logits_metrics: dlogits must match the logits (contiguous fp32)")
    out = torch.empty((S, 4), dtype=torch.float64, device=logits.device)
    nbytes = query("sm_logits_metrics_workspace_bytes", rows)
    ws = _ws(nbytes, logits.device)
    call("sm_logits_metrics", ptr(logits), rows, C, ptr(labels), N, int(k), ptr(dlogits), float(grad_scale), ptr(out),
         ptr(ws), nbytes, stream())
    return out


def soft_ce(logits, labels_a, labels_b=None, lam=None, eps=0.0, dlogits=None, grad_scale=1.0):
    """logits fp32 [N, C], labels_a (and labels_b) int64 [N], lam fp32 [N] -> fp64 [2]: the sum of the
    cross-entropies against t = lam s(labels_a) + (1 - lam) s(labels_b), s(y) = eps / C + (1 - eps)
    onehot(y), and the rows whose arg-max is labels_a (sm_soft_ce).  labels_b and lam come together
    or not at all (then t = s(labels_a)).  dlogits (fp32, logits' shape, optional) receives
    (softmax - t) * grad_scale.  With eps == 0 and no partner the sum, the hits and dlogits have
    logits_metrics(logits, labels_a, 1)'s bits."""
    _f32_2d(logits, "soft_ce: logits")
    _chk(labels_a, labels_b, lam, dlogits)
    N, C = logits.shape
    if not 1 <= C <= LOGITS_MAX_CLASSES:
        raise _lib.KernelError(f"soft_ce: the class count must be in [1, {LOGITS_MAX_CLASSES}], got {C}")
    if (labels_b is None) != (lam is None):
        raise _lib.KernelError("soft_ce: give both labels_b and lam (a mixed target) or neither")
    for t, what in ((labels_a, "labels_a"), (labels_b, "labels_b")):
        if t is not None and (t.dtype != torch.int64 or tuple(t.shape) != (N,) or not t.is_contiguous()
                              or t.device != logits.device):
            raise _lib.KernelError(f"soft_ce: {what} must be a contiguous int64 [{N}] vector on the logits' device")
    if lam is not None and (lam.dtype != torch.float32 or tuple(lam.shape) != (N,) or not lam.is_contiguous()
                            or lam.device != logits.device):
        raise _lib.KernelError(f"soft_ce: lam must be a contiguous fp32 [{N}] vector on the logits' device")
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise _lib.KernelError(f"soft_ce: eps must lie in [0, 1), got {eps}")
    if dlogits is not None and (dlogits.dtype != torch.float32 or dlogits.shape != logits.shape
                                or not dlogits.is_contiguous()):
        raise _lib.KernelError("soft_ce: dlogits must match the logits (contiguous fp32)")
    out = torch.empty(2, dtype=torch.float64, device=logits.device)
    nbytes = query("sm_soft_ce_workspace_bytes", N)
    ws = _ws(nbytes, logits.device)
    call("sm_soft_ce", ptr(logits), N, C, ptr(labels_a), ptr(labels_b), ptr(lam), eps, ptr(dlogits), float(grad_scale),
         ptr(out), ptr(ws), nbytes, stream())
    return out


def relu_fwd(pre):
    """h = max(pre, 0), fp32."""
    _chk(pre)
    if pre.dtype != torch.float32 or not pre.is_contiguous():
        raise _lib.KernelError("relu_fwd takes a contiguous fp32 tensor")
    h = torch.empty_like(pre)
    call("sm_relu_fwd", ptr(pre), pre.numel(), ptr(h), stream())
    return h


def relu_bias_bwd(dh, h, db):
    """-> dpre = dh * (h > 0); db [C] <- the column sums of dpre (written, not accumulated)."""
    _f32_2d(dh, "relu_bias_bwd: dh")
    _f32_2d(h, "relu_bias_bwd: h")
    _chk(db)
    M, C = dh.shape
    if h.shape != dh.shape or db.dtype != torch.float32 or db.numel() != C or not db.is_contiguous():
        raise _lib.KernelError("relu_bias_bwd: h must match dh and db be contiguous fp32 [C]")
    dpre = torch.empty_like(dh)
    nbytes = query("sm_relu_bias_bwd_workspace_bytes", M, C)
    ws = _ws(nbytes, dh.device)
    call("sm_relu_bias_bwd", ptr(dh), ptr(h), M, C, ptr(dpre), ptr(db), ptr(ws), nbytes, stream())
    return dpre


# ------------------------------------------------------------------ MAE reconstruction evaluation
def mae_reconstruct(pred, clip, mask_u8, mean, std, norm_pix=True, paste_visible=True, bgr_swap=True,
                    want_recon=True):
    """pred [B,T*L,192] (fp32 / bf16), clip fp32 [B,3,T,H,W] (any strides), mask uint8 [B,T,L] ->
    (panels uint8 [B,T,H,3W,3], recon fp32 [B,3,T,H,W] or an empty tensor, token_err fp32 [B*T*L,2])
    (include/sm_api.h); mean / std are the three display constants by RGB position."""
    import ctypes
    _chk(pred, clip, mask_u8)
    if clip.dim() != 5 or clip.shape[1] != 3 or clip.dtype != torch.float32:
        raise _lib.KernelError("mae_reconstruct takes an fp32 [B,3,T,H,W] clip")
    B, T, H, W, sB, sC, sT, sH, sW = _clip_args(clip)
    L = (H // 8) * (W // 8)
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.KernelError(f"mae_reconstruct: pred must be fp32 or bf16, not {pred.dtype}")
    if clip.device != pred.device or mask_u8.device != pred.device:
        raise _lib.KernelError("mae_reconstruct: pred, clip and mask must be on one device")
    if not pred.is_contiguous() or pred.numel() != B * T * L * 192:
        raise _lib.KernelError(f"mae_reconstruct: pred must be contiguous [{B},{T * L},192]")
    if mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous() or mask_u8.numel() != B * T * L:
        raise _lib.KernelError(f"mae_reconstruct: mask must be contiguous uint8 [{B},{T},{L}]")
    if len(mean) != 3 or len(std) != 3:
        raise _lib.KernelError("mae_reconstruct: mean and std have three entries")
    dev = pred.device
    panels = torch.empty((B, T, H, 3 * W, 3), dtype=torch.uint8, device=dev)
    recon = torch.empty((B, 3, T, H, W) if want_recon else (0,), dtype=torch.float32, device=dev)
    token_err = torch.empty((B * T * L, 2), dtype=torch.float32, device=dev)
    m = (ctypes.c_float * 3)(*[float(x) for x in mean])
    s = (ctypes.c_float * 3)(*[float(x) for x in std])
    call("sm_mae_reconstruct", dt(pred), ptr(pred), ptr(clip), sB, sC, sT, sH, sW, ptr(mask_u8), B, T, H, W,
         ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), 1 if norm_pix else 0,
         1 if paste_visible else 0, 1 if bgr_swap else 0, ptr(panels), ptr(recon) if want_recon else None,
         ptr(token_err), stream())
    return panels, recon, token_err


def recon_clip_metrics(token_err, mask_u8):
    """token_err fp32 [B*T*L,2], mask uint8 [B,T,L] -> fp32 [B,4]: masked-mean normalised error,
    masked-mean pixel error, PSNR dB, n_masked."""
    _chk(token_err, mask_u8)
    if mask_u8.dim() != 3 or mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous():
        raise _lib.KernelError("recon_clip_metrics: mask must be contiguous uint8 [B,T,L]")
    B, T, L = mask_u8.shape
    if token_err.device != mask_u8.device:
        raise _lib.KernelError("recon_clip_metrics: token_err and mask must be on one device")
    if token_err.dtype != torch.float32 or not token_err.is_contiguous() or token_err.numel() != B * T * L * 2:
        raise _lib.KernelError(f"recon_clip_metrics: token_err must be contiguous fp32 [{B * T * L},2]")
    out = torch.empty((B, 4), dtype=torch.float32, device=token_err.device)
    call("sm_recon_clip_metrics", ptr(token_err), ptr(mask_u8), B, T, L, ptr(out), stream())
    return out


# ------------------------------------------------------------------ temporal SSL pretraining
def _mfm_args(pred, teacher, idx, what):
    """Shapes and dtypes only.  The CALLER guarantees that idx is strictly ascending with every
    entry in [0, R): it lives on the device and is not read back here.  The backward finds a row
    by binary search, so an unsorted or repeated list gives zero or wrong gradient rows although
    the forward looks right (temporal_ssl builds it as nonzero() of the host mask: ascending)."""
    _chk(pred, teacher, idx)
    if pred.dim() != 2 or not pred.is_contiguous() or pred.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.KernelError(f"{what}: pred must be a contiguous fp32 or bf16 matrix")
    R, D = pred.shape
    if teacher.dtype != torch.float32 or teacher.shape != pred.shape or not teacher.is_contiguous():
        raise _lib.KernelError(f"{what}: teacher must be contiguous fp32 [{R},{D}]")
    if idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
        raise _lib.KernelError(f"{what}: idx must be a contiguous int32 vector")
    N = idx.numel()
    if not 1 <= N <= R:
        raise _lib.KernelError(f"{what}: {N} masked rows of a [{R},{D}] matrix")
    if pred.device != teacher.device or pred.device != idx.device:
        raise _lib.KernelError(f"{what}: pred, teacher and idx must be on one device")
    return R, N, D


def mfm_loss_fwd(pred, teacher, idx, w_mfm=1.0, w_var=1.0, target_std=1.0, eps=1e-4):
    """pred [R,D] (fp32 / bf16), teacher fp32 [R,D], idx int32 [N] strictly ascending (the
    caller's guarantee, see _mfm_args) ->
    (out fp32 [3] = mfm, var, w_mfm mfm + w_var var; stats fp32 [3N + 2D] for mfm_loss_bwd)."""
    R, N, D = _mfm_args(pred, teacher, idx, "mfm_loss_fwd")
    out = torch.empty(3, dtype=torch.float32, device=pred.device)
    stats = torch.empty(3 * N + 2 * D, dtype=torch.float32, device=pred.device)
    nbytes = query("sm_mfm_loss_workspace_bytes", N, D)
    ws = _ws(nbytes, pred.device)
    call("sm_mfm_loss_fwd", dt(pred), ptr(pred), ptr(teacher), ptr(idx), R, N, D, float(w_mfm), float(w_var),
         float(target_std), float(eps), ptr(out), ptr(stats), ptr(ws), nbytes, stream())
    return out, stats


def mfm_loss_bwd(pred, teacher, idx, stats, grad_out, w_mfm=1.0, w_var=1.0, out_dtype=None):
    """-> dpred [R,D] (out_dtype, default pred's) = grad_out (device scalar) x d total / d pred;
    rows outside idx are exact zeros."""
    R, N, D = _mfm_args(pred, teacher, idx, "mfm_loss_bwd")
    _chk(stats, grad_out)
    if stats.dtype != torch.float32 or stats.numel() != 3 * N + 2 * D or not stats.is_contiguous():
        raise _lib.KernelError("mfm_loss_bwd: stats must be the forward's fp32 [3N + 2D] buffer")
    if grad_out.dtype != torch.float32 or grad_out.numel() != 1:
        raise _lib.KernelError("mfm_loss_bwd: grad_out must be one fp32 value on the device")
    dpred = torch.empty((R, D), dtype=out_dtype or pred.dtype, device=pred.device)
    call("sm_mfm_loss_bwd", dt(pred), dt(dpred), ptr(pred), ptr(teacher), ptr(idx), R, N, D, ptr(stats),
         ptr(grad_out), float(w_mfm), float(w_var), ptr(dpred), stream())
    return dpred


def ema_update(dst, src, m):
    """dst = m dst + (1 - m) src over contiguous fp32 buffers of one length, in place."""
    _chk(dst, src)
    if dst.dtype != torch.float32 or src.dtype != torch.float32 or dst.numel() != src.numel() \
            or not dst.is_contiguous() or not src.is_contiguous() or dst.device != src.device:
        raise _lib.KernelError("ema_update takes two contiguous fp32 buffers of one length on one device")
    m = float(m)
    call("sm_ema_update", ptr(dst), ptr(src), dst.numel(), m, 1.0 - m, stream())    # each rounded to fp32 by ctypes
    return dst


def grad_clip(grad, ranges, max_norm, norm_out=None):
    """clip_grad_norm_ over the element ranges [(start, end), ...] of the flat fp32 gradient
    buffer, in place; -> the total norm as a device tensor (no host synchronise)."""
    import ctypes
    _chk(grad, norm_out)
    if grad.dtype != torch.float32 or grad.dim() != 1 or not grad.is_contiguous():
        raise _lib.KernelError("grad_clip takes a contiguous flat fp32 gradient buffer")
    n = len(ranges)
    prev = 0
    for s, e in ranges:
        if not prev <= s <= e <= grad.numel():
            raise _lib.KernelError(f"grad_clip: range [{s},{e}) is out of order or outside the {grad.numel()} elements")
        prev = e
    if norm_out is None:
        norm_out = torch.empty(1, dtype=torch.float32, device=grad.device)
    elif norm_out.dtype != torch.float32 or norm_out.numel() != 1 or norm_out.device != grad.device:
        raise _lib.KernelError("grad_clip: norm_out must be one fp32 value on the gradient's device")
    starts = (ctypes.c_int64 * max(n, 1))(*[int(s) for s, _ in ranges])
    ends = (ctypes.c_int64 * max(n, 1))(*[int(e) for _, e in ranges])
    sp, ep = ctypes.cast(starts, ctypes.c_void_p), ctypes.cast(ends, ctypes.c_void_p)
    nbytes = query("sm_grad_clip_workspace_bytes", sp, ep, n)
    if nbytes < 0:
        raise _lib.KernelError("grad_clip: bad ranges")
    ws = _ws(nbytes, grad.device)
    call("sm_grad_clip", ptr(grad), sp, ep, n, float(max_norm), ptr(norm_out), ptr(ws), nbytes, stream())
    return norm_out


def _relu_dropout_args(x, what):
    _chk(x)
    if x.dim() < 1 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.bfloat16) \
            or x.shape[-1] % 8 or x.data_ptr() % 16:
        raise _lib.KernelError(f"{what} takes contiguous 16-byte aligned fp32 / bf16 rows of a multiple of 8 columns")


def relu_dropout_fwd(x, drop_p=0.0, seed=0):
    """y = relu(x) * keep * drop_scale(p), the mask a function of (seed, row, column)."""
    _relu_dropout_args(x, "relu_dropout_fwd")
    y = torch.empty_like(x)
    call("sm_relu_dropout_fwd", dt(x), x.numel(), x.shape[-1], ptr(x), ptr(y), float(drop_p),
         int(seed) & ((1 << 64) - 1), stream())
    return y


def relu_dropout_bwd(ref, dy, drop_p=0.0, seed=0):
    """dx = dy * keep * drop_scale(p) where ref > 0 (ref: the forward's input or output)."""
    _relu_dropout_args(ref, "relu_dropout_bwd")
    _relu_dropout_args(dy, "relu_dropout_bwd")
    if dy.shape != ref.shape or dy.dtype != ref.dtype or dy.device != ref.device:
        raise _lib.KernelError("relu_dropout_bwd: dy must match ref")
    dx = torch.empty_like(dy)
    call("sm_relu_dropout_bwd", dt(ref), ref.numel(), ref.shape[-1], ptr(ref), ptr(dy), ptr(dx), float(drop_p),
         int(seed) & ((1 << 64) - 1), stream())
    return dx


# ------------------------------------------------------------------ kNN evaluation
KNN_MAX_K = 64     # one list entry per lane
KNN_MAX_KS = 8     # SM_KNN_MAX_KS


def _f32_rows(t, what):
    """fp32 [N, D] device rows, contiguous (a view at any 4-byte offset is fine)."""
    _chk(t)
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
        raise _lib.KernelError(f"{what} must be a non-empty contiguous fp32 matrix")


def row_rnorm(x):
    """x fp32 [N,D] -> fp32 [N]: 1 / sqrt(sum_d x^2) in sm_row_rnorm's summation order, 0 for a zero row."""
    _f32_rows(x, "row_rnorm: x")
    N, D = x.shape
    rn = torch.empty(N, dtype=torch.float32, device=x.device)
    call("sm_row_rnorm", ptr(x), N, D, ptr(rn), stream())
    return rn


def knn_topk(q, bank, rq, rb, k, self_offset=-1, splits=0):
    """q fp32 [Nq,D], bank fp32 [Nb,D], rq [Nq] / rb [Nb] (both or neither) -> (idx int32 [Nq,k],
    sim fp32 [Nq,k]): each query's first k bank rows under sm_knn_topk's total order, slots past
    the candidates idx = -1 / sim = -inf.  self_offset >= 0 drops bank row i + self_offset for
    query i; splits bank partitions (0 = auto), the result the same bits for every value."""
    _f32_rows(q, "knn_topk: q")
    _f32_rows(bank, "knn_topk: bank")
    _chk(rq, rb)
    (Nq, D), Nb = q.shape, bank.shape[0]
    if bank.shape[1] != D or bank.device != q.device:
        raise _lib.KernelError("knn_topk: q and bank must share the feature width and the device")
    if (rq is None) != (rb is None):
        raise _lib.KernelError("knn_topk: give both norm vectors (cosine) or neither (dot)")
    for t, n, what in ((rq, Nq, "rq"), (rb, Nb, "rb")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n,) or not t.is_contiguous()):
            raise _lib.KernelError(f"knn_topk: {what} must be contiguous fp32 [{n}]")
    k, splits = int(k), int(splits)
    if not 1 <= k <= KNN_MAX_K:
        raise _lib.KernelError(f"knn_topk: k must be in [1, {KNN_MAX_K}]")
    idx = torch.empty((Nq, k), dtype=torch.int32, device=q.device)
    sim = torch.empty((Nq, k), dtype=torch.float32, device=q.device)
    nbytes = query("sm_knn_topk_workspace_bytes", Nq, Nb, k, splits)
    ws = _ws(nbytes, q.device)
    call("sm_knn_topk", ptr(q), Nq, ptr(bank), Nb, D, ptr(rq), ptr(rb), k, int(self_offset), splits, ptr(idx),
         ptr(sim), ptr(ws), nbytes, stream())
    return idx, sim


def knn_vote(idx, sim, labels, num_classes, inv_temperature, ks):
    """idx int32 / sim fp32 [Nq,k], labels int64 [Nb] -> scores fp32 [len(ks), Nq, C]: the
    exp(sim * inv_temperature) weights of the first ks[s] neighbours added per class in rank
    order (sm_knn_vote).  ks strictly ascending within [1, k]."""
    import ctypes
    _chk(idx, sim, labels)
    if idx.dim() != 2 or idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() == 0:
        raise _lib.KernelError("knn_vote: idx must be a non-empty contiguous int32 matrix")
    if sim.dtype != torch.float32 or sim.shape != idx.shape or not sim.is_contiguous():
        raise _lib.KernelError("knn_vote: sim must match idx (contiguous fp32)")
    if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous() or labels.numel() == 0:
        raise _lib.KernelError("knn_vote: labels must be a non-empty contiguous int64 vector")
    ks = [int(v) for v in ks]
    Nq, k = idx.shape
    C = int(num_classes)
    if not 1 <= len(ks) <= KNN_MAX_KS or ks[0] < 1 or ks[-1] > k or any(b <= a for a, b in zip(ks, ks[1:])):
        raise _lib.KernelError(f"knn_vote: ks must be 1..{KNN_MAX_KS} strictly ascending values within [1, {k}]")
    if not 1 <= C <= LOGITS_MAX_CLASSES:
        raise _lib.KernelError(f"knn_vote: num_classes must be in [1, {LOGITS_MAX_CLASSES}]")
    scores = torch.empty((len(ks), Nq, C), dtype=torch.float32, device=idx.device)
    arr = (ctypes.c_int32 * len(ks))(*ks)
    call("sm_knn_vote", ptr(idx), ptr(sim), Nq, k, ptr(labels), labels.numel(), C, float(inv_temperature),
         ctypes.cast(arr, ctypes.c_void_p), len(ks), ptr(scores), stream())
    return scores

"""numpy mirror of sm_frames_resize_normalize's arithmetic (include/sm_api.h), bit for bit.

Every product and sum below is one fp32 numpy operation (numpy never fuses), and the one
fused step of the kernel, src = fma(scale, d + 0.5, -0.5), is formed in float64 and rounded
once: scale has 24 significant bits and d + 0.5 at most 14, so the float64 product and the
subtraction of 0.5 are exact and the single conversion to fp32 is the fma's single rounding.
"""
import numpy as np

F32 = np.float32
FLAG_FLIP, FLAG_INVALID = 1, 2
MAX_SOURCE_SIDE = 8192


def axis(n_in, n_out):
    """-> (i0, i1 int64 [n_out], l0, l1 fp32 [n_out]) of one axis."""
    d = np.arange(n_out, dtype=np.int64)
    if n_in == n_out:
        return d, d.copy(), np.ones(n_out, F32), np.zeros(n_out, F32)
    scale = F32(n_in) / F32(n_out)
    src = (np.float64(scale) * (d.astype(np.float64) + 0.5) - 0.5).astype(F32)
    src = np.maximum(src, F32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = np.clip(src - i0.astype(F32), F32(0), F32(1)).astype(F32)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, (F32(1) - l1).astype(F32), l1


def resize_normalize(frames_u8, out_hw, mean, std, bgr_swap=True, flip=False):
    """uint8 [T,Hs,Ws,3] (RGB) -> fp32 [3,T,Ho,Wo]."""
    T, Hs, Ws, _ = frames_u8.shape
    Ho, Wo = out_hw
    mean, std = np.asarray(mean, F32), np.asarray(std, F32)
    y0, y1, l0y, l1y = axis(Hs, Ho)
    x0, x1, l0x, l1x = axis(Ws, Wo)
    p = frames_u8.astype(F32) / F32(255)
    l0x, l1x = l0x[None, None, :, None], l1x[None, None, :, None]
    l0y, l1y = l0y[None, :, None, None], l1y[None, :, None, None]
    top = l0x * p[:, y0][:, :, x0] + l1x * p[:, y0][:, :, x1]
    bot = l0x * p[:, y1][:, :, x0] + l1x * p[:, y1][:, :, x1]
    r = l0y * top + l1y * bot                      # [T,Ho,Wo,3], source channel order
    if flip:
        r = r[:, :, ::-1]
    out = (r - mean) / std
    if bgr_swap:
        out = out[..., ::-1]
    assert out.dtype == F32
    return np.ascontiguousarray(out.transpose(3, 0, 1, 2))


def resize_normalize_batch(packed, desc, T, out_hw, mean, std, bgr_swap=True):
    """packed uint8 1-D + desc int64 [B,4] -> fp32 [B,3,T,Ho,Wo], with the kernel's rule for
    an invalid clip (flag, size outside [1, 8192], range outside the buffer): zeros."""
    out = np.zeros((len(desc), 3, T) + tuple(out_hw), F32)
    for b, (off, hs, ws, flags) in enumerate(np.asarray(desc).tolist()):
        n = T * hs * ws * 3
        if flags & FLAG_INVALID or not (1 <= hs <= MAX_SOURCE_SIDE and 1 <= ws <= MAX_SOURCE_SIDE):
            continue
        if off < 0 or off + n > packed.size:
            continue
        frames = packed[off:off + n].reshape(T, hs, ws, 3)
        out[b] = resize_normalize(frames, out_hw, mean, std, bgr_swap, bool(flags & FLAG_FLIP))
    return out


def atol(hs, ws, std):
    """Bound against torch's F.interpolate path: 2 ulp of the source coordinate (torch rounds
    its index arithmetic differently from the fused form) plus 8 half-ulps of a value in [0, 1]
    for the seven rounded interpolation operations, scaled by the normalisation."""
    return float((2 * np.spacing(F32(max(hs, ws))) + 8 * 2.0 ** -24) / min(std))

"""numpy statement of sm_frames_crop_resize_normalize's window rule (include/sm_api.h): the
result is sm_frames_resize_normalize applied to a buffer that holds only the window's pixels.
So the window is sliced out on the host and resize_mirror.resize_normalize runs unchanged on
the slice: no second arithmetic, and a pixel outside the window cannot reach the result."""
import numpy as np

import resize_mirror as M


def crop_resize_normalize(frames_u8, window, out_hw, mean, std, bgr_swap=True, flip=False):
    """uint8 [T,Hs,Ws,3] + window (y0, x0, Hc, Wc) -> fp32 [3,T,Ho,Wo]."""
    y0, x0, hc, wc = window
    return M.resize_normalize(np.ascontiguousarray(frames_u8[:, y0:y0 + hc, x0:x0 + wc]), out_hw, mean, std,
                              bgr_swap, flip)


def window_ok(hs, ws, y0, x0, hc, wc):
    return y0 >= 0 and x0 >= 0 and hc >= 1 and wc >= 1 and y0 + hc <= hs and x0 + wc <= ws


def crop_resize_normalize_batch(packed, desc, T, out_hw, mean, std, bgr_swap=True):
    """packed uint8 1-D + desc int64 [B,8] -> fp32 [B,3,T,Ho,Wo]; zeros for a clip the kernel
    rejects (resize_mirror's rules, or a window that is empty or leaves its frame)."""
    out = np.zeros((len(desc), 3, T) + tuple(out_hw), M.F32)
    for b, (off, hs, ws, flags, y0, x0, hc, wc) in enumerate(np.asarray(desc).tolist()):
        n = T * hs * ws * 3
        if flags & M.FLAG_INVALID or not (1 <= hs <= M.MAX_SOURCE_SIDE and 1 <= ws <= M.MAX_SOURCE_SIDE):
            continue
        if off < 0 or off + n > packed.size or not window_ok(hs, ws, y0, x0, hc, wc):
            continue
        frames = packed[off:off + n].reshape(T, hs, ws, 3)
        out[b] = crop_resize_normalize(frames, (y0, x0, hc, wc), out_hw, mean, std, bgr_swap,
                                       bool(flags & M.FLAG_FLIP))
    return out

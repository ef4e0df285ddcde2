"""numpy mirror of sm_frames_box_blur and sm_box_region_stats (include/sm_api.h), bit for bit.

Every product and every sum of the blur is one fp32 numpy operation (numpy never fuses), taken in
the kernel's order: acc = acc + w[i] * value for i ascending from acc = 0.  np.rint rounds half to
even as rintf does.  The weights are an input, so the mirror and the kernel share them.
"""
import numpy as np

F32 = np.float32
MAX_SIDE = 8192


def refl(i, n):
    """Reflect-101 index of integer array i into [0, n): periodic, defined for any i and n >= 1."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def blur_frame(u8, weights):
    """uint8 [H,W,3] -> uint8 [H,W,3]: the separable Gaussian at EVERY pixel."""
    w = np.asarray(weights, F32)
    k = w.size
    r = (k - 1) // 2
    H, W, _ = u8.shape
    src = u8.astype(F32)
    xs, ys = np.arange(W), np.arange(H)
    h = np.zeros((H, W, 3), F32)
    for i in range(k):
        h = h + w[i] * src[:, refl(xs + i - r, W)]
    v = np.zeros((H, W, 3), F32)
    for i in range(k):
        v = v + w[i] * h[refl(ys + i - r, H)]
    return np.minimum(F32(255), np.maximum(F32(0), np.rint(v))).astype(np.uint8)


def frame_ok(off, h, w, packed_bytes, max_h, max_w):
    return (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and h <= max_h and w <= max_w and 0 <= off <= packed_bytes
            and h * w * 3 <= packed_bytes - off)


def union_mask(boxes, H, W):
    """bool [H,W]: the union of the boxes (x, y, w, h) clipped to the frame."""
    m = np.zeros((H, W), bool)
    for x, y, w, h in boxes:
        x, y, w, h = int(x), int(y), int(w), int(h)
        if w <= 0 or h <= 0:
            continue
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
        if x1 > x0 and y1 > y0:
            m[y0:y1, x0:x1] = True
    return m


def frame_boxes(boxes, box_start, n):
    nb = len(boxes)
    b0, b1 = (min(max(int(box_start[n + k]), 0), nb) for k in (0, 1))
    return boxes[b0:b1] if b1 > b0 else boxes[:0]


def box_blur_batch(packed, desc, boxes, box_start, weights, max_h, max_w, out_prefill):
    """-> uint8 [packed_bytes]: out_prefill with every valid frame's bytes replaced."""
    out = np.array(out_prefill, np.uint8, copy=True)
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    for n, (off, h, w) in enumerate(np.asarray(desc, np.int64).tolist()):
        if not frame_ok(off, h, w, packed.size, max_h, max_w):
            continue
        u8 = packed[off:off + h * w * 3].reshape(h, w, 3)
        m = union_mask(frame_boxes(boxes, box_start, n), h, w)
        res = u8.copy()
        if m.any():
            res[m] = blur_frame(u8, weights)[m]
        out[off:off + h * w * 3] = res.reshape(-1)
    return out


def region_stats(a, b, desc, boxes, box_start, max_h, max_w):
    """-> int64 [N,4] = {P, SSE, Ea, Eb}."""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 4)
    desc = np.asarray(desc, np.int64)
    stats = np.zeros((len(desc), 4), np.int64)
    for n, (off, h, w) in enumerate(desc.tolist()):
        if not frame_ok(off, h, w, a.size, max_h, max_w):
            continue
        m = union_mask(frame_boxes(boxes, box_start, n), h, w)
        fa, fb = (t[off:off + h * w * 3].reshape(h, w, 3).astype(np.int64) for t in (a, b))

        def energy(img):
            e = np.zeros((h, w), np.int64)
            e[:, :-1] += ((img[:, 1:] - img[:, :-1]) ** 2).sum(2)
            e[:-1, :] += ((img[1:] - img[:-1]) ** 2).sum(2)
            return int(e[m].sum())

        stats[n] = [int(m.sum()), int((((fa - fb) ** 2).sum(2))[m].sum()), energy(fa), energy(fb)]
    return stats

"""Numpy statements of csrc/mix.hip's pixel rule (fp32, the kernel's operations in the kernel's
order: bit for bit) and of sm_soft_ce's loss and gradient (fp64: the reference the kernel is
measured against)."""
import numpy as np


def clip_mix_mirror(x, lam_px, box):
    """x fp32 [B, planes, H, W] (or [B, 3, T, H, W]), lam_px fp32 [B // 2], box int [B // 2, 4] =
    (y0, x0, h, w) -> the mixed batch.  Clip b is paired with clip B - 1 - b.  Inside the box, on
    every plane, the partner's pixel; outside it the clip's own pixel when lam_px == 1 (a select),
    otherwise fl(fl(lam a) + fl(fl(1 - lam) q)); the middle clip of an odd batch is copied."""
    x = np.asarray(x, dtype=np.float32)
    out = x.copy()
    B, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    lam_px = np.asarray(lam_px, dtype=np.float32).reshape(-1)
    box = np.asarray(box, dtype=np.int64).reshape(-1, 4)
    for p in range(B // 2):
        b, q = p, B - 1 - p
        lam = np.float32(lam_px[p])
        oml = np.float32(np.float32(1.0) - lam)
        y0, x0, h, w = (int(v) for v in box[p])
        inside = np.zeros((H, W), dtype=bool)
        inside[y0:y0 + h, x0:x0 + w] = True
        for own, other in ((b, q), (q, b)):
            a, o = x[own], x[other]
            if lam == np.float32(1.0):
                blend = a
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    blend = (lam * a).astype(np.float32) + (oml * o).astype(np.float32)
            out[own] = np.where(inside, o, blend.astype(np.float32))
    return out


def batch_flip_reference(x, lam_px, box):
    """The eager formula in float64: x * lam + x[::-1] * (1 - lam), then the slice paste of the
    flipped batch inside every pair's box."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    lam = np.ones(B, dtype=np.float64)
    for p in range(B // 2):
        lam[p] = lam[B - 1 - p] = float(np.float32(lam_px[p]))
    lam = lam.reshape((B,) + (1,) * (x.ndim - 1))
    flipped = x[::-1]
    out = x * lam + flipped * (1.0 - lam)
    for p in range(B // 2):
        y0, x0, h, w = (int(v) for v in box[p])
        for b in (p, B - 1 - p):
            out[b][..., y0:y0 + h, x0:x0 + w] = flipped[b][..., y0:y0 + h, x0:x0 + w]
    return out


def soft_target(C, labels_a, labels_b=None, lam=None, eps=0.0):
    """fp64 [N, C]: lam s(ya) + (1 - lam) s(yb), s(y) = eps / C + (1 - eps) onehot(y)."""
    ya = np.asarray(labels_a, dtype=np.int64)
    N = ya.shape[0]

    def s(y):
        t = np.full((N, C), eps / C, dtype=np.float64)
        t[np.arange(N), y] += 1.0 - eps
        return t

    if labels_b is None or lam is None:
        return s(ya)
    lam = np.asarray(lam, dtype=np.float64).reshape(N, 1)
    return lam * s(ya) + (1.0 - lam) * s(np.asarray(labels_b, dtype=np.int64))


def soft_ce_mirror(logits, labels_a, labels_b=None, lam=None, eps=0.0, grad_scale=1.0):
    """logits [N, C] -> (row losses fp64 [N], dlogits fp64 [N, C], top-1 hits of labels_a): loss_i =
    -sum_c t_c (l_c - logsumexp(l)) from the max-subtracted logits, dlogits = (softmax - t) *
    grad_scale, a hit when no logit is larger than the label's and no equal one has a lower index."""
    l = np.asarray(logits, dtype=np.float64)
    N, C = l.shape
    t = soft_target(C, labels_a, labels_b, lam, eps)
    z = l - l.max(axis=1, keepdims=True)
    e = np.exp(z)
    s = e.sum(axis=1, keepdims=True)
    logp = z - np.log(s)
    loss = -(t * logp).sum(axis=1)
    ya = np.asarray(labels_a, dtype=np.int64)
    ly = l[np.arange(N), ya][:, None]
    rank = (l > ly).sum(axis=1) + ((l == ly) & (np.arange(C)[None, :] < ya[:, None])).sum(axis=1)
    return loss, (e / s - t) * grad_scale, int((rank < 1).sum())

"""Weighted k-nearest-neighbour evaluation of frozen features (Wu et al. 2018; the training-free
probe of DINO and others), MI355X-native.  No counterpart in the reference.

A labelled bank and a query set are embedded; each query takes its k most similar bank rows and
votes with weights exp(sim / T); top-1 / top-5 are reported for a few k.

Search      knn_topk runs sm_knn_topk: fp32-input MFMA similarities and a streaming top-k that
  never writes the Nq x Nb matrix.  The neighbour order is total (larger sim first, equal sims by
  lower bank index, NaN last by index), fewer than k candidates pad with idx = -1 / sim = -inf,
  and the result does not depend on `splits`.
Vote        knn_vote runs sm_knn_vote: one pass fills the class tables of every k of `ks` (each a
  prefix of the next); the [nk * Nq, C] table then goes through sm_logits_metrics with nk
  segments for top-1 / top-5 (ties between classes: the lower class index wins).
knn_eval    the whole evaluation, one readback for the whole table; impl="reference" is the same
  result from eager torch ops on the device (knn_reference), the thing to time against.
Mirrors     knn_mirror, vote_mirror and metrics_mirror state the order, the padding, the vote and
  the hit rule on the host in numpy: they are the specification the kernels are tested against.
"""
import numpy as np
import torch

from . import ops as K

MAX_K = 64          # sm_knn_topk: one list entry per lane
MAX_KS = 8          # SM_KNN_MAX_KS
METRICS = ("cosine", "dot")


def check_ks(ks, k_max=MAX_K):
    """The list of k values as ints: 1..MAX_KS strictly ascending entries within [1, k_max]."""
    if not isinstance(ks, (list, tuple)) or not 1 <= len(ks) <= MAX_KS:
        raise ValueError(f"[ERROR] knn.ks needs 1 to {MAX_KS} entries")
    out = [int(v) for v in ks]
    if any(float(v) != float(o) for v, o in zip(ks, out)):
        raise ValueError("[ERROR] knn.ks entries must be integers")
    if out[0] < 1 or out[-1] > k_max or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"[ERROR] knn.ks must be strictly ascending within [1, {k_max}]")
    return out


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"[ERROR] knn metric must be one of {METRICS}, got {metric!r}")
    return metric


# ------------------------------------------------------------------ kernels
def row_rnorm(x):
    """x fp32 [N, D] -> fp32 [N]: 1 / ||x_i||, 0 for a zero row (sm_row_rnorm)."""
    return K.row_rnorm(x)


def knn_topk(q, bank, k, metric="cosine", leave_one_out_offset=None, splits=0):
    """q [Nq, D], bank [Nb, D] fp32 -> (idx int32 [Nq, k], sim fp32 [Nq, k]).  cosine scales the
    dot products by both rows' row_rnorm; leave_one_out_offset = o drops bank row i + o for query i."""
    rq = rb = None
    if _metric(metric) == "cosine":
        rq, rb = K.row_rnorm(q), K.row_rnorm(bank)
    off = -1 if leave_one_out_offset is None else int(leave_one_out_offset)
    if leave_one_out_offset is not None and off < 0:
        raise ValueError("[ERROR] leave_one_out_offset must be >= 0")
    return K.knn_topk(q, bank, rq, rb, int(k), off, int(splits))


def knn_vote(idx, sim, bank_labels, num_classes, temperature, ks):
    """-> scores fp32 [len(ks), Nq, C] (sm_knn_vote with inv_temperature = 1 / temperature)."""
    return K.knn_vote(idx, sim, bank_labels, int(num_classes), 1.0 / float(temperature), ks)


def _rows(z):
    return z.detach().float().contiguous()


def knn_eval(zq, yq, zb, yb, ks, temperature, num_classes, metric="cosine", leave_one_out=False, impl="fused"):
    """Top-1 / top-5 of the weighted kNN classifier for every k of `ks`.
    -> {"ks", "top1", "top5" (lists of floats), "idx" int32 [Nq, max k], "sim" fp32 [Nq, max k]}.
    leave_one_out drops bank row i for query i (the bank evaluated against itself)."""
    ks = check_ks(ks)
    _metric(metric)
    if impl == "reference":
        return knn_reference(zq, yq, zb, yb, ks, temperature, num_classes, metric, leave_one_out)
    if impl != "fused":
        raise ValueError(f"[ERROR] knn impl must be fused or reference, got {impl!r}")
    zq, zb = _rows(zq), _rows(zb)
    yq, yb = yq.long().contiguous(), yb.long().contiguous()
    C, nk, Nq = int(num_classes), len(ks), zq.shape[0]
    idx, sim = knn_topk(zq, zb, ks[-1], metric, 0 if leave_one_out else None)
    scores = knn_vote(idx, sim, yb, C, temperature, ks)
    hits = K.logits_metrics(scores.view(nk * Nq, C), yq, min(5, C), nk)
    table = hits[:, 2:4].cpu().tolist()                        # the evaluation's one readback
    return {"ks": ks, "top1": [r[0] / Nq for r in table], "top5": [r[1] / Nq for r in table], "idx": idx, "sim": sim}


# ------------------------------------------------------------------ eager reference (device)
_I32_MIN = -(1 << 31)


def _order_keys(sim, excluded=None):
    """int32 keys whose descending stable sort is the search's total order: the fp32 order with
    -0 == +0, NaN below -inf, an excluded candidate below NaN."""
    bits = (sim + 0.0).view(torch.int32)
    key = torch.where(bits >= 0, bits, bits ^ 0x7FFFFFFF)
    key = torch.where(torch.isnan(sim), torch.full_like(key, _I32_MIN + 1), key)
    if excluded is not None:
        key = torch.where(excluded, torch.full_like(key, _I32_MIN), key)
    return key


@torch.no_grad()
def knn_reference(zq, yq, zb, yb, ks, temperature, num_classes, metric="cosine", leave_one_out=False,
                  chunk_bytes=1 << 30):
    """knn_eval's result from eager torch ops on the inputs' device: mm, a stable descending sort
    (ties take the lower index), scatter_add for the vote and a rank count for the hits; chunked
    over the queries so the similarity slab stays under chunk_bytes."""
    ks = check_ks(ks)
    _metric(metric)
    zq, zb = _rows(zq), _rows(zb)
    yq, yb = yq.long(), yb.long()
    (Nq, _), Nb, C, k = zq.shape, zb.shape[0], int(num_classes), ks[-1]
    kk = min(k, Nb)
    if metric == "cosine":
        def rnorm(z):
            ss = (z * z).sum(1)
            return torch.where(ss > 0, 1.0 / torch.sqrt(ss), torch.zeros_like(ss))
        rq, rb = rnorm(zq), rnorm(zb)
    cols = torch.arange(Nb, device=zq.device)
    step = max(1, min(Nq, int(chunk_bytes) // (Nb * 16)))        # sim + keys + sorted keys + order
    idx = torch.full((Nq, k), -1, dtype=torch.int32, device=zq.device)
    sim = torch.full((Nq, k), float("-inf"), dtype=torch.float32, device=zq.device)
    for s in range(0, Nq, step):
        e = min(Nq, s + step)
        d = zq[s:e] @ zb.t()
        if metric == "cosine":
            d = (d * rq[s:e, None]) * rb[None, :]
        excl = (cols[None, :] == torch.arange(s, e, device=zq.device)[:, None]) if leave_one_out else None
        skey, order = torch.sort(_order_keys(d, excl), dim=1, descending=True, stable=True)
        order, live = order[:, :kk], skey[:, :kk] != _I32_MIN
        idx[s:e, :kk] = torch.where(live, order, torch.full_like(order, -1)).int()
        sim[s:e, :kk] = torch.where(live, d.gather(1, order), torch.full_like(d[:, :kk], float("-inf")))
    lab = yb[idx.clamp(min=0).long()]
    ok = (idx >= 0) & ~torch.isnan(sim) & (lab >= 0) & (lab < C)
    w = torch.where(ok, torch.exp(sim * (1.0 / float(temperature))), torch.zeros_like(sim))
    lab = torch.where(ok, lab, torch.zeros_like(lab))
    scores, acc, r0 = [], torch.zeros((Nq, C), dtype=torch.float32, device=zq.device), 0
    for kv in ks:
        acc = acc.scatter_add(1, lab[:, r0:kv], w[:, r0:kv])
        scores.append(acc)
        r0 = kv
    scores = torch.stack(scores)                                  # [nk, Nq, C]
    y = yq.view(1, Nq, 1).expand(len(ks), Nq, 1)
    y_ok = (y >= 0) & (y < C)
    ly = scores.gather(2, y.clamp(0, C - 1))
    cls = torch.arange(C, device=zq.device).view(1, 1, C)
    rank = ((scores > ly) | ((scores == ly) & (cls < y))).sum(2, keepdim=True)
    fin = torch.isfinite(scores).all(2, keepdim=True) & y_ok
    hit = torch.stack([(fin & (rank < 1)).sum((1, 2)), (fin & (rank < min(5, C))).sum((1, 2))], dim=1)
    table = hit.cpu().tolist()
    return {"ks": ks, "top1": [r[0] / Nq for r in table], "top5": [r[1] / Nq for r in table], "idx": idx, "sim": sim}


# ------------------------------------------------------------------ host mirrors (numpy)
def rnorm_mirror(x):
    """sm_row_rnorm on the host, fp32: 1 / sqrt(ss), 0 where ss is not > 0.  ss is formed in fp64 and
    rounded once, which equals the kernel's fp32 sum wherever that sum is exact (integer data)."""
    x = np.asarray(x, dtype=np.float32)
    ss = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = np.float32(1.0) / np.sqrt(ss)
    return np.where(ss > 0, rn, np.float32(0.0)).astype(np.float32)


def knn_mirror(q, bank, k, metric="cosine", leave_one_out_offset=None, precision="fp32"):
    """The search's specification on the host -> (idx int32 [Nq, k], sim [Nq, k]).
    Similarity: the fp64 dot product; precision="fp32" rounds it to fp32 and applies the two
    cosine scalings as separately rounded fp32 products with rnorm_mirror's vectors (the kernel's
    bits wherever the dot product is exact in fp32), "fp64" keeps everything in fp64.
    Order: larger sim first, equal sims (-0 == +0) by lower bank index, NaN after every number by
    index.  leave_one_out_offset = o removes bank row i + o from query i's candidates.  With
    fewer than k candidates the remaining slots are idx = -1, sim = -inf."""
    _metric(metric)
    if precision not in ("fp32", "fp64"):
        raise ValueError("precision must be fp32 or fp64")
    q32, b32 = np.asarray(q, dtype=np.float32), np.asarray(bank, dtype=np.float32)
    q64, b64 = q32.astype(np.float64), b32.astype(np.float64)
    Nq, Nb, k = q64.shape[0], b64.shape[0], int(k)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sim = q64 @ b64.T
        if precision == "fp32":
            sim = sim.astype(np.float32)
            if metric == "cosine":
                sim = (sim * rnorm_mirror(q32)[:, None]).astype(np.float32) * rnorm_mirror(b32)[None, :]
        elif metric == "cosine":
            def rn64(z):
                ss = (z * z).sum(1)
                return np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)
            sim = (sim * rn64(q64)[:, None]) * rn64(b64)[None, :]
    idx = np.full((Nq, k), -1, dtype=np.int32)
    out = np.full((Nq, k), -np.inf, dtype=sim.dtype)
    cols = np.arange(Nb)
    for i in range(Nq):
        keep = np.ones(Nb, dtype=bool)
        if leave_one_out_offset is not None and 0 <= i + int(leave_one_out_offset) < Nb:
            keep[i + int(leave_one_out_offset)] = False
        s, c = sim[i][keep], cols[keep]
        nan = np.isnan(s)
        order = np.lexsort((c, np.where(nan, 0.0, -s), nan))[:k]      # NaN class, then sim, then index
        idx[i, :len(order)] = c[order]
        out[i, :len(order)] = s[order]
    return idx, out


def vote_mirror(idx, sim, bank_labels, num_classes, inv_temperature, ks):
    """sm_knn_vote in fp64 -> [len(ks), Nq, C]: neighbour r adds exp(sim * inv_temperature) to its
    bank row's class for every ks[s] > r; idx outside [0, Nb), a label outside [0, C) or a NaN sim
    adds nothing."""
    idx, sim = np.asarray(idx), np.asarray(sim, dtype=np.float64)
    labels, C, ks = np.asarray(bank_labels), int(num_classes), [int(v) for v in ks]
    Nq, k = idx.shape
    out = np.zeros((len(ks), Nq, C), dtype=np.float64)
    for i in range(Nq):
        for r in range(min(k, ks[-1])):
            j = int(idx[i, r])
            if j < 0 or j >= len(labels) or np.isnan(sim[i, r]):
                continue
            y = int(labels[j])
            if 0 <= y < C:
                w = np.exp(sim[i, r] * float(inv_temperature))
                for s, kv in enumerate(ks):
                    if r < kv:
                        out[s, i, y] += w
    return out


def metrics_mirror(scores, labels, k):
    """Hit counts of sm_logits_metrics on a [S, N, C] table -> (top1 [S], topk [S]) ints: the label
    ranks after every larger score and after equal scores of a lower class index."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    S, N, C = scores.shape
    cls = np.arange(C)
    top1, topk = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    for s in range(S):
        for i in range(N):
            y = int(labels[i])
            if not 0 <= y < C or not np.all(np.isfinite(scores[s, i])):
                continue
            ly = scores[s, i, y]
            rank = int(((scores[s, i] > ly) | ((scores[s, i] == ly) & (cls < y))).sum())
            top1[s] += rank < 1
            topk[s] += rank < k
    return top1, topk

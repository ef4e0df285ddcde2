"""kNN evaluation on the GPU (csrc/knn.hip, ssl_mae_amd/knn.py) against the host mirrors.

Exact cases.  Features drawn as integers in [-2, 2] stored as fp32: every product and partial sum
  is an exact small integer (|dot| <= 4 D < 2^24), so the dot product is the same in any summation
  order, ties are frequent, and idx and the bits of sim must equal the mirror's: for `dot`, and for
  `cosine` with the norm vectors of sm_row_rnorm (ss an exact integer, 1.0f / sqrtf correctly rounded).
Real-valued inputs.  Per pair eps_ij = (D + 2) 2^-24 sum_d |q_id b_jd| rq_i rb_j, the standard
  forward bound of an fp32 dot product in any order plus the two scalings, in fp64.  Every returned
  sim is within eps of fp64, every returned j has sim64 >= s_k - eps, every excluded j has
  sim64 <= s_k + eps (s_k the k-th largest in fp64), and on rows whose fp64 top-(k+1) has no adjacent
  pair closer than the sum of their eps, idx is the fp64 order exactly.
Vote.  scores against the fp64 mirror at 1e-5 relative of each row's largest score, the project's
  tolerance for fused reductions; the hit counts are exact, on a table
  whose compared class scores are >= 1e-3 relative apart (asserted).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _offset_view(t):
    """The same values at a storage offset of one element: contiguous, 4-byte aligned only."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _ints(seed, n, d, lo=-2, hi=2):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=(n, d)).astype(np.float32)


def _search(q, b, k, metric, off=None, splits=0, offset=False):
    from ssl_mae_amd import knn
    tq, tb = torch.from_numpy(q).to(DEV), torch.from_numpy(b).to(DEV)
    if offset:
        tq, tb = _offset_view(tq), _offset_view(tb)
    idx, sim = knn.knn_topk(tq, tb, k, metric, off, splits)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and sim.dtype == torch.float32 and tuple(idx.shape) == tuple(sim.shape) == (len(q), k)
    return idx.cpu().numpy(), sim.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32),
                          np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


def _assert_matches_mirror(q, b, k, metric, off=None, splits=0, offset=False):
    from ssl_mae_amd import knn
    idx, sim = _search(q, b, k, metric, off, splits, offset)
    want_idx, want_sim = knn.knn_mirror(q, b, k, metric, off)
    assert np.array_equal(idx, want_idx), (metric, np.argwhere(idx != want_idx)[:5])
    assert _same_bits(sim, want_sim), metric
    return idx, sim


# ------------------------------------------------------------------ row norms
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (130, 576), (7, 131)])
def test_row_rnorm_is_exact_on_integer_rows(shape):
    from ssl_mae_amd import knn
    x = _ints(sum(shape), *shape)
    x[0] = 0                                               # a zero row: 0, not inf
    for offset in (False, True):
        t = torch.from_numpy(x).to(DEV)
        rn = knn.row_rnorm(_offset_view(t) if offset else t).cpu().numpy()
        assert _same_bits(rn, knn.rnorm_mirror(x)) and rn[0] == 0


# ------------------------------------------------------------------ exact cases
EXACT_SHAPES = [(1, 1, 1, 1), (5, 7, 3, 4), (3, 5, 8, 8), (70, 333, 37, 20), (64, 256, 576, 1), (130, 777, 576, 64)]
EXACT_CASES = [(s, False) for s in EXACT_SHAPES] + [(s, True) for s in EXACT_SHAPES[3:]]


@pytest.mark.parametrize("shape,offset", EXACT_CASES)
def test_topk_equals_the_mirror_on_integer_features(shape, offset):
    Nq, Nb, D, k = shape
    q, b = _ints(11 + D, Nq, D), _ints(12 + D, Nb, D)
    for metric in ("dot", "cosine"):
        idx, sim = _assert_matches_mirror(q, b, k, metric, offset=offset)
        if k > Nb:
            assert np.all(idx[:, Nb:] == -1) and np.all(np.isneginf(sim[:, Nb:])) and np.all(idx[:, :Nb] >= 0)


@pytest.mark.parametrize("shape,splits", [((70, 333, 37, 20), (1, 2, 3, 7)), ((130, 777, 576, 64), (1, 5, 16))])
def test_topk_is_bit_identical_for_every_split(shape, splits):
    Nq, Nb, D, k = shape
    q, b = _ints(11 + D, Nq, D), _ints(12 + D, Nb, D)
    for metric in ("dot", "cosine"):
        base_idx, base_sim = _assert_matches_mirror(q, b, k, metric, splits=0)
        for s in splits:
            idx, sim = _search(q, b, k, metric, splits=s)
            assert np.array_equal(idx, base_idx) and _same_bits(sim, base_sim), (metric, s)


def test_split_invariance_holds_on_real_valued_features():
    """The similarity of a pair has one summation order, so real-valued inputs split alike too."""
    rs = np.random.RandomState(5)
    q, b = rs.standard_normal((70, 40)).astype(np.float32), rs.standard_normal((333, 40)).astype(np.float32)
    base_idx, base_sim = _search(q, b, 20, "cosine")
    for s in (1, 2, 7):
        idx, sim = _search(q, b, 20, "cosine", splits=s)
        assert np.array_equal(idx, base_idx) and _same_bits(sim, base_sim), s
    idx, sim = _search(q, b, 20, "cosine", splits=3, offset=True)   # and the scalar load form
    assert np.array_equal(idx, base_idx) and _same_bits(sim, base_sim)


@pytest.mark.parametrize("order", ["ascending", "descending", "identical"])
def test_topk_adversarial_bank_orders(order):
    Nq, Nb, D, k = 64, 512, 16, 20
    q, b = _ints(21, Nq, D), _ints(22, Nb, D)
    if order == "identical":
        b[:] = b[0]
    else:
        key = b.astype(np.float64) @ q[0].astype(np.float64)       # similarity to the fixed query 0
        perm = np.argsort(key, kind="stable")
        b = np.ascontiguousarray(b[perm if order == "ascending" else perm[::-1]])
        d0 = b.astype(np.float64) @ q[0].astype(np.float64)
        assert np.all(np.diff(d0) >= 0) if order == "ascending" else np.all(np.diff(d0) <= 0)
    for metric in ("dot", "cosine"):
        idx, _ = _assert_matches_mirror(q, b, k, metric)
        if order == "identical":
            assert np.array_equal(idx, np.tile(np.arange(k, dtype=np.int32), (Nq, 1)))


# ------------------------------------------------------------------ leave-one-out
def test_leave_one_out_removes_the_offset_row():
    N, D, k = 70, 37, 20
    z = _ints(31, N, D)
    assert len({r.tobytes() for r in z}) == N              # distinct rows
    for metric in ("dot", "cosine"):
        for off in (0, 3):
            idx, _ = _assert_matches_mirror(z, z, k, metric, off=off)
            rows = np.arange(N)[:, None]
            assert not np.any(idx == rows + off)
    idx, _ = _assert_matches_mirror(z, z, k, "cosine")
    assert np.array_equal(idx[:, 0], np.arange(N))         # without it every query finds itself first
    idx, _ = _assert_matches_mirror(z, z, 64, "dot", off=69)   # only query 0 has its row 69 in the bank
    assert 69 not in idx[0] and 69 in idx[1]


# ------------------------------------------------------------------ non-finite similarities
def test_nan_comes_last_by_index_and_minus_inf_is_a_value():
    from ssl_mae_amd import knn
    Nq, Nb, D, k = 9, 50, 8, 50
    q, b = _ints(41, Nq, D, 1, 3), _ints(42, Nb, D)        # positive queries: a -inf feature gives a -inf dot
    b[7, 2] = np.nan
    b[30, 5] = np.nan
    b[19, 0] = -np.inf
    for splits in (0, 4):
        idx, sim = _search(q, b, k, "dot", splits=splits)
        want_idx, want_sim = knn.knn_mirror(q, b, k, "dot")
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(sim, want_sim, equal_nan=True)
        assert np.all(idx[:, -2:] == [7, 30]) and np.all(idx[:, -3] == 19)
        assert np.isnan(sim[:, -2:]).all() and np.isneginf(sim[:, -3]).all()
    idx, sim = _search(q, b, 5, "dot")                     # and none of them among the first five
    assert not np.isin(idx, [7, 19, 30]).any() and np.isfinite(sim).all()


# ------------------------------------------------------------------ real-valued inputs
@pytest.fixture(scope="module")
def real_cases():
    out = {}
    for D in (40, 576):
        rs = np.random.RandomState(100 + D)
        q, b = rs.standard_normal((70, D)).astype(np.float32), rs.standard_normal((333, D)).astype(np.float32)
        q64, b64 = q.astype(np.float64), b.astype(np.float64)
        rq, rb = 1.0 / np.sqrt((q64 ** 2).sum(1)), 1.0 / np.sqrt((b64 ** 2).sum(1))
        sim64 = (q64 @ b64.T) * rq[:, None] * rb[None, :]
        eps = (D + 2) * 2.0 ** -24 * (np.abs(q64) @ np.abs(b64).T) * rq[:, None] * rb[None, :]
        out[D] = (q, b, sim64, eps)
    return out


@pytest.mark.parametrize("D", [40, 576])
def test_topk_on_standard_normal_features(real_cases, D):
    q, b, sim64, eps = real_cases[D]
    Nq, Nb, k = 70, 333, 20
    idx, sim = _search(q, b, k, "cosine")
    rows = np.arange(Nq)[:, None]
    assert np.all(idx >= 0) and all(len(set(r.tolist())) == k for r in idx)
    err = np.abs(sim.astype(np.float64) - sim64[rows, idx]) / eps[rows, idx]
    print(f"D={D}: worst |sim - fp64| / eps = {err.max():.4f}")
    assert err.max() <= 1.0
    order64 = np.argsort(-sim64, axis=1, kind="stable")
    s_k = sim64[np.arange(Nq), order64[:, k - 1]][:, None]
    assert np.all(sim64[rows, idx] >= s_k - eps[rows, idx])
    excluded = np.ones((Nq, Nb), dtype=bool)
    excluded[rows, idx] = False
    assert np.all((sim64 <= s_k + eps)[excluded])
    assert np.all(np.diff(sim.astype(np.float64), axis=1) <= 0)           # the returned list is sorted
    if D == 40:
        top = order64[:, :k + 1]
        s, e = sim64[rows, top], eps[rows, top]
        ambiguous = np.any(s[:, :-1] - s[:, 1:] <= e[:, :-1] + e[:, 1:], axis=1)
        print(f"D={D}: {int(ambiguous.sum())} of {Nq} rows ambiguous")
        assert ambiguous.mean() <= 0.10
        assert np.array_equal(idx[~ambiguous], order64[~ambiguous, :k].astype(np.int32))


# ------------------------------------------------------------------ vote
def _vote(idx, sim, labels, C, inv_t, ks):
    from ssl_mae_amd import kernels as Kn
    out = Kn.knn_vote(torch.from_numpy(idx).to(DEV), torch.from_numpy(sim).to(DEV), torch.from_numpy(labels).to(DEV),
                      C, inv_t, ks)
    torch.cuda.synchronize()
    return out


def test_vote_matches_the_mirror_and_is_a_prefix_table(real_cases):
    from ssl_mae_amd import knn
    q, b, _, _ = real_cases[40]
    C, ks, inv_t = 7, [1, 5, 20], 1.0 / 0.07
    idx, sim = _search(q, b, 20, "cosine")
    labels = np.random.RandomState(51).randint(0, C, size=len(b)).astype(np.int64)
    labels[idx[0, 1]] = C + 3                              # labels outside [0, C) add nothing
    labels[idx[1, 0]] = -1
    idx, sim = idx.copy(), sim.copy()
    idx[2, 3] = -1                                         # an empty slot, an index past the bank and a NaN sim neither
    idx[3, 0] = len(b)
    sim[4, 2] = np.nan
    got = _vote(idx, sim, labels, C, inv_t, ks).cpu().numpy()
    want = knn.vote_mirror(idx, sim, labels, C, inv_t, ks)
    assert got.shape == want.shape == (3, 70, C)
    err, top = np.abs(got - want).max(axis=2), want.max(axis=2)
    assert np.all(err[top == 0] == 0) and (top == 0).any()  # a row whose only neighbours are ignored stays 0
    print(f"vote: worst error relative to the row's largest score = {(err[top > 0] / top[top > 0]).max():.3e}")
    assert np.all(err <= 1e-5 * top)
    for s, kv in enumerate(ks):                            # one pass fills what three single-k calls fill
        single = _vote(idx, sim, labels, C, inv_t, [kv]).cpu().numpy()
        assert _same_bits(got[s], single[0]), kv
    clean = knn.vote_mirror(idx, sim, np.where((labels < 0) | (labels >= C), 0, labels), C, inv_t, ks)
    assert want[0, 1].sum() == 0 and want[2, 0].sum() < clean[2, 0].sum()   # the ignored slots were live ones


def _distinct_weight_case():
    """Integer-valued similarities, strictly descending per query, inv_temperature = 0.25: weights
    e^(s / 4) are distinct within a query, so class scores are sums over disjoint weight sets."""
    rs = np.random.RandomState(61)
    Nq, k, Nb, C = 40, 20, 96, 7
    sim = np.stack([np.sort(rs.choice(np.arange(-30, 31), size=k, replace=False))[::-1] for _ in range(Nq)])
    idx = np.stack([rs.choice(Nb, size=k, replace=False) for _ in range(Nq)]).astype(np.int32)
    bank_labels = rs.randint(0, C, size=Nb).astype(np.int64)
    query_labels = rs.randint(0, C, size=Nq).astype(np.int64)
    return idx, np.ascontiguousarray(sim, dtype=np.float32), bank_labels, query_labels, C


def test_hit_counts_through_logits_metrics_equal_the_mirror():
    from ssl_mae_amd import kernels as Kn
    from ssl_mae_amd import knn
    idx, sim, yb, yq, C = _distinct_weight_case()
    ks, inv_t = [1, 5, 20], 0.25
    want = knn.vote_mirror(idx, sim, yb, C, inv_t, ks)
    ly = np.take_along_axis(want, np.broadcast_to(yq[None, :, None], (3, 40, 1)), axis=2)
    others = np.ones((1, 40, C), dtype=bool)
    others[0, np.arange(40), yq] = False
    both_zero = (want == 0) & (ly == 0)                    # an exact tie at 0: settled by the class index
    margin = np.abs(want - ly) / np.maximum(np.maximum(want, ly), 1e-300)
    assert np.all((margin >= 1e-3) | both_zero | ~others)
    scores = _vote(idx, sim, yb, C, inv_t, ks)
    out = Kn.logits_metrics(scores.view(3 * 40, C), torch.from_numpy(yq).to(DEV), 5, 3).cpu().numpy()
    top1, top5 = knn.metrics_mirror(want, yq, 5)
    assert out[:, 2].tolist() == top1.tolist() and out[:, 3].tolist() == top5.tolist()
    assert 0 < top1.sum() and np.all(top5 >= top1) and top5[2] > top1[2]


def test_vote_rejects_bad_ks():
    from ssl_mae_amd import _lib
    idx, sim, yb, _, C = _distinct_weight_case()
    for ks in ([], [0, 1], [5, 5], [5, 1], [1, 21], list(range(1, 10))):
        with pytest.raises(_lib.KernelError):
            _vote(idx, sim, yb, C, 0.25, ks)


def test_topk_rejects_unsupported_arguments():
    from ssl_mae_amd import _lib, kernels as Kn
    q, b = torch.zeros(4, 8, device=DEV), torch.zeros(6, 8, device=DEV)
    rq = torch.ones(4, device=DEV)
    for call in (lambda: Kn.knn_topk(q, b, None, None, 0), lambda: Kn.knn_topk(q, b, None, None, 65),
                 lambda: Kn.knn_topk(q, b, rq, None, 2), lambda: Kn.knn_topk(q, b[:, :4].contiguous(), None, None, 2),
                 lambda: Kn.knn_topk(q, b, None, None, 2, -1, -1), lambda: Kn.knn_topk(q, b, None, None, 2, -1, 5000),
                 lambda: Kn.knn_topk(q.cpu(), b.cpu(), None, None, 2)):
        with pytest.raises(_lib.KernelError):
            call()


# ------------------------------------------------------------------ knn_eval
def test_knn_eval_fused_equals_the_eager_reference():
    from ssl_mae_amd import knn
    Nb, Nq, D, C, ks = 96, 40, 576, 7, [1, 5, 10, 20]
    zb, zq = _ints(71, Nb, D), _ints(72, Nq, D)
    rs = np.random.RandomState(82)      # a label draw that keeps every compared pair of class scores apart (asserted)
    yb, yq = rs.randint(0, C, size=Nb).astype(np.int64), rs.randint(0, C, size=Nq).astype(np.int64)
    t = [torch.from_numpy(a).to(DEV) for a in (zq, yq, zb, yb)]
    for metric, loo in (("cosine", False), ("dot", False), ("cosine", True)):
        qa = (t[2], t[3]) if loo else (t[0], t[1])
        temp = 0.07 if metric == "cosine" else 40.0        # dot products reach +-200: keep exp finite
        fused = knn.knn_eval(*qa, t[2], t[3], ks, temp, C, metric, leave_one_out=loo)
        ref = knn.knn_eval(*qa, t[2], t[3], ks, temp, C, metric, leave_one_out=loo, impl="reference")
        assert torch.equal(fused["idx"], ref["idx"]) and torch.equal(fused["sim"], ref["sim"]), (metric, loo)
        # the class scores the hits are read from are well apart, so the two summation orders agree
        idx, sim = fused["idx"].cpu().numpy(), fused["sim"].cpu().numpy()
        want = knn.vote_mirror(idx, sim, yb, C, 1.0 / temp, ks)
        y = (yb if loo else yq)
        ly = np.take_along_axis(want, np.broadcast_to(y[None, :, None], (len(ks), len(y), 1)), axis=2)
        far = (np.abs(want - ly) >= 1e-3 * np.maximum(want, ly)) | ((want == 0) & (ly == 0))
        far[:, np.arange(len(y)), y] = True
        assert far.all(), (metric, loo)
        top1, top5 = knn.metrics_mirror(want, y, 5)
        assert fused["top1"] == ref["top1"] == (top1 / len(y)).tolist(), (metric, loo)
        assert fused["top5"] == ref["top5"] == (top5 / len(y)).tolist(), (metric, loo)
        assert fused["ks"] == ks
        if loo:
            assert not np.any(idx == np.arange(Nb)[:, None])

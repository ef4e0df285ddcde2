"""kNN evaluation without a GPU: the host mirrors of ssl_mae_amd/knn.py (the specification the
kernels are tested against) and run_knn's config resolution and CSV line.

The mirror is checked against a brute-force argsort of fp64 similarities on integer-valued
features (every similarity exact, ties frequent) with the stated rule: larger first, ties by lower
bank index, NaN last by index, padding idx = -1 / sim = -inf.
"""
import numpy as np
import pytest


def _ints(seed, n, d):
    return np.random.RandomState(seed).randint(-2, 3, size=(n, d)).astype(np.float32)


def _brute(sim_row, k, drop=None):
    """Python sort with the tie rule spelled out as a key."""
    cands = [j for j in range(len(sim_row)) if j != drop]
    cands.sort(key=lambda j: (np.isnan(sim_row[j]), 0.0 if np.isnan(sim_row[j]) else -sim_row[j], j))
    idx = cands[:k] + [-1] * (k - len(cands[:k]))
    sim = [sim_row[j] if j >= 0 else -np.inf for j in idx]
    return idx, sim


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (5, 7, 3, 4), (70, 333, 40, 20)])
def test_mirror_matches_brute_force_on_integer_features(shape):
    from ssl_mae_amd import knn
    Nq, Nb, D, k = shape
    q, b = _ints(1, Nq, D), _ints(2, Nb, D)
    dot = q.astype(np.float64) @ b.astype(np.float64).T
    idx, sim = knn.knn_mirror(q, b, k, metric="dot")
    ties = 0
    for i in range(Nq):
        want_idx, want_sim = _brute(dot[i], k)
        assert idx[i].tolist() == want_idx
        assert sim[i].tolist() == want_sim
        if k < Nb:
            ties += np.sort(dot[i])[::-1][k - 1] == np.sort(dot[i])[::-1][k]
    if shape == (70, 333, 40, 20):
        assert ties >= 20          # ties across the k boundary are the common case here
    assert sim.dtype == np.float32 and idx.dtype == np.int32


def test_mirror_cosine_is_two_separately_rounded_fp32_scalings():
    from ssl_mae_amd import knn
    q, b = _ints(3, 9, 12), _ints(4, 31, 12)
    b[5] = 0                                             # a zero row: similarity 0, not NaN
    rq, rb = knn.rnorm_mirror(q), knn.rnorm_mirror(b)
    assert rb[5] == 0 and np.all(np.isfinite(rq))
    ss = (b.astype(np.float64) ** 2).sum(1)
    nz = ss > 0
    assert np.array_equal(rb[nz], (np.float32(1) / np.sqrt(ss[nz].astype(np.float32))).astype(np.float32))
    dot = (q.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
    want = (dot * rq[:, None]).astype(np.float32) * rb[None, :]
    idx, sim = knn.knn_mirror(q, b, 31, metric="cosine")
    for i in range(9):
        assert np.array_equal(sim[i], want[i][idx[i]])
        assert idx[i].tolist() == _brute(want[i].astype(np.float64), 31)[0]
    assert not np.isnan(sim).any()


def test_mirror_pads_when_k_exceeds_the_bank_and_leaves_one_out():
    from ssl_mae_amd import knn
    q, b = _ints(5, 3, 8), _ints(6, 5, 8)
    idx, sim = knn.knn_mirror(q, b, 8, metric="dot")
    assert np.all(idx[:, 5:] == -1) and np.all(np.isneginf(sim[:, 5:]))
    assert all(sorted(idx[i, :5].tolist()) == [0, 1, 2, 3, 4] for i in range(3))
    z = _ints(7, 6, 8)
    dot = z.astype(np.float64) @ z.astype(np.float64).T
    for off in (0, 3):
        idx, sim = knn.knn_mirror(z, z, 6, metric="dot", leave_one_out_offset=off)
        for i in range(6):
            drop = i + off if i + off < 6 else None
            want_idx, want_sim = _brute(dot[i], 6, drop)
            assert idx[i].tolist() == want_idx and sim[i].tolist() == want_sim
            assert (i + off) not in idx[i].tolist()


def test_mirror_orders_nan_last_and_minus_inf_as_a_value():
    from ssl_mae_amd import knn
    q = np.ones((2, 2), dtype=np.float32)
    b = np.array([[1, 1], [np.nan, 0], [-np.inf, 0], [3, 0], [0, np.nan], [-0.0, 0.0], [0, 0]], dtype=np.float32)
    idx, sim = knn.knn_mirror(q, b, 7, metric="dot")
    assert idx[0].tolist() == [3, 0, 5, 6, 2, 1, 4]        # -0 == +0 by index; -inf before the NaNs; NaNs by index
    assert np.isneginf(sim[0, 4]) and np.isnan(sim[0, 5:]).all()


def test_vote_mirror_prefix_property_and_ignored_slots():
    from ssl_mae_amd import knn
    rs = np.random.RandomState(8)
    Nq, k, Nb, C = 6, 20, 50, 7
    idx = rs.randint(0, Nb, size=(Nq, k)).astype(np.int32)
    sim = rs.uniform(-1, 1, size=(Nq, k)).astype(np.float32)
    labels = rs.randint(0, C, size=Nb)
    labels[3] = C + 2                                    # out of range: adds nothing
    labels[4] = -1
    idx[0, 2] = -1
    sim[1, 0] = np.nan
    table = knn.vote_mirror(idx, sim, labels, C, 1 / 0.07, [1, 5, 20])
    for s, kv in enumerate((1, 5, 20)):
        single = knn.vote_mirror(idx, sim, labels, C, 1 / 0.07, [kv])
        assert np.array_equal(table[s], single[0])
    assert np.all(table[1] >= table[0]) and np.all(table[2] >= table[1])
    want = np.zeros((Nq, C))
    for i in range(Nq):
        for r in range(k):
            j = idx[i, r]
            if j >= 0 and 0 <= labels[j] < C and not np.isnan(sim[i, r]):
                want[i, labels[j]] += np.exp(np.float64(sim[i, r]) / 0.07)
    assert np.allclose(table[2], want, rtol=1e-12)
    assert table[0][1].sum() == 0                        # query 1's only k = 1 neighbour has a NaN sim


def test_metrics_mirror_tie_rule():
    from ssl_mae_amd import knn
    scores = np.array([[[1.0, 1.0, 0.5], [0.0, 0.0, 0.0], [3.0, 2.0, 1.0]]])
    top1, top2 = knn.metrics_mirror(scores, np.array([1, 0, 2]), 2)
    assert top1.tolist() == [1] and top2.tolist() == [2]  # row 0: class 0 wins the tie; row 1: label 0 wins it


def test_resolve_config_defaults_overrides_and_errors():
    from ssl_mae_amd import run_knn as R
    cfg = R.resolve_config({})
    assert cfg["knn"] == {"ks": [1, 5, 10, 20], "temperature": 0.07, "metric": "cosine", "leave_one_out": False,
                          "impl": "fused"}
    assert cfg["model"]["ckpts"] == [None] and cfg["output"]["save_dir"] == "results/knn"
    assert R.DEFAULTS["model"]["ckpts"] is None          # the defaults are not shared with a resolved config
    cfg = R.resolve_config({"knn": {"ks": [3, 64], "metric": "dot", "leave_one_out": True}, "model": {"ckpts": "a.pth"}},
                           ckpts=["b.pth", "c.pth"], save_dir="out", impl="reference")
    assert cfg["model"]["ckpts"] == ["b.pth", "c.pth"] and cfg["output"]["save_dir"] == "out"
    assert cfg["knn"]["ks"] == [3, 64] and cfg["knn"]["impl"] == "reference" and cfg["knn"]["leave_one_out"] is True
    assert R.resolve_config({"model": {"ckpts": "a.pth"}})["model"]["ckpts"] == ["a.pth"]
    bad = [{"knn": {"ks": [1, 65]}}, {"knn": {"ks": [5, 1]}}, {"knn": {"ks": [1, 1]}}, {"knn": {"ks": []}},
           {"knn": {"ks": [0, 1]}}, {"knn": {"ks": list(range(1, 10))}}, {"knn": {"ks": 5}},
           {"knn": {"ks": [1.5]}}, {"knn": {"temperature": 0}}, {"knn": {"metric": "l2"}}, {"knn": {"impl": "triton"}},
           {"knn": {"bogus": 1}}, {"bogus": {}}, {"dataset": {"val_split": "v.txt"}},
           {"dataset": {"train_split": "t.txt", "val_split": "v.txt"}, "knn": {"leave_one_out": True}},
           {"runtime": {"num_batches": 0}}, {"model": {"ckpts": [1, 2]}}]
    for c in bad:
        with pytest.raises(ValueError):
            R.resolve_config(c)


def test_shipped_config_resolves_to_the_defaults():
    import os
    from conftest import ROOT
    from ssl_mae_amd import run_knn as R
    from ssl_mae_amd.utils import load_config
    cfg = R.resolve_config(load_config(os.path.join(ROOT, "configs", "knn.yaml")))
    assert cfg == R.resolve_config({})


def test_csv_line_format():
    from ssl_mae_amd import run_knn as R
    assert R.CSV_HEADER == "ckpt,k,top1,top5,n_bank,n_query\n"
    row = {"ckpt": "runs/ssl_ep3.pth", "k": 20, "top1": 0.123456789, "top5": 2 / 3, "n_bank": 9537, "n_query": 3783}
    assert R.format_row(row) == "runs/ssl_ep3.pth,20,0.123457,0.666667,9537,3783\n"
    assert R.format_row(dict(row, ckpt="none", top1=1.0, top5=0)) == "none,20,1.0,0.0,9537,3783\n"

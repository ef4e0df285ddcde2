"""The DP-FedAvg round exchange (sm_fedavg_dp_exchange, federated.FedCohort.aggregate_dp,
dp_aggregate_reference, the run_federated driver with federated.dp enabled): norms against fp64,
scales and the noiseless update bit for bit against the numpy mirror, the noise against the draw
specification of privacy.perturb_draws, plain segments against the FedAvg oracle, in-place
aggregation, the grid-stride path, status codes, and the driver's fifth CSV."""
import copy
import csv
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

pytestmark = pytest.mark.gpu

SEG_LENS = (1, 3, 4, 5, 96, 257, 2048, 2049, 4099, 70_001)
SEG_CLIP = (1, 1, 0, 1, 1, 0, 1, 1, 1, 1)
# segment index -> the models whose copy of it starts 4 bytes off a 16-byte boundary
# (model 0 is theta, models 1..K the sources; -1 = the last source)
MISALIGNED = {4: (-1,), 8: (0,)}
CLIP = 1.0
# update norms as multiples of CLIP, client by client: one >= 1.5, one <= 0.5, none within 1 % of 1
TARGETS = (2.0, 0.3, 1.7, 0.45, 3.0, 0.8, 1.2, 0.1)
NUM_CHUNKS = sum(-(-n // 2048) for n in SEG_LENS)


def _segment(values, misaligned):
    """A device tensor holding `values`; misaligned: a `t[1:]` view (4-byte offset)."""
    n = len(values)
    base = torch.empty(n + 1, dtype=torch.float32, device="cuda")
    t = base[1:] if misaligned else base[:n]
    t.copy_(torch.from_numpy(values))
    assert (t.data_ptr() % 16 != 0) == bool(misaligned)
    return t


@functools.lru_cache(maxsize=None)
def _case(k, lens=SEG_LENS, modes=SEG_CLIP):
    """Host side of a cohort, computed once per k and never written: theta, the k sources theta +
    delta_c with the norm of delta_c over the clipped segments set to TARGETS, raw weights, their
    normalised fp32 values, and the fp64 update norms of the fp32 values."""
    from ssl_mae_amd import federated as F
    rng = np.random.default_rng(400 + k)
    theta = [rng.standard_normal(n).astype(np.float32) for n in lens]
    sources = []
    for c in range(k):
        d = [rng.standard_normal(n) for n in lens]
        nrm = np.sqrt(sum(float(np.sum(x * x)) for x, m in zip(d, modes) if m))
        scale = TARGETS[c % len(TARGETS)] * CLIP / nrm
        sources.append([(t.astype(np.float64) + x * scale).astype(np.float32) for t, x in zip(theta, d)])
    raw_w = [float(x) for x in rng.integers(1, 1000, k)]
    w = F._norm_weights(raw_w, float(sum(raw_w)))
    _, norms = F.dp_aggregate_mirror(theta, sources, w, modes, CLIP)
    # the clip decisions are far from borderline, so they cannot hide a failure
    assert np.all(np.isfinite(norms)) and np.all(np.abs(norms / CLIP - 1.0) > 0.01)
    if k >= 2:
        assert norms.max() >= 1.5 * CLIP and norms.min() <= 0.5 * CLIP
    return theta, sources, raw_w, w, norms


def _device(theta, sources, lens=SEG_LENS):
    k = len(sources)
    models = []
    for p, segs in enumerate([theta] + list(sources)):
        models.append([_segment(v, len(lens) > 1 and any((m if m >= 0 else k) == p for m in MISALIGNED.get(s, ())))
                       for s, v in enumerate(segs)])
    return models


def _restore(model, host):
    for t, v in zip(model, host):
        t.copy_(torch.from_numpy(v))


def _bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


def _seg_clip(modes=SEG_CLIP):
    return torch.tensor(modes, dtype=torch.uint8, device="cuda")


K_VALUES = [1, 2, 3, 4, 8, 32]


@pytest.mark.parametrize("k", K_VALUES)
def test_norms_and_scales(k):
    """Norms within 1e-5 relative of fp64 (the project's tolerance for fused reductions, SURVEY
    8(a) row A3); scales = min(1, C / (norm + 1e-6)) in np.float32 from the device's own norms,
    bit for bit; a second call on the same data gives the same bits."""
    from ssl_mae_amd import kernels as K
    theta, sources, _, w, norms64 = _case(k)
    models = _device(theta, sources)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    src = list(range(1, k + 1))
    stats = K.fedavg_dp_exchange(src, w, 0, [0], table, NUM_CHUNKS, _seg_clip(), CLIP, 0.0, 1).cpu().numpy()
    norms, scales = stats[:k], stats[k:]
    rel = np.abs(norms.astype(np.float64) - norms64) / norms64
    print(f"k={k}: largest relative norm error {rel.max():.3e}")
    assert np.all(rel <= 1e-5)
    want = np.minimum(np.float32(1.0), np.float32(CLIP) / (norms + np.float32(1e-6)))
    assert want.dtype == np.float32 and np.array_equal(scales.view(np.int32), want.view(np.int32))
    assert np.array_equal(scales < 1.0, norms64 > CLIP)
    _restore(models[0], theta)
    again = K.fedavg_dp_exchange(src, w, 0, [0], table, NUM_CHUNKS, _seg_clip(), CLIP, 0.0, 1).cpu().numpy()
    assert np.array_equal(again.view(np.int32), stats.view(np.int32))


@pytest.mark.parametrize("n", [5, 256 * 2048 + 1], ids=["1chunk", "257chunks"])
def test_norms_over_1_and_257_chunks(n):
    """One clipped segment of 1 chunk and of 257 chunks: the finalise block's 256 strided sums hold one
    partial in thread 0 only, and two in thread 0 next to one in every other thread.  The checks of
    test_norms_and_scales, and the update against the mirror bit for bit."""
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    k, lens, modes = 2, (n,), (1,)
    theta, sources, _, w, norms64 = _case(k, lens, modes)
    models = _device(theta, sources, lens)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    chunks = -(-n // 2048)
    stats = K.fedavg_dp_exchange([1, 2], w, 0, [0], table, chunks, _seg_clip(modes), CLIP, 0.0, 1).cpu().numpy()
    norms, scales = stats[:k], stats[k:]
    rel = np.abs(norms.astype(np.float64) - norms64) / norms64
    print(f"{chunks} chunks: largest relative norm error {rel.max():.3e}")
    assert np.all(rel <= 1e-5)
    want = np.minimum(np.float32(1.0), np.float32(CLIP) / (norms + np.float32(1e-6)))
    assert want.dtype == np.float32 and np.array_equal(scales.view(np.int32), want.view(np.int32))
    assert np.array_equal(scales < 1.0, norms64 > CLIP)
    mirror, _ = F.dp_aggregate_mirror(theta, sources, w, modes, CLIP, scales=scales)
    assert np.array_equal(_bits(models[0][0]), mirror[0].view(np.int32))


@pytest.mark.parametrize("k", K_VALUES)
def test_update_without_noise_is_the_mirror(k):
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    theta, sources, raw_w, w, _ = _case(k)
    models = _device(theta, sources)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    src = list(range(1, k + 1))
    stats = K.fedavg_dp_exchange(src, w, 0, [0], table, NUM_CHUNKS, _seg_clip(), CLIP, 0.0, 1).cpu().numpy()
    want, _ = F.dp_aggregate_mirror(theta, sources, w, SEG_CLIP, CLIP, scales=stats[k:])
    for s, n in enumerate(SEG_LENS):
        assert np.array_equal(_bits(models[0][s]), want[s].view(np.int32)), (k, n)
        if not SEG_CLIP[s]:
            plain = O.weighted_sum([sources[c][s] for c in range(k)], raw_w)
            assert np.array_equal(_bits(models[0][s]), plain.view(np.int32)), (k, n)
        for c in range(k):                                       # sources untouched
            assert np.array_equal(_bits(models[c + 1][s]), sources[c][s].view(np.int32)), (k, c, n)
    # in place: destinations = sources + theta give the same bits in every model
    _restore(models[0], theta)
    stats2 = K.fedavg_dp_exchange(src, w, 0, src + [0], table, NUM_CHUNKS, _seg_clip(), CLIP, 0.0, 1).cpu().numpy()
    assert np.array_equal(stats2.view(np.int32), stats.view(np.int32))
    for p in range(k + 1):
        for s, n in enumerate(SEG_LENS):
            assert np.array_equal(_bits(models[p][s]), want[s].view(np.int32)), (k, p, n)


def _noise_bound(out, clean, noise_std, n64):
    """|out - want| <= 1e-5 noise_std + 2^-23 |want|, want = clean + fp32(noise_std) n in fp64: the
    bound tests/test_privacy_gpu.py holds the generator to."""
    sig = float(np.float32(noise_std))
    want = clean.astype(np.float64) + sig * n64
    err = np.abs(out.astype(np.float64) - want)
    return err, 1e-5 * sig + 2.0 ** -23 * np.abs(want)


def test_update_with_noise():
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd import privacy as P
    k, noise_std, seed = 3, 0.25, F.dp_round_seed(42, 1)
    theta, sources, _, w, _ = _case(k)
    models = _device(theta, sources)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    src = [1, 2, 3]
    run = functools.partial(K.fedavg_dp_exchange, src, w, 0, [0], table, NUM_CHUNKS, _seg_clip(), CLIP)
    stats = run(noise_std, seed).cpu().numpy()
    out = [t.cpu().numpy() for t in models[0]]
    clean, _ = F.dp_aggregate_mirror(theta, sources, w, SEG_CLIP, CLIP, scales=stats[k:])
    h0, h1, _ = P.perturb_draws(seed, len(SEG_LENS), max(SEG_LENS))        # row = segment, column = element
    gauss = P.gaussian_from_draws(h0, h1)
    for s, n in enumerate(SEG_LENS):
        if SEG_CLIP[s]:
            err, bound = _noise_bound(out[s], clean[s], noise_std, gauss[s, :n])
            assert np.all(err <= bound), (n, float((err / bound).max()))
        else:                                                    # no noise on a plain segment
            assert np.array_equal(out[s].view(np.int32), clean[s].view(np.int32)), n
    big = out[-1].astype(np.float64) - clean[-1]
    assert 0.9 * noise_std < big.std() < 1.1 * noise_std         # the noise is really there
    _restore(models[0], theta)
    run(noise_std, seed)
    for s in range(len(SEG_LENS)):                               # same seed, same bits
        assert np.array_equal(_bits(models[0][s]), out[s].view(np.int32))
    _restore(models[0], theta)
    run(noise_std, F.dp_round_seed(42, 2))
    for s, n in enumerate(SEG_LENS):
        same = np.array_equal(_bits(models[0][s]), out[s].view(np.int32))
        assert same == (not SEG_CLIP[s]), n                      # another seed changes the clipped segments only


def test_grid_stride_and_noise_statistics():
    """One clipped segment of 2049 * 2048 + 5 elements: more chunks than the largest grid (2048
    blocks).  (out - mirror) / noise_std is the Gaussian: mean within 5 / sqrt(n) of 0, variance
    within 1 % of 1 (the estimator's standard deviation at n = 4.2 M is sqrt(2 / n) = 0.07 %)."""
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd import privacy as P
    n, k, noise_std, seed = 2049 * 2048 + 5, 2, 0.5, 0xDEADBEEF12345678
    theta, sources, _, w, norms64 = _case(k, (n,), (1,))
    models = _device(theta, sources, (n,))
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    stats = K.fedavg_dp_exchange([1, 2], w, 0, [0], table, 2050, _seg_clip((1,)), CLIP, noise_std, seed).cpu().numpy()
    assert np.all(np.abs(stats[:k].astype(np.float64) - norms64) <= 1e-5 * norms64)
    out = models[0][0].cpu().numpy()
    clean, _ = F.dp_aggregate_mirror(theta, sources, w, (1,), CLIP, scales=stats[k:])
    h0, h1, _ = P.perturb_draws(seed, 1, n)
    err, bound = _noise_bound(out, clean[0], noise_std, P.gaussian_from_draws(h0, h1)[0])
    assert np.all(err <= bound), float((err / bound).max())
    r = (out.astype(np.float64) - clean[0]) / noise_std
    print(f"noise mean {r.mean():.3e} (gate {5 / np.sqrt(n):.3e}), variance {r.var():.6f}")
    assert abs(r.mean()) <= 5.0 / np.sqrt(n)
    assert abs(r.var() - 1.0) <= 0.01


def test_status_codes():
    """-2 / -4 straight from the C entry point; nothing is written in any of these cases."""
    from ssl_mae_amd import _lib
    from ssl_mae_amd import kernels as K
    lib = _lib.load()
    models = [[torch.ones(8, device="cuda"), torch.ones(5, device="cuda")] for _ in range(3)]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    seg_clip = _seg_clip((1, 0))
    stats = torch.full((4,), -7.0, device="cuda")
    need = lib.sm_fedavg_dp_exchange_workspace_bytes(2, 2)
    assert need >= 2 * 2 * 8 and need % 16 == 0
    assert lib.sm_fedavg_dp_exchange_workspace_bytes(0, 2) == -1 and lib.sm_fedavg_dp_exchange_workspace_bytes(33, 2) == -1
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    p = ws.data_ptr()
    assert p % 16 == 0

    def call(src=(1, 2), weights=(0.5, 0.5), theta=0, dst=(0,), clip=1.0, noise=0.0, seg=seg_clip, w=p, w_bytes=need):
        ns = len(src)
        s = (ctypes.c_int32 * max(1, len(src)))(*src)
        d = (ctypes.c_int32 * max(1, len(dst)))(*dst)
        wt = (ctypes.c_float * max(1, len(weights)))(*weights)
        return lib.sm_fedavg_dp_exchange(ns, ctypes.cast(s, ctypes.c_void_p), ctypes.cast(wt, ctypes.c_void_p), theta,
                                         len(dst), ctypes.cast(d, ctypes.c_void_p), _lib.ptr(table), table.numel(),
                                         _lib.ptr(seg), clip, noise, 1, _lib.ptr(stats), ctypes.c_void_p(w),
                                         w_bytes, _lib.stream())

    assert call(clip=0.0) == -2 and call(clip=-1.0) == -2 and call(clip=float("nan")) == -2
    assert call(noise=-0.5) == -2 and call(noise=float("nan")) == -2
    assert call(src=(), weights=()) == -2                                            # num_src = 0
    assert call(src=(1,) * 33, weights=(1.0 / 33,) * 33) == -2                       # num_src = 33
    assert call(src=(1, 3)) == -2 and call(dst=(3,)) == -2                           # a model index of P
    assert call(theta=3) == -2 and call(theta=-1) == -2
    assert call(seg=None) == -2                                                      # null seg_clip
    assert call(w_bytes=need - 1) == -4                                              # short
    assert call(w=p + 8) == -4                                                       # misaligned
    assert call(w=0) == -4
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for m in models for t in m)
    assert bool((stats == -7.0).all()) and bool((ws == 0x5A).all())
    assert call() == 0                                                               # and the good call runs
    torch.cuda.synchronize()
    assert bool((stats[:2] == 0.0).all()) and bool((stats[2:] == 1.0).all())


def test_clipped_segment_longer_than_2_32_elements_is_refused():
    """A hand-built table of one segment and 2^21 + 1 chunk entries, the smallest that could hold
    a segment of more than 2^32 elements.  No launch touches its (null) addresses: every chunk
    entry points past the end of its segment, so the kernels skip it.  A clipped segment of
    2^32 + 1 elements is -2 with nothing written; 2^32 elements, or 2^32 + 1 unclipped, pass."""
    from ssl_mae_amd import _lib
    from ssl_mae_amd import kernels as K
    lib = _lib.load()
    C, S, P = (1 << 21) + 1, 1, 2
    total = (64 + 8 * P * S + 8 * S + 12 * C + 15) // 16 * 16
    need = lib.sm_fedavg_dp_exchange_workspace_bytes(1, C)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    stats = torch.full((2,), -7.0, device="cuda")

    def call(n, mode):
        header = np.array([K._FEDAVG_TABLE_MAGIC, P, S, C, 4, 2048, total, 0], dtype=np.int64)
        parts = (header, np.zeros(P * S, dtype=np.uint64), np.array([n], dtype=np.int64),
                 np.full(C, 1 << 40, dtype=np.int64), np.zeros(C, dtype=np.int32))
        raw = b"".join(a.tobytes() for a in parts)
        table = torch.frombuffer(bytearray(raw + b"\0" * (total - len(raw))), dtype=torch.uint8).cuda()
        src, dst, w = (ctypes.c_int32 * 1)(1), (ctypes.c_int32 * 1)(0), (ctypes.c_float * 1)(1.0)
        rc = lib.sm_fedavg_dp_exchange(1, ctypes.cast(src, ctypes.c_void_p), ctypes.cast(w, ctypes.c_void_p), 0, 1,
                                       ctypes.cast(dst, ctypes.c_void_p), _lib.ptr(table), table.numel(),
                                       _lib.ptr(_seg_clip((mode,))), 1.0, 0.5, 1, _lib.ptr(stats), _lib.ptr(ws),
                                       ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        return rc

    assert call((1 << 32) + 1, 1) == -2
    assert bool((stats == -7.0).all())
    assert call(1 << 32, 1) == 0 and stats.tolist() == [0.0, 1.0]
    stats.fill_(-7.0)
    assert call((1 << 32) + 1, 0) == 0 and stats.tolist() == [0.0, 1.0]


def test_nan_in_a_source_shows_in_its_norm():
    from ssl_mae_amd import kernels as K
    theta, sources, _, w, _ = _case(2)
    sources = [[x.copy() for x in src] for src in sources]
    sources[1][7][2048] = np.nan                                 # the second chunk of a clipped segment
    models = _device(theta, sources)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    stats = K.fedavg_dp_exchange([1, 2], w, 0, [0], table, NUM_CHUNKS, _seg_clip(), CLIP, 0.0, 1).cpu().numpy()
    assert np.isfinite(stats[0]) and np.isnan(stats[1]) and np.isnan(stats[3])


# ------------------------------------------------------------------ FedCohort on small models
W4 = [1200.0, 800.0, 1500.0, 500.0]
COHORT_CLIP = 0.5


def _net():
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Flatten(), nn.Linear(4 * 6 * 6, 5))


@pytest.fixture(scope="module")
def nets():
    """A global model and four clients = global + an update of norm about 0.06, 0.3, 1.5 and 3 (clip
    0.5), with their own running statistics and counters; never written: tests use deep copies."""
    torch.manual_seed(3)
    g = _net().cuda()
    clients = []
    for i, std in enumerate((0.002, 0.01, 0.05, 0.1)):
        m = copy.deepcopy(g)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * std)
            m[1].running_mean.add_(torch.randn(4, device="cuda"))
            m[1].running_var.mul_(1.0 + 0.1 * i)
            m[1].num_batches_tracked.fill_(3 * i + 1)
        clients.append(m)
    return [g] + clients


def _host_segments(model, keys):
    st = model.state_dict()
    return [st[k].detach().cpu().numpy().reshape(-1).copy() for k in keys]


def _check_cohort_result(models, nets, cohort, stats):
    from ssl_mae_amd import federated as F
    keys = cohort.float_keys
    modes = cohort._clip_modes
    assert sum(modes) == 6 and len(modes) == 8                   # 6 parameters, running_mean and running_var
    theta = _host_segments(nets[0], keys)
    sources = [_host_segments(m, keys) for m in nets[1:]]
    w = F._norm_weights(W4, float(sum(W4)))
    stats = stats.cpu().numpy()
    want, norms64 = F.dp_aggregate_mirror(theta, sources, w, modes, COHORT_CLIP, scales=stats[4:])
    assert np.all(np.abs(norms64 / COHORT_CLIP - 1.0) > 0.01) and (norms64 > COHORT_CLIP).tolist() == [False, False,
                                                                                                     True, True]
    assert np.all(np.abs(stats[:4] - norms64) <= 1e-5 * norms64)
    got = _host_segments(models[0], keys)
    ref = copy.deepcopy(nets[0])
    F.fedavg_aggregate(ref, [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in nets[1:]], W4)
    plain = _host_segments(ref, keys)
    moved = 0.0
    for s, k in enumerate(keys):
        if modes[s]:
            assert np.array_equal(got[s].view(np.int32), want[s].view(np.int32)), k
            moved += float(np.sum((got[s].astype(np.float64) - theta[s].astype(np.float64)) ** 2))
        else:                                                    # running statistics: fedavg_aggregate's
            assert "running_" in k and np.array_equal(got[s].view(np.int32), plain[s].view(np.int32)), k
    assert int(models[0][1].num_batches_tracked) == 10
    # the weights sum to 1 and every clipped update is at most clip_norm long
    assert np.sqrt(moved) <= COHORT_CLIP * (1 + 1e-5)
    for m, orig in zip(models[1:], nets[1:]):                    # sources untouched
        for (k, a), b in zip(m.state_dict().items(), orig.state_dict().values()):
            assert torch.equal(a, b), k


def test_cohort_aggregate_dp(nets):
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(nets)
    cohort = F.FedCohort(models[0], models[1:])
    stats = cohort.aggregate_dp([0, 1, 2, 3], W4, COHORT_CLIP, 0.0, seed=5)
    assert stats.is_cuda and stats.shape == (8,) and cohort.rebuilds == 1
    _check_cohort_result(models, nets, cohort, stats)


def test_cohort_dp_rebuilds_after_parameters_move(nets):
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(nets)
    cohort = F.FedCohort(models[0], models[1:])
    with torch.no_grad():
        for p in models[2].parameters():                         # what `.to()` does: new storage, same values
            p.data = p.data.clone()
    stats = cohort.aggregate_dp([0, 1, 2, 3], W4, COHORT_CLIP, 0.0, seed=5)
    assert cohort.rebuilds == 2
    _check_cohort_result(models, nets, cohort, stats)


def test_reference_agrees_with_the_fused_exchange(nets):
    """Noise 0.  Every parameter of dp_aggregate_reference within (K + 4) 2^-23 (|theta_i| + sum_c
    |ws_c d_c,i|) of the fused result: one rounding per subtraction, per product and for each of
    the K + 1 additions at 2^-24 each, doubled."""
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(nets)
    cohort = F.FedCohort(models[0], models[1:])
    stats = cohort.aggregate_dp([0, 1, 2, 3], W4, COHORT_CLIP, 0.0, seed=5).cpu().numpy()
    ref = copy.deepcopy(nets[0])
    states = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in nets[1:]]
    new_state, ref_stats = F.dp_aggregate_reference(ref, states, W4, COHORT_CLIP, 0.0, seed=5)
    assert list(new_state) == list(nets[0].state_dict())
    assert np.allclose(ref_stats.cpu().numpy(), stats, rtol=1e-5, atol=0.0)
    w = F._norm_weights(W4, float(sum(W4)))
    params = dict(nets[0].named_parameters())
    worst = 0.0
    for k, v in ref.state_dict().items():
        fused = models[0].state_dict()[k]
        if k in params:
            theta = params[k].detach().double()
            mag = theta.abs()
            for c in range(4):
                mag = mag + (float(w[c]) * float(stats[4 + c]) * (states[c][k].double() - theta)).abs()
            ratio = ((v.double() - fused.double()).abs() / ((4 + 4) * 2.0 ** -23 * mag)).max().item()
            worst = max(worst, ratio)
            assert ratio <= 1.0, (k, ratio)
        else:
            assert torch.equal(v, fused), k                      # buffers and counters: the same rules
    print(f"largest |reference - fused| / bound {worst:.3f}")


# ------------------------------------------------------------------ driver end to end
NC, T, S = 4, 2, 112
DP_HEADER = ["round", "clients", "dp_clipped", "dp_norm_mean", "dp_norm_max", "dp_noise_std", "epsilon_est", "delta"]
CSVS = ("fed_summary.csv", "fed_dp_summary.csv", "fed_client_stats.csv", "system_privacy_summary.csv")


def _config(tmp_path, name, exchange, dp):
    fed = {"num_clients": 3, "rounds": 2, "local_epochs": 1, "batch_size": 2, "exchange": exchange,
           "non_iid": {"shards_per_client": 1, "min_samples_per_client": 2}}
    if dp is not None:
        fed["dp"] = dp
    cfg = {"dataset": {"num_classes": NC, "clip_len": T, "image_size": S}, "federated": fed,
           "centralized": {"enabled": False}, "synthetic": {"num_train": 6, "num_val": 2},
           "output": {"save_dir": str(tmp_path / name)}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), tmp_path / name


def _rows(path):
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _check_dp_csv(out_dir):
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import run_federated as R
    head, rows = _rows(out_dir / "fed_dp_summary.csv")
    assert head == DP_HEADER == list(R.DP_COLUMNS) and [r[0] for r in rows] == ["1", "2"]
    _, stats = _rows(out_dir / "fed_client_stats.csv")
    sizes = [float(s[1]) for s in stats]
    noise_std = 0.5 * 0.5 * max(F._norm_weights(sizes, sum(sizes)))
    eps = [float(r[6]) for r in rows]
    assert all(np.isfinite(e) and e > 0.0 for e in eps) and eps[0] <= eps[1]
    for r in rows:
        assert r[1] == "3" and 0 <= int(r[2]) <= 3 and 0.0 < float(r[3]) <= float(r[4])
        assert float(r[5]) == round(noise_std, 6) and float(r[7]) == 1e-5
    head, _ = _rows(out_dir / "fed_summary.csv")
    assert head == list(R.FED_COLUMNS)
    assert "dp_clipped=" in (out_dir / "federated.log").read_text()


def test_driver_with_dp_is_reproducible(tmp_path):
    """3 clients, 2 rounds, T=2, 112^2, 4 classes on synthetic clips with clip_norm 0.5 and noise
    multiplier 0.5: the fifth CSV, and byte-identical files from a second run with the same seed."""
    from ssl_mae_amd import run_federated as R
    dp = {"enabled": True, "clip_norm": 0.5, "noise_multiplier": 0.5}
    cfg_a, dir_a = _config(tmp_path, "a", "fused", dp)
    cfg_b, dir_b = _config(tmp_path, "b", "fused", dp)
    R.main(["--config", cfg_a])
    _check_dp_csv(dir_a)
    R.main(["--config", cfg_b])
    for name in CSVS:
        assert (dir_a / name).read_text() == (dir_b / name).read_text(), name


def test_driver_reference_exchange_with_dp_and_dp_disabled(tmp_path):
    from ssl_mae_amd import run_federated as R
    cfg_ref, dir_ref = _config(tmp_path, "ref", "fused", {"enabled": True, "clip_norm": 0.5, "noise_multiplier": 0.5})
    R.main(["--config", cfg_ref, "--exchange", "reference"])
    _check_dp_csv(dir_ref)
    assert "exchange=reference" in (dir_ref / "federated.log").read_text()
    cfg_off, dir_off = _config(tmp_path, "off", "fused", {"enabled": False, "clip_norm": 0.5, "noise_multiplier": 0.5})
    R.main(["--config", cfg_off])
    assert (dir_off / "fed_summary.csv").exists() and not (dir_off / "fed_dp_summary.csv").exists()
    assert "dp_" not in (dir_off / "federated.log").read_text()

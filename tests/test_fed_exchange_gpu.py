"""The one-launch FedAvg round exchange (sm_fedavg_exchange / _counters, federated.FedCohort,
run_fedavg_fused): bit-exact against the numpy oracle over ragged, partly misaligned segments,
bit copies, in-place aggregation, status codes, and equality with the fedavg_aggregate /
run_fedavg path on whole models."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

# 2047, 2048, 2049: the edge of a 2048-element chunk, with and without a whole last 4-element group
SEG_LENS = (1, 3, 4, 5, 96, 257, 4099, 1_000_003, 2047, 2048, 2049)
# segment index -> the models whose copy of it starts 4 bytes off a 16-byte boundary
# (model 0 is the destination, models 1..K the sources; -1 = the last source)
MISALIGNED = {4: (-1,), 6: (0,)}


def _segment(values, misaligned):
    """A device tensor holding `values`; misaligned: a `t[1:]` view (4-byte offset)."""
    n = len(values)
    base = torch.empty(n + 1, dtype=torch.float32, device="cuda")
    t = base[1:] if misaligned else base[:n]
    t.copy_(torch.from_numpy(values))
    assert (t.data_ptr() % 16 != 0) == bool(misaligned)
    return t


def _cohort(k, seed):
    """-> (models [k + 1][S] device tensors, host arrays of the k sources, raw weights)."""
    rng = np.random.default_rng(seed)
    host = []
    for j in range(k):
        segs = [(rng.standard_normal(n) * 10 ** rng.uniform(-3, 3)).astype(np.float32) for n in SEG_LENS]
        host.append(segs)
    # specials in the 96-element segment: -0.0 in every source, a NaN, an inf and inf - inf
    for j in range(k):
        host[j][4][5] = -0.0
    host[0][4][7] = np.nan
    host[0][4][9] = np.inf
    host[k - 1][4][11] = -np.inf
    if k > 1:
        host[0][4][11] = np.inf
    models = []
    for p in range(k + 1):
        segs = []
        for s, n in enumerate(SEG_LENS):
            mis = any((m if m >= 0 else k) == p for m in MISALIGNED.get(s, ()))
            vals = host[p - 1][s] if p > 0 else np.full(n, 7.0, dtype=np.float32)
            segs.append(_segment(vals, mis))
        models.append(segs)
    w = [float(x) for x in rng.integers(1, 1000, k)]
    return models, host, w


def _assert_bits(got, want, what):
    """Bit equality; where the oracle has a NaN the result must be a NaN (IEEE 754 leaves the
    payload of an arithmetic NaN to the implementation)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), what


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 32])
def test_exchange_bit_exact_and_in_place(k):
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    models, host, w = _cohort(k, 100 + k)
    norm = F._norm_weights(w, float(sum(w)))
    table, addr = K.fedavg_exchange_table(models, torch.float32)
    assert len(addr) == (k + 1) * len(SEG_LENS)
    src = list(range(1, k + 1))
    K.fedavg_exchange(src, norm, [0], table)
    with np.errstate(invalid="ignore"):                          # inf - inf in the specials
        want = [O.weighted_sum([host[j][s] for j in range(k)], w) for s in range(len(SEG_LENS))]
    for s, n in enumerate(SEG_LENS):
        _assert_bits(models[0][s].cpu().numpy(), want[s], (k, n))
        for j in range(k):                                     # sources untouched
            assert np.array_equal(models[j + 1][s].cpu().numpy().view(np.int32), host[j][s].view(np.int32))
    assert not np.signbit(want[4][5]) and not np.signbit(np.float32(models[0][4][5].item()))   # +0 + (-0 w) = +0
    # in place: destinations = sources + global equals the out-of-place result bit for bit
    out = [models[0][s].cpu().numpy().copy() for s in range(len(SEG_LENS))]
    for seg in models[0]:
        seg.fill_(-1.0)
    K.fedavg_exchange(src, norm, src + [0], table)
    for p in range(k + 1):
        for s, n in enumerate(SEG_LENS):
            got = models[p][s].cpu().numpy()
            nan = np.isnan(out[s])
            assert np.array_equal(np.isnan(got), nan), (k, p, n)
            assert np.array_equal(got.view(np.int32)[~nan], out[s].view(np.int32)[~nan]), (k, p, n)


def test_copy_only_is_a_bit_copy():
    from ssl_mae_amd import kernels as K
    rng = np.random.default_rng(3)
    src = [rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32) for n in SEG_LENS]
    # -0.0, a quiet and a signalling NaN with payloads, -inf
    src[4][:4] = np.array([0x80000000, 0x7fc12345, 0x7f812345, 0xff800000], dtype=np.uint32).view(np.int32)
    models = []
    for p in range(4):
        segs = []
        for s, n in enumerate(SEG_LENS):
            mis = p in {4: (3,), 6: (0,)}.get(s, ())
            vals = src[s].view(np.float32) if p == 0 else np.zeros(n, dtype=np.float32)
            segs.append(_segment(vals, mis))
        models.append(segs)
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    K.fedavg_exchange([0], [1.0], [1, 2, 3], table, copy_only=True)
    for p in range(4):
        for s in range(len(SEG_LENS)):
            assert np.array_equal(models[p][s].cpu().numpy().view(np.int32), src[s]), (p, SEG_LENS[s])


@pytest.mark.parametrize("k", [3, 5])           # a compile-time and a runtime source count
def test_exchange_into_a_misaligned_destination_only(k):
    """A multi-chunk segment that is 16-byte aligned in every source and in one destination, and 4
    bytes off in another destination that is no source: both receive the oracle's bits."""
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    n = 4099                                     # two whole chunks and a 3-element tail
    rng = np.random.default_rng(40 + k)
    host = [rng.standard_normal(n).astype(np.float32) for _ in range(k)]
    w = [float(x) for x in rng.integers(1, 1000, k)]
    fill = np.full(n, 7.0, dtype=np.float32)
    models = [[_segment(fill, True)]] + [[_segment(h, False)] for h in host] + [[_segment(fill, False)]]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    K.fedavg_exchange(list(range(1, k + 1)), F._norm_weights(w, float(sum(w))), [0, k + 1], table)
    want = O.weighted_sum(host, w)
    _assert_bits(models[0][0].cpu().numpy(), want, (k, "misaligned destination"))
    _assert_bits(models[k + 1][0].cpu().numpy(), want, (k, "aligned destination"))
    for j in range(k):                           # sources untouched
        assert np.array_equal(models[j + 1][0].cpu().numpy().view(np.int32), host[j].view(np.int32))


def test_copy_only_into_a_misaligned_destination():
    from ssl_mae_amd import kernels as K
    n = 2049                                     # a whole chunk and a chunk of one element
    rng = np.random.default_rng(5)
    src = rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int64).astype(np.int32)
    src[-4:] = np.array([0x80000000, 0x7fc12345, 0x7f812345, 0xff800000], dtype=np.uint32).view(np.int32)
    zeros = np.zeros(n, dtype=np.float32)
    models = [[_segment(src.view(np.float32), False)], [_segment(zeros, True)], [_segment(zeros, False)]]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    K.fedavg_exchange([0], [1.0], [1, 2], table, copy_only=True)
    for p in range(3):
        assert np.array_equal(models[p][0].cpu().numpy().view(np.int32), src), p


def test_exchange_counters_max():
    from ssl_mae_amd import kernels as K
    c = [torch.zeros(4, dtype=torch.int64, device="cuda"),
         torch.tensor([3, -5, 1 << 40, 7], dtype=torch.int64, device="cuda"),
         torch.tensor([9, -6, 2, 7], dtype=torch.int64, device="cuda")]
    big = [torch.arange(5000, dtype=torch.int64, device="cuda") * s for s in (0, 1, -1)]   # three chunks
    table, _ = K.fedavg_exchange_table([[c[p], big[p]] for p in range(3)], torch.int64)
    K.fedavg_exchange_counters([1, 2], [0, 2], table)
    assert c[0].tolist() == [9, -5, 1 << 40, 7] and c[2].tolist() == [9, -5, 1 << 40, 7]
    assert c[1].tolist() == [3, -5, 1 << 40, 7]
    assert torch.equal(big[0], torch.arange(5000, device="cuda")) and torch.equal(big[2], big[0])


def test_exchange_status_codes():
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd._lib import KernelError
    models = [[torch.ones(8, device="cuda"), torch.ones(5, device="cuda")] for _ in range(3)]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    counters, _ = K.fedavg_exchange_table([[torch.ones(3, dtype=torch.int64, device="cuda")] for _ in range(3)],
                                          torch.int64)
    with pytest.raises(KernelError):
        K.fedavg_exchange([1] * 33, [1.0 / 33] * 33, [0], table)          # 33 sources
    with pytest.raises(KernelError):
        K.fedavg_exchange([1, 3], [0.5, 0.5], [0], table)                 # a model index of P
    with pytest.raises(KernelError):
        K.fedavg_exchange([1, 2], [0.5, 0.5], [3], table)
    with pytest.raises(KernelError):
        K.fedavg_exchange([1, 2], [0.5, 0.5], [0], table[:-16])           # a truncated table
    with pytest.raises(KernelError):
        K.fedavg_exchange([1, 2], [0.5, 0.5], [0], table, copy_only=True)  # copy_only with 2 sources
    with pytest.raises(KernelError):
        K.fedavg_exchange([1, 2], [0.5, 0.5], [0], counters)              # an int64 table
    with pytest.raises(KernelError):
        K.fedavg_exchange_counters([1, 3], [0], counters)
    with pytest.raises(KernelError):
        K.fedavg_exchange_counters([1], [0], counters[:-16])
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for m in models for t in m)           # nothing was launched


# ------------------------------------------------------------------ FedCohort on whole models
@pytest.fixture(scope="module")
def classifiers():
    """Five VideoClassifier(7, 112^2) models with different seeds and per-client counters; never
    run and never written: each test works on deep copies."""
    from ssl_mae_amd.finetune import VideoClassifier
    models = []
    for s in range(5):
        torch.manual_seed(s)
        models.append(VideoClassifier(7, img_size=112).cuda())
    for i, m in enumerate(models):
        for name, b in m.named_buffers():
            if "num_batches_tracked" in name:
                b.fill_(3 * i + 1)
    return models


def _states(models):
    return [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in models]


def _assert_states_equal(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


W4 = [1200.0, 800.0, 1500.0, 500.0]


def test_cohort_aggregate_equals_fedavg_aggregate(classifiers):
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(classifiers)
    ref_global = copy.deepcopy(classifiers[0])
    keys = list(ref_global.state_dict())
    assert any(k.startswith("classifier.") for k in keys) and any("running_var" in k for k in keys)
    assert any("num_batches_tracked" in k for k in keys)
    F.fedavg_aggregate(ref_global, _states(classifiers[1:]), W4)
    cohort = F.FedCohort(models[0], models[1:])
    cohort.aggregate([0, 1, 2, 3], W4)
    _assert_states_equal(models[0].state_dict(), ref_global.state_dict())
    for m, orig in zip(models[1:], classifiers[1:]):            # sources untouched
        _assert_states_equal(m.state_dict(), orig.state_dict())
    # a subset in another order, written into the global model and two clients as well
    ref2 = copy.deepcopy(classifiers[0])
    F.fedavg_aggregate(ref2, _states([classifiers[3], classifiers[1]]), [5.0, 2.0])
    cohort.aggregate([2, 0], [5.0, 2.0], also=[0, 3])
    for m in (models[0], models[1], models[4]):
        _assert_states_equal(m.state_dict(), ref2.state_dict())
    cohort.broadcast([1])
    _assert_states_equal(models[2].state_dict(), ref2.state_dict())
    assert cohort.rebuilds == 1


def test_cohort_rebuilds_after_parameters_move(classifiers):
    """The first forward re-homes the backbone's parameters into its flat buffer: a cohort built
    before it holds stale addresses and has to notice."""
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(classifiers)
    cohort = F.FedCohort(models[0], models[1:])
    before = [next(m.backbone.parameters()).data_ptr() for m in models]
    clip = torch.randn(1, 3, 1, 112, 112, device="cuda")
    with torch.no_grad():
        for m in models:
            m.eval()
            m(clip)
    after = [next(m.backbone.parameters()).data_ptr() for m in models]
    assert all(a != b for a, b in zip(after, before))
    ref_global = copy.deepcopy(classifiers[0])
    F.fedavg_aggregate(ref_global, _states(models[1:]), W4)
    cohort.aggregate([0, 1, 2, 3], W4)
    assert cohort.rebuilds == 2
    _assert_states_equal(models[0].state_dict(), ref_global.state_dict())
    cohort.broadcast([0, 1, 2, 3])
    assert cohort.rebuilds == 2
    for m in models[1:]:
        _assert_states_equal(m.state_dict(), ref_global.state_dict())


class Net(nn.Module):   # the entries of test_fedavg_gpu.py's Net
    def __init__(self, fc_out=13, extra_dtype=torch.float32, more=False):
        super().__init__()
        self.conv = nn.Conv2d(3, 8, 3, bias=False)
        self.bn = nn.BatchNorm2d(8)
        self.fc = nn.Linear(37, fc_out)
        self.register_buffer("idx", torch.arange(5, dtype=torch.int32))
        self.register_buffer("extra", torch.zeros(3, dtype=extra_dtype))
        if more:
            self.register_buffer("more", torch.zeros(2))


def test_cohort_validation():
    from ssl_mae_amd import federated as F
    g = Net().cuda()
    with pytest.raises(RuntimeError, match="keys differ"):
        F.FedCohort(g, [Net().cuda(), Net(more=True).cuda()])
    with pytest.raises(RuntimeError, match="fc.weight"):
        F.FedCohort(g, [Net(fc_out=12).cuda()])
    with pytest.raises(RuntimeError, match="fedavg_aggregate"):
        F.FedCohort(Net(extra_dtype=torch.bfloat16).cuda(), [Net(extra_dtype=torch.bfloat16).cuda()])
    with pytest.raises(RuntimeError, match="one cuda device"):
        F.FedCohort(g, [Net()])
    cohort = F.FedCohort(g, [Net().cuda()])
    with pytest.raises(RuntimeError, match="length mismatch"):
        cohort.aggregate([0], [1.0, 2.0])
    with pytest.raises(RuntimeError, match="No client states"):
        cohort.aggregate([], [])
    with pytest.raises(RuntimeError, match="must be > 0"):
        cohort.aggregate([0], [0.0])
    with pytest.raises(RuntimeError, match="no client 1"):
        cohort.aggregate([1], [1.0])


def test_run_fedavg_fused_equals_run_fedavg():
    """3 rounds, 5 clients, client_fraction 0.6: random.Random(42) selects [0,4,2], [2,1,0],
    [1,0,2].  The update perturbs every parameter from a generator seeded by (client, call
    count) and bumps the counters and the integer buffer."""
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    assert O.client_schedule(5, 3, 0.6) == [[0, 4, 2], [2, 1, 0], [1, 0, 2]]
    torch.manual_seed(11)
    g0 = Net().cuda()
    c0 = [Net().cuda() for _ in range(5)]
    sizes = [120, 45, 300, 77, 210]

    def world(run):
        g, clients = copy.deepcopy(g0), copy.deepcopy(c0)
        calls, snaps = [0] * 5, []

        def update_fn(cid):
            def fn(model):
                calls[cid] += 1
                gen = torch.Generator().manual_seed(1000 * cid + calls[cid])
                with torch.no_grad():
                    for p in model.parameters():
                        p.add_(torch.randn(p.shape, generator=gen).cuda() * 0.05)
                    model.bn.running_mean.add_(torch.randn(8, generator=gen).cuda())
                    model.bn.num_batches_tracked.add_(cid + calls[cid])
                    model.idx.add_(cid + 1)
                return 0.25 * cid + calls[cid]
            return fn

        def evaluate_fn(model):
            assert model is g
            snaps.append(_states([g] + clients))
            s = float(model.fc.weight.double().sum())
            return s, 2.0 * s

        loaders = [{"loader": None, "update_fn": update_fn(cid)} for cid in range(5)]
        recs = run(g, clients, loaders, sizes, evaluate_fn, torch.device("cuda"), rounds=3, client_fraction=0.6)
        return recs, snaps

    recs_ref, snaps_ref = world(F.run_fedavg)
    recs, snaps = world(F.run_fedavg_fused)
    assert recs == recs_ref and [r["clients"] for r in recs] == [3, 3, 3]
    assert len(snaps) == len(snaps_ref) == 3
    for rnd, rnd_ref in zip(snaps, snaps_ref):
        for st, st_ref in zip(rnd, rnd_ref):
            _assert_states_equal(st, st_ref)

"""The compressed FedAvg round exchange (sm_fedavg_q8_exchange, federated.FedCohort.aggregate_q8,
q8_aggregate_reference, the run_federated driver with federated.compress enabled): results,
residuals, codes, scales and chunk statistics bit for bit against the numpy mirror, the payload
decoded on the host, in-place aggregation, the grid-stride path, status codes, a NaN in a client,
residuals across rounds and table rebuilds, the fused loop against the reference loop, and the
driver's compression CSV."""
import copy
import csv
import ctypes
import functools
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
import yaml

pytestmark = pytest.mark.gpu

f32 = np.float32
CHUNK = 2048
# float entries in state order: (length, kind); "special" holds an all-zero block, a block below
# 1e-30 and an ordinary block
SEGS = ((1, "p"), (3, "p"), (4, "p"), (5, "p"), (255, "p"), (256, "p"), (300, "buffer"), (257, "p"), (2047, "p"),
        (2048, "p"), (2049, "p"), (4099, "p"), (768, "special"))
LENS = tuple(n for n, _ in SEGS)
MODES = tuple(0 if kind == "buffer" else 1 for _, kind in SEGS)
NUM_CHUNKS = sum(-(-n // CHUNK) for n in LENS)
K_VALUES = (1, 3, 5, 8)


class Leaf(nn.Module):
    """One state entry: a parameter `w` or a buffer `running_w`; misaligned: a `t[1:]` view, 4
    bytes off a 16-byte boundary."""

    def __init__(self, values, buffer, misaligned):
        super().__init__()
        n = len(values)
        base = torch.empty(n + 1, dtype=torch.float32, device="cuda")
        t = base[1:] if misaligned else base[:n]
        t.copy_(torch.from_numpy(values))
        assert (t.data_ptr() % 16 != 0) == bool(misaligned)
        if buffer:
            self.register_buffer("running_w", t)
        else:
            self.w = nn.Parameter(t)


class Counter(nn.Module):
    def __init__(self, value):
        super().__init__()
        self.register_buffer("num_batches_tracked", torch.tensor(value, dtype=torch.int64, device="cuda"))


def _model(segments, counter):
    """Every third float entry misaligned, an int64 counter after the fourth."""
    leaves = [Leaf(v, MODES[s] == 0, s % 3 == 2) for s, v in enumerate(segments)]
    leaves.insert(4, Counter(counter))
    return nn.Sequential(*leaves)


@functools.lru_cache(maxsize=None)
def _case(k):
    """Host side of a cohort, computed once per k and never written: theta, k sources, k starting
    residuals, raw weights, their normalised fp32 values and the mirror's answer."""
    from ssl_mae_amd import federated as F
    rng = np.random.default_rng(800 + k)
    theta = [rng.standard_normal(n).astype(f32) for n in LENS]
    sources = [[t + (f32(0.02) * rng.standard_normal(t.size)).astype(f32) for t in theta] for _ in range(k)]
    resid = [[(f32(2e-4) * rng.standard_normal(t.size)).astype(f32) for t in theta] for _ in range(k)]
    sp = len(LENS) - 1
    theta[sp][:512] = 0.0
    for c in range(k):
        resid[c][sp][:512] = 0.0
        sources[c][sp][:256] = 0.0                                             # v = 0 over the block
        sources[c][sp][256:512] = (f32(1e-31) * rng.uniform(-1, 1, 256)).astype(f32)
        sources[c][sp][300] = f32(9e-31)                                       # the block's maximum, below 1e-30
    raw_w = [float(x) for x in rng.integers(1, 1000, k)]
    w = F._norm_weights(raw_w, float(sum(raw_w)))
    want = F.q8_aggregate_mirror(theta, sources, resid, w, MODES, with_part=True)
    for c in range(k):                                           # the special blocks are what they claim to be
        assert want[3][c][sp][0] == 0.0 and want[3][c][sp][1] == 0.0 and want[3][c][sp][2] > 0.0
        assert np.any(want[1][c][sp][256:512] != 0.0)
    return theta, sources, resid, raw_w, w, want


def _rows(per_client, dtype=f32, per=CHUNK, lens=LENS):
    """K lists of S per-entry arrays -> the kernel's layout [K, chunks * per] with `per` values per
    chunk (2048 elements, or 8 scales), every entry padded with zeros to whole chunks."""
    out = np.zeros((len(per_client), sum(-(-n // CHUNK) for n in lens) * per), dtype=dtype)
    for c, segs in enumerate(per_client):
        o = 0
        for n, a in zip(lens, segs):
            out[c, o:o + a.size] = a
            o += -(-n // CHUNK) * per
    return out


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.reshape(-1).view({1: np.int8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _float_entries(model):
    return [v for v in model.state_dict().values() if v.is_floating_point()]


def _cohort(k):
    from ssl_mae_amd import federated as F
    theta, sources, resid, _, _, _ = _case(k)
    models = [_model(theta, 7)] + [_model(src, 3 * c + 1) for c, src in enumerate(sources)]
    cohort = F.FedCohort(models[0], models[1:])
    assert cohort._clip_modes == list(MODES) and cohort._float_chunks == NUM_CHUNKS and len(cohort.count_keys) == 1
    cohort._residuals().copy_(torch.from_numpy(_rows(resid)))
    return models, cohort


def _check_against_mirror(k, models, cohort, part, dst=(0,)):
    out, new_res, _, _, want_part = _case(k)[5]
    for p in dst:
        for s, t in enumerate(_float_entries(models[p])):
            assert np.array_equal(_bits(t), _bits(out[s])), (k, p, LENS[s])
    assert np.array_equal(_bits(cohort._residuals()), _bits(_rows(new_res))), k
    got = part.cpu().numpy()
    assert got.shape == (k, NUM_CHUNKS, 2)
    assert np.array_equal(got[:, :, 0], want_part[:, :, 0])                  # the chunk maximum is exact
    assert np.array_equal(_bits(got[:, :, 1]), _bits(want_part[:, :, 1])), k
    assert int(models[0][4].num_batches_tracked) == 3 * (k - 1) + 1         # the counters' max


@pytest.mark.parametrize("k", K_VALUES)
def test_kernel_is_the_mirror(k):
    """Results, residuals, codes, scales and chunk statistics, bit for bit: templated (1, 3, 8) and
    runtime (5) source counts, 16-byte and element-wise chunks, a plain segment in the middle,
    non-zero starting residuals, an all-zero block and a block below 1e-30."""
    _, sources, _, raw_w, _, want = _case(k)
    models, cohort = _cohort(k)
    part, (codes, scales) = cohort.aggregate_q8(list(range(k)), raw_w, payload=True)
    assert part.is_cuda and part.dtype == torch.float64 and cohort.rebuilds == 1
    _check_against_mirror(k, models, cohort, part)
    assert codes.shape == (k, NUM_CHUNKS, CHUNK) and codes.dtype == torch.int8
    assert scales.shape == (k, NUM_CHUNKS, CHUNK // 256) and scales.dtype == torch.float32
    assert np.array_equal(_bits(codes), _bits(_rows(want[2], np.int8)))
    assert np.array_equal(_bits(scales), _bits(_rows(want[3], f32, CHUNK // 256)))
    for c in range(k):                                           # sources untouched
        for s, t in enumerate(_float_entries(models[c + 1])):
            assert np.array_equal(_bits(t), _bits(sources[c][s])), (k, c, LENS[s])


def test_payload_decodes_to_the_global_model():
    """theta + sum of w q s, formed on the host in np.float32 in source order from the codes and
    scales the kernel wrote, is the global model bit for bit; the call without the payload leaves
    the same model and residuals."""
    k = 3
    theta, _, _, raw_w, w, _ = _case(k)
    models, cohort = _cohort(k)
    part, (codes, scales) = cohort.aggregate_q8([0, 1, 2], raw_w, payload=True)
    codes, scales = codes.cpu().numpy(), scales.cpu().numpy()
    got = _float_entries(models[0])
    chunk0 = 0
    for s, n in enumerate(LENS):
        C = -(-n // CHUNK)
        if MODES[s]:
            acc = theta[s].copy()
            for c in range(k):
                q = codes[c, chunk0:chunk0 + C].reshape(-1)[:n].astype(f32)
                sc = np.repeat(scales[c, chunk0:chunk0 + C].reshape(-1), 256)[:n]
                acc = acc + f32(w[c]) * (q * sc)
            assert np.array_equal(_bits(got[s]), _bits(acc)), n
        else:
            assert not codes[:, chunk0:chunk0 + C].any() and not scales[:, chunk0:chunk0 + C].any()
        chunk0 += C
    models2, cohort2 = _cohort(k)
    part2 = cohort2.aggregate_q8([0, 1, 2], raw_w)
    assert torch.is_tensor(part2) and np.array_equal(_bits(part2), _bits(part))
    _check_against_mirror(k, models2, cohort2, part2)


def test_destinations_may_alias_sources():
    k = 3
    _, _, _, raw_w, _, _ = _case(k)
    models, cohort = _cohort(k)
    part = cohort.aggregate_q8([0, 1, 2], raw_w, also=[0, 1, 2])
    _check_against_mirror(k, models, cohort, part, dst=(0, 1, 2, 3))


def test_grid_stride():
    """One quantised segment of 2049 * 2048 + 5 elements: more chunks than the largest grid."""
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import kernels as K
    n, k, C = 2049 * 2048 + 5, 2, 2050
    rng = np.random.default_rng(77)
    theta = [rng.standard_normal(n).astype(f32)]
    sources = [[theta[0] + (f32(0.02) * rng.standard_normal(n)).astype(f32)] for _ in range(k)]
    resid = [[(f32(2e-4) * rng.standard_normal(n)).astype(f32)] for _ in range(k)]
    w = F._norm_weights([300.0, 500.0], 800.0)
    out, new_res, codes, scales, want_part = F.q8_aggregate_mirror(theta, sources, resid, w, (1,), with_part=True)
    models = [[torch.from_numpy(m[0]).cuda()] for m in [theta] + sources]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    rows = torch.from_numpy(_rows(resid, lens=(n,))).cuda()
    dcodes = torch.empty((k, C, CHUNK), dtype=torch.int8, device="cuda")
    dscales = torch.empty((k, C, 8), dtype=torch.float32, device="cuda")
    part = K.fedavg_q8_exchange([1, 2], w, 0, [0], table, C, torch.ones(1, dtype=torch.uint8, device="cuda"), rows,
                                dcodes, dscales)
    assert np.array_equal(_bits(models[0][0]), _bits(out[0]))
    assert np.array_equal(_bits(rows), _bits(_rows(new_res, lens=(n,))))
    assert np.array_equal(_bits(dcodes), _bits(_rows(codes, np.int8, lens=(n,))))
    assert np.array_equal(_bits(dscales), _bits(_rows(scales, f32, 8, lens=(n,))))
    assert np.array_equal(_bits(part), _bits(want_part))


def test_status_codes():
    """-2 / -4 straight from the C entry point; nothing is written in any of these cases."""
    from ssl_mae_amd import _lib
    from ssl_mae_amd import kernels as K
    lib = _lib.load()
    models = [[torch.ones(8, device="cuda"), torch.ones(5, device="cuda")] for _ in range(3)]
    table, _ = K.fedavg_exchange_table(models, torch.float32)
    seg_mode = torch.tensor([1, 0], dtype=torch.uint8, device="cuda")
    flat = torch.full((2 * 2 * CHUNK + 4,), 0.25, device="cuda")             # 2 rows of 2 chunks, and a guard
    resid = flat[:2 * 2 * CHUNK].view(2, 2 * CHUNK)
    part = torch.full((2 * 2 * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
    codes = torch.full((2 * 2 * CHUNK + 4,), 0x5A, dtype=torch.int8, device="cuda")
    scales = torch.full((2 * 2 * 8,), -7.0, device="cuda")
    rp, pp, cp = resid.data_ptr(), part.data_ptr(), codes.data_ptr()
    assert rp % 16 == 0 and pp % 8 == 0 and cp % 4 == 0

    def call(src=(1, 2), weights=(0.5, 0.5), theta=0, dst=(0,), seg=seg_mode, r=rp, rows=2, c=cp, s=scales.data_ptr(),
             p=pp, table_bytes=table.numel()):
        sa = (ctypes.c_int32 * max(1, len(src)))(*src)
        da = (ctypes.c_int32 * max(1, len(dst)))(*dst)
        wa = (ctypes.c_float * max(1, len(weights)))(*weights)
        return lib.sm_fedavg_q8_exchange(len(src), ctypes.cast(sa, ctypes.c_void_p), ctypes.cast(wa, ctypes.c_void_p),
                                         theta, len(dst), ctypes.cast(da, ctypes.c_void_p), _lib.ptr(table),
                                         table_bytes, _lib.ptr(seg), ctypes.c_void_p(r), rows, ctypes.c_void_p(c),
                                         ctypes.c_void_p(s), ctypes.c_void_p(p), _lib.stream())

    assert call(src=(0, 2)) == -2 and call(src=(1, 2), theta=1) == -2            # a source is the global model
    assert call(rows=1) == -2 and call(rows=0) == -2                             # a residual row out of range
    assert call(src=(1, 2), theta=2) == -2
    assert call(r=0) == -2 and call(p=0) == -2 and call(seg=None) == -2          # NULL resid / part / seg_mode
    assert call(src=(), weights=()) == -2 and call(src=(1,) * 33, weights=(1.0 / 33,) * 33) == -2
    assert call(src=(1, 3)) == -2 and call(dst=(3,)) == -2 and call(dst=()) == -2   # exchange_args' checks
    assert call(theta=3) == -2 and call(theta=-1) == -2
    assert call(table_bytes=table.numel() - 16) == -2
    assert call(r=rp + 4) == -4 and call(p=pp + 4) == -4 and call(c=cp + 1) == -4 and call(s=scales.data_ptr() + 2) == -4
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for m in models for t in m)
    assert bool((flat == 0.25).all()) and bool((part == -7.0).all()) and bool((codes == 0x5A).all())
    assert bool((scales == -7.0).all())
    assert call(c=0) == 0                                                        # no payload: codes and scales stay
    torch.cuda.synchronize()
    assert bool((codes == 0x5A).all()) and bool((scales == -7.0).all())
    # v = (1 - 1) + 0.25: every code 127, the residual 0.25 - 127 (0.25 / 127); the plain segment is the sum
    d = f32(127.0) * (f32(0.25) / f32(127.0))
    e = f32(0.25) - d
    assert bool((models[0][0] == float((f32(1.0) + f32(0.5) * d) + f32(0.5) * d)).all())
    assert bool((models[0][1] == 1.0).all())
    assert bool((resid[:, :8] == float(e)).all()) and bool((resid[:, 8:] == 0.25).all()) and bool((flat[-4:] == 0.25).all())
    lane = ((e * e + e * e) + e * e) + e * e                     # a lane's 4 squares in fp32; two lanes hold the 8
    assert part[:8].tolist() == [0.25, float(lane) + float(lane), 0.0, 0.0] * 2 and part[8].item() == -7.0


def test_nan_in_a_client_shows_in_its_maximum():
    from ssl_mae_amd import federated as F
    k = 2
    _, _, _, raw_w, _, _ = _case(k)
    models, cohort = _cohort(k)
    s, i = 11, 2048 + 700                                        # entry of 4099: chunk 1, block 2
    with torch.no_grad():
        _float_entries(models[2])[s + 0][i] = float("nan")
    chunk = sum(-(-n // CHUNK) for n in LENS[:s]) + 1
    part, (codes, scales) = cohort.aggregate_q8([0, 1], raw_w, payload=True)
    mx = part[:, :, 0].cpu().numpy()
    assert np.all(np.isfinite(mx[0])) and np.isnan(mx[1, chunk]) and np.isnan(mx[1]).sum() == 1
    assert not codes[1, chunk, 512:768].any() and scales[1, chunk, 2].item() == 0.0
    assert codes[1, chunk, :512].any() and codes[0, chunk].any()
    with pytest.raises(RuntimeError, match="client 1 "):
        F._q8_round(lambda line: None, 1, {}, part, [0, 1], models[0], models[0].state_dict())


# ------------------------------------------------------------------ FedCohort on small models
W4 = [1200.0, 800.0, 1500.0, 500.0]


def _net():
    return nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Flatten(), nn.Linear(4 * 6 * 6, 5))


def _perturb(m, seed, std):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((torch.randn(p.shape, generator=g) * std).to(p.device))
        m[1].running_mean.add_(torch.randn(4, generator=g).to(p.device))
        m[1].num_batches_tracked.add_(seed % 5 + 1)


@pytest.fixture(scope="module")
def nets():
    """A global model and four clients = global + an update; never written: tests use deep copies."""
    torch.manual_seed(3)
    g = _net().cuda()
    clients = [copy.deepcopy(g) for _ in range(4)]
    for i, m in enumerate(clients):
        _perturb(m, 10 + i, 0.01 * (i + 1))
    return [g] + clients


def _host(model, keys):
    st = model.state_dict()
    return [st[k].detach().cpu().numpy().reshape(-1).copy() for k in keys]


def _cohort_rows(cohort, per_client):
    lens = [v.numel() for v in _float_entries(cohort.global_model)]
    return _rows(per_client, lens=lens)


def test_cohort_residuals_persist_reset_and_survive_a_rebuild(nets):
    from ssl_mae_amd import federated as F
    models = copy.deepcopy(nets)
    cohort = F.FedCohort(models[0], models[1:])
    keys, modes = cohort.float_keys, cohort._clip_modes
    assert sum(modes) == 6 and len(modes) == 8
    w = F._norm_weights(W4, float(sum(W4)))
    theta = _host(models[0], keys)
    sources = [_host(m, keys) for m in models[1:]]
    zeros = [[np.zeros_like(t) for t in theta] for _ in range(4)]
    out1, res1, _, _ = F.q8_aggregate_mirror(theta, sources, zeros, w, modes)
    cohort.aggregate_q8([0, 1, 2, 3], W4)
    assert np.array_equal(_bits(cohort._residuals()), _bits(_cohort_rows(cohort, res1)))
    assert float(cohort._residuals().abs().max()) > 0.0
    for s, t in enumerate(_host(models[0], keys)):
        assert np.array_equal(_bits(t), _bits(out1[s])), keys[s]
    assert int(models[0][1].num_batches_tracked) == max(int(m[1].num_batches_tracked) for m in nets[1:])
    # round 2: two clients, in another order, trained on; client 2's parameters re-homed first
    cohort.broadcast([3, 1])
    _perturb(models[4], 21, 0.02)
    _perturb(models[2], 22, 0.02)
    with torch.no_grad():
        for p in models[2].parameters():                         # what `.to()` does: new storage, same values
            p.data = p.data.clone()
    theta = _host(models[0], keys)
    sources = [_host(models[4], keys), _host(models[2], keys)]
    w2 = F._norm_weights([W4[3], W4[1]], W4[3] + W4[1])
    out2, res2, _, _ = F.q8_aggregate_mirror(theta, sources, [res1[3], res1[1]], w2, modes)
    assert cohort.rebuilds == 1
    cohort.aggregate_q8([3, 1], [W4[3], W4[1]])
    assert cohort.rebuilds == 2
    for s, t in enumerate(_host(models[0], keys)):
        assert np.array_equal(_bits(t), _bits(out2[s])), keys[s]
    assert np.array_equal(_bits(cohort._residuals()), _bits(_cohort_rows(cohort, [res1[0], res2[1], res1[2], res2[0]])))
    cohort.reset_residuals()
    assert not bool(cohort._residuals().any())


def _loop_setup(nets):
    models = copy.deepcopy(nets)
    calls = [0]

    def update_fn(cid):
        def fn(model):
            calls[0] += 1
            _perturb(model, 100 * calls[0] + cid, 0.01)
            return 0.5 + cid
        return fn

    loaders = [{"loader": None, "update_fn": update_fn(c)} for c in range(4)]
    return models, loaders


@pytest.mark.parametrize("error_feedback", [True, False])
def test_fused_loop_is_the_reference_loop(nets, error_feedback):
    """run_fedavg_fused and run_fedavg with `compress`: bit-identical global and client states and
    identical records over 2 rounds of 3 of 4 clients."""
    from ssl_mae_amd import federated as F
    compress = {"method": "q8", "error_feedback": error_feedback}
    results = []
    for run in (F.run_fedavg_fused, F.run_fedavg):
        models, loaders = _loop_setup(nets)
        log = io.StringIO()
        recs = run(models[0], models[1:], loaders, W4, lambda m: (0.25, 0.5), "cuda", rounds=2, client_fraction=0.75,
                   log_f=log, compress=compress)
        results.append((models, recs, log.getvalue()))
    (fused, recs_f, log_f), (ref, recs_r, log_r) = results
    assert recs_f == recs_r and len(recs_f) == 2 and log_f == log_r
    for rec in recs_f:
        assert rec["clients"] == 3 and rec["q8_absmax"] > 0.0 and rec["q8_resid_norm"] > 0.0
        assert rec["comm_mb_round"] == rec["upload_mb_fp32"] + rec["upload_mb_q8"] and rec["upload_mb_q8"] < rec[
            "upload_mb_fp32"]
    for a, b in zip(fused, ref):
        for (k, x), y in zip(a.state_dict().items(), b.state_dict().values()):
            assert torch.equal(x, y) and np.array_equal(_bits(x), _bits(y)), k


# ------------------------------------------------------------------ driver end to end
NC, T, S = 4, 2, 112
CSVS = ("fed_summary.csv", "fed_compress_summary.csv", "fed_client_stats.csv", "system_privacy_summary.csv")


def _config(tmp_path, name, compress):
    fed = {"num_clients": 3, "rounds": 2, "local_epochs": 1, "batch_size": 2, "exchange": "fused",
           "non_iid": {"shards_per_client": 1, "min_samples_per_client": 2}}
    if compress is not None:
        fed["compress"] = compress
    cfg = {"dataset": {"num_classes": NC, "clip_len": T, "image_size": S}, "federated": fed,
           "centralized": {"enabled": False}, "synthetic": {"num_train": 6, "num_val": 2},
           "output": {"save_dir": str(tmp_path / name)}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), tmp_path / name


def _csv(path):
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_driver_with_compression(tmp_path):
    """3 clients, 2 rounds, T=2, 112^2, 4 classes on synthetic clips, once per exchange: the same
    CSVs, the upload ratio of q8_upload_bytes, totals that add up; no compression CSV when off."""
    from ssl_mae_amd import driver as D
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.utils import load_config
    on = {"enabled": True, "method": "q8", "error_feedback": True}
    cfg_a, dir_a = _config(tmp_path, "fused", on)
    cfg_b, dir_b = _config(tmp_path, "ref", on)
    R.main(["--config", cfg_a])
    R.main(["--config", cfg_b, "--exchange", "reference"])
    assert "exchange=reference" in (dir_b / "federated.log").read_text()
    for name in CSVS:
        assert (dir_a / name).read_text() == (dir_b / name).read_text(), name
    head, rows = _csv(dir_a / "fed_compress_summary.csv")
    assert head == list(R.COMPRESS_COLUMNS) and [r[0] for r in rows] == ["1", "2"]
    model = D.build_classifier(R.resolve_config(load_config(cfg_a)), None, torch.device("cuda"), load=None)
    state = model.state_dict()
    ratio = F.q8_upload_bytes(state, {k for k, _ in model.named_parameters()}) / F.model_size_bytes(state)
    assert 0.25 < ratio < 0.27
    fhead, frows = _csv(dir_a / "fed_summary.csv")
    assert fhead == list(R.FED_COLUMNS)
    total = 0.0
    for r, fr in zip(rows, frows):
        fp32_mb, q8_mb = float(r[2]), float(r[3])
        assert r[1] == "3" and float(r[4]) == round(ratio, 6) and abs(q8_mb / fp32_mb - ratio) < 1e-6
        assert abs(fp32_mb - 3 * float(fr[5])) < 2.5e-6                       # 3 x model_mb
        assert abs(float(fr[6]) - (fp32_mb + q8_mb)) < 2e-6                 # comm_mb_round: broadcast + upload
        assert float(r[5]) > 0.0 and float(r[6]) > 0.0
        total += float(fr[6])
        assert abs(float(fr[7]) - total) < 2e-6                             # comm_mb_total: the running sum
    _, srow = _csv(dir_a / "system_privacy_summary.csv")
    assert abs(float(srow[0][1]) - total) < 2e-6
    assert "upload_mb_q8=" in (dir_a / "federated.log").read_text()
    cfg_off, dir_off = _config(tmp_path, "off", {"enabled": False, "method": "q8", "error_feedback": True})
    R.main(["--config", cfg_off])
    assert (dir_off / "fed_summary.csv").exists() and not (dir_off / "fed_compress_summary.csv").exists()
    assert "q8" not in (dir_off / "federated.log").read_text()
    _, off_rows = _csv(dir_off / "fed_summary.csv")
    assert abs(float(off_rows[0][6]) - 2 * 3 * float(off_rows[0][5])) < 2e-6

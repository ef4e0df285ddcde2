"""Host side of the compressed FedAvg exchange (federated.q8_aggregate_mirror, q8_upload_bytes, the
`compress` option of the round loops, run_federated's federated.compress section): the quantiser's
error bound and its dead blocks, error feedback telescoping over rounds, wire sizes, config
validation, and the round's call order and communication record."""
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

f32 = np.float32


def _v(theta, source, resid):
    return (source - theta) + resid


def _blocks(a, fill=0.0):
    nb = -(-a.size // 256)
    out = np.full(nb * 256, fill, dtype=a.dtype)
    out[:a.size] = a
    return out.reshape(nb, 256)


def test_mirror_error_bound_and_dead_blocks():
    """|new residual| <= (0.5 + 1e-4) s on live blocks: half a step from the rounding, and the four
    roundings of inv, v inv, s and q s, each 2^-24 relative, times 127, under the 1e-4.  Dead
    blocks (all zero, or max |v| = 1e-31) keep v and upload codes 0, scale 0; a block of identical
    values uploads +-127."""
    from ssl_mae_amd import federated as F
    rng = np.random.default_rng(11)
    lens = (1, 3, 255, 256, 257, 2049, 4099, 1024)
    theta = [rng.standard_normal(n).astype(f32) for n in lens]
    sources = [[(t + f32(0.05) * rng.standard_normal(t.size).astype(f32)) for t in theta] for _ in range(2)]
    resid = [[(f32(1e-3) * rng.standard_normal(t.size)).astype(f32) for t in theta] for _ in range(2)]
    # segment 7 (1024 elements): block 0 all zero, block 1 at 1e-31, block 2 one positive value, block 3 its negative
    theta[7][:] = 0.0
    for c in range(2):
        resid[c][7][:] = 0.0
        sources[c][7][:256] = 0.0
        sources[c][7][256:512] = (f32(1e-31) * rng.uniform(-1, 1, 256)).astype(f32)
        sources[c][7][256] = f32(1e-31)
        sources[c][7][512:768] = f32(0.37)
        sources[c][7][768:] = f32(-0.37)
    modes = (1, 1, 1, 0, 1, 1, 1, 1)
    w = F._norm_weights([3.0, 1.0], 4.0)
    out, new_res, codes, scales = F.q8_aggregate_mirror(theta, sources, resid, w, modes)
    live_blocks = dead_blocks = 0
    for c in range(2):
        for s, n in enumerate(lens):
            assert new_res[c][s].dtype == f32 and codes[c][s].dtype == np.int8 and scales[c][s].dtype == f32
            assert new_res[c][s].shape == (n,) and codes[c][s].shape == (n,) and scales[c][s].shape == (-(-n // 256),)
            if not modes[s]:
                assert np.array_equal(new_res[c][s], resid[c][s]) and not codes[c][s].any() and not scales[c][s].any()
                continue
            v = _blocks(_v(theta[s], sources[c][s], resid[c][s]))
            e, q, sc = _blocks(new_res[c][s]), _blocks(codes[c][s]), scales[c][s]
            live = sc > 0
            live_blocks += int(live.sum())
            dead_blocks += int((~live).sum())
            assert np.all(np.abs(e[live]) <= (0.5 + 1e-4) * sc[live, None].astype(np.float64))
            assert np.array_equal(e[~live].view(np.int32), v[~live].view(np.int32)) and not q[~live].any()
            assert np.all(np.abs(q.astype(np.int32)) <= 127)
            assert np.array_equal(np.abs(q[live]).max(axis=1), np.full(int(live.sum()), 127))   # the maximum is a code
    assert live_blocks > 40 and dead_blocks == 4
    for c in range(2):
        assert scales[c][7][0] == 0.0 and scales[c][7][1] == 0.0
        assert np.all(codes[c][7][512:768] == 127) and np.all(codes[c][7][768:] == -127)
        assert scales[c][7][2] == f32(0.37) / f32(127.0)
    # mode 0: the plain weighted sum; mode 1: theta + sum of w q s
    assert np.array_equal(out[3], (np.zeros_like(theta[3]) + sources[0][3] * f32(w[0])) + sources[1][3] * f32(w[1]))
    acc = theta[5].copy()
    for c in range(2):
        d = codes[c][5].astype(f32) * np.repeat(scales[c][5], 256)[:lens[5]]
        acc = acc + f32(w[c]) * d
    assert np.array_equal(acc.view(np.int32), out[5].view(np.int32))


def _rounds(error_feedback):
    """4 rounds of one client against theta = 0 with fixed updates: (sum of the updates in fp64,
    sum of the dequantised uploads in fp64, the final residual, the largest |v| and scale seen)."""
    from ssl_mae_amd import federated as F
    rng = np.random.default_rng(5)
    n = 1000
    theta = [np.zeros(n, dtype=f32)]
    resid = [[np.zeros(n, dtype=f32)]]
    total, sent, vmax, smax = np.zeros(n), np.zeros(n), 0.0, 0.0
    for _ in range(4):
        u = rng.standard_normal(n).astype(f32)
        if not error_feedback:
            resid = [[np.zeros(n, dtype=f32)]]
        vmax = max(vmax, float(np.abs(u + resid[0][0]).max()))
        _, resid, codes, scales = F.q8_aggregate_mirror(theta, [[u]], resid, [1.0], (1,))
        total += u
        sent += (codes[0][0].astype(f32) * np.repeat(scales[0][0], 256)[:n]).astype(np.float64)
        smax = max(smax, float(scales[0][0].max()))
    return total, sent, resid[0][0].astype(np.float64), vmax, smax


def test_error_feedback_telescopes_over_rounds():
    """sum of the dequantised uploads + the final residual = sum of the updates, to 1e-5 of the
    largest |v| per element (fp32 accumulation over 4 rounds); without error feedback the earlier
    rounds' errors are lost."""
    total, sent, last, vmax, _ = _rounds(True)
    assert np.all(np.abs(sent + last - total) <= 1e-5 * vmax)
    total, sent, last, _, smax = _rounds(False)
    assert np.abs(sent + last - total).max() > 0.1 * smax


def test_q8_upload_bytes():
    from ssl_mae_amd import federated as F
    lens = (1, 255, 256, 257, 2049)
    state = {f"p{n}": torch.zeros(n) for n in lens}
    state["bn.running_mean"] = torch.zeros(10)
    state["bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    params = {f"p{n}" for n in lens}
    for n, want in zip(lens, (1 + 4, 255 + 4, 256 + 4, 257 + 8, 2049 + 36)):
        assert F.q8_upload_bytes({f"p{n}": state[f"p{n}"]}, params) == want
    assert F.q8_upload_bytes(state, params) == 5 + 259 + 260 + 265 + 2085 + 40 + 8
    assert F.q8_upload_bytes(state, set()) == F.model_size_bytes(state) == 4 * (sum(lens) + 10) + 8
    assert F.q8_upload_bytes({"p": torch.zeros(3, 100)}, {"p"}) == 300 + 8


def test_config_validation():
    import os
    from conftest import ROOT
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.utils import load_config
    want = {"enabled": False, "method": "q8", "error_feedback": True}
    assert R.resolve_config({})["federated"]["compress"] == want
    assert R.resolve_config(load_config(os.path.join(ROOT, "configs", "federated.yaml")))["federated"]["compress"] == want
    on = R.resolve_config({"federated": {"compress": {"enabled": True, "error_feedback": False}}})
    assert on["federated"]["compress"] == {"enabled": True, "method": "q8", "error_feedback": False}
    with pytest.raises(ValueError, match="federated.compress.method"):
        R.resolve_config({"federated": {"compress": {"method": "topk"}}})
    with pytest.raises(ValueError, match="Unknown keys in federated.compress"):
        R.resolve_config({"federated": {"compress": {"bits": 4}}})
    with pytest.raises(ValueError, match="exclusive"):
        R.resolve_config({"federated": {"dp": {"enabled": True}, "compress": {"enabled": True}}})
    R.resolve_config({"federated": {"dp": {"enabled": True}, "compress": {"enabled": False}}})
    assert ",".join(R.COMPRESS_COLUMNS) == "round,clients,upload_mb_fp32,upload_mb_q8,upload_ratio,q8_absmax," \
                                           "q8_resid_norm"
    rec = {"round": 2, "clients": 3, "upload_mb_fp32": 3.0, "upload_mb_q8": 0.8, "q8_absmax": 0.12345678,
           "q8_resid_norm": 1.0 / 3.0}
    assert R.compress_summary_rows([rec]) == [{"round": 2, "clients": 3, "upload_mb_fp32": 3.0, "upload_mb_q8": 0.8,
                                               "upload_ratio": 0.266667, "q8_absmax": 0.123457,
                                               "q8_resid_norm": 0.333333}]


def test_round_call_order_and_record_with_compress(monkeypatch):
    """With `compress`, run_fedavg_fused draws the same clients and runs broadcast -> updates ->
    aggregate_q8 per round; the record's comm_mb_round is the fp32 broadcast plus the compressed
    upload.  The cohort (the GPU part) is replaced by a recorder."""
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    calls = []

    class Recorder:
        def __init__(self, global_model, client_models):
            calls.append(("cohort", len(client_models)))

        def broadcast(self, selected):
            calls.append(("broadcast", list(selected)))

        def reset_residuals(self):
            calls.append(("reset",))

        def aggregate_q8(self, selected, weights, also=(), payload=False):
            calls.append(("aggregate_q8", list(selected), list(weights)))
            part = torch.zeros((len(selected), 2, 2), dtype=torch.float64)
            part[:, 0, 0] = torch.tensor([0.5, 0.25, 0.125])[:len(selected)]
            part[:, :, 1] = 2.0
            return part

    monkeypatch.setattr(F, "FedCohort", Recorder)
    g, clients = nn.Linear(300, 2), [nn.Linear(300, 2) for _ in range(5)]
    sizes = [10, 20, 30, 40, 50]

    def update_fn(cid):
        def fn(model):
            calls.append(("update", cid))
            return float(cid)
        return fn

    loaders = [{"loader": None, "update_fn": update_fn(c)} for c in range(5)]
    log = io.StringIO()
    run = lambda **kw: F.run_fedavg_fused(g, clients, loaders, sizes, lambda m: (0.25, 0.5), None, rounds=3,
                                          client_fraction=0.6, log_f=log, **kw)
    recs = run(compress={"method": "q8", "error_feedback": True})
    schedule = O.client_schedule(5, 3, 0.6)
    want = [("cohort", 5)]
    for sel in schedule:
        want += [("broadcast", sel)] + [("update", c) for c in sel] + [("aggregate_q8", sel, [float(sizes[c]) for c in sel])]
    assert calls == want
    size_b = 4 * (600 + 2)
    q8_b = (600 + 4 * 3) + (2 + 4)
    assert F.q8_upload_bytes(g.state_dict(), {"weight", "bias"}) == q8_b
    for r, (rec, sel) in enumerate(zip(recs, schedule), 1):
        assert rec == {"round": r, "val_top1": 0.25, "val_top5": 0.5, "avg_local_loss": sum(sel) / 3.0, "clients": 3,
                       "model_mb": size_b / 2 ** 20, "comm_mb_round": 3 * size_b / 2 ** 20 + 3 * q8_b / 2 ** 20,
                       "upload_mb_fp32": 3 * size_b / 2 ** 20, "upload_mb_q8": 3 * q8_b / 2 ** 20, "q8_absmax": 0.5,
                       "q8_resid_norm": 12.0 ** 0.5}
    assert "upload_mb_q8=" in log.getvalue()
    del calls[:]
    run(compress={"method": "q8", "error_feedback": False})
    assert calls.count(("reset",)) == 3 and calls[1 + 1 + 3] == ("reset",)       # before the round's aggregation
    with pytest.raises(ValueError, match="exclusive"):
        run(compress={"method": "q8", "error_feedback": True}, dp={"clip_norm": 1.0, "noise_multiplier": 0.0, "seed": 1})
    with pytest.raises(ValueError, match="unknown compression method"):
        run(compress={"method": "topk"})
    with pytest.raises(ValueError, match="exclusive"):
        F.run_fedavg(g, clients, loaders, sizes, lambda m: (0, 0), None, rounds=1,
                     compress={"method": "q8"}, dp={"clip_norm": 1.0, "noise_multiplier": 0.0, "seed": 1})


def test_nonfinite_maximum_names_the_client():
    from ssl_mae_amd import federated as F
    part = torch.zeros((2, 3, 2), dtype=torch.float64)
    part[1, 2, 0] = float("nan")
    g = nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="client 7"):
        F._q8_round(lambda s: None, 1, {}, part, [4, 7], g, g.state_dict())

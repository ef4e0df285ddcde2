"""Host-side pieces of DP-FedAvg (ssl_mae_amd.federated, run_federated): the RDP accountant against
its closed form, the `federated.dp` config section, the numpy mirror against a hand-written fp64
computation, the round seed, the torch noise against the draw specification, and the fused host
loop with `dp=None` against the existing records."""
import math

import numpy as np
import pytest


# ------------------------------------------------------------------ dp_epsilon
def _closed_form(z, T, delta, orders=range(2, 256)):
    """sample_rate = 1: the Gaussian mechanism's RDP alpha / (2 z^2)."""
    return min(T * a / (2.0 * z * z) + math.log(1.0 / delta) / (a - 1) for a in orders)


@pytest.mark.parametrize("z,T,delta", [(1.1, 100, 1e-5), (0.5, 3, 1e-5), (4.0, 1, 1e-6), (20.0, 1000, 1e-3)])
def test_epsilon_full_participation_is_the_closed_form(z, T, delta):
    from ssl_mae_amd.federated import dp_epsilon
    got, want = dp_epsilon(z, 1.0, T, delta), _closed_form(z, T, delta)
    print(f"z={z} T={T} delta={delta}: dp_epsilon {got!r}, closed form {want!r}")
    assert abs(got - want) <= 1e-12 * want


def test_epsilon_monotone_and_limits():
    from ssl_mae_amd.federated import dp_epsilon
    by_rounds = [dp_epsilon(1.1, 0.1, T, 1e-5) for T in (1, 2, 10, 100, 1000)]
    assert all(a <= b for a, b in zip(by_rounds, by_rounds[1:])) and by_rounds[0] < by_rounds[-1]
    by_rate = [dp_epsilon(1.1, q, 100, 1e-5) for q in (0.0, 0.01, 0.1, 0.5, 0.9, 1.0)]
    assert all(a <= b for a, b in zip(by_rate, by_rate[1:])) and by_rate[1] < by_rate[-1]
    by_noise = [dp_epsilon(z, 0.1, 100, 1e-5) for z in (0.5, 0.8, 1.1, 2.0, 8.0)]
    assert all(a > b for a, b in zip(by_noise, by_noise[1:]))
    assert dp_epsilon(0.0, 0.1, 100, 1e-5) == math.inf
    eps = dp_epsilon(1.1, 0.1, 100, 1e-5)
    print(f"q=0.1 z=1.1 T=100 delta=1e-5: epsilon {eps!r}")
    assert math.isfinite(eps) and eps > 0.0
    assert eps < _closed_form(1.1, 100, 1e-5)                  # subsampling amplifies
    for bad in ((-1.0, 0.1, 1, 1e-5), (1.0, 1.5, 1, 1e-5), (1.0, 0.1, 1, 0.0), (1.0, 0.1, 1, 1.0)):
        with pytest.raises(ValueError):
            dp_epsilon(*bad)


# ------------------------------------------------------------------ config
def test_dp_config_section(tmp_path):
    import yaml
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.utils import load_config
    want = {"enabled": False, "clip_norm": 1.0, "noise_multiplier": 0.0, "delta": 1e-5, "seed": None}
    assert R.resolve_config({})["federated"]["dp"] == want
    assert R.DEFAULTS["federated"]["dp"] == want
    with pytest.raises(ValueError, match="Unknown keys in federated.dp"):
        R.resolve_config({"federated": {"dp": {"clip": 1.0}}})
    for bad in ({"clip_norm": 0.0}, {"clip_norm": -1.0}, {"clip_norm": float("nan")}, {"noise_multiplier": -0.1},
                {"delta": 0.0}, {"delta": 1.0}):
        with pytest.raises(ValueError, match="federated.dp"):
            R.resolve_config({"federated": {"dp": bad}})
    path = tmp_path / "dp.yaml"
    path.write_text(yaml.safe_dump({"federated": {"dp": {"enabled": True}}}))
    got = R.resolve_config(load_config(str(path)))["federated"]
    assert got["dp"] == dict(want, enabled=True) and got["exchange"] == "fused"
    assert R.DEFAULTS["federated"]["dp"]["enabled"] is False      # defaults not written through
    assert ",".join(R.DP_COLUMNS) == "round,clients,dp_clipped,dp_norm_mean,dp_norm_max,dp_noise_std,epsilon_est,delta"


def test_shipped_config_has_the_block_disabled():
    import os
    from conftest import ROOT
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.utils import load_config
    cfg = R.resolve_config(load_config(os.path.join(ROOT, "configs", "federated.yaml")))
    assert cfg["federated"]["dp"] == {"enabled": False, "clip_norm": 1.0, "noise_multiplier": 0.0, "delta": 1e-5,
                                      "seed": None}


def test_dp_summary_rows():
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.federated import dp_epsilon
    dp = {"noise_multiplier": 1.1, "delta": 1e-5}
    recs = [{"round": r, "clients": 2, "dp_clipped": r - 1, "dp_norm_mean": 1 / 3, "dp_norm_max": 2 / 3,
             "dp_noise_std": 0.123456789} for r in (1, 2)]
    rows = R.dp_summary_rows(recs, dp, 8)
    assert [list(r) for r in rows] == [list(R.DP_COLUMNS)] * 2
    assert rows[0] == {"round": 1, "clients": 2, "dp_clipped": 0, "dp_norm_mean": 0.333333, "dp_norm_max": 0.666667,
                       "dp_noise_std": 0.123457, "epsilon_est": round(dp_epsilon(1.1, 0.25, 1, 1e-5), 6),
                       "delta": 1e-5}
    assert rows[1]["epsilon_est"] == round(dp_epsilon(1.1, 0.25, 2, 1e-5), 6) >= rows[0]["epsilon_est"]


# ------------------------------------------------------------------ mirror
def test_mirror_on_a_three_client_toy():
    """Segments of 5 and 7 elements (clipped) and one buffer segment of 4 (plain FedAvg).  The
    updates have norms 0.5, 2 and 4 against clip_norm 1: client 0 keeps its update, clients 1 and
    2 are scaled.  Expected values are computed here in fp64; the mirror's fp32 result may differ
    from them by the roundings of pass 2: (K + 4) 2^-23 (|theta| + sum |ws d|), the bound the
    GPU test uses for the eager reference."""
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    rng = np.random.default_rng(5)
    lens, modes, clip = (5, 7, 4), (1, 1, 0), 1.0
    theta = [rng.standard_normal(n).astype(np.float32) for n in lens]
    target = (0.5, 2.0, 4.0)
    sources = []
    for c in range(3):
        d = [rng.standard_normal(n) for n in lens]
        nrm = math.sqrt(sum(float(np.sum(x * x)) for x, m in zip(d, modes) if m))
        sources.append([(t.astype(np.float64) + x * (target[c] / nrm)).astype(np.float32) for t, x in zip(theta, d)])
    raw_w = [3.0, 1.0, 4.0]
    w = F._norm_weights(raw_w, sum(raw_w))
    # by hand, fp64
    norms = [math.sqrt(sum(float(np.sum((x.astype(np.float64) - t.astype(np.float64)) ** 2))
                           for x, t, m in zip(src, theta, modes) if m)) for src in sources]
    assert all(abs(n - t) < 1e-6 * t for n, t in zip(norms, target))
    scales = [min(1.0, clip / (n + 1e-6)) for n in norms]
    assert scales[0] == 1.0 and scales[1] < 1.0 and scales[2] < 1.0
    out, got_norms = F.dp_aggregate_mirror(theta, sources, w, modes, clip)
    assert got_norms.dtype == np.float64 and np.allclose(got_norms, norms, rtol=1e-14, atol=0.0)
    for s in (0, 1):
        t64 = theta[s].astype(np.float64)
        want, mag = t64.copy(), np.abs(t64)
        for c in range(3):
            term = w[c] * scales[c] * (sources[c][s].astype(np.float64) - t64)
            want += term
            mag += np.abs(term)
        assert out[s].dtype == np.float32
        assert np.all(np.abs(out[s].astype(np.float64) - want) <= (3 + 4) * 2.0 ** -23 * mag), s
    # the clipped update's norm is at most clip_norm (the weights sum to 1)
    moved = math.sqrt(sum(float(np.sum((out[s].astype(np.float64) - theta[s].astype(np.float64)) ** 2)) for s in (0, 1)))
    assert moved <= clip * (1 + 1e-5)
    # the buffer segment: fedavg_aggregate's weighted sum, bit for bit
    assert np.array_equal(out[2].view(np.int32), O.weighted_sum([src[2] for src in sources], raw_w).view(np.int32))
    # given scales are used as given
    out2, _ = F.dp_aggregate_mirror(theta, sources, w, modes, clip, scales=np.ones(3, dtype=np.float32))
    unclipped = theta[0].copy()
    for c in range(3):
        unclipped = unclipped + np.float32(w[c]) * (sources[c][0] - theta[0])
    assert np.array_equal(out2[0].view(np.int32), unclipped.view(np.int32))
    assert not np.array_equal(out2[0], out[0])


def test_round_seed():
    from ssl_mae_amd import federated as F
    from ssl_mae_amd.privacy import config_seed
    seeds = [F.dp_round_seed(42, r) for r in range(1, 6)]
    assert seeds == [F.dp_round_seed(42, r) for r in range(1, 6)] == [config_seed(42, r) for r in range(1, 6)]
    assert len(set(seeds)) == 5 and F.dp_round_seed(43, 1) != seeds[0]
    assert all(0 <= s < 1 << 64 for s in seeds)


def test_torch_noise_is_the_draw_specification():
    """dp_noise (eager torch, one row) against privacy.perturb_draws / gaussian_from_draws: the
    same integers, so the fp64 Gaussians agree to the rounding of log / cos."""
    import torch
    from ssl_mae_amd import federated as F
    from ssl_mae_amd import privacy as P
    seed = F.dp_round_seed(7, 3)
    h0, h1, _ = P.perturb_draws(seed, 6, 1000)
    want = P.gaussian_from_draws(h0, h1)
    for seg in (0, 5):
        got = F.dp_noise(seed, seg, 1000, torch.device("cpu")).numpy()
        assert got.dtype == np.float64 and np.allclose(got, want[seg], rtol=0.0, atol=1e-12)
    assert F.dp_noise_std([0.25, 0.5, 0.25], 0.5, 0.5) == 0.125


# ------------------------------------------------------------------ host loop, dp=None
def test_fused_loop_without_dp_keeps_its_calls_and_records(monkeypatch):
    """The stub pattern of tests/test_run_federated_cpu.py: with dp=None the cohort sees broadcast ->
    aggregate only (never aggregate_dp) and the records have exactly the existing keys."""
    import io
    import torch.nn as nn
    from ssl_mae_amd import federated as F
    calls = []

    class Recorder:
        def __init__(self, global_model, client_models):
            calls.append(("cohort", len(client_models)))

        def broadcast(self, selected):
            calls.append(("broadcast", list(selected)))

        def aggregate(self, selected, weights, also=()):
            calls.append(("aggregate", list(selected), list(weights)))

        def aggregate_dp(self, *a, **k):
            raise AssertionError("aggregate_dp without dp")

    monkeypatch.setattr(F, "FedCohort", Recorder)
    g, clients = nn.Linear(2, 2), [nn.Linear(2, 2) for _ in range(5)]
    sizes = [10, 20, 30, 40, 50]
    loaders = [{"loader": None, "update_fn": (lambda m, c=c: float(c))} for c in range(5)]
    log = io.StringIO()
    recs = F.run_fedavg_fused(g, clients, loaders, sizes, lambda m: (0.25, 0.5), None, rounds=3, client_fraction=0.6,
                              log_f=log, dp=None)
    schedule = [[0, 4, 2], [2, 1, 0], [1, 0, 2]]
    want = [("cohort", 5)]
    for sel in schedule:
        want += [("broadcast", sel), ("aggregate", sel, [float(sizes[c]) for c in sel])]
    assert calls == want
    keys = ["round", "val_top1", "val_top5", "avg_local_loss", "clients", "model_mb", "comm_mb_round"]
    assert all(list(r) == keys for r in recs) and len(recs) == 3
    assert "dp_" not in log.getvalue()
    for bad in ({"clip_norm": 0.0, "noise_multiplier": 0.0, "seed": 1}, {"clip_norm": 1.0, "noise_multiplier": -1.0,
                                                                          "seed": 1}):
        with pytest.raises(ValueError):
            F.run_fedavg_fused(g, clients, loaders, sizes, lambda m: (0, 0), None, rounds=1, dp=bad)

"""Host-side pieces of the federated driver (ssl_mae_amd.run_federated): the class-shard splits
against fixtures recorded from the reference's splitter (tests/golden/make_golden_federated.py),
the raw-upload estimate, CSV headers and rounding, config validation and client selection."""
import json
import os

import pytest

from conftest import GOLDEN

SPLITS = os.path.join(GOLDEN, "federated_splits")
# (clients, shards_per_client, min_samples_per_client, seed) -> the reference's client sizes
CASES = {(4, 3, 10, 42): [38, 68, 58, 64],
         (4, 2, 40, 42): [40, 56, 54, 78],          # after rebalancing
         (5, 1, 30, 42): [30, 38, 72, 38, 50],
         (3, 6, 200, 42): [106, 122, 0]}            # the rebalance loop leaves one client empty


def test_base_split_fixture():
    import random
    from ssl_mae_amd import run_federated as R
    lines = [f"videos/class{c:02d}/clip_{i:03d} {c}" for c in range(12) for i in range(6 + 5 * (c % 4) + c)]
    random.Random(7).shuffle(lines)
    items = R.read_split(os.path.join(SPLITS, "base.txt"))
    assert len(items) == 228 and [f"{p} {y}" for p, y in items] == lines


@pytest.mark.parametrize("case", sorted(CASES))
def test_class_shard_splits_match_reference(case, tmp_path):
    from ssl_mae_amd import run_federated as R
    clients, shards, min_samples, seed = case
    ref_dir = os.path.join(SPLITS, f"c{clients}_s{shards}_m{min_samples}_seed{seed}")
    paths, stats = R.make_class_shard_splits(os.path.join(SPLITS, "base.txt"), clients, shards_per_client=shards,
                                             seed=seed, min_samples_per_client=min_samples, out_prefix="fx",
                                             out_dir=str(tmp_path / "out"))
    assert [s["num_samples"] for s in stats] == CASES[case]
    with open(os.path.join(ref_dir, "stats.json"), encoding="utf-8") as f:
        assert stats == json.load(f)                 # client, num_samples, num_classes, the classes string
    assert [os.path.basename(p) for p in paths] == [f"fx_client_{i}_train.txt" for i in range(clients)]
    for i, p in enumerate(paths):
        with open(p, encoding="utf-8") as got, open(os.path.join(ref_dir, f"client_{i}.txt"), encoding="utf-8") as ref:
            assert got.read() == ref.read(), (case, i)
        assert len(R.read_split(p)) == CASES[case][i]


def test_read_write_split_round_trip(tmp_path):
    from ssl_mae_amd import run_federated as R
    items = [("a/b", 3), ("c", 0)]
    R.write_split(items, tmp_path / "deep" / "s.txt")
    assert (tmp_path / "deep" / "s.txt").read_text() == "a/b 3\nc 0\n"
    (tmp_path / "blank.txt").write_text("\na/b 3\n\n  c 0  \n")
    assert R.read_split(tmp_path / "blank.txt") == items


def test_estimate_raw_upload_mb(tmp_path):
    from ssl_mae_amd import run_federated as R
    split = tmp_path / "train.txt"
    split.write_text("a 0\n\nb 1\nc 2\n")
    cfg = R.resolve_config({"dataset": {"clip_len": 16, "image_size": 112}})
    assert R.estimate_raw_upload_mb(cfg, split) == 3 * (3 * 16 * 112 * 112) / (1024.0 * 1024.0)
    cfg = R.resolve_config({"dataset": {"clip_len": 4, "image_size": 8}, "system_privacy": {"raw_dtype_bytes": 4}})
    assert R.estimate_raw_upload_mb(cfg, split) == 3 * (3 * 4 * 8 * 8 * 4) / (1024.0 * 1024.0)
    cfg = R.resolve_config({"system_privacy": {"estimate_raw_upload": False}})
    assert R.estimate_raw_upload_mb(cfg, split) is None


def test_csv_headers_and_rounding(tmp_path):
    from ssl_mae_amd import run_federated as R
    assert R.CLIENT_STATS_HEADER == "client,num_samples,num_classes,classes\n"
    assert ",".join(R.FED_COLUMNS) == "round,val_top1,val_top5,avg_local_loss,clients,model_mb,comm_mb_round," \
                                      "comm_mb_total"
    assert ",".join(R.CENTRALIZED_COLUMNS) == "epoch,train_loss,val_top1,val_top5"
    assert ",".join(R.SYSTEM_COLUMNS) == "raw_upload_mb_est,fed_comm_total_mb,reduction_ratio"
    records = [{"round": 1, "val_top1": 1 / 3, "val_top5": 2 / 3, "avg_local_loss": 1.23456789, "clients": 3,
                "model_mb": 80.1234567, "comm_mb_round": 480.7407402},
               {"round": 2, "val_top1": 0.5, "val_top5": 1.0, "avg_local_loss": 0.1, "clients": 3,
                "model_mb": 80.1234567, "comm_mb_round": 480.7407402}]
    rows, total = R.fed_summary_rows(records)
    assert total == 480.7407402 * 2
    assert rows[0] == {"round": 1, "val_top1": 0.333333, "val_top5": 0.666667, "avg_local_loss": 1.234568,
                       "clients": 3, "model_mb": 80.123457, "comm_mb_round": 480.74074, "comm_mb_total": 480.74074}
    assert rows[1]["comm_mb_total"] == 961.48148
    R._write_csv(tmp_path / "fed_summary.csv", R.FED_COLUMNS, rows)
    lines = (tmp_path / "fed_summary.csv").read_text().splitlines()
    assert lines[0] == ",".join(R.FED_COLUMNS)
    assert lines[1] == "1,0.333333,0.666667,1.234568,3,80.123457,480.74074,480.74074"
    assert R.system_privacy_row(1000.0, 250.0) == {"raw_upload_mb_est": 1000.0, "fed_comm_total_mb": 250.0,
                                                   "reduction_ratio": 0.25}
    assert R.system_privacy_row(3.0, 1.0)["reduction_ratio"] == 0.333333
    assert R.system_privacy_row(None, 1.0) == {"raw_upload_mb_est": "", "fed_comm_total_mb": 1.0,
                                               "reduction_ratio": ""}
    assert R.system_privacy_row(0.0, 1.0)["reduction_ratio"] == ""


def test_config_validation():
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.utils import load_config
    from conftest import ROOT
    cfg = R.resolve_config(load_config(os.path.join(ROOT, "configs", "federated.yaml")))
    assert cfg["federated"]["exchange"] == "fused" and cfg["dataset"]["train_split"] is None
    assert R.resolve_config({})["federated"]["exchange"] == "fused"
    assert R.resolve_config({}, exchange="reference", save_dir="x")["output"]["save_dir"] == "x"
    over = R.resolve_config({"federated": {"rounds": 7, "non_iid": {"shards_per_client": 2}}})
    assert over["federated"]["rounds"] == 7 and over["federated"]["non_iid"] == {
        "enabled": True, "strategy": "class_shard", "shards_per_client": 2, "min_samples_per_client": 200}
    assert R.DEFAULTS["federated"]["non_iid"]["shards_per_client"] == 6        # defaults not written through
    with pytest.raises(ValueError, match="Unknown config section"):
        R.resolve_config({"federate": {}})
    with pytest.raises(ValueError, match="Unknown keys in federated"):
        R.resolve_config({"federated": {"round": 3}})
    with pytest.raises(ValueError, match="Unknown keys in federated.non_iid"):
        R.resolve_config({"federated": {"non_iid": {"shards": 3}}})
    with pytest.raises(ValueError, match="federated.exchange"):
        R.resolve_config({"federated": {"exchange": "nccl"}})
    with pytest.raises(RuntimeError, match="IID mode not implemented"):
        R.resolve_config({"federated": {"non_iid": {"enabled": False}}})
    with pytest.raises(ValueError):
        R.resolve_config({"federated": {"num_clients": 0}})


def test_round_client_selection_and_call_order(monkeypatch):
    """run_fedavg_fused draws from random.Random(42) exactly as run_fedavg and runs broadcast ->
    updates -> aggregate per round; the cohort (the GPU part) is replaced by a recorder here."""
    import io
    import torch.nn as nn
    from oracle import fedavg_oracle as O
    from ssl_mae_amd import federated as F
    calls = []

    class Recorder:
        def __init__(self, global_model, client_models):
            calls.append(("cohort", len(client_models)))

        def broadcast(self, selected):
            calls.append(("broadcast", list(selected)))

        def aggregate(self, selected, weights, also=()):
            calls.append(("aggregate", list(selected), list(weights)))

    monkeypatch.setattr(F, "FedCohort", Recorder)
    g, clients = nn.Linear(2, 2), [nn.Linear(2, 2) for _ in range(5)]
    sizes = [10, 20, 30, 40, 50]

    def update_fn(cid):
        def fn(model):
            assert model is clients[cid]
            calls.append(("update", cid))
            return float(cid)
        return fn

    loaders = [{"loader": None, "update_fn": update_fn(c)} for c in range(5)]
    log = io.StringIO()
    recs = F.run_fedavg_fused(g, clients, loaders, sizes, lambda m: (0.25, 0.5), None, rounds=3, client_fraction=0.6,
                              log_f=log)
    schedule = O.client_schedule(5, 3, 0.6)
    assert schedule == [[0, 4, 2], [2, 1, 0], [1, 0, 2]]
    want = [("cohort", 5)]
    for sel in schedule:
        want += [("broadcast", sel)] + [("update", c) for c in sel] + [("aggregate", sel, [float(sizes[c]) for c in sel])]
    assert calls == want
    size_b = sum(p.numel() * 4 for p in g.parameters())
    for r, (rec, sel) in enumerate(zip(recs, schedule), 1):
        assert rec == {"round": r, "val_top1": 0.25, "val_top5": 0.5, "avg_local_loss": sum(sel) / 3.0, "clients": 3,
                       "model_mb": size_b / 2 ** 20, "comm_mb_round": 2 * 3 * size_b / 2 ** 20}
    text = log.getvalue()
    assert "[INFO] Round 1/3 selected_clients=[0, 4, 2]" in text and "[INFO] Round 3 val_top1=0.2500" in text
    assert F.run_fedavg_fused(g, clients, loaders, sizes, lambda m: (0, 0), None, rounds=2, client_fraction=0.1)[0][
        "clients"] == 1

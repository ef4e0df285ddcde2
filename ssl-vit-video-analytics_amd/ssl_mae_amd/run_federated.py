"""Federated fine-tuning experiment, the reference's "system-level privacy" study
(src/run_federated.py), MI355X-native: a centralized baseline, class-shard non-IID FedAvg over
finetune.VideoClassifier models on one GPU, and a communication summary.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.run_federated \
        --config configs/federated.yaml [--save_dir results/federated] [--exchange fused|reference]

Flow (run_federated.py:209-363): centralized baseline -> client splits + fed_client_stats.csv ->
global and client models -> FedAvg rounds -> fed_summary.csv, centralized_summary.csv and
system_privacy_summary.csv, with the reference's columns and 6-decimal rounding.  The round's
exchange goes through federated.run_fedavg_fused (one broadcast launch and one aggregation launch
over the models' tensors where they live); `federated.exchange: reference` keeps run_fedavg's
state_dict path, with bit-identical model states.  `federated.dp.enabled: true` turns the
aggregation into DP-FedAvg (clipped client updates, Gaussian noise on the aggregate; federated.
FedCohort.aggregate_dp / dp_aggregate_reference) and adds fed_dp_summary.csv with the round's
clipping statistics and the accountant's cumulative epsilon ESTIMATE (federated.dp_epsilon).
`federated.compress.enabled: true` uploads every client's update as int8 codes with one fp32 scale
per 256 elements, with error feedback (federated.FedCohort.aggregate_q8 / q8_aggregate_reference):
fed_summary.csv and system_privacy_summary.csv then carry the compressed communication, and
fed_compress_summary.csv the round's upload sizes and quantisation statistics.  DP and compression
are exclusive.

`make_class_shard_splits` / `read_split` / `write_split` are src/datasets/federated_split.py
(same random.Random(seed) call order: the same seed writes the same files), `client_update` is
src/federated/client_sim.py under bf16 autocast with the cross-entropy from sm_logits_metrics
(driver.train_pass), `evaluate_topk` is run_federated.py:20-39 through the same kernel
(driver.evaluate).  Without `dataset.train_split` the driver runs on labelled synthetic clips
(driver.SyntheticClips), partitioned by the same class-shard rule.
"""
import argparse
import functools
import random
from collections import defaultdict
from pathlib import Path

import torch

from .driver import SyntheticClips, build_classifier, evaluate, merge_config, split_file_loader, start, train_pass
from .federated import bytes_to_mb, dp_epsilon, run_fedavg, run_fedavg_fused
from .utils import load_config, log_line
from .utils import write_csv as _write_csv

CLIENT_STATS_HEADER = "client,num_samples,num_classes,classes\n"
FED_COLUMNS = ("round", "val_top1", "val_top5", "avg_local_loss", "clients", "model_mb", "comm_mb_round",
               "comm_mb_total")
CENTRALIZED_COLUMNS = ("epoch", "train_loss", "val_top1", "val_top5")
SYSTEM_COLUMNS = ("raw_upload_mb_est", "fed_comm_total_mb", "reduction_ratio")
DP_COLUMNS = ("round", "clients", "dp_clipped", "dp_norm_mean", "dp_norm_max", "dp_noise_std", "epsilon_est", "delta")
COMPRESS_COLUMNS = ("round", "clients", "upload_mb_fp32", "upload_mb_q8", "upload_ratio", "q8_absmax", "q8_resid_norm")
COMPRESS_METHODS = ("q8",)
EXCHANGES = {"fused": run_fedavg_fused, "reference": run_fedavg}

DEFAULTS = {
    "dataset": {"name": None, "train_split": None, "val_split": None, "num_classes": 101, "clip_len": 16,
                "stride": 4, "image_size": 112},
    "model": {"embed_dim": 576, "init_ckpt": None},
    "federated": {"num_clients": 4, "rounds": 3, "local_epochs": 1, "client_fraction": 1.0, "batch_size": 8,
                  "lr": 3e-4, "weight_decay": 0.01, "exchange": "fused",
                  "non_iid": {"enabled": True, "strategy": "class_shard", "shards_per_client": 6,
                              "min_samples_per_client": 200},
                  # DP-FedAvg; seed None: runtime.seed
                  "dp": {"enabled": False, "clip_norm": 1.0, "noise_multiplier": 0.0, "delta": 1e-5, "seed": None},
                  # int8 block-quantised uploads; error_feedback false drops the residuals every round
                  "compress": {"enabled": False, "method": "q8", "error_feedback": True}},
    # None: the federated value (epochs: rounds * local_epochs, the same training budget)
    "centralized": {"enabled": True, "epochs": None, "batch_size": None, "lr": None, "weight_decay": None},
    "system_privacy": {"estimate_raw_upload": True, "raw_dtype_bytes": 1},
    "synthetic": {"num_train": 96, "num_val": 32},
    "runtime": {"amp": True, "seed": 42, "num_workers": 4},
    "output": {"save_dir": "results/federated", "split_prefix": "fed"},
}


def resolve_config(cfg, save_dir=None, exchange=None):
    """The file's values over DEFAULTS, the command line over both; unknown sections or keys
    raise, and so does `non_iid.enabled: false` (run_federated.py:263-264)."""
    out = merge_config(DEFAULTS, cfg)
    if save_dir is not None:
        out["output"]["save_dir"] = save_dir
    if exchange is not None:
        out["federated"]["exchange"] = exchange
    fed = out["federated"]
    if fed["exchange"] not in EXCHANGES:
        raise ValueError(f"[ERROR] Unknown federated.exchange: {fed['exchange']}, must be one of {sorted(EXCHANGES)}")
    if not fed["non_iid"]["enabled"]:
        raise RuntimeError("[ERROR] IID mode not implemented; enable non_iid.")
    if int(fed["num_clients"]) < 1 or int(fed["rounds"]) < 0 or int(fed["local_epochs"]) < 0 \
            or int(fed["batch_size"]) < 1 or int(fed["non_iid"]["shards_per_client"]) < 1:
        raise ValueError("[ERROR] federated: num_clients, batch_size, shards_per_client >= 1; rounds, "
                         "local_epochs >= 0")
    dp = fed["dp"]
    if not float(dp["clip_norm"]) > 0.0 or not float(dp["noise_multiplier"]) >= 0.0 \
            or not 0.0 < float(dp["delta"]) < 1.0:
        raise ValueError("[ERROR] federated.dp: clip_norm > 0, noise_multiplier >= 0, 0 < delta < 1")
    comp = fed["compress"]
    if comp["method"] not in COMPRESS_METHODS:
        raise ValueError(f"[ERROR] Unknown federated.compress.method: {comp['method']}, must be one of "
                         f"{sorted(COMPRESS_METHODS)}")
    if bool(dp["enabled"]) and bool(comp["enabled"]):
        raise ValueError("[ERROR] federated.dp and federated.compress are exclusive: quantising a clipped, noised "
                         "aggregate changes the sensitivity analysis")
    return out


# ------------------------------------------------------------------ class-shard splits (federated_split.py)
def read_split(split_file):
    items = []
    with open(split_file, "r", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if not line:
                continue
            p, y = line.split()
            items.append((p, int(y)))
    return items


def write_split(items, out_path):
    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    with open(out_path, "w", encoding="utf-8") as f:
        for p, y in items:
            f.write(f"{p} {y}\n")


def shard_items(items, num_clients, shards_per_client=6, seed=42, min_samples_per_client=200):
    """federated_split.py:43-86 on a list of (path, label): every class is one shard, shuffled
    within; the shuffled class list is dealt out `shards_per_client` classes per client with
    wrap-around; then up to 200 moves of at most 200 samples from the largest client to the
    smallest while one is below `min_samples_per_client` (which can leave a client empty)."""
    rng = random.Random(seed)
    by_class = defaultdict(list)
    for p, y in items:
        by_class[y].append((p, y))
    for y in by_class:
        rng.shuffle(by_class[y])
    class_ids = sorted(by_class.keys())
    rng.shuffle(class_ids)
    client_items = [[] for _ in range(num_clients)]
    for idx, cid in enumerate(class_ids):
        client_items[(idx // shards_per_client) % num_clients].extend(by_class[cid])
    for _ in range(200):
        s = [len(ci) for ci in client_items]
        mn, mx = min(s), max(s)
        if mn >= min_samples_per_client:
            break
        small, large = s.index(mn), s.index(mx)
        if len(client_items[large]) <= min_samples_per_client:
            break
        move_n = min(200, len(client_items[large]) - min_samples_per_client)
        client_items[small].extend(client_items[large][:move_n])
        client_items[large] = client_items[large][move_n:]
    return client_items


def make_class_shard_splits(base_split_file, num_clients, shards_per_client=6, seed=42, min_samples_per_client=200,
                            out_prefix="fed", out_dir="data/splits"):
    """federated_split.py:26-105 -> (paths of {out_dir}/{out_prefix}_client_{i}_train.txt, stats)."""
    client_items = shard_items(read_split(base_split_file), num_clients, shards_per_client, seed,
                               min_samples_per_client)
    out_paths, out_stats = [], []
    for i, items in enumerate(client_items):
        out_path = Path(out_dir) / f"{out_prefix}_client_{i}_train.txt"
        write_split(items, out_path)
        out_paths.append(str(out_path))
        cls_set = sorted({y for _, y in items})
        out_stats.append({"client": i, "num_samples": len(items), "num_classes": len(cls_set),
                          "classes": " ".join(map(str, cls_set[:50]))})
    return out_paths, out_stats


# ------------------------------------------------------------------ client update / evaluation
def client_update(model, loader, device, epochs=1, lr=3e-4, weight_decay=0.01, amp=True):
    """client_sim.py:30-67: `epochs` local passes with a fresh AdamW over all parameters; returns
    the average loss.  The running loss * batch sum stays on the device: one read-back per call."""
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=float(lr), weight_decay=float(weight_decay))
    sums = torch.zeros(2, dtype=torch.float64, device=device)     # (loss, loss * batch)
    total = 0
    for _ in range(int(epochs)):
        _, samples = train_pass(model, loader, opt, device, amp, sums)
        total += samples
    return float(sums[1].item()) / max(1, total)


def evaluate_topk(model, loader, device):
    """run_federated.py:20-39 -> (top1, top5) with k = min(5, classes): driver.evaluate."""
    acc = evaluate(model, loader, device, topk=(1, 5))
    return acc[1], acc[5]


def train_centralized(cfg, device, train_loader, val_loader, out_dir, log=print):
    """run_federated.py:100-180: the baseline under the same budget, epochs = rounds *
    local_epochs unless overridden, one AdamW across all epochs.  `train_loader(batch_size)`
    builds the shuffled loader over the whole training split.  Returns the rows of
    centralized_summary.csv, or None when disabled."""
    c_cfg, fed = cfg["centralized"], cfg["federated"]
    if not bool(c_cfg["enabled"]):
        return None
    epochs = c_cfg["epochs"]
    epochs = int(fed["rounds"]) * int(fed["local_epochs"]) if epochs is None else int(epochs)

    def pick(key):
        return fed[key] if c_cfg[key] is None else c_cfg[key]

    loader = train_loader(int(pick("batch_size")))
    model = build_classifier(cfg, cfg["model"]["init_ckpt"], device)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=float(pick("lr")), weight_decay=float(pick("weight_decay")))
    rows = []
    for ep in range(1, epochs + 1):
        model.train()
        sums = torch.zeros(2, dtype=torch.float64, device=device)
        _, total = train_pass(model, loader, opt, device, cfg["runtime"]["amp"], sums)
        avg_loss = float(sums[1].item()) / max(1, total)
        top1, top5 = evaluate_topk(model, val_loader, device)
        log(f"[INFO][Centralized] ep={ep}/{epochs} train_loss={avg_loss:.4f} val_top1={top1:.4f} "
            f"val_top5={top5:.4f}")
        rows.append({"epoch": ep, "train_loss": round(avg_loss, 6), "val_top1": round(top1, 6),
                     "val_top5": round(top5, 6)})
    out_csv = Path(out_dir) / "centralized_summary.csv"
    _write_csv(out_csv, CENTRALIZED_COLUMNS, rows)
    log(f"[INFO] Saved centralized summary: {out_csv}")
    return rows


def estimate_raw_upload_mb(cfg, train_split):
    """run_federated.py:183-206: the MiB a centralized run would upload once, samples x
    3 x clip_len x image_size^2 x raw_dtype_bytes; None when switched off."""
    sp = cfg["system_privacy"]
    if not bool(sp["estimate_raw_upload"]):
        return None
    clip_len, img = int(cfg["dataset"]["clip_len"]), int(cfg["dataset"]["image_size"])
    per_sample_bytes = 3 * clip_len * img * img * int(sp["raw_dtype_bytes"])
    with open(train_split, "r", encoding="utf-8") as f:
        n = sum(1 for line in f if line.strip())
    return bytes_to_mb(n * per_sample_bytes)


def fed_summary_rows(records):
    """run_federated.py:328-341 -> (rows of fed_summary.csv, total communication in MiB)."""
    comm_total, rows = 0.0, []
    for r in records:
        comm_total += float(r["comm_mb_round"])
        rows.append({"round": r["round"], "val_top1": round(float(r["val_top1"]), 6),
                     "val_top5": round(float(r["val_top5"]), 6),
                     "avg_local_loss": round(float(r["avg_local_loss"]), 6), "clients": int(r["clients"]),
                     "model_mb": round(float(r["model_mb"]), 6),
                     "comm_mb_round": round(float(r["comm_mb_round"]), 6),
                     "comm_mb_total": round(float(comm_total), 6)})
    return rows, comm_total


def dp_summary_rows(records, dp, num_clients):
    """The rows of fed_dp_summary.csv: the round's clipping statistics and the accountant's
    estimate of the epsilon spent up to and including that round, at sample rate clients /
    num_clients (federated.dp_epsilon states what the estimate assumes)."""
    rows = []
    for i, r in enumerate(records, 1):
        eps = dp_epsilon(float(dp["noise_multiplier"]), min(1.0, int(r["clients"]) / max(1, int(num_clients))), i,
                         float(dp["delta"]))
        rows.append({"round": r["round"], "clients": int(r["clients"]), "dp_clipped": int(r["dp_clipped"]),
                     "dp_norm_mean": round(float(r["dp_norm_mean"]), 6),
                     "dp_norm_max": round(float(r["dp_norm_max"]), 6),
                     "dp_noise_std": round(float(r["dp_noise_std"]), 6), "epsilon_est": round(eps, 6),
                     "delta": float(dp["delta"])})
    return rows


def compress_summary_rows(records):
    """The rows of fed_compress_summary.csv: the round's fp32 and compressed upload sizes, their
    ratio, and the quantiser's statistics (the largest |update + residual| over the clients, the
    L2 norm of all their new residuals)."""
    return [{"round": r["round"], "clients": int(r["clients"]),
             "upload_mb_fp32": round(float(r["upload_mb_fp32"]), 6),
             "upload_mb_q8": round(float(r["upload_mb_q8"]), 6),
             "upload_ratio": round(float(r["upload_mb_q8"]) / float(r["upload_mb_fp32"]), 6),
             "q8_absmax": round(float(r["q8_absmax"]), 6),
             "q8_resid_norm": round(float(r["q8_resid_norm"]), 6)} for r in records]


def system_privacy_row(raw_upload_mb, fed_comm_mb):
    """run_federated.py:356-360."""
    has_raw = raw_upload_mb is not None
    return {"raw_upload_mb_est": round(raw_upload_mb, 6) if has_raw else "",
            "fed_comm_total_mb": round(fed_comm_mb, 6),
            "reduction_ratio": round(fed_comm_mb / raw_upload_mb, 6) if has_raw and raw_upload_mb > 0 else ""}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Federated fine-tuning: centralized baseline, non-IID FedAvg, "
                                             "communication summary.")
    ap.add_argument("--config", default="configs/federated.yaml")
    ap.add_argument("--save_dir", default=None, help="override output.save_dir")
    ap.add_argument("--exchange", default=None, help="override federated.exchange (fused|reference)")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config), args.save_dir, args.exchange)
    seed = int(cfg["runtime"]["seed"])
    device = start("run_federated", seed)
    fed, ds = cfg["federated"], cfg["dataset"]
    out_dir = Path(cfg["output"]["save_dir"])
    out_dir.mkdir(parents=True, exist_ok=True)
    batch_size = int(fed["batch_size"])

    if ds["train_split"]:
        if not ds["val_split"]:
            raise ValueError("[ERROR] dataset.val_split is needed with dataset.train_split")
        train_split, split_dir = Path(ds["train_split"]), Path(ds["train_split"]).parent

        def loader_of(split_file, bs, shuffle, s):
            return split_file_loader(str(split_file), clip_len=ds["clip_len"], stride=ds["stride"],
                                     image_size=ds["image_size"], batch_size=bs,
                                     num_workers=cfg["runtime"]["num_workers"], device=device, shuffle=shuffle,
                                     drop_last=shuffle, seed=s)
    else:
        # labelled synthetic clips, listed in a split file so the same class-shard rule applies
        split_dir = out_dir / "splits"
        train_split = split_dir / "synthetic_train.txt"
        train_set = SyntheticClips(cfg, int(cfg["synthetic"]["num_train"]), seed, device)
        val_set = SyntheticClips(cfg, int(cfg["synthetic"]["num_val"]), seed + 1, device)
        write_split(train_set.items(), train_split)
        write_split(val_set.items(), split_dir / "synthetic_val.txt")

        def loader_of(split_file, bs, shuffle, s):
            data = val_set if Path(split_file).name == "synthetic_val.txt" else train_set
            return data.loader(read_split(split_file), bs, shuffle, s)
    val_split = Path(ds["val_split"]) if ds["train_split"] else split_dir / "synthetic_val.txt"

    with open(out_dir / "federated.log", "a", encoding="utf-8") as log_f:
        log = functools.partial(log_line, log_f)
        log(f"[INFO] Federated experiment started, exchange={fed['exchange']}")
        val_loader = loader_of(val_split, batch_size, False, seed + 999)
        centralized_rows = train_centralized(cfg, device, lambda bs: loader_of(train_split, bs, True, seed + 123),
                                             val_loader, out_dir, log)

        num_clients = int(fed["num_clients"])
        split_paths, client_stats = make_class_shard_splits(
            str(train_split), num_clients, shards_per_client=int(fed["non_iid"]["shards_per_client"]), seed=seed,
            min_samples_per_client=int(fed["non_iid"]["min_samples_per_client"]),
            out_prefix=cfg["output"]["split_prefix"], out_dir=str(split_dir))
        stats_csv = out_dir / "fed_client_stats.csv"
        stats_csv.write_text(CLIENT_STATS_HEADER + "".join(
            f"{s['client']},{s['num_samples']},{s['num_classes']},{s['classes']}\n" for s in client_stats),
            encoding="utf-8")
        log(f"[INFO] Saved client stats: {stats_csv}")

        global_model = build_classifier(cfg, cfg["model"]["init_ckpt"], device)
        client_models = [build_classifier(cfg, None, device, load=None) for _ in range(num_clients)]
        client_sizes, client_loaders = [], []
        for cid in range(num_clients):
            loader = loader_of(split_paths[cid], batch_size, True, seed + cid)
            client_sizes.append(client_stats[cid]["num_samples"])

            def update_fn(model, _loader=loader):
                return client_update(model, _loader, device, epochs=int(fed["local_epochs"]), lr=float(fed["lr"]),
                                     weight_decay=float(fed["weight_decay"]), amp=bool(cfg["runtime"]["amp"]))

            client_loaders.append({"loader": loader, "update_fn": update_fn})

        dp = fed["dp"]
        round_args = {}
        if bool(dp["enabled"]):        # off: the call below is exactly the plain one
            round_args["dp"] = {"clip_norm": float(dp["clip_norm"]), "noise_multiplier": float(dp["noise_multiplier"]),
                             "seed": seed if dp["seed"] is None else int(dp["seed"])}
            log(f"[INFO] DP-FedAvg: clip_norm={round_args['dp']['clip_norm']} "
                f"noise_multiplier={round_args['dp']['noise_multiplier']} delta={float(dp['delta'])}")
        comp = fed["compress"]
        if bool(comp["enabled"]):      # off: the call below is exactly the plain one
            round_args["compress"] = {"method": comp["method"], "error_feedback": bool(comp["error_feedback"])}
            log(f"[INFO] Compressed uploads: method={comp['method']} error_feedback={bool(comp['error_feedback'])}")
        records = EXCHANGES[fed["exchange"]](
            global_model, client_models, client_loaders, client_sizes, lambda m: evaluate_topk(m, val_loader, device),
            device, rounds=int(fed["rounds"]), client_fraction=float(fed["client_fraction"]),
            amp=bool(cfg["runtime"]["amp"]), log_f=log_f, **round_args)

        rows, comm_total = fed_summary_rows(records)
        fed_csv = out_dir / "fed_summary.csv"
        _write_csv(fed_csv, FED_COLUMNS, rows)
        log(f"[INFO] Saved federated summary: {fed_csv}")
        if "compress" in round_args:
            comp_csv = out_dir / "fed_compress_summary.csv"
            _write_csv(comp_csv, COMPRESS_COLUMNS, compress_summary_rows(records))
            log(f"[INFO] Saved compression summary: {comp_csv}")
        if "dp" in round_args:
            dp_csv = out_dir / "fed_dp_summary.csv"
            _write_csv(dp_csv, DP_COLUMNS, dp_summary_rows(records, dp, num_clients))
            log(f"[INFO] Saved DP summary (epsilon_est is an estimate): {dp_csv}")
        sys_row = system_privacy_row(estimate_raw_upload_mb(cfg, train_split), comm_total)
        sys_csv = out_dir / "system_privacy_summary.csv"
        _write_csv(sys_csv, SYSTEM_COLUMNS, [sys_row])
        log(f"[INFO] Saved system privacy summary: {sys_csv}")
    return {"centralized": centralized_rows, "federated": rows, "system": sys_row, "client_stats": client_stats,
            "save_dir": out_dir}


if __name__ == "__main__":
    main()

"""Weighted kNN evaluation of pretrained features: how good is a representation, without training
anything on it (Wu et al. 2018; the probe DINO and others report).  MI355X-native, no counterpart
in the reference.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.run_knn \
        --config configs/knn.yaml [--ckpt A.pth [B.pth ...]] [--save_dir DIR] [--impl fused|reference]

Every checkpoint (an `ssl_ep{N}.pth`, an MAE `encoder_ep{N}.pth` or a fine-tuned classifier: what
finetune.load_finetune_ckpt reads) is embedded and evaluated in turn: the bank from
`dataset.train_split`, the queries from `dataset.val_split`, each query voting with its k nearest
bank rows (knn.knn_eval).  `knn_eval.csv` gets one row per checkpoint and k.  Without a
`val_split` the bank is evaluated against itself: with `knn.leave_one_out` every query's own row
is removed, without it k = 1 finds the query itself.  Without splits the driver runs on labelled
synthetic clips (random labels: the accuracy columns then only show chance).  `runtime.amp`
governs only the backbone pass; the search and the vote are always fp32.
"""
import argparse
import time
from pathlib import Path

import torch

from . import knn as KNN
from . import privacy as P
from .driver import SyntheticBatches, build_classifier, merge_config, split_file_loader, start
from .utils import load_config, log_line

CSV_COLUMNS = ("ckpt", "k", "top1", "top5", "n_bank", "n_query")
CSV_HEADER = ",".join(CSV_COLUMNS) + "\n"

DEFAULTS = {
    "dataset": {"name": None, "train_split": None, "val_split": None, "num_classes": 101, "clip_len": 16,
                "stride": 4, "image_size": 112},
    "model": {"embed_dim": 576, "ckpts": None},
    "knn": {"ks": [1, 5, 10, 20], "temperature": 0.07, "metric": "cosine", "leave_one_out": False, "impl": "fused"},
    "runtime": {"batch_size": 16, "num_batches": 6, "amp": True, "seed": 42, "num_workers": 4},
    "output": {"save_dir": "results/knn"},
}


def resolve_config(cfg, ckpts=None, save_dir=None, impl=None):
    """The file's values over DEFAULTS, the command line over both; unknown sections or keys
    raise.  `model.ckpts` becomes a list (None: one run on the portable-rule initialisation);
    `knn.ks` must be 1 to 8 strictly ascending integers within [1, 64]."""
    out = merge_config(DEFAULTS, cfg)
    if ckpts:
        out["model"]["ckpts"] = list(ckpts)
    if save_dir is not None:
        out["output"]["save_dir"] = save_dir
    if impl is not None:
        out["knn"]["impl"] = impl
    ck = out["model"]["ckpts"]
    if ck is None or ck == []:
        ck = [None]
    elif isinstance(ck, str):
        ck = [ck]
    elif not isinstance(ck, (list, tuple)) or not all(isinstance(c, str) for c in ck):
        raise ValueError("[ERROR] model.ckpts must be a path or a list of paths")
    out["model"]["ckpts"] = list(ck)
    kn, ds = out["knn"], out["dataset"]
    kn["ks"] = KNN.check_ks(kn["ks"])
    kn["temperature"] = float(kn["temperature"])
    if not kn["temperature"] > 0.0:
        raise ValueError("[ERROR] knn.temperature must be > 0")
    if kn["metric"] not in KNN.METRICS:
        raise ValueError(f"[ERROR] knn.metric must be one of {KNN.METRICS}")
    if kn["impl"] not in ("fused", "reference"):
        raise ValueError("[ERROR] knn.impl must be fused or reference")
    kn["leave_one_out"] = bool(kn["leave_one_out"])
    if ds["val_split"] and not ds["train_split"]:
        raise ValueError("[ERROR] dataset.val_split needs dataset.train_split for the bank")
    if kn["leave_one_out"] and ds["val_split"]:
        raise ValueError("[ERROR] knn.leave_one_out evaluates the bank against itself: leave dataset.val_split empty")
    if int(ds["num_classes"]) < 1 or int(out["runtime"]["num_batches"]) < 1 or int(out["runtime"]["batch_size"]) < 1:
        raise ValueError("[ERROR] dataset.num_classes, runtime.num_batches and runtime.batch_size must be >= 1")
    return out


def format_row(row):
    """One CSV line: the two accuracies rounded to 6 places (as run_privacy.format_row)."""
    return (f"{row['ckpt']},{int(row['k'])},{round(float(row['top1']), 6)},{round(float(row['top5']), 6)},"
            f"{int(row['n_bank'])},{int(row['n_query'])}\n")


def _loader(cfg, split, device):
    ds, rt = cfg["dataset"], cfg["runtime"]
    if split:
        return split_file_loader(split, clip_len=ds["clip_len"], stride=ds["stride"], image_size=ds["image_size"],
                                 batch_size=rt["batch_size"], num_workers=rt["num_workers"], device=device)
    return SyntheticBatches(rt["num_batches"], rt["batch_size"], ds["clip_len"], ds["image_size"], device,
                            seed=rt["seed"], num_classes=ds["num_classes"])


@torch.no_grad()
def extract_embeddings(model, loader, cfg):
    """-> (z fp32 [N, D], y int64 [N]) on the device."""
    zs, ys = [], []
    for clip, label in loader:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(cfg["runtime"]["amp"])):
            z = P.video_embeddings(model, clip)
        zs.append(z.float())
        ys.append(label.long())
    return torch.cat(zs).contiguous(), torch.cat(ys).contiguous()


def evaluate_ckpt(cfg, ckpt, device, log_f):
    """One checkpoint -> (rows, knn_eval's result)."""
    kn, ds = cfg["knn"], cfg["dataset"]
    model = build_classifier(cfg, ckpt, device).eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    zb, yb = extract_embeddings(model, _loader(cfg, ds["train_split"], device), cfg)
    zq, yq = extract_embeddings(model, _loader(cfg, ds["val_split"], device), cfg) if ds["val_split"] else (zb, yb)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = KNN.knn_eval(zq, yq, zb, yb, kn["ks"], kn["temperature"], int(ds["num_classes"]), kn["metric"],
                       leave_one_out=kn["leave_one_out"], impl=kn["impl"])
    t2 = time.perf_counter()
    name = "none" if ckpt is None else str(ckpt)
    rows = [{"ckpt": name, "k": k, "top1": a, "top5": b, "n_bank": zb.shape[0], "n_query": zq.shape[0]}
            for k, a, b in zip(res["ks"], res["top1"], res["top5"])]
    for r in rows:
        log_line(log_f, f"[INFO] ckpt={name} k={r['k']} | top1={r['top1']:.4f} top5={r['top5']:.4f}")
    log_line(log_f, f"[INFO] embedding pass {t1 - t0:.3f} s ({zb.shape[0]} bank, {zq.shape[0]} query clips), "
                    f"kNN ({kn['impl']}) {t2 - t1:.3f} s")
    return rows, res


def main(argv=None):
    ap = argparse.ArgumentParser(description="Weighted kNN evaluation of pretrained features.")
    ap.add_argument("--config", default="configs/knn.yaml")
    ap.add_argument("--ckpt", nargs="+", default=None, help="override model.ckpts: one or more checkpoints")
    ap.add_argument("--save_dir", default=None, help="override output.save_dir")
    ap.add_argument("--impl", default=None, choices=("fused", "reference"), help="override knn.impl")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config), args.ckpt, args.save_dir, args.impl)
    device = start("run_knn", cfg["runtime"]["seed"])
    save_dir = Path(cfg["output"]["save_dir"])
    save_dir.mkdir(parents=True, exist_ok=True)
    out_csv = save_dir / "knn_eval.csv"
    rows, results = [], []
    with open(save_dir / "knn.log", "a", encoding="utf-8") as log_f:
        log_line(log_f, "[INFO] kNN evaluation started")
        ds = cfg["dataset"]
        if not ds["train_split"]:
            log_line(log_f, "[INFO] No dataset.train_split: synthetic clips with random labels, the accuracies only "
                            "show chance")
        if not ds["val_split"]:
            log_line(log_f, "[INFO] No dataset.val_split: the bank is evaluated against itself "
                            + ("(leave-one-out)" if cfg["knn"]["leave_one_out"]
                               else "(every query finds itself first: set knn.leave_one_out)"))
        for ckpt in cfg["model"]["ckpts"]:
            r, res = evaluate_ckpt(cfg, ckpt, device, log_f)
            rows += r
            results.append(res)
        out_csv.write_text(CSV_HEADER + "".join(format_row(r) for r in rows), encoding="utf-8")
        log_line(log_f, f"[INFO] Saved kNN CSV: {out_csv}")
        log_line(log_f, "[INFO] kNN evaluation finished.")
    return {"rows": rows, "results": results, "csv": out_csv}


if __name__ == "__main__":
    main()

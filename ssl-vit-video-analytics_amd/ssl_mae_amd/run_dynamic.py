"""Dynamic-inference experiments on a fine-tuned VideoClassifier: confidence early-exit,
motion frame gating and their hybrid (reference src/run_dynamic.py), MI355X-native.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.run_dynamic \
        --config configs/dynamic.yaml [--mode early_exit|frame_gating|hybrid] [--ckpt model.pth]

`run_early_exit` (:78-163), `run_frame_gating` (:167-232) and `run_hybrid` (:236-324) keep
the reference's loops, metrics and CSV columns; latency is taken with HIP events over the
batches [num_warmup, num_warmup + num_measure).  The model is finetune.VideoClassifier
(TinyViT backbone, eval mode); frames go through ssl_mae_amd.dynamic_infer, so a decided
sample is never encoded again.  Without `dataset.split` the driver runs on synthetic clips
(random labels: the accuracy columns then only show chance), as bench.py does.
"""
import argparse
from pathlib import Path

import torch

from .driver import SyntheticBatches, build_classifier, merge_config, split_file_loader, start
from .dynamic_infer import select_topk_frames, streaming_early_exit
from .finetune import accuracy_topk
from .finetune import load_finetune_ckpt  # noqa: F401  (callers import it from here)
from .utils import load_config, log_line

MODES = ("early_exit", "frame_gating", "hybrid")
EARLY_EXIT_HEADER = "threshold,top1,top5,avg_frames,avg_conf,avg_latency_ms,throughput_fps\n"
FRAME_GATING_HEADER = "k,top1,top5,avg_latency_ms,throughput_clips_per_s\n"
HYBRID_HEADER = "k,threshold,top1,top5,avg_used_frames,avg_conf,avg_latency_ms\n"

DEFAULTS = {
    "dataset": {"split": None, "num_classes": 101, "clip_len": 16, "stride": 4, "image_size": 112},
    "model": {"embed_dim": 576, "finetune_ckpt": None},
    "dynamic": {"mode": "early_exit", "confidence_thresholds": [0.5, 0.7, 0.9], "min_frames": 4, "max_frames": 16,
                "frame_step": 1, "gating_topk_list": [4, 8], "gating_score": "motion"},
    "runtime": {"batch_size": 16, "num_warmup": 2, "num_measure": 4, "amp": True, "seed": 42, "num_workers": 4},
    "output": {"save_dir": "results/dynamic", "save_csv": True},
}


def resolve_config(cfg, mode=None, ckpt=None, save_dir=None):
    """The file's values over DEFAULTS, the command line over both; validates the mode, the
    gating score and the list-valued keys."""
    out = merge_config(DEFAULTS, cfg)
    if mode is not None:
        out["dynamic"]["mode"] = mode
    if ckpt is not None:
        out["model"]["finetune_ckpt"] = ckpt
    if save_dir is not None:
        out["output"]["save_dir"] = save_dir
    dyn = out["dynamic"]
    if dyn["mode"] not in MODES:
        raise ValueError(f"[ERROR] Unknown dynamic.mode: {dyn['mode']}, must be one of {list(MODES)}")
    if dyn["gating_score"] not in ("motion", "random"):
        raise ValueError(f"[ERROR] Unknown dynamic.gating_score: {dyn['gating_score']}")
    dyn["confidence_thresholds"] = [float(t) for t in dyn["confidence_thresholds"]]
    dyn["gating_topk_list"] = [int(k) for k in dyn["gating_topk_list"]]
    if not dyn["confidence_thresholds"] or not dyn["gating_topk_list"] or min(dyn["gating_topk_list"]) < 1:
        raise ValueError("[ERROR] confidence_thresholds and gating_topk_list need at least one entry; k >= 1")
    return out


class SyntheticLoader(SyntheticBatches):
    """num_warmup + num_measure fixed batches of synthetic clips with random labels, already on
    the device, seeded with `runtime.seed`."""

    def __init__(self, cfg, device):
        ds, rt = cfg["dataset"], cfg["runtime"]
        super().__init__(int(rt["num_warmup"]) + int(rt["num_measure"]), rt["batch_size"], ds["clip_len"],
                         ds["image_size"], device, seed=rt["seed"], num_classes=ds["num_classes"])


def split_loader(cfg, device, shuffle=False, drop_last=False, seed=None):
    """`dataset.split` (lines of `<frame directory> <label>`) through driver.split_file_loader;
    `shuffle` / `drop_last` draw their order from a generator seeded with `seed`."""
    ds, rt = cfg["dataset"], cfg["runtime"]
    return split_file_loader(ds["split"], clip_len=ds["clip_len"], stride=ds["stride"], image_size=ds["image_size"],
                             batch_size=rt["batch_size"], num_workers=rt["num_workers"], device=device,
                             shuffle=shuffle, drop_last=drop_last, seed=seed)


class _Timer:
    """HIP-event latency of the measured batches."""

    def __init__(self, cfg):
        self.lo = int(cfg["runtime"]["num_warmup"])
        self.hi = self.lo + int(cfg["runtime"]["num_measure"])
        self.ms = []

    def start(self, i):
        self.on = self.lo <= i < self.hi
        if self.on:
            self.t0 = torch.cuda.Event(enable_timing=True)
            self.t1 = torch.cuda.Event(enable_timing=True)
            self.t0.record()

    def stop(self):
        if self.on:
            self.t1.record()
            torch.cuda.synchronize()
            self.ms.append(self.t0.elapsed_time(self.t1))

    def mean(self):
        return sum(self.ms) / len(self.ms) if self.ms else 0.0


def _autocast(cfg):
    return torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(cfg["runtime"]["amp"]))


def _emit(cfg, name, lines, log_f, msg=None):
    if msg:
        log_line(log_f, msg)
    if lines is not None and cfg["output"]["save_csv"]:
        path = Path(cfg["output"]["save_dir"]) / name
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text("".join(lines), encoding="utf-8")
        print(f"[INFO] Saved summary CSV: {path}")


def _topk(nc):
    return (1, min(5, nc))


@torch.no_grad()
def run_early_exit(model, loader, device, cfg, log_f):
    dyn = cfg["dynamic"]
    lines = [EARLY_EXIT_HEADER]
    for thr in dyn["confidence_thresholds"]:
        c1 = c5 = fsum = csum = 0.0
        total = 0
        timer = _Timer(cfg)
        for i, (clip, label) in enumerate(loader):
            B, T = clip.shape[0], min(clip.shape[2], int(dyn["max_frames"]))
            timer.start(i)
            with _autocast(cfg):
                logits, stats = streaming_early_exit(model.backbone, model.classifier, clip[:, :, :T], float(thr),
                                                     min_frames=int(dyn["min_frames"]), max_frames=T,
                                                     frame_step=int(dyn["frame_step"]))
            timer.stop()
            k1, k5 = _topk(logits.shape[1])
            acc = accuracy_topk(logits, label, topk=(k1, k5))
            c1, c5, total = c1 + acc[k1] * B, c5 + acc[k5] * B, total + B
            fsum += stats.used_frames.float().sum().item()
            csum += stats.final_conf.sum().item()
        avg_frames, lat = fsum / total, timer.mean()
        fps = loader.batch_size / (lat / 1000.0) * avg_frames if lat > 0 else 0.0
        lines.append(f"{thr:.2f},{c1 / total:.6f},{c5 / total:.6f},{avg_frames:.3f},{csum / total:.4f},{lat:.3f},{fps:.2f}\n")
        _emit(cfg, "", None, log_f, f"[INFO] EarlyExit thr={thr:.2f} Top1={c1 / total:.4f} Top5={c5 / total:.4f} "
                                    f"avg_frames={avg_frames:.2f} avg_latency_ms={lat:.2f}")
    _emit(cfg, "early_exit_results.csv", lines, log_f)
    return lines


@torch.no_grad()
def run_frame_gating(model, loader, device, cfg, log_f):
    dyn = cfg["dynamic"]
    lines = [FRAME_GATING_HEADER]
    for k in dyn["gating_topk_list"]:
        c1 = c5 = 0.0
        total = 0
        timer = _Timer(cfg)
        for i, (clip, label) in enumerate(loader):
            B = clip.shape[0]
            k_eff = min(int(k), clip.shape[2])
            clip_sel, _ = select_topk_frames(clip, k=k_eff, score_type=dyn["gating_score"])
            timer.start(i)
            with _autocast(cfg):
                logits = model(clip_sel)
            timer.stop()
            k1, k5 = _topk(logits.shape[1])
            acc = accuracy_topk(logits, label, topk=(k1, k5))
            c1, c5, total = c1 + acc[k1] * B, c5 + acc[k5] * B, total + B
        lat = timer.mean()
        cps = loader.batch_size / (lat / 1000.0) if lat > 0 else 0.0
        lines.append(f"{k_eff},{c1 / total:.6f},{c5 / total:.6f},{lat:.3f},{cps:.2f}\n")
        _emit(cfg, "", None, log_f, f"[INFO] FrameGating k={k_eff} Top1={c1 / total:.4f} Top5={c5 / total:.4f} "
                                    f"avg_latency_ms={lat:.2f}")
    _emit(cfg, "frame_gating_results.csv", lines, log_f)
    return lines


@torch.no_grad()
def run_hybrid(model, loader, device, cfg, log_f):
    """Frame gating, then streaming early-exit over the kept frames."""
    dyn = cfg["dynamic"]
    lines = [HYBRID_HEADER]
    for k in dyn["gating_topk_list"]:
        for thr in dyn["confidence_thresholds"]:
            c1 = c5 = fsum = csum = 0.0
            total = 0
            timer = _Timer(cfg)
            for i, (clip, label) in enumerate(loader):
                B = clip.shape[0]
                k_eff = min(int(k), clip.shape[2])
                clip_sel, _ = select_topk_frames(clip, k=k_eff, score_type=dyn["gating_score"])
                timer.start(i)
                with _autocast(cfg):
                    logits, stats = streaming_early_exit(model.backbone, model.classifier, clip_sel, float(thr),
                                                         min_frames=int(dyn["min_frames"]), max_frames=k_eff,
                                                         frame_step=int(dyn["frame_step"]))
                timer.stop()
                k1, k5 = _topk(logits.shape[1])
                acc = accuracy_topk(logits, label, topk=(k1, k5))
                c1, c5, total = c1 + acc[k1] * B, c5 + acc[k5] * B, total + B
                fsum += stats.used_frames.float().sum().item()
                csum += stats.final_conf.sum().item()
            lat = timer.mean()
            lines.append(f"{k_eff},{thr:.2f},{c1 / total:.6f},{c5 / total:.6f},{fsum / total:.3f},{csum / total:.4f},"
                         f"{lat:.3f}\n")
            _emit(cfg, "", None, log_f, f"[INFO] Hybrid k={k_eff} thr={thr:.2f} Top1={c1 / total:.4f} "
                                        f"Top5={c5 / total:.4f} avg_used={fsum / total:.2f} lat_ms={lat:.2f}")
    _emit(cfg, "hybrid_results.csv", lines, log_f)
    return lines


RUNNERS = {"early_exit": run_early_exit, "frame_gating": run_frame_gating, "hybrid": run_hybrid}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Dynamic inference experiments (early-exit / frame-gating / hybrid).")
    ap.add_argument("--config", default="configs/dynamic.yaml")
    ap.add_argument("--mode", default=None, help="override dynamic.mode (early_exit|frame_gating|hybrid)")
    ap.add_argument("--ckpt", default=None, help="override model.finetune_ckpt")
    ap.add_argument("--save_dir", default=None, help="override output.save_dir")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config), args.mode, args.ckpt, args.save_dir)
    device = start("run_dynamic", cfg["runtime"]["seed"])
    model = build_classifier(cfg, cfg["model"]["finetune_ckpt"], device).eval()
    loader = split_loader(cfg, device) if cfg["dataset"]["split"] else SyntheticLoader(cfg, device)
    save_dir = Path(cfg["output"]["save_dir"])
    save_dir.mkdir(parents=True, exist_ok=True)
    mode = cfg["dynamic"]["mode"]
    with open(save_dir / "dynamic.log", "a", encoding="utf-8") as log_f:
        _emit(cfg, "", None, log_f, f"[INFO] Dynamic inference started, mode={mode}")
        RUNNERS[mode](model, loader, device, cfg, log_f)
    print("[INFO] Dynamic inference finished")


if __name__ == "__main__":
    main()

"""Feature-privacy evaluation of a fine-tuned VideoClassifier: the utility-against-leakage
curve of its video embeddings under Gaussian noise and random feature masking, with an
auxiliary attacker classifier as the leakage probe (reference src/run_privacy.py:229-348
run_feature_privacy), MI355X-native.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.run_privacy \
        --config configs/privacy.yaml [--ckpt model.pth] [--save_dir results/privacy]

The embeddings, labels and clean logits are extracted once; the whole noise x mask grid then
takes three launches for its utility numbers (privacy.perturb_grid, one head GEMM over G * N
rows, privacy.logits_metrics with G segments) and one freshly initialised attacker per
configuration, trained one after another (privacy.train_attacker).  `feature_privacy.csv` has
the reference's columns and rounding.  `runtime.amp` governs only the backbone pass; the sweep
is always fp32.  Without `dataset.split` the driver runs on synthetic clips (random labels:
the accuracy columns then only show chance).

The reference's visual half (:118-226) detects faces with YuNet and blurs the boxes with
cv2.GaussianBlur.  Detection needs OpenCV and a downloaded model and is not part of this build: an
enabled `visual_privacy` section with the default `detector: yunet` is accepted, logged and
skipped.  With `detector: boxes` the boxes come from `boxes_file` (lines `relative/path,x,y,w,h`)
and the anonymisation and its measurement run on the GPU (visual_privacy.BoxBlur: one blur and one
statistics launch per `batch_frames` frames); `visual_privacy.csv` then has visual_privacy.CSV_COLUMNS,
the examples grid is `visual_privacy_examples.jpg`, and `overwrite: true` writes the anonymised
frames next to `frame_root`.  Without `frame_root` the stage runs on synthetic frames.
"""
import argparse
import time
from pathlib import Path

import torch

from . import privacy as P
from .driver import SyntheticBatches, build_classifier, merge_config, split_file_loader, start
from .utils import load_config, log_line

CSV_COLUMNS = ("sigma", "mask_ratio", "top1", "top5", "entropy", "attacker_top1", "per_vs_clean")
CSV_HEADER = ",".join(CSV_COLUMNS) + "\n"

DEFAULTS = {
    "dataset": {"name": None, "split": None, "num_classes": 101, "clip_len": 16, "stride": 4, "image_size": 112},
    "model": {"embed_dim": 576, "finetune_ckpt": None},
    # the reference's keys, accepted so its config loads (detector yunet: the stage is skipped), and
    # boxes_file / batch_frames of this build's `detector: boxes`
    "visual_privacy": {"enabled": False, "frame_root": None, "max_images": 2000, "save_examples": 8,
                       "detector": "yunet", "yunet_model": None, "yunet_url": None, "conf_threshold": 0.6,
                       "nms_threshold": 0.3, "method": "face_blur", "blur_kernel": 31, "overwrite": False,
                       "output_suffix": "_frames_privacy", "boxes_file": None, "batch_frames": 64},
    "feature_privacy": {"enabled": True, "noise_sigmas": [0.0, 0.05, 0.1, 0.2], "mask_ratios": [0.0, 0.2, 0.4],
                        "attacker_epochs": 10, "attacker_lr": 1e-3},
    "runtime": {"batch_size": 16, "num_batches": 6, "amp": True, "seed": 42, "num_workers": 4},
    "output": {"save_dir": "results/privacy"},
}


def resolve_config(cfg, ckpt=None, save_dir=None):
    """The file's values over DEFAULTS, the command line over both; unknown sections or keys
    raise, the two grid lists are coerced to float and must not be empty."""
    out = merge_config(DEFAULTS, cfg)
    if ckpt is not None:
        out["model"]["finetune_ckpt"] = ckpt
    if save_dir is not None:
        out["output"]["save_dir"] = save_dir
    fp = out["feature_privacy"]
    for key in ("noise_sigmas", "mask_ratios"):
        vals = fp[key]
        if not isinstance(vals, (list, tuple)) or len(vals) == 0:
            raise ValueError(f"[ERROR] feature_privacy.{key} needs at least one entry")
        fp[key] = [float(v) for v in vals]
    if len(fp["noise_sigmas"]) * len(fp["mask_ratios"]) > 64:
        raise ValueError("[ERROR] at most 64 (sigma, mask_ratio) configurations per sweep")
    fp["attacker_epochs"] = int(fp["attacker_epochs"])
    fp["attacker_lr"] = float(fp["attacker_lr"])
    if fp["attacker_epochs"] < 0 or int(out["runtime"]["num_batches"]) < 1:
        raise ValueError("[ERROR] attacker_epochs >= 0 and runtime.num_batches >= 1")
    vp = out["visual_privacy"]
    if vp["enabled"] and vp["detector"] == "boxes":
        from .visual_privacy import odd_kernel
        if vp["method"] != "face_blur":
            raise ValueError(f"[ERROR] visual_privacy.method {vp['method']!r}: detector boxes supports face_blur only")
        vp["blur_kernel"] = odd_kernel(vp["blur_kernel"])
        if not 3 <= vp["blur_kernel"] <= 63:
            raise ValueError("[ERROR] visual_privacy.blur_kernel must lie in [3, 63] (after an even size became size + 1)")
        vp["batch_frames"], vp["max_images"] = int(vp["batch_frames"]), int(vp["max_images"])
        vp["save_examples"] = int(vp["save_examples"])
        if vp["batch_frames"] < 1 or vp["max_images"] < 1 or vp["save_examples"] < 0:
            raise ValueError("[ERROR] visual_privacy needs batch_frames >= 1, max_images >= 1 and save_examples >= 0")
        if vp["frame_root"] and not vp["boxes_file"]:
            raise ValueError("[ERROR] visual_privacy.detector boxes needs boxes_file next to frame_root")
    return out


def format_row(row):
    """One CSV line with the reference's rounding (run_privacy.py:329-337)."""
    vals = [float(row["sigma"]), float(row["mask_ratio"])] + [round(float(row[c]), 6) for c in CSV_COLUMNS[2:]]
    return ",".join(str(v) for v in vals) + "\n"


def run_visual_privacy(cfg, log_f, device=None):
    """-> None when the stage is off or skipped, else the CSV row (unrounded) plus "csv"."""
    vp = cfg["visual_privacy"]
    if not vp["enabled"]:
        return None
    if vp["detector"] != "boxes":
        log_line(log_f, "[INFO] visual_privacy needs OpenCV (YuNet face detection + GaussianBlur) and is not part of "
                        "this build -> skip")
        return None
    import numpy as np
    from PIL import Image
    from . import visual_privacy as V
    save_dir = Path(cfg["output"]["save_dir"])
    save_dir.mkdir(parents=True, exist_ok=True)
    seed = int(cfg["runtime"]["seed"])
    blur = V.BoxBlur(vp["blur_kernel"], device or torch.device("cuda"))
    t0 = time.perf_counter()
    out_root = ""
    if vp["frame_root"]:
        frame_root = Path(vp["frame_root"])
        files = V.scan_images(frame_root, vp["max_images"], seed)
        listed = V.read_boxes(vp["boxes_file"])
        rels = [p.relative_to(frame_root).as_posix() for p in files]
        unmatched = len(set(listed) - set(rels))
        log_line(log_f, f"[INFO] Visual privacy: {len(files)} sampled frames from {frame_root}, boxes for "
                        f"{len(set(listed) & set(rels))} of them; {unmatched} listed paths match no sampled frame")
        if vp["overwrite"]:
            out_root = frame_root.parent / (frame_root.name + vp["output_suffix"])

        def batches():
            for i in range(0, len(files), vp["batch_frames"]):
                frames, boxes, names = [], [], []
                for p, rel in zip(files[i:i + vp["batch_frames"]], rels[i:i + vp["batch_frames"]]):
                    try:
                        with Image.open(p) as im:
                            frames.append(np.array(im.convert("RGB")))
                    except OSError:
                        continue                     # unreadable: skipped, as the reference's imread None
                    boxes.append(listed.get(rel, []))
                    names.append(rel)
                if frames:
                    yield frames, boxes, names
    else:
        frame_root = "synthetic"
        frames_all, boxes_all = V.synthetic_frames(min(vp["max_images"], 64), seed)
        log_line(log_f, f"[INFO] Visual privacy: {len(frames_all)} synthetic frames (no frame_root)")

        def batches():
            for i in range(0, len(frames_all), vp["batch_frames"]):
                yield frames_all[i:i + vp["batch_frames"]], boxes_all[i:i + vp["batch_frames"]], None

    stats, sizes, counts, examples = [], [], [], []
    want_pixels = bool(out_root) or vp["save_examples"] > 0
    for frames, boxes, names in batches():
        packed, desc = V.pack_frames(frames)
        blurred, st = blur(packed, desc, boxes, with_stats=True)
        stats.append(st)
        sizes += [f.shape[:2] for f in frames]
        counts += [len(b) for b in boxes]
        if not want_pixels:
            continue
        host = blurred.cpu().numpy()
        for n, (fr, bs) in enumerate(zip(frames, boxes)):
            off, (h, w) = int(desc[n, 0]), fr.shape[:2]
            after = host[off:off + h * w * 3].reshape(h, w, 3)
            if len(examples) < vp["save_examples"] and any(V.clip_box(b, h, w) for b in bs):
                examples.append((fr, after.copy()))
            if out_root:
                dst = Path(out_root) / names[n]
                dst.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(after).save(dst)
        want_pixels = bool(out_root) or len(examples) < vp["save_examples"]
    if not sizes:
        raise RuntimeError("[ERROR] No valid frames read in visual privacy eval.")
    row = V.summarise(torch.cat(stats).cpu().tolist(), sizes, counts)       # the stage's one statistics readback
    row.update({"frame_root": str(frame_root), "blur_kernel": blur.ksize, "seconds": time.perf_counter() - t0,
                "overwrite_saved_root": str(out_root)})
    out_csv = save_dir / "visual_privacy.csv"
    out_csv.write_text(V.CSV_HEADER + V.format_row(row), encoding="utf-8")
    log_line(log_f, f"[INFO] Saved visual privacy CSV: {out_csv}")
    if examples:
        out_img = save_dir / "visual_privacy_examples.jpg"
        Image.fromarray(V.example_grid(examples, cols=4)).save(out_img, quality=92)
        log_line(log_f, f"[INFO] Saved visual examples: {out_img}")
    row["csv"] = out_csv
    return row


def _loader(cfg, device):
    ds, rt = cfg["dataset"], cfg["runtime"]
    if ds["split"]:
        return split_file_loader(ds["split"], clip_len=ds["clip_len"], stride=ds["stride"],
                                 image_size=ds["image_size"], batch_size=rt["batch_size"],
                                 num_workers=rt["num_workers"], device=device)
    return SyntheticBatches(rt["num_batches"], rt["batch_size"], ds["clip_len"], ds["image_size"], device,
                            seed=rt["seed"], num_classes=ds["num_classes"])


@torch.no_grad()
def extract_embeddings(model, loader, cfg):
    """-> (z [N, D], y [N], clean logits [N, C]) on the device (run_privacy.py:264-280)."""
    zs, ys, ls = [], [], []
    for clip, label in loader:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(cfg["runtime"]["amp"])):
            z = P.video_embeddings(model, clip)
        zs.append(z)
        ys.append(label.long())
        ls.append(model.classifier(z))
    return torch.cat(zs), torch.cat(ys), torch.cat(ls)


def run_feature_privacy(model, loader, device, cfg, log_f):
    """-> {"rows", "clean_top1", "clean_entropy", "embed_s", "sweep_s", "csv"}."""
    fp = cfg["feature_privacy"]
    save_dir = Path(cfg["output"]["save_dir"])
    out_csv = save_dir / "feature_privacy.csv"
    if not fp["enabled"]:
        log_line(log_f, "[INFO] feature_privacy disabled -> skip")
        return {"rows": [], "csv": out_csv}
    nc = int(cfg["dataset"]["num_classes"])
    k5 = min(5, nc)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z, y, logits_clean = extract_embeddings(model, loader, cfg)
    _, ent, top1, _ = P.logits_metrics(logits_clean, y, k5)
    clean_top1, clean_ent = top1.item(), ent.item()
    t1 = time.perf_counter()
    log_line(log_f, f"[INFO] Clean embeddings -> Top-1={clean_top1:.4f}, Entropy={clean_ent:.4f}")

    P.route_head(model)                          # model.classifier on the project's GEMM
    cfgs = P.grid_configs(fp["noise_sigmas"], fp["mask_ratios"], int(cfg["runtime"]["seed"]))
    G, (N, D) = len(cfgs), z.shape
    with torch.no_grad():
        z_priv = P.perturb_grid(z, fp["noise_sigmas"], fp["mask_ratios"], int(cfg["runtime"]["seed"]))
        _, g_ent, g_top1, g_top5 = P.logits_metrics(model.classifier(z_priv.view(G * N, D)), y, k5, segments=G)
        atk = []
        for g in range(G):                       # one fresh attacker per configuration, one after another
            attacker = P.FeatureAttacker(D, nc).to(device)
            P.train_attacker(attacker, z_priv[g], y, fp["attacker_epochs"], fp["attacker_lr"])
            atk.append(P.logits_metrics(attacker(z_priv[g]), y, 1)[2])
        util = torch.stack([g_top1, g_top5, g_ent, torch.cat(atk)], dim=1).cpu().tolist()   # the sweep's one readback
    t2 = time.perf_counter()

    rows, lines = [], [CSV_HEADER]
    for (sigma, ratio, _), (t1_, t5_, e_, a_) in zip(cfgs, util):
        row = {"sigma": sigma, "mask_ratio": ratio, "top1": t1_, "top5": t5_, "entropy": e_, "attacker_top1": a_,
               "per_vs_clean": P.privacy_exposure_rate(clean_top1, a_)}
        rows.append(row)
        lines.append(format_row(row))
        log_line(log_f, f"[INFO] sigma={sigma} mask={ratio} | top1={t1_:.4f} top5={t5_:.4f} | attacker={a_:.4f} | "
                        f"ent={e_:.4f}")
    out_csv.write_text("".join(lines), encoding="utf-8")
    log_line(log_f, f"[INFO] Saved feature privacy CSV: {out_csv}")
    log_line(log_f,
             f"[INFO] embedding pass {t1 - t0:.3f} s ({N} clips), sweep {t2 - t1:.3f} s ({G} configurations)")
    return {"rows": rows, "clean_top1": clean_top1, "clean_entropy": clean_ent, "embed_s": t1 - t0,
            "sweep_s": t2 - t1, "csv": out_csv}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Privacy evaluation (feature noise / mask sweep with attacker probe).")
    ap.add_argument("--config", default="configs/privacy.yaml")
    ap.add_argument("--ckpt", default=None, help="override model.finetune_ckpt")
    ap.add_argument("--save_dir", default=None, help="override output.save_dir")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config), args.ckpt, args.save_dir)
    device = start("run_privacy", cfg["runtime"]["seed"])
    save_dir = Path(cfg["output"]["save_dir"])
    save_dir.mkdir(parents=True, exist_ok=True)
    with open(save_dir / "privacy.log", "a", encoding="utf-8") as log_f:
        log_line(log_f, "[INFO] Privacy evaluation started")
        visual = run_visual_privacy(cfg, log_f, device)
        result = {"rows": []}
        if cfg["feature_privacy"]["enabled"]:
            model = build_classifier(cfg, cfg["model"]["finetune_ckpt"], device).eval()
            result = run_feature_privacy(model, _loader(cfg, device), device, cfg, log_f)
        result["visual"] = visual
        log_line(log_f, "[INFO] Privacy evaluation finished.")
    return result


if __name__ == "__main__":
    main()

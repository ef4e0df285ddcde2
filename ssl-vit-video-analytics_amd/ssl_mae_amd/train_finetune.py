"""Supervised fine-tuning of finetune.VideoClassifier (the reference's src/train_finetune.py),
MI355X-native: the stage between SSL pre-training and the evaluation drivers.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.train_finetune --config configs/finetune.yaml \
        [--mode ft_random|linear_probe|ft_ssl|two_stage] [--pretrained_ssl PATH] [--epochs N] [--batch_size B] \
        [--save_dir DIR] [--optimizer fused|torch]

Flow (train_finetune.py:213-353): loaders -> model -> the mode's SSL load and freeze rule
(:280-313) -> optimizer -> per epoch: the two_stage unfreeze at epoch stage1_epochs + 1 (fresh
optimizer state), one training pass, one validation pass, a checkpoint whenever validation top-1
improves.  Outputs: `{log_dir}/finetune_{mode}.log`, `{save_dir}/{mode}/finetune_epoch_{E}_top1_
{acc:.4f}.pth` (model.state_dict(), what finetune.load_finetune_ckpt reads) and
`{save_dir}/{mode}/finetune_summary.csv`.

The step: bf16 autocast when `training.amp`, the cross-entropy through sm_logits_metrics
(finetune.TopCEFn, driver.train_pass), optim.GroupedAdamW over finetune.param_groups (one sm_adamw_table launch
for every parameter group; the non-finite skip happens inside it, so optim.GradScaler is the
shim).  `optimizer.type: adamw_torch` keeps torch.optim.AdamW over the same groups.  The running
loss stays on the device: one read-back per log_interval and one per epoch.  Without
`dataset.train_split` the driver runs on labelled synthetic clips (driver.SyntheticClips).

`augment.enabled` (off by default; the reference has no augmentation) gives every training clip a
random-resized crop and a horizontal flip, the same for all its frames and fresh in every epoch
(mae_loader.RandomResizedCropFlip, seeded from runtime.seed): the window goes into the
descriptor of the one resize launch (sm_frames_crop_resize_normalize), so it costs no pixel work
on the host.  The validation loader is never augmented.

`mix.enabled` (off by default) mixes every training batch with its own flip, clip b with clip
B-1-b: Mixup or CutMix per pair, the CutMix box the same on every frame of the clip
(mae_loader.ClipMixer, seeded from runtime.seed; one small upload and one sm_clip_mix launch per
step, on synthetic clips too).  `training.label_smoothing` smooths the target.  With either, the
loss is the soft cross-entropy of sm_soft_ce (finetune.SoftCEFn) and `train_loss` in the CSV is
that soft loss, not the hard-label cross-entropy.  Validation is never mixed or smoothed.
"""
import argparse
import functools
import os
import time
from pathlib import Path

import torch

from . import driver
from .finetune import epoch_lr_mult, load_pretrained_ssl, param_groups, resolve_mode, set_requires_grad
from .optim import GradScaler, GroupedAdamW
from .utils import load_config, log_line, write_csv

SUMMARY_COLUMNS = ("epoch", "train_loss", "val_top1", "val_topk", "lr", "seconds")
OPTIMIZERS = {"adamw": "fused", "adamw_torch": "torch"}
SSL_MODES = ("linear_probe", "ft_ssl", "two_stage")

DEFAULTS = {
    "experiment": {"mode": "ft_random"},
    "dataset": {"name": None, "train_split": None, "val_split": None, "num_classes": 101, "clip_len": 16,
                "stride": 4, "image_size": 112},
    "training": {"epochs": 30, "batch_size": 64, "learning_rate": 1e-4, "weight_decay": 0.01, "log_interval": 20,
                 "amp": True, "stage1_epochs": 0, "head_lr": 1e-3, "backbone_lr": 1e-4, "layer_decay": 1.0,
                 "no_decay_1d": False, "schedule": "constant", "warmup_epochs": 0, "min_lr": 0.0,
                 "label_smoothing": 0.0},
    "model": {"embed_dim": 576, "pretrained_ssl": None, "freeze_backbone": False},
    "optimizer": {"type": "adamw"},
    "evaluation": {"topk": [1, 5]},
    "augment": {"enabled": False, "scale": [0.35, 1.0], "ratio": [0.75, 1.3333], "flip": 0.5},
    "mix": {"enabled": False, "mixup_alpha": 0.8, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5},
    "synthetic": {"num_train": 96, "num_val": 32},
    "runtime": {"seed": 42, "num_workers": 4},
    "paths": {"save_dir": "results/finetune", "log_dir": "results/logs"},
}


def resolve_config(cfg, mode=None, pretrained_ssl=None, epochs=None, batch_size=None, save_dir=None,
                   optimizer=None):
    """The file's values over DEFAULTS, the command line over both; unknown sections or keys
    raise, and so do an unknown mode, two_stage without stage1_epochs, an SSL mode whose
    checkpoint is missing (train_finetune.py:198-210, :284-286, :306-307), an `augment` section
    out of range or enabled without a training split, and `training.label_smoothing` or a `mix`
    value out of range."""
    out = driver.merge_config(DEFAULTS, cfg)
    tr = out["training"]
    out["experiment"]["mode"] = resolve_mode(out, mode)
    if pretrained_ssl is not None:
        out["model"]["pretrained_ssl"] = pretrained_ssl
    if epochs is not None:
        tr["epochs"] = int(epochs)
    if batch_size is not None:
        tr["batch_size"] = int(batch_size)
    if save_dir is not None:
        out["paths"]["save_dir"] = save_dir
    if optimizer is not None:
        by_cli = {v: k for k, v in OPTIMIZERS.items()}
        if optimizer not in by_cli:
            raise ValueError(f"[ERROR] Unknown --optimizer {optimizer}, must be one of {sorted(by_cli)}")
        out["optimizer"]["type"] = by_cli[optimizer]
    if out["optimizer"]["type"] not in OPTIMIZERS:
        raise ValueError(f"[ERROR] Unknown optimizer.type: {out['optimizer']['type']}, must be one of "
                         f"{sorted(OPTIMIZERS)}")
    if tr["schedule"] not in ("constant", "cosine"):
        raise ValueError(f"[ERROR] Unknown training.schedule={tr['schedule']}, must be constant or cosine")
    if int(tr["epochs"]) < 0 or int(tr["batch_size"]) < 1 or int(tr["log_interval"]) < 1 \
            or int(tr["warmup_epochs"]) < 0 or not 0.0 < float(tr["layer_decay"]) <= 1.0:
        raise ValueError("[ERROR] training: epochs, warmup_epochs >= 0; batch_size, log_interval >= 1; "
                         "0 < layer_decay <= 1")
    out["evaluation"]["topk"] = [int(k) for k in out["evaluation"]["topk"]]
    if not out["evaluation"]["topk"] or min(out["evaluation"]["topk"]) < 1:
        raise ValueError("[ERROR] evaluation.topk needs at least one entry; k >= 1")
    mode = out["experiment"]["mode"]
    if mode == "two_stage" and int(tr["stage1_epochs"]) <= 0:
        raise ValueError("[ERROR] two_stage requires training.stage1_epochs > 0")
    ssl = out["model"]["pretrained_ssl"]
    if mode in SSL_MODES and (ssl is None or not os.path.isfile(ssl)):
        raise RuntimeError("[ERROR] SSL mode selected but pretrained_ssl checkpoint not found!")
    if out["dataset"]["train_split"] and not out["dataset"]["val_split"]:
        raise ValueError("[ERROR] dataset.val_split is needed with dataset.train_split")
    aug = out["augment"]
    for key in ("scale", "ratio"):
        if not isinstance(aug[key], (list, tuple)) or len(aug[key]) != 2:
            raise ValueError(f"[ERROR] augment.{key}={aug[key]}: needs a [low, high] pair")
    if not 0.0 < float(aug["scale"][0]) <= float(aug["scale"][1]) <= 1.0:
        raise ValueError(f"[ERROR] augment.scale={aug['scale']}: needs 0 < scale[0] <= scale[1] <= 1")
    if not 0.0 < float(aug["ratio"][0]) <= float(aug["ratio"][1]):
        raise ValueError(f"[ERROR] augment.ratio={aug['ratio']}: needs 0 < ratio[0] <= ratio[1]")
    if not 0.0 <= float(aug["flip"]) <= 1.0:
        raise ValueError(f"[ERROR] augment.flip={aug['flip']}: must lie in [0, 1]")
    if aug["enabled"] and not out["dataset"]["train_split"]:
        raise ValueError("[ERROR] augment.enabled needs dataset.train_split: the synthetic clips are drawn on the "
                         "device at image_size and have no source frames to crop")
    if not 0.0 <= float(tr["label_smoothing"]) < 1.0:
        raise ValueError(f"[ERROR] training.label_smoothing={tr['label_smoothing']}: must lie in [0, 1)")
    mix = out["mix"]
    for key in ("mixup_alpha", "cutmix_alpha"):
        if not float(mix[key]) >= 0.0:
            raise ValueError(f"[ERROR] mix.{key}={mix[key]}: must be >= 0")
    if mix["enabled"] and float(mix["mixup_alpha"]) == 0.0 and float(mix["cutmix_alpha"]) == 0.0:
        raise ValueError("[ERROR] mix.enabled needs mixup_alpha > 0 or cutmix_alpha > 0")
    for key in ("prob", "switch_prob"):
        if not 0.0 <= float(mix[key]) <= 1.0:
            raise ValueError(f"[ERROR] mix.{key}={mix[key]}: must lie in [0, 1]")
    return out


def build_mixer(cfg):
    """The training batches' mae_loader.ClipMixer, seeded from runtime.seed; None when `mix` is off."""
    mix = cfg["mix"]
    if not mix["enabled"]:
        return None
    from .mae_loader import ClipMixer
    return ClipMixer(mix["mixup_alpha"], mix["cutmix_alpha"], mix["prob"], mix["switch_prob"],
                     seed=int(cfg["runtime"]["seed"]))


def freeze_rule(cfg):
    """train_finetune.py:288-307 -> (backbone frozen at the start, two-stage schedule)."""
    mode = cfg["experiment"]["mode"]
    if mode == "linear_probe":
        return True, False
    if mode == "two_stage":
        return True, True
    return False, False      # ft_ssl, ft_random: the mode overrides model.freeze_backbone


def build_optimizer(cfg, model):
    """GroupedAdamW (`optimizer.type: adamw`) or torch.optim.AdamW (`adamw_torch`) over
    finetune.param_groups."""
    groups = param_groups(model, cfg, cfg["experiment"]["mode"])
    if OPTIMIZERS[cfg["optimizer"]["type"]] == "fused":
        return GroupedAdamW(groups)
    return torch.optim.AdamW([{k: v for k, v in g.items() if k != "names"} for g in groups])


def set_lr_mult(optimizer, base_lrs, mult):
    """The epoch's schedule multiplier: an attribute of GroupedAdamW (no table rebuild, no
    upload), the groups' lr for a torch optimizer."""
    if isinstance(optimizer, GroupedAdamW):
        optimizer.lr_mult = float(mult)
    else:
        for g, base in zip(optimizer.param_groups, base_lrs):
            g["lr"] = base * float(mult)


def train_one_epoch(model, loader, optimizer, scaler, device, cfg, log, step_hook=None, mixer=None, mix_hook=None):
    """train_finetune.py:84-124 as driver.train_pass, the loss sum kept on the device; returns the
    average loss over the steps (the soft loss with `mixer` or training.label_smoothing).
    `mix_hook(step, info)` gets every step's {"labels_b", "lam", "draws"}."""
    model.train()
    tr = cfg["training"]
    t0 = time.time()
    n = len(loader) if hasattr(loader, "__len__") else "?"

    def on_step(step, loss, logits, label):
        if step_hook is not None:
            step_hook(step, logits, label)
        if (step + 1) % int(tr["log_interval"]) == 0:
            log(f"[INFO] step={step + 1}/{n} loss={loss.item():.4f}")

    sums = torch.zeros(2, dtype=torch.float64, device=device)     # (loss, loss * batch)
    def on_mix(step, labels_b, lam):
        mix_hook(step, {"labels_b": labels_b, "lam": lam, "draws": mixer.last})

    steps, _ = driver.train_pass(model, loader, optimizer, device, tr["amp"], sums, scaler, on_step, mixer=mixer,
                                 label_smoothing=float(tr["label_smoothing"]),
                                 on_mix=on_mix if mixer is not None and mix_hook is not None else None)
    avg_loss = float(sums[0].item()) / max(1, steps)
    log(f"[INFO] Epoch train finished, avg_loss={avg_loss:.4f}, time={time.time() - t0:.1f}s")
    return avg_loss


def evaluate(model, loader, device, topk, log, split="val"):
    """train_finetune.py:127-153 -> {k: accuracy} for k = 1 and every k of `topk`
    (driver.evaluate) and the pass's log line."""
    acc = driver.evaluate(model, loader, device, topk)
    log(f"[INFO] {split} results: " + ", ".join(f"Top-{k}: {acc[k]:.4f}" for k in topk))
    return acc


def save_checkpoint(model, epoch, acc1, save_dir, log):
    """train_finetune.py:156-161."""
    path = Path(save_dir) / f"finetune_epoch_{epoch}_top1_{acc1:.4f}.pth"
    torch.save(model.state_dict(), path)
    log(f"[INFO] Saved checkpoint: {path}")
    return path


def build_loaders(cfg, device):
    """(training loader: shuffled, drop_last, augmented when `augment.enabled`; validation loader,
    seed + 999, never augmented)."""
    ds, tr, seed = cfg["dataset"], cfg["training"], int(cfg["runtime"]["seed"])
    bs = int(tr["batch_size"])
    if ds["train_split"]:
        def of(split, shuffle, s, **kw):
            return driver.split_file_loader(str(split), clip_len=ds["clip_len"], stride=ds["stride"],
                                            image_size=ds["image_size"], batch_size=bs,
                                            num_workers=cfg["runtime"]["num_workers"], device=device,
                                            shuffle=shuffle, drop_last=shuffle, seed=s, **kw)

        aug, kw = cfg["augment"], {}
        if aug["enabled"]:
            from .mae_loader import RandomResizedCropFlip
            kw["augment"] = RandomResizedCropFlip(aug["scale"], aug["ratio"], aug["flip"], seed=seed)
        return of(ds["train_split"], True, seed, **kw), of(ds["val_split"], False, seed + 999)
    train_set = driver.SyntheticClips(cfg, int(cfg["synthetic"]["num_train"]), seed, device)
    val_set = driver.SyntheticClips(cfg, int(cfg["synthetic"]["num_val"]), seed + 999, device)
    return train_set.loader(train_set.items(), bs, True, seed), val_set.loader(val_set.items(), bs, False, seed + 999)


def main(argv=None, hooks=None):
    """`hooks` (tests, measurement scripts): {"step": f(epoch, step, logits, label), "epoch":
    f(epoch, model, optimizer), "mix": f(epoch, step, info)}, called after every optimizer step / at
    the end of every epoch / after every batch's mix with info = {"labels_b", "lam", "draws"}: the
    partner labels and the labels' weights on the device, and ClipMixer.last."""
    ap = argparse.ArgumentParser(description="Fine-tune VideoClassifier: ft_random, linear_probe, ft_ssl, two_stage.")
    ap.add_argument("--config", default="configs/finetune.yaml")
    ap.add_argument("--mode", default=None, help="override experiment.mode (ft_random|linear_probe|ft_ssl|two_stage)")
    ap.add_argument("--pretrained_ssl", default=None, help="override model.pretrained_ssl")
    ap.add_argument("--epochs", type=int, default=None, help="override training.epochs")
    ap.add_argument("--batch_size", type=int, default=None, help="override training.batch_size")
    ap.add_argument("--save_dir", default=None, help="override paths.save_dir")
    ap.add_argument("--optimizer", default=None, help="override optimizer.type (fused|torch)")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config), args.mode, args.pretrained_ssl, args.epochs, args.batch_size,
                         args.save_dir, args.optimizer)
    hooks = hooks or {}
    mode, tr = cfg["experiment"]["mode"], cfg["training"]
    device = driver.start("train_finetune", cfg["runtime"]["seed"])
    print(f"[INFO] Using device: {device}")
    print(f"[INFO] Finetune mode: {mode}")

    log_dir = Path(cfg["paths"]["log_dir"])
    log_dir.mkdir(parents=True, exist_ok=True)
    save_dir = Path(cfg["paths"]["save_dir"]) / mode
    save_dir.mkdir(parents=True, exist_ok=True)
    train_loader, val_loader = build_loaders(cfg, device)
    if cfg["augment"]["enabled"]:
        aug = cfg["augment"]
        print(f"[INFO] Augmentation: clip-consistent random-resized crop scale={list(aug['scale'])} "
              f"ratio={list(aug['ratio'])}, flip p={aug['flip']} (training split only, seed {cfg['runtime']['seed']})")

    mixer = build_mixer(cfg)

    def load_for_mode(model, ssl):
        if mode == "ft_random":
            print("[INFO] ft_random: skip SSL loading (random init)")
        elif not load_pretrained_ssl(model, ssl):
            raise RuntimeError("[ERROR] SSL mode selected but pretrained_ssl checkpoint not found!")

    model = driver.build_classifier(cfg, cfg["model"]["pretrained_ssl"], device, load=load_for_mode)
    frozen, two_stage = freeze_rule(cfg)
    set_requires_grad(model.backbone, not frozen)
    if frozen:
        print("[INFO] Backbone frozen")

    optimizer = build_optimizer(cfg, model)
    base_lrs = [g["lr"] for g in optimizer.param_groups]
    scaler = GradScaler(enabled=bool(tr["amp"]))
    epochs, stage1 = int(tr["epochs"]), int(tr["stage1_epochs"])
    topk = tuple(cfg["evaluation"]["topk"])
    k_max = max(topk)
    print(f"[INFO] Start finetuning for {epochs} epochs, save_dir={save_dir}")

    rows, ckpts = [], []
    with open(log_dir / f"finetune_{mode}.log", "a", encoding="utf-8") as log_f:
        log = functools.partial(log_line, log_f)
        if mixer is not None:
            mix = cfg["mix"]
            log(f"[INFO] Mixing: clip-consistent Mixup alpha={mix['mixup_alpha']} / CutMix alpha={mix['cutmix_alpha']} "
                f"of clip b with clip B-1-b, p={mix['prob']}, CutMix share {mix['switch_prob']}, label smoothing "
                f"{tr['label_smoothing']} (training batches only, seed {cfg['runtime']['seed']})")
        best_top1 = -1.0      # the first validated epoch always leaves a checkpoint
        for epoch in range(1, epochs + 1):
            if two_stage and epoch == stage1 + 1:
                log("[INFO] two_stage: unfreeze backbone and rebuild optimizer")
                set_requires_grad(model.backbone, True)
                optimizer = build_optimizer(cfg, model)
                base_lrs = [g["lr"] for g in optimizer.param_groups]
            log(f"[INFO] Epoch {epoch}/{epochs} started")
            mult = epoch_lr_mult(epoch - 1, cfg)
            set_lr_mult(optimizer, base_lrs, mult)
            t0 = time.time()
            step_hook, mix_hook = hooks.get("step"), hooks.get("mix")
            avg_loss = train_one_epoch(model, train_loader, optimizer, scaler, device, cfg, log,
                                       (lambda s, lg, y, _e=epoch: step_hook(_e, s, lg, y)) if step_hook else None,
                                       mixer, (lambda s, info, _e=epoch: mix_hook(_e, s, info)) if mix_hook else None)
            acc = evaluate(model, val_loader, device, topk, log, split="val")
            rows.append({"epoch": epoch, "train_loss": round(avg_loss, 6), "val_top1": round(acc[1], 6),
                         "val_topk": round(acc[k_max], 6), "lr": round(max(base_lrs) * mult, 6) if base_lrs else 0.0,
                         "seconds": round(time.time() - t0, 6)})
            if acc[1] > best_top1:
                best_top1 = acc[1]
                ckpts.append(save_checkpoint(model, epoch, best_top1, save_dir, log))
            if "epoch" in hooks:
                hooks["epoch"](epoch, model, optimizer)
        summary = save_dir / "finetune_summary.csv"
        write_csv(summary, SUMMARY_COLUMNS, rows)
        log(f"[INFO] Saved finetune summary: {summary}")
    return {"rows": rows, "checkpoints": ckpts, "model": model, "optimizer": optimizer, "save_dir": save_dir,
            "config": cfg}


if __name__ == "__main__":
    main()

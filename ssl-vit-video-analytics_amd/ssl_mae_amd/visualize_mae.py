"""MAE reconstruction evaluation and visualiser (reference: src/visualize_mae.py and the mask /
token-error maps of src/mae/visualize.py:10-84), MI355X-native.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.visualize_mae \
        --config configs/ssl_mae.yaml --ckpt results/tinymae_v1/last_state.pth \
        --frames data/UCF101_frames/ApplyEyeMakeup/v_ApplyEyeMakeup_g01_c01 --out visual_results

`visualize(checkpoint_path, video_path, output_path)` keeps the reference's positional signature
and its `frame_{i:02d}.png` strips [ original | masked input | reconstruction ].  What differs
from the reference, which cannot run as written:

  * its `unpatchify_auto` einsum 'bthwpqc->bcthpw' drops q; the inverse of patchify is
    'bthwpqc->bcthpwq', and here no token tensor is un-patchified at all: sm_mae_reconstruct reads
    pred, clip and mask once and writes the byte strips, the display-space reconstruction and the
    per-token errors in one launch (include/sm_api.h);
  * it hard-codes 16 frames of 112^2; clip length and image size come from the config;
  * it de-normalises a `norm_pix_loss` prediction with the ImageNet constants alone; a model
    trained on per-patch normalised targets predicts (x - mu) / sqrt(var + 1e-6) of each patch, so
    the reconstruction is pred * sqrt(var + 1e-6) + mu with the patch's own statistics first;
  * the frames take the project's input path (ClipNormalizer: /255, ImageNet mean / std, BGR swap),
    so the clip is what the model was trained on, and the display undoes the swap;
  * the checkpoint is read with weights_only=True.

Next to the strips it scores the reconstruction: `reconstruction.csv` (one row per clip: masked
loss, pixel MSE and PSNR in display space), `token_err.npy`, and, when matplotlib imports, the
mask grid and the token-error heat map (T rows, L columns).
"""
import argparse
import warnings
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher
from .mae_loader import IMAGENET_MEAN, IMAGENET_STD, ClipNormalizer, get_tube_mask
from .utils import load_config

CSV_COLUMNS = ("clip", "mask_ratio", "n_masked", "loss_norm", "mse_pix", "psnr_db")
CSV_HEADER = ",".join(CSV_COLUMNS) + "\n"
FORMATS = ("training_state", "state_dict", "encoder")


def reconstruct(model, clip, mask, norm_pix=True, paste_visible=True, bgr_swap=True, mean=IMAGENET_MEAN,
                std=IMAGENET_STD, bf16=True):
    """clip fp32 [B,3,T,H,W] (device), mask bool / uint8 [B,T,L] (True = masked) -> an object with
    panels uint8 [B,T,H,3W,3], recon fp32 [B,3,T,H,W] (display space, RGB, not clamped), token_err
    fp32 [B,T,L,2] (normalised-target MSE, display-space pixel MSE), clip_metrics fp32 [B,4]
    (masked-mean loss, masked-mean pixel MSE, PSNR dB, n_masked), pred, and mask, the uint8 [B,T,L]
    mask the kernels read."""
    B, _, T, H, W = clip.shape
    L = (H // 8) * (W // 8)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(bf16)):
            pred = model(clip, mask)
    finally:
        model.train(was_training)
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
    pred = pred.contiguous()
    m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else mask.to(torch.uint8)
    m8 = m8.to(pred.device).reshape(B, T, L).contiguous()
    panels, recon, token_err = K.mae_reconstruct(pred, clip, m8, mean, std, norm_pix, paste_visible, bgr_swap)
    clip_metrics = K.recon_clip_metrics(token_err, m8)
    return SimpleNamespace(panels=panels, recon=recon, token_err=token_err.view(B, T, L, 2),
                           clip_metrics=clip_metrics, pred=pred, mask=m8)


def load_mae_checkpoint(model, path):
    """Load `path` into a TinyVideoMAE and return which format it held: "training_state" (a
    save_training_state file, key "model"), "state_dict" (a bare full state dict) or "encoder" (an
    encoder-only encoder_ep{N}.pth, loaded into model.encoder; the decoder stays as initialised)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("model"), dict):
        fmt, state = "training_state", ckpt["model"]
    else:
        fmt, state = "state_dict", ckpt
    if not isinstance(state, dict) or not state:
        raise ValueError(f"[ERROR] {path} holds no state dict")
    if any("decoder" in k for k in state):
        model.load_state_dict(state, strict=True)
        return fmt
    warnings.warn(f"[WARNING] {path} seems to hold the encoder only! MAE reconstruction needs the decoder "
                  "weights; continuing with an untrained decoder, so the result may be garbage.")
    model.encoder.load_state_dict(state, strict=True)
    return "encoder"


def list_frames(video_path):
    """The sorted *.jpg / *.png files of a frame directory (visualize_mae.py:119-121)."""
    p = Path(video_path)
    if not p.is_dir():
        raise RuntimeError(f"[ERROR] invalid frame directory: {video_path}")
    return sorted(f for f in p.glob("*") if f.suffix.lower() in (".jpg", ".png"))


def load_frames(files, image_size):
    """-> uint8 [T,S,S,3] decoded RGB, resized as the reference does (PIL's default filter)."""
    from PIL import Image
    return torch.from_numpy(np.stack([
        np.asarray(Image.open(f).convert("RGB").resize((image_size, image_size)), dtype=np.uint8) for f in files]))


def _psnr_mean(psnr):
    finite = [p for p in psnr if np.isfinite(p)]
    return float(np.mean(finite)) if finite else float("inf")


def evaluate_reconstruction(model, clips, mask_ratios=(0.5, 0.75, 0.9), seed=0, norm_pix=True, batch_size=16):
    """The clip metrics averaged over `clips` (fp32 [N,3,T,H,W] on the device) for each mask ratio:
    a list of {"mask_ratio", "n_masked", "loss_norm", "mse_pix", "psnr_db"} (psnr_db: the mean of
    the clips' finite PSNRs).  The tube masks are drawn from a generator seeded with `seed`; the
    global stream is left as it was."""
    N, _, T, H, W = clips.shape
    L = (H // 8) * (W // 8)
    rows = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(int(seed))
        for ratio in mask_ratios:
            cms = []
            for i in range(0, N, batch_size):
                chunk = clips[i:i + batch_size]
                mask = get_tube_mask(chunk.shape[0], T, L, float(ratio), device=clips.device)
                cms.append(reconstruct(model, chunk, mask, norm_pix=norm_pix).clip_metrics)
            cm = torch.cat(cms).double().cpu().numpy()
            rows.append({"mask_ratio": float(ratio), "n_masked": float(cm[:, 3].mean()),
                         "loss_norm": float(cm[:, 0].mean()), "mse_pix": float(cm[:, 1].mean()),
                         "psnr_db": _psnr_mean(cm[:, 2])})
    return rows


def format_row(clip, mask_ratio, n_masked, loss_norm, mse_pix, psnr_db):
    """One CSV line; the floats are written with repr, so they read back exactly."""
    n = int(n_masked) if float(n_masked).is_integer() else float(n_masked)
    return f"{clip},{float(mask_ratio)!r},{n},{float(loss_norm)!r},{float(mse_pix)!r},{float(psnr_db)!r}\n"


def save_maps(mask_grid, err_grid, out_dir, mask_ratio):
    """The mask grid and the masked-token error heat map of src/mae/visualize.py:63-81, T rows and
    L columns; returns the two paths, or None when matplotlib does not import."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return None
    paths = []
    for name, grid, title in (("mask_grid.png", mask_grid, f"mask grid mode=tube ratio={mask_ratio:.2f}"),
                              ("token_err.png", err_grid, "masked token error (visible=0)")):
        plt.figure()
        plt.imshow(grid, aspect="auto")
        plt.title(title)
        plt.xlabel("spatial token")
        plt.ylabel("time")
        paths.append(Path(out_dir) / name)
        plt.savefig(paths[-1], dpi=150, bbox_inches="tight")
        plt.close()
    return paths


@torch.no_grad()
def visualize(checkpoint_path, video_path, output_path="visual_results", config="configs/ssl_mae.yaml",
              mask_ratio=0.9, clips=1, sweep=False):
    """Reconstruct `clips` clips of `clip_len` consecutive frames from the sorted *.jpg / *.png
    files of `video_path` (synthetic clips when it is None) with the checkpoint's model and write
    the strips of the first clip, reconstruction.csv, token_err.npy and the two maps into
    `output_path`.  `config` is a yaml path or a loaded dict; `checkpoint_path` None keeps the
    initial weights.  Returns the reconstruct() object, with `format`, `rows` and `out_dir` added."""
    from .train_ssl_mae import build_model
    if not torch.cuda.is_available():
        raise RuntimeError("[ERROR] visualize_mae needs an MI355X: the HIP kernels have no CPU fallback")
    cfg = config if isinstance(config, dict) else load_config(config)
    device = torch.device("cuda")
    out_dir = Path(output_path)
    out_dir.mkdir(parents=True, exist_ok=True)
    T, S = int(cfg["dataset"]["clip_len"]), int(cfg["dataset"]["image_size"])
    L = (S // 8) * (S // 8)
    clips = int(clips)
    if clips < 1:
        raise ValueError("[ERROR] clips >= 1")

    model = build_model(cfg, "cpu")
    fmt = None
    if checkpoint_path is not None:
        if not Path(checkpoint_path).exists():
            raise RuntimeError(f"[ERROR] checkpoint not found: {checkpoint_path}")
        fmt = load_mae_checkpoint(model, checkpoint_path)
        print(f"[INFO] checkpoint {checkpoint_path}: {fmt}")
    else:
        print("[WARNING] no checkpoint: the model keeps its initial weights")
    model.to(device).eval()

    if video_path is not None:
        files = list_frames(video_path)
        if len(files) < T:
            raise RuntimeError(f"[ERROR] {len(files)} frames in {video_path}, a clip needs {T}")
        clips = min(clips, len(files) // T)
        frames = torch.stack([load_frames(files[i * T:(i + 1) * T], S) for i in range(clips)])
        clip = ClipNormalizer(device=device)(frames)
    else:
        from .init_rule import synthetic_clip
        clip = torch.from_numpy(synthetic_clip(clips, T, S)).to(device)
    mask = get_tube_mask(clips, T, L, float(mask_ratio), device=device)
    rec = reconstruct(model, clip, mask, norm_pix=bool(cfg.get("ssl", {}).get("norm_pix_loss", True)))

    from PIL import Image
    strips = rec.panels[0].cpu().numpy()
    for i in range(T):
        Image.fromarray(strips[i]).save(out_dir / f"frame_{i:02d}.png")
    cm = rec.clip_metrics.cpu().numpy()
    lines = [CSV_HEADER] + [format_row(b, mask_ratio, *cm[b, [3, 0, 1, 2]]) for b in range(clips)]
    rows = []
    if sweep:
        rows = evaluate_reconstruction(model, clip, norm_pix=bool(cfg.get("ssl", {}).get("norm_pix_loss", True)))
        lines += [format_row("mean", r["mask_ratio"], r["n_masked"], r["loss_norm"], r["mse_pix"], r["psnr_db"])
                  for r in rows]
    (out_dir / "reconstruction.csv").write_text("".join(lines), encoding="utf-8")
    m = rec.mask.cpu().numpy().astype(np.float32)
    err = rec.token_err[..., 0].cpu().numpy() * m                      # visible tokens 0
    np.save(out_dir / "token_err.npy", err)
    save_maps(m[0], err[0], out_dir, float(mask_ratio))
    print(f"[SUCCESS] {T} strips [ original | masked input ({mask_ratio:.0%}) | reconstruction ] and "
          f"reconstruction.csv written to {out_dir}")
    rec.format, rec.rows, rec.out_dir = fmt, rows, out_dir
    return rec


def build_parser():
    ap = argparse.ArgumentParser(description="MAE reconstruction strips and scores for a checkpoint.")
    ap.add_argument("--config", default="configs/ssl_mae.yaml")
    ap.add_argument("--ckpt", default=None, help="training-state file, full state dict or encoder_ep{N}.pth")
    ap.add_argument("--frames", default=None, help="directory of *.jpg / *.png frames (default: synthetic clips)")
    ap.add_argument("--out", default="visual_results")
    ap.add_argument("--mask_ratio", type=float, default=0.9)
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--sweep", action="store_true", help="add the mask-ratio sweep (0.5, 0.75, 0.9) to the CSV")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .build import build
    build()
    return visualize(args.ckpt, args.frames, args.out, config=args.config, mask_ratio=args.mask_ratio,
                     clips=args.clips, sweep=args.sweep)


if __name__ == "__main__":
    main()

"""Wall time of the feature-privacy sweep next to the embedding pass that feeds it, on
ssl_mae_amd.run_privacy's synthetic default (configs/privacy.yaml: 96 clips of 16 frames at
112^2, 101 classes, 4 sigmas x 3 mask ratios = 12 configurations, 10 attacker epochs), and the
same sweep written in plain torch on the same device for comparison.

    PYTHONPATH=ssl-vit-video-analytics_amd python scripts/privacy_sweep_bench.py [--runs 4]

Every figure is a host clock around work that ends in a device synchronise.  Run 0 of each
variant includes first-launch costs (code-object loading, rocBLAS algorithm selection); the
later runs are steady state.  The two sweeps draw different random numbers (counter-based
against torch's generator), so only their times are compared here; tests/test_privacy_gpu.py
pins the values.
"""
import argparse
import contextlib
import io
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ssl-vit-video-analytics_amd"))


def torch_sweep(head_w, head_b, z, y, sigmas, ratios, epochs, lr, nc):
    """The sweep in eager torch: per configuration perturb, head, top-1 / top-5 / entropy, then a
    fresh two-layer attacker trained full-batch with torch.optim.Adam."""
    rows = []
    k5 = min(5, nc)
    for sigma in sigmas:
        for ratio in ratios:
            zp = z + sigma * torch.randn_like(z) if sigma > 0 else z
            if ratio > 0:
                zp = zp * torch.bernoulli(torch.full_like(zp, 1.0 - ratio))
            with torch.no_grad():
                logits = F.linear(zp, head_w, head_b)
                top1 = (logits.argmax(1) == y).float().mean()
                top5 = (logits.topk(k5, dim=1).indices == y[:, None]).any(1).float().mean()
                p = logits.softmax(1)
                ent = -(p * (p + 1e-12).log()).sum(1).mean()
            net = nn.Sequential(nn.Linear(z.shape[1], z.shape[1]), nn.ReLU(), nn.Linear(z.shape[1], nc)).to(z.device)
            opt = torch.optim.Adam(net.parameters(), lr=lr)
            for _ in range(epochs):
                opt.zero_grad()
                F.cross_entropy(net(zp), y).backward()
                opt.step()
            with torch.no_grad():
                atk = (net(zp).argmax(1) == y).float().mean()
            rows.append(torch.stack([top1, top5, ent, atk]))
    return torch.stack(rows).cpu()           # one readback, as the HIP sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    args = ap.parse_args()
    from ssl_mae_amd import run_privacy as RP
    from ssl_mae_amd.build import build
    from ssl_mae_amd.finetune import VideoClassifier, load_finetune_ckpt
    from ssl_mae_amd.utils import load_config, set_seed
    if not torch.cuda.is_available():
        raise RuntimeError("privacy_sweep_bench needs an MI355X")
    build()
    cfg = RP.resolve_config(load_config(os.path.join(ROOT, "configs", "privacy.yaml")), save_dir="bench_out/privacy_sweep")
    os.makedirs(cfg["output"]["save_dir"], exist_ok=True)
    set_seed(cfg["runtime"]["seed"])
    device = torch.device("cuda")
    nc = int(cfg["dataset"]["num_classes"])
    model = VideoClassifier(nc, embed_dim=int(cfg["model"]["embed_dim"]), img_size=int(cfg["dataset"]["image_size"]))
    load_finetune_ckpt(model, None)
    model.to(device).eval()
    loader = RP._loader(cfg, device)
    fp = cfg["feature_privacy"]
    print(f"device: {torch.cuda.get_device_name(0)}; {len(loader.batches)} batches of {loader.batch_size} clips, "
          f"T={cfg['dataset']['clip_len']}, {cfg['dataset']['image_size']}^2, amp={cfg['runtime']['amp']}; "
          f"{len(fp['noise_sigmas']) * len(fp['mask_ratios'])} configurations, {fp['attacker_epochs']} attacker epochs")
    print("run  embedding_pass_s  hip_sweep_s  torch_sweep_s  hip_sweep/embedding  torch_sweep/hip_sweep")
    for run in range(args.runs):
        with contextlib.redirect_stdout(io.StringIO()):
            res = RP.run_feature_privacy(model, loader, device, cfg, io.StringIO())
        with torch.no_grad():
            z, y, _ = RP.extract_embeddings(model, loader, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_sweep(model.classifier.weight.detach(), model.classifier.bias.detach(), z, y, fp["noise_sigmas"],
                    fp["mask_ratios"], fp["attacker_epochs"], fp["attacker_lr"], nc)
        torch.cuda.synchronize()
        tt = time.perf_counter() - t0
        print(f"{run:3d}  {res['embed_s']:16.4f}  {res['sweep_s']:11.4f}  {tt:13.4f}  {res['sweep_s'] / res['embed_s']:19.3f}  "
              f"{tt / res['sweep_s']:21.2f}")


if __name__ == "__main__":
    main()

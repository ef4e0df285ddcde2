"""Time of the temporal-SSL step (ssl_mae_amd.temporal_ssl) at the default config
(configs/ssl_train.yaml: TinyViT encoder, 576-d, 4 temporal layers of 9 heads, mask ratio 0.75,
TOP every 2nd step on half the batch) with B = 48 clips of T = 16 frames at 112^2 under bf16
autocast, its split, and the three new kernels next to their eager-torch equivalents.

    PYTHONPATH=ssl-vit-video-analytics_amd python scripts/temporal_ssl_bench.py [--out FILE]

Without --part the script is the driver of one GPU visit: it runs the parts below as child
processes, each under its own `timeout`, one after the other, and stops at the first that fails.

    --part step      whole step (TOP off / TOP on), teacher forward, student forward + backward
                     of the masked pass, forward + backward of the TOP pass
    --part kernels   masked-frame loss forward + backward, EMA update, gradient clip: the HIP
                     kernels and eager torch on the same tensors, the forms alternating

Every figure is HIP-event time of work enqueued on one stream, the median of the timed
repetitions after warm-up repetitions of the same shapes.  The split is measured piece by piece
in repetitions of its own, so the pieces need not add up to the whole step.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ssl-vit-video-analytics_amd"))

PARTS = (("step", 420), ("kernels", 240))          # (name, time limit in seconds)
B, T, S = 48, 16, 112


def driver(out):
    lines = []
    for part, limit in PARTS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--part", part]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        lines.append(r.stdout)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(f"[FAIL] part {part} ended with status {r.returncode}; nothing further is started")
            return r.returncode
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w", encoding="utf-8") as f:
            f.write("".join(lines))
    return 0


def timed(torch, fn, reps, warm):
    """Median / min / max ms of `reps` runs of fn() after `warm` runs, one event pair per run."""
    ms = []
    for i in range(warm + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        if i >= warm:
            ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def fmt(name, r):
    return f"{name:<58s} {r[0]:10.3f} ms   (min {r[1]:.3f}, max {r[2]:.3f})"


def setup():
    import torch
    from ssl_mae_amd import temporal_ssl as TS
    from ssl_mae_amd.build import build
    from ssl_mae_amd.utils import load_config, set_seed
    if not torch.cuda.is_available():
        raise RuntimeError("temporal_ssl_bench needs an MI355X: no figure is taken without one")
    build()
    cfg = TS.resolve_config(load_config(os.path.join(ROOT, "configs", "ssl_train.yaml")))
    set_seed(42)
    dev = torch.device("cuda")
    model, ema = TS.build_model(cfg, dev)
    model.train()
    clip = TS.SyntheticClips(1, B, T, S, dev).batches[0]
    return torch, TS, cfg, model, ema, clip


def part_step(reps=6, warm=2):
    torch, TS, cfg, model, ema, clip = setup()
    from ssl_mae_amd.finetune import SegMeanFn
    from ssl_mae_amd.optim import FusedAdamW
    ssl, tr = cfg["ssl_objectives"], cfg["training"]
    opt = FusedAdamW(model.parameters(), lr=float(tr["learning_rate"]), weight_decay=float(tr["weight_decay"]))
    print(f"# temporal SSL step: B={B} T={T} {S}x{S} bf16, {torch.cuda.get_device_name(0)}, "
          f"{sum(p.numel() for p in model.parameters()) / 1e6:.2f} M parameters, N = {B * max(1, int(T * ssl['mask_ratio']))} "
          f"masked rows, TOP on {max(2, int(B * ssl['top_subsample']))} clips")
    top_epoch = int(ssl["top_start_epoch"])
    print(fmt("step, TOP off (teacher + student + clip + AdamW + EMA)",
              timed(torch, lambda: TS.ssl_step(model, ema, clip, cfg, 1, 1, opt=opt), reps, warm)))
    print(fmt("step, TOP on  (+ the TOP pass on half the batch)",
              timed(torch, lambda: TS.ssl_step(model, ema, clip, cfg, top_epoch, 2, opt=opt), reps, warm)))

    def autocast():
        return torch.autocast("cuda", dtype=torch.bfloat16)

    def teacher():
        with torch.no_grad(), autocast():
            return ema.forward_tokens(clip, mask=None)

    print(fmt("teacher forward (eval, no_grad)", timed(torch, teacher, reps, warm)))
    ctx_t = teacher().reshape(B * T, -1)
    mask = TS._host_mask(B, T, ssl["mask_ratio"])
    idx = mask.reshape(-1).nonzero().reshape(-1).to(torch.int32).cuda()

    def student():
        with autocast():
            pred = model.predictor(model.forward_tokens(clip, mask=mask).reshape(B * T, -1))
            out = TS.MFMLossFn.apply(pred, ctx_t, idx, float(ssl["mfm_weight"]), float(ssl["var_weight"]),
                                     float(ssl["var_target_std"]), float(ssl["var_eps"]))
        out[2].backward()

    print(fmt("student forward + backward (masked pass, predictor, loss)", timed(torch, student, reps, warm)))
    nb = max(2, int(B * ssl["top_subsample"]))
    idx_b = torch.randperm(B)[:nb]
    labels = torch.randint(0, 4, (nb,))

    def top():
        frames = TS._top_frames(clip, idx_b, labels)
        with autocast():
            ctx = model.forward_tokens(frames.view(nb, T, 3, S, S).permute(0, 2, 1, 3, 4), mask=None)
            loss = TS.TopCEFn.apply(model.top_logits(SegMeanFn.apply(ctx.reshape(nb * T, -1), nb, T)), labels.cuda())
        loss.backward()

    print(fmt(f"TOP pass forward + backward ({nb} clips, frame gather incl.)", timed(torch, top, reps, warm)))
    print(f"# peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def part_kernels(reps=30, warm=5):
    torch, TS, cfg, model, ema, clip = setup()
    import torch.nn.functional as F
    from ssl_mae_amd import ops as K
    ssl = cfg["ssl_objectives"]
    D = int(cfg["model"]["embed_dim"])
    R, N = B * T, B * max(1, int(T * ssl["mask_ratio"]))
    g = torch.Generator().manual_seed(1)
    pred = torch.randn(R, D, generator=g).to(torch.bfloat16).cuda()
    teacher = torch.randn(R, D, generator=g).cuda()
    mask = TS._host_mask(B, T, ssl["mask_ratio"]).reshape(-1)
    idx = mask.nonzero().reshape(-1).to(torch.int32).cuda()
    mask_d = mask.cuda()
    w_mfm, w_var, tgt, eps = float(ssl["mfm_weight"]), float(ssl["var_weight"]), float(ssl["var_target_std"]), \
        float(ssl["var_eps"])
    one = torch.ones(1, device="cuda")

    def loss_hip():
        out, stats = K.mfm_loss_fwd(pred, teacher, idx, w_mfm, w_var, tgt, eps)
        return K.mfm_loss_bwd(pred, teacher, idx, stats, one, w_mfm, w_var)

    def loss_torch():                                       # train_ssl.py:205-220 under autocast, then backward
        p = pred.detach().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            z_t = F.normalize(teacher[mask_d], dim=-1)
            z_s = F.normalize(p[mask_d], dim=-1)
            mfm = 2.0 - 2.0 * (F.normalize(z_s, dim=-1) * F.normalize(z_t, dim=-1)).sum(dim=-1).mean()
            var = torch.mean(F.relu(tgt - torch.sqrt(z_s.var(dim=0, unbiased=False) + eps)))
            loss = w_mfm * mfm + w_var * var
        loss.backward()
        return p.grad

    # parameters and gradients: the student's flat buffers after one forward
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        small = clip[:1, :, :2]
        model.forward_tokens(small)
        ema.forward_tokens(small)
    flat, flat_e = TS._flat_of(model), TS._flat_of(ema)
    params = list(model.parameters())
    flat.touch(*params)                                     # (zeroes the gradient buffer once after a forward)
    flat.grad.copy_(torch.randn(flat.total, generator=g) * 1e-2)
    for p in params:
        p.grad = p._sm_grad
    ranges = flat.touched_ranges()
    grad0 = flat.grad.clone()
    eparams = list(ema.parameters())
    m = float(ssl["ema_momentum"])

    def ema_hip():
        K.ema_update(flat_e.data, flat.data, m)

    def ema_torch_params():                                 # update_ema as the reference writes it
        with torch.no_grad():
            for pe, p in zip(eparams, params):
                pe.data.mul_(m).add_(p.data, alpha=1.0 - m)

    def ema_torch_flat():                                   # the same two ops on the flat buffers
        with torch.no_grad():
            flat_e.data.mul_(m).add_(flat.data, alpha=1.0 - m)

    def clip_hip():
        flat.grad.copy_(grad0)
        return K.grad_clip(flat.grad, ranges, 1.0)

    def clip_torch():
        flat.grad.copy_(grad0)
        return torch.nn.utils.clip_grad_norm_(params, 1.0)

    def clip_copy_only():
        flat.grad.copy_(grad0)

    print(f"# new kernels against eager torch, the forms alternating: R={R} D={D} N={N} rows, "
          f"{flat.total / 1e6:.2f} M flat elements in {len(ranges)} range(s), {len(params)} parameters")
    forms = [("masked-frame loss fwd + bwd, HIP (4 launches)", loss_hip), ("masked-frame loss fwd + bwd, eager torch", loss_torch),
             ("EMA update, HIP (1 launch)", ema_hip), ("EMA update, eager torch per parameter (reference form)", ema_torch_params),
             ("EMA update, eager torch on the flat buffers (2 launches)", ema_torch_flat),
             ("gradient clip, HIP (3 launches) + restore copy", clip_hip),
             ("gradient clip, torch clip_grad_norm_ + restore copy", clip_torch),
             ("restore copy alone", clip_copy_only)]
    ms = {name: [] for name, _ in forms}
    for i in range(warm + reps):                            # alternate: one run of every form per round
        for name, fn in forms:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if i >= warm:
                ms[name].append(t0.elapsed_time(t1))
    for name, _ in forms:
        print(fmt(name, (statistics.median(ms[name]), min(ms[name]), max(ms[name]))))
    a, b = loss_hip().float(), loss_torch().float()
    print(f"# loss gradient, HIP against eager torch (bf16 autocast): max |diff| {float((a - b).abs().max()):.3e} "
          f"of max {float(b.abs().max()):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=[p for p, _ in PARTS], default=None)
    ap.add_argument("--out", default=None, help="driver: also write the parts' output to this file")
    args = ap.parse_args()
    if args.part is None:
        return driver(args.out)
    {"step": part_step, "kernels": part_kernels}[args.part]()
    return 0


if __name__ == "__main__":
    sys.exit(main())

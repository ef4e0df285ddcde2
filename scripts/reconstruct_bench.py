"""sm_mae_reconstruct at the C2 shape (B=256, T=8, 224^2, bf16 pred) against the same result
composed from eager torch ops on the device (patchify, var / mean, the blends, clamp, byte cast),
next to a device-to-device copy of bench.py's calibration size.

    PYTHONPATH=ssl-vit-video-analytics_amd python scripts/reconstruct_bench.py [--out profiles/reconstruct.txt]

Kernel times are HIP events around `--reps` back-to-back launches after a warm-up, `--rounds`
times over, the variants alternating inside a round; the line gives the median round and the
spread.  The kernel's two panel-store forms are timed through the C entry point on caller-owned
buffers: a panels buffer shifted off 4-byte alignment selects the byte stores (include/sm_api.h),
so no switch exists for the measurement alone.  Bytes per launch are the algorithm's: every input
read once, every output written once.
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ssl-vit-video-analytics_amd"))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def eager(pred, clip, mask, norm_pix=True, paste=True, bgr=True):
    """The kernel's three outputs from torch tensor ops (fp32 on the device)."""
    B, C, T, H, W = clip.shape
    hp, wp = H // 8, W // 8
    x = torch.einsum("bcthpwq->bthwpqc", clip.reshape(B, C, T, hp, 8, wp, 8)).reshape(B, T * hp * wp, 192)
    p = pred.float()
    src = [2, 1, 0] if bgr else [0, 1, 2]
    mean_f = torch.tensor([MEAN[s] for s in src], device=clip.device).repeat(64)
    std_f = torch.tensor([STD[s] for s in src], device=clip.device).repeat(64)
    if norm_pix:
        var, mu = torch.var_mean(x, dim=-1, keepdim=True)
        sd = (var + 1e-6).sqrt()
        tgt, r = (x - mu) / sd, p * sd + mu
    else:
        tgt, r = x, p
    v_x, v_r = x * std_f + mean_f, r * std_f + mean_f
    te = torch.stack([((p - tgt) ** 2).mean(-1).reshape(-1),
                      ((v_r.clamp(0, 1) - v_x.clamp(0, 1)) ** 2).mean(-1).reshape(-1)], dim=-1)
    m = mask.reshape(B, T * hp * wp, 1).bool()
    v_out = torch.where(m, v_r, v_x) if paste else v_r

    def rgb(tok):
        img = torch.einsum("bthwpqc->bcthpwq", tok.reshape(B, T, hp, wp, 8, 8, 3)).reshape(B, 3, T, H, W)
        return img.flip(1) if bgr else img

    orig, recon = rgb(v_x), rgb(v_out).contiguous()
    keep = 1.0 - mask.reshape(B, 1, T, hp, wp).float().repeat_interleave(8, 3).repeat_interleave(8, 4)
    strip = torch.cat([orig, orig * keep, recon], dim=4)
    panels = strip.clamp(0, 1).mul(255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    return panels, recon, te


def event_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ssl_mae_amd import _lib, kernels
    if not torch.cuda.is_available():
        raise RuntimeError("reconstruct_bench needs an MI355X")
    _lib.load()
    dev = torch.device("cuda")
    B, T, S = args.batch, args.frames, args.size
    L = (S // 8) ** 2
    ntok = B * T * L
    g = torch.Generator(device=dev).manual_seed(0)
    clip = torch.randn(B, 3, T, S, S, device=dev, generator=g)
    pred = torch.randn(B, T * L, 192, device=dev, generator=g).to(torch.bfloat16)
    mask = (torch.rand(B, 1, L, device=dev, generator=g) < 0.75).expand(B, T, L).to(torch.uint8).contiguous()
    panels = torch.empty(B * T * S * 3 * S * 3 + 4, dtype=torch.uint8, device=dev)
    recon = torch.empty(B, 3, T, S, S, device=dev)
    te = torch.empty(ntok, 2, device=dev)
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)

    def raw(panel_off, want_recon):
        rc = _lib.query("sm_mae_reconstruct", _lib.dt(pred), _lib.ptr(pred), _lib.ptr(clip), *clip.stride(), _lib.ptr(mask),
                        B, T, S, S, ctypes.cast(m3, ctypes.c_void_p), ctypes.cast(s3, ctypes.c_void_p), 1, 1, 1,
                        _lib.ptr(panels[panel_off:]), _lib.ptr(recon) if want_recon else None, _lib.ptr(te),
                        _lib.stream())
        assert rc == 0, rc

    per_tok = 384 + 768 + 1 + 576 + 8
    variants = [("packed dword panel stores (aligned panels)", 0, True, per_tok + 768),
                ("packed dword panel stores, no recon output", 0, False, per_tok),
                ("byte panel stores (panels off 4-byte alignment)", 1, True, per_tok + 768)]
    lines = [f"device: {torch.cuda.get_device_name(0)}; sm_mae_reconstruct B={B} T={T} {S}^2 ({ntok} tokens), bf16 pred, "
             f"norm_pix, paste_visible, bgr_swap; {args.rounds} rounds of {args.reps} launches, median [min .. max]"]
    times = {name: [] for name, *_ in variants}
    for name, off, wr, _ in variants:               # warm-up: code objects, caches
        for _ in range(3):
            raw(off, wr)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, off, wr, _ in variants:
            times[name].append(event_ms(lambda: raw(off, wr), args.reps))
    for name, _, _, nbytes in variants:
        t = times[name]
        med = statistics.median(t)
        lines.append(f"kernel, {name}: {med:.3f} ms [{min(t):.3f} .. {max(t):.3f}]  "
                     f"{nbytes * ntok / 1e9:.2f} GB per launch  {nbytes * ntok / med / 1e6:.0f} GB/s")

    # the same result from eager torch ops, and the two agree
    ek = kernels.mae_reconstruct(pred, clip, mask, MEAN, STD)
    ee = eager(pred, clip, mask)
    differ, nbytes_panels = int((ek[0] != ee[0]).sum()), ek[0].numel()
    off_by = int((ek[0].to(torch.int16) - ee[0].to(torch.int16)).abs().max())
    rel = float((ek[1] - ee[1]).abs().max() / ee[1].abs().max())
    rel_te = float(((ek[2] - ee[2]).abs().max(0).values / ee[2].abs().max(0).values).max())
    del ek, ee
    torch.cuda.empty_cache()
    eager(pred, clip, mask)
    torch.cuda.synchronize()
    t = [event_ms(lambda: eager(pred, clip, mask), 3) for _ in range(args.rounds)]
    med_e = statistics.median(t)
    med_k = statistics.median(times[variants[0][0]])
    lines.append(f"eager torch composition (patchify, var_mean, blends, clamp, byte cast): {med_e:.3f} ms "
                 f"[{min(t):.3f} .. {max(t):.3f}]  {med_e / med_k:.1f}x the kernel")
    lines.append(f"kernel vs eager: {differ} of {nbytes_panels} bytes differ (by at most {off_by}), recon max diff "
                 f"{rel:.1e} of its range, token_err {rel_te:.1e}")

    # bench.py --full's copy calibration: a device-to-device copy of 4.9 GB, read + write bytes / time
    n = int(4.9e9) // 4
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dst.copy_(src)
    torch.cuda.synchronize()
    t = [event_ms(lambda: dst.copy_(src), 5) for _ in range(args.rounds)]
    med_c = statistics.median(t)
    lines.append(f"copy calibration (4.9 GB device-to-device, read + write): {med_c:.3f} ms [{min(t):.3f} .. {max(t):.3f}]  "
                 f"{2 * n * 4 / med_c / 1e6:.0f} GB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

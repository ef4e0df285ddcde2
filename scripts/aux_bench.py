"""Time the kernels of the rows next to the hot path:

* FedAvg aggregation (sm_fedavg_weighted_sum) at BASELINE config C5: 4 clients x
  the full MAE state (TinyViT-21M variant + 4x384 decoder, fp32).  Algorithmic
  bytes per launch = (K + 1) x n x 4 (K client reads + one write).
* clip normalisation (sm_frames_normalize) at the bench batch: 256 clips x 8 frames
  x 224^2.  Algorithmic bytes = 3 (uint8 RGB read) + 12 (3 fp32 written) per pixel.

* `aux_bench.py resize [--out profiles/resize.txt]`: clip resize + normalisation
  (sm_frames_resize_normalize) at 256 clips x 8 frames, 112^2 -> 224^2 and 240x320 ->
  112^2, next to sm_frames_normalize at the same output size, eager torch ops, the host
  path on 16 threads and the 4.9 GB copy calibration (see `resize`).

* `aux_bench.py fedround [--out profiles/fed_exchange.txt]`: one FedAvg round's exchange through
  federated.FedCohort against run_fedavg's state_dict path, and the fused launches' bandwidth
  against the copy calibration (see `fedround`).

* `aux_bench.py finetune [--out profiles/finetune.txt]`: the optimizer step of a full fine-tune
  (torch.optim.AdamW against optim.GroupedAdamW) and one epoch of configs/finetune.yaml (see
  `finetune`).

* `aux_bench.py fed_dp [--out profiles/fed_dp.txt]`: the DP-FedAvg aggregation
  (FedCohort.aggregate_dp, three launches) against the plain aggregate and the eager
  dp_aggregate_reference in the same process, with each launch's time and bandwidth (see `fed_dp`).

* `aux_bench.py fed_q8 [--out profiles/fed_q8.txt]`: the compressed aggregation
  (FedCohort.aggregate_q8, one launch) with and without the payload against the plain aggregate
  and the eager q8_aggregate_reference in the same process, with the launch's bandwidth (see
  `fed_q8`).

* `aux_bench.py knn [--out profiles/knn.txt]`: the kNN evaluation (knn.knn_eval: fused search,
  vote, metrics) against the eager knn_reference in the same process at UCF101's list sizes and
  at 16384 x 262144, and the search's achieved fp32 FLOP/s (see `knn`).

* `aux_bench.py crop [--out profiles/crop_resize.txt]`: the random-resized-crop launch
  (sm_frames_crop_resize_normalize) at the `resize` shapes with windows from the default sampler,
  against sm_frames_resize_normalize on the full frames and against the same crop in eager torch
  ops, alternating, and the 4.9 GB copy calibration (see `crop`).

* `aux_bench.py blur [--out profiles/box_blur.txt]`: the box blur (sm_frames_box_blur) at k = 15, 31,
  51 on 2048 frames with and without boxes, against a plain device copy of the same bytes and the
  same result in eager torch ops, the statistics launch, and the 4.9 GB copy calibration (see `blur`).

* `aux_bench.py mix [--out profiles/mix.txt]`: the Mixup / CutMix launch (sm_clip_mix) at 256 clips x 8
  frames, 112^2 and 224^2, all-Mixup and all-CutMix pairs, against a plain device copy of the same
  tensor and the same result in eager torch ops, the device operations ClipMixer adds to a step, and
  the 4.9 GB copy calibration (see `mix`).

Prints one JSON line per kernel; run under rocprofv3 --kernel-trace --stats to
cross-check the average launch durations."""
import json
import os
import sys

import torch

sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "ssl-vit-video-analytics_amd")]
from ssl_mae_amd import federated as F  # noqa: E402
from ssl_mae_amd import kernels as K  # noqa: E402


def _time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def frames(B=256, T=8, S=224, iters=30):
    f = torch.randint(0, 256, (B, T, S, S, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 3, T, S, S), dtype=torch.float32, device="cuda")
    ms = _time(lambda: K.frames_normalize(f, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), True, None, out), iters)
    gb = B * T * S * S * 15 / 1e9
    print(json.dumps({"kernel": "frames_norm4_kernel", "clips": B, "frames": T, "size": S,
                      "avg_launch_ms": round(ms, 4), "algorithmic_gb_per_launch": round(gb, 4),
                      "achieved_gbs": round(gb / ms * 1e3, 1), "peak_gbs": 8000.0,
                      "frac": round(gb / ms * 1e3 / 8000.0, 3)}))


def main(k=4, iters=50):
    from ssl_mae_amd.mae_vit_adapter import TinyVideoMAE
    from ssl_mae_amd.tiny_vit import tiny_vit_21m_variant
    cfg = {"dataset": {"clip_len": 8, "image_size": 224},
           "model": {"decoder_embed_dim": 384, "decoder_depth": 4, "decoder_num_heads": 6}}
    m = TinyVideoMAE(tiny_vit_21m_variant(img_size=224), cfg)
    n = sum(v.numel() for v in m.state_dict().values() if v.is_floating_point())
    bufs = [torch.randn(n, device="cuda") for _ in range(k)]
    w = F._norm_weights([1.0 + i for i in range(k)], float(sum(1.0 + i for i in range(k))))
    out = torch.empty_like(bufs[0])
    for _ in range(5):
        K.fedavg_weighted_sum(bufs, w, out)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        K.fedavg_weighted_sum(bufs, w, out)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / iters
    gb = (k + 1) * n * 4 / 1e9
    print(json.dumps({"kernel": "fedavg_sum4_kernel", "clients": k, "elements": n, "avg_launch_ms": round(ms, 4),
                      "algorithmic_gb_per_launch": round(gb, 4), "achieved_gbs": round(gb / ms * 1e3, 1),
                      "peak_gbs": 8000.0, "frac": round(gb / ms * 1e3 / 8000.0, 3)}))


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _rounds(fn, reps, rounds):
    """[ms per call] over `rounds` event-timed windows of `reps` calls."""
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) / reps)
    return out


def _fmt(t):
    import statistics
    return f"{statistics.median(t):.3f} ms [{min(t):.3f} .. {max(t):.3f}]"


def _copy_calibration(rounds):
    """(report line, GB/s) of a 4.9 GB device-to-device copy, read + write."""
    import statistics
    n = int(4.9e9) // 4
    a, b = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    b.copy_(a)
    torch.cuda.synchronize()
    tc = _rounds(lambda: b.copy_(a), 5, rounds)
    gbs = 2 * n * 4 / statistics.median(tc) / 1e6
    return f"copy calibration (4.9 GB device-to-device, read + write): {_fmt(tc)}  {gbs:.0f} GB/s", gbs


def resize(out_path=None, B=256, T=8, reps=20, rounds=5, host_threads=16):
    """sm_frames_resize_normalize at the bench batch for 112^2 -> 224^2 and 240x320 -> 112^2,
    next to sm_frames_normalize at the same output size (same bytes written) in alternating
    rounds, the same result from eager torch ops on the GPU, the host path
    (mae_dataset.MAEVideoDataset(raw=False)'s per-frame arithmetic on `host_threads` threads,
    decoding excluded) and the 4.9 GB copy calibration.  Algorithmic bytes of the resize:
    every source byte once + 12 per output pixel."""
    import statistics
    import tempfile
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch.nn.functional as Fn
    from ssl_mae_amd.mae_dataset import MAEVideoDataset
    dev = torch.device("cuda")
    lines = [f"device: {torch.cuda.get_device_name(0)}; B={B} T={T}; {rounds} rounds of {reps} launches, "
             "median [min .. max]"]
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    for hs, ws, S in ((112, 112, 224), (240, 320, 112)):
        src = torch.randint(0, 256, (B, T, hs, ws, 3), dtype=torch.uint8, device=dev)
        desc = torch.tensor([[b * T * hs * ws * 3, hs, ws, b & 1] for b in range(B)], device=dev)   # every other clip flipped
        same = torch.randint(0, 256, (B, T, S, S, 3), dtype=torch.uint8, device=dev)
        out = torch.empty((B, 3, T, S, S), dtype=torch.float32, device=dev)
        out2 = torch.empty_like(out)
        packed = src.view(-1)

        def k_resize():
            K.frames_resize_normalize(packed, desc, T, (S, S), MEAN, STD, False, out)

        def k_norm():
            K.frames_normalize(same, MEAN, STD, False, None, out2)

        def eager():
            x = src.view(B * T, hs, ws, 3).permute(0, 3, 1, 2).float().div_(255.0)
            x = Fn.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)
            x = torch.where((desc[:, 3] & 1).bool().repeat_interleave(T).view(-1, 1, 1, 1), x.flip(3), x)
            x = (x - mean_t) / std_t
            return x.view(B, T, 3, S, S).permute(0, 2, 1, 3, 4).contiguous()

        for fn in (k_resize, k_norm, eager):            # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        diff = float((eager() - out).abs().max())
        tr, tn = [], []
        for _ in range(rounds):                         # alternate the two kernels
            tr += _rounds(k_resize, reps, 1)
            tn += _rounds(k_norm, reps, 1)
        te = _rounds(eager, 3, rounds)
        gb_r = (B * T * hs * ws * 3 + out.numel() * 4) / 1e9
        gb_n = (same.numel() + out.numel() * 4) / 1e9
        mr, mn = statistics.median(tr), statistics.median(tn)
        lines.append(f"{hs}x{ws} -> {S}x{S}:")
        lines.append(f"  sm_frames_resize_normalize: {_fmt(tr)}  {gb_r:.3f} GB per launch  {gb_r / mr * 1e3:.0f} GB/s")
        lines.append(f"  sm_frames_normalize at {S}x{S}: {_fmt(tn)}  {gb_n:.3f} GB per launch  {gb_n / mn * 1e3:.0f} GB/s"
                     f"  (resize / normalize time: {mr / mn:.2f})")
        lines.append(f"  eager torch ops on the GPU (float, div, interpolate, flip, normalize, permute): {_fmt(te)}  "
                     f"{statistics.median(te) / mr:.1f}x the kernel; max |eager - kernel| = {diff:.2e}")
        # host path: the reference item's arithmetic per frame, one torch thread per worker
        frames_np = src.cpu().numpy()
        with tempfile.NamedTemporaryFile("w", suffix=".txt") as f:
            ds = MAEVideoDataset(f.name, image_size=S, clip_len=T)

        def host_clip(b):
            flip = bool(b & 1)
            imgs = []
            for t in range(T):
                x = ds._resize_tensor(frames_np[b, t])
                if flip:
                    x = torch.flip(x, dims=[2])
                imgs.append((x - ds.mean) / ds.std)
            return torch.stack(imgs, dim=0).permute(1, 0, 2, 3).contiguous()

        nt = torch.get_num_threads()
        torch.set_num_threads(1)
        th = []
        with ThreadPoolExecutor(host_threads) as ex:
            list(ex.map(host_clip, range(min(B, 2 * host_threads))))          # warm-up
            for _ in range(3):
                t0 = time.perf_counter()
                list(ex.map(host_clip, range(B)))
                th.append((time.perf_counter() - t0) * 1e3)
        torch.set_num_threads(nt)
        lines.append(f"  host path, {host_threads} threads (resize + flip + normalize of {B * T} decoded frames): "
                     f"{_fmt(th)}  {statistics.median(th) / mr:.0f}x the kernel")
        del src, same, out, out2, packed
        torch.cuda.empty_cache()
    lines.append(_copy_calibration(rounds)[0])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def crop(out_path=None, B=256, T=8, reps=20, rounds=5, seed=0):
    """sm_frames_crop_resize_normalize at the `resize` benchmark's shapes (112^2 -> 224^2 and
    240x320 -> 112^2) with one window and flip per clip from mae_loader.RandomResizedCropFlip's
    defaults at a fixed seed, alternating in every round with sm_frames_resize_normalize on the
    full frames at the same output size (same bytes written, no fewer read) and with the same
    crop in eager torch ops on the device (per clip: slice, float, div, interpolate, flip,
    normalize, permute).  The crop's ratio to the full-frame launch stands beside that launch's own
    spread over the rounds, (max - min) / median.  Algorithmic bytes of the crop: every byte of the
    windows once + 12 per output pixel.  Ends with the 4.9 GB copy calibration."""
    import statistics
    import torch.nn.functional as Fn
    from ssl_mae_amd.mae_loader import RandomResizedCropFlip
    dev = torch.device("cuda")
    lines = [f"device: {torch.cuda.get_device_name(0)}; B={B} T={T}; windows: RandomResizedCropFlip(seed={seed}) "
             f"defaults; {rounds} rounds of {reps} launches, alternating, median [min .. max]"]
    mean_t = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    for hs, ws, S in ((112, 112, 224), (240, 320, 112)):
        src = torch.randint(0, 256, (B, T, hs, ws, 3), dtype=torch.uint8, device=dev)
        desc4 = torch.tensor([[b * T * hs * ws * 3, hs, ws, 0] for b in range(B)])
        aug = RandomResizedCropFlip(seed=seed)
        desc8_host = aug.windows(desc4)
        wins = desc8_host[:, 3:].tolist()
        desc8 = desc8_host.to(dev)
        desc4 = desc8[:, :4].contiguous()               # the same flips on the full frames
        out = torch.empty((B, 3, T, S, S), dtype=torch.float32, device=dev)
        out2 = torch.empty_like(out)
        packed = src.view(-1)

        def k_crop():
            K.frames_crop_resize_normalize(packed, desc8, T, (S, S), MEAN, STD, False, out)

        def k_full():
            K.frames_resize_normalize(packed, desc4, T, (S, S), MEAN, STD, False, out2)

        def eager():
            clips = []
            for b, (fl, y0, x0, hc, wc) in enumerate(wins):
                x = src[b, :, y0:y0 + hc, x0:x0 + wc].permute(0, 3, 1, 2).float().div_(255.0)
                x = Fn.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)
                if fl & 1:
                    x = x.flip(3)
                clips.append(((x - mean_t) / std_t).permute(1, 0, 2, 3))
            return torch.stack(clips)

        for fn in (k_crop, k_full, eager):              # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        diff = float((eager() - out).abs().max())
        tc, tf, te = [], [], []
        for _ in range(rounds):                         # alternate the three paths
            tc += _rounds(k_crop, reps, 1)
            tf += _rounds(k_full, reps, 1)
            te += _rounds(eager, 2, 1)
        win_px = sum(hc * wc for _, _, _, hc, wc in wins)
        gb_c = (T * win_px * 3 + out.numel() * 4) / 1e9
        gb_f = (src.numel() + out.numel() * 4) / 1e9
        mc, mf, me = statistics.median(tc), statistics.median(tf), statistics.median(te)
        spread = (max(tf) - min(tf)) / mf
        lines.append(f"{hs}x{ws} -> {S}x{S}: mean window {win_px / B / (hs * ws):.3f} of the frame, "
                     f"{sum(fl & 1 for fl, *_ in wins)} of {B} clips flipped, {sum(aug.last_fallback)} fallbacks")
        lines.append(f"  sm_frames_crop_resize_normalize: {_fmt(tc)}  {gb_c:.3f} GB per launch  {gb_c / mc * 1e3:.0f} GB/s")
        lines.append(f"  sm_frames_resize_normalize, full frames: {_fmt(tf)}  {gb_f:.3f} GB per launch  "
                     f"{gb_f / mf * 1e3:.0f} GB/s")
        lines.append(f"  crop / full-frame time: {mc / mf:.3f}; the full-frame launch's own spread over the rounds, "
                     f"(max - min) / median: {spread:.3f}")
        lines.append(f"  eager torch ops on the GPU (per clip: slice, float, div, interpolate, flip, normalize, permute; "
                     f"stack): {_fmt(te)}  {me / mc:.1f}x the kernel; max |eager - kernel| = {diff:.2e}")
        lines.append(f"  the fused launch is {'FASTER' if mc < me else 'NOT faster'} than the eager path here")
        del src, out, out2, packed
        torch.cuda.empty_cache()
    lines.append(_copy_calibration(rounds)[0])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    if "NOT faster" in text:
        raise SystemExit("the fused crop launch is not faster than the eager path")


def fedround(out_path=None, reps=5, rounds=5, num_classes=101):
    """One FedAvg round's exchange (broadcast + aggregate) over VideoClassifier models at 112^2
    that have each run one forward (parameters in their flat buffers), K = 4 and K = 8 selected
    clients: (a) federated.FedCohort, one launch each way, against (b) run_fedavg's path in the
    same process -- K strict load_state_dict broadcasts, then fedavg_aggregate (torch.cat
    gathers, one launch, un-flatten, load_state_dict).  The fused launches alone are timed
    through kernels.fedavg_exchange (each call includes its 64-byte header read-back); bytes
    moved = (sources + destinations) x fp32 state bytes.  Ends with the 4.9 GB copy calibration."""
    import statistics
    from ssl_mae_amd.finetune import VideoClassifier
    lines = [f"device: {torch.cuda.get_device_name(0)}; VideoClassifier({num_classes}) at 112^2; {rounds} rounds of "
             f"{reps} exchanges, median [min .. max]"]
    clip = torch.randn(1, 3, 1, 112, 112, device="cuda")
    models = []
    for s in range(9):
        torch.manual_seed(s)
        m = VideoClassifier(num_classes, img_size=112).cuda().eval()
        with torch.no_grad():
            m(clip)
        models.append(m)
    glob = models[0]
    results = []
    for k in (4, 8):
        clients = models[1:k + 1]
        sel = list(range(k))
        sizes = [100.0 + 10 * i for i in sel]
        cohort = F.FedCohort(glob, clients)
        fbytes = sum(v.numel() * 4 for v in glob.state_dict().values() if v.is_floating_point())
        entries = len(glob.state_dict())

        def fused():
            cohort.broadcast(sel)
            cohort.aggregate(sel, sizes)

        def parent():
            g = {n: v.detach().clone() for n, v in glob.state_dict().items()}
            for c in clients:
                c.load_state_dict(g, strict=True)
            states = [{n: v.detach() for n, v in c.state_dict().items()} for c in clients]
            F.fedavg_aggregate(glob, states, sizes)

        norm = F._norm_weights(sizes, float(sum(sizes)))
        src = [c + 1 for c in sel]

        def k_aggregate():
            K.fedavg_exchange(src, norm, [0], cohort._float_table)

        def k_broadcast():
            K.fedavg_exchange([0], [1.0], src, cohort._float_table, copy_only=True)

        for fn in (fused, parent, k_aggregate, k_broadcast):
            fn()
        torch.cuda.synchronize()
        tf, tp = [], []
        for _ in range(rounds):                         # alternate the two paths
            tf += _rounds(fused, reps, 1)
            tp += _rounds(parent, reps, 1)
        ta, tb = _rounds(k_aggregate, reps, rounds), _rounds(k_broadcast, reps, rounds)
        gb = (k + 1) * fbytes / 1e9
        ga, gbb = gb / statistics.median(ta) * 1e3, gb / statistics.median(tb) * 1e3
        assert cohort.rebuilds == 1
        lines.append(f"K={k} selected clients, {entries} state entries, {fbytes / 2 ** 20:.1f} MiB fp32 state per model:")
        lines.append(f"  (a) FedCohort broadcast + aggregate: {_fmt(tf)}")
        lines.append(f"  (b) load_state_dict broadcast + fedavg_aggregate: {_fmt(tp)}  "
                     f"{statistics.median(tp) / statistics.median(tf):.1f}x (a)")
        lines.append(f"  fused aggregate launch ({k} sources -> 1 destination): {_fmt(ta)}  {gb:.3f} GB moved  {ga:.0f} GB/s")
        lines.append(f"  fused broadcast launch (1 source -> {k} destinations): {_fmt(tb)}  {gb:.3f} GB moved  {gbb:.0f} GB/s")
        results.append((k, ga, gbb))
    del models, clients, cohort
    torch.cuda.empty_cache()
    line, copy_gbs = _copy_calibration(rounds)
    lines.append(line)
    for k, ga, gbb in results:
        lines.append(f"K={k}: fused aggregate at {ga / copy_gbs:.2f}, fused broadcast at {gbb / copy_gbs:.2f} of the copy "
                     "calibration's bandwidth")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def _kernel_times(fn, reps, names):
    """{name: ms per call} of the device kernels whose name contains one of `names`, from
    torch.profiler's trace of `reps` calls."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    out = dict.fromkeys(names, 0.0)
    for e in prof.key_averages():
        if not str(getattr(e, "device_type", "")).endswith("CUDA"):
            continue
        us = getattr(e, "device_time_total", None)
        us = getattr(e, "cuda_time_total", 0.0) if us is None else us
        for n in names:
            if n in e.key:
                out[n] += float(us) / 1e3 / reps
    return out


def fed_dp(out_path=None, reps=5, rounds=5, num_classes=101):
    """The DP-FedAvg aggregation over VideoClassifier models at 112^2 that have each run one forward,
    K = 4 and K = 8 selected clients, clip_norm 1 and noise multiplier 1: FedCohort.aggregate_dp
    (norms, finalise, update: three launches plus the counter launch) with and without noise, the
    plain FedCohort.aggregate, and the eager dp_aggregate_reference over state_dicts, alternating in
    one process.  The three launches' own times come from torch.profiler's trace of the same
    calls; GB/s against algorithmic bytes, (K + 1) x 4 B per clipped element for the norms and
    (K + 2) x 4 B per fp32 element for the update ((K + 1) x 4 B for the plain aggregate).  Ends
    with the 4.9 GB copy calibration."""
    import statistics
    from ssl_mae_amd.finetune import VideoClassifier
    lines = [f"device: {torch.cuda.get_device_name(0)}; VideoClassifier({num_classes}) at 112^2; {rounds} rounds of "
             f"{reps} aggregations ({max(1, reps // 2)} for the eager reference), median [min .. max]"]
    clip = torch.randn(1, 3, 1, 112, 112, device="cuda")
    models = []
    for s in range(9):
        torch.manual_seed(s)
        m = VideoClassifier(num_classes, img_size=112).cuda().eval()
        with torch.no_grad():
            m(clip)
        models.append(m)
    glob = models[0]
    kernels = ("dp_norms_kernel", "dp_finalise_kernel", "dp_update_kernel")
    results = []
    for k in (4, 8):
        clients = models[1:k + 1]
        sel = list(range(k))
        sizes = [100.0 + 10 * i for i in sel]
        cohort = F.FedCohort(glob, clients)
        n_all = sum(glob.state_dict()[key].numel() for key in cohort.float_keys)
        n_clip = sum(glob.state_dict()[key].numel() for key, m in zip(cohort.float_keys, cohort._clip_modes) if m)
        seed = F.dp_round_seed(42, 1)

        def dp_noise():
            cohort.aggregate_dp(sel, sizes, 1.0, 1.0, seed)

        def dp_clean():
            cohort.aggregate_dp(sel, sizes, 1.0, 0.0, seed)

        def plain():
            cohort.aggregate(sel, sizes)

        def reference():
            states = [{n: v.detach() for n, v in c.state_dict().items()} for c in clients]
            F.dp_aggregate_reference(glob, states, sizes, 1.0, 1.0, seed)

        for fn in (dp_noise, dp_clean, plain, reference):
            fn()
        torch.cuda.synchronize()
        td, tc, tp, tr = [], [], [], []
        for _ in range(rounds):                         # alternate the paths
            td += _rounds(dp_noise, reps, 1)
            tc += _rounds(dp_clean, reps, 1)
            tp += _rounds(plain, reps, 1)
            tr += _rounds(reference, max(1, reps // 2), 1)
        md, mr = statistics.median(td), statistics.median(tr)
        gb1, gb2, gbp = (k + 1) * 4 * n_clip / 1e9, (k + 2) * 4 * n_all / 1e9, (k + 1) * 4 * n_all / 1e9
        lines.append(f"K={k} selected clients, {len(cohort.float_keys)} fp32 entries ({sum(cohort._clip_modes)} clipped), "
                     f"{n_all} fp32 elements ({n_clip} clipped) per model:")
        lines.append(f"  FedCohort.aggregate_dp, noise multiplier 1: {_fmt(td)}")
        lines.append(f"  FedCohort.aggregate_dp, noise multiplier 0: {_fmt(tc)}")
        lines.append(f"  FedCohort.aggregate (plain FedAvg): {_fmt(tp)}")
        lines.append(f"  dp_aggregate_reference (eager torch over state_dicts), noise multiplier 1: {_fmt(tr)}  "
                     f"{mr / md:.1f}x aggregate_dp")
        try:
            for label, fn in (("noise multiplier 1", dp_noise), ("noise multiplier 0", dp_clean)):
                kt = _kernel_times(fn, reps, kernels)
                lines.append(f"  launches, {label}: norms {kt[kernels[0]]:.3f} ms ({gb1:.3f} GB, "
                             f"{gb1 / max(kt[kernels[0]], 1e-9) * 1e3:.0f} GB/s), finalise {kt[kernels[1]]:.3f} ms, update "
                             f"{kt[kernels[2]]:.3f} ms ({gb2:.3f} GB, {gb2 / max(kt[kernels[2]], 1e-9) * 1e3:.0f} GB/s)")
            tk = _kernel_times(plain, reps, ("fedavg_exchange_kernel",))["fedavg_exchange_kernel"]
            plain_gbs = gbp / max(tk, 1e-9) * 1e3
            lines.append(f"  launch of the plain aggregate: {tk:.3f} ms ({gbp:.3f} GB, {plain_gbs:.0f} GB/s)")
        except Exception as exc:  # the trace splits the total; the totals above are the measurement
            plain_gbs = float("nan")
            lines.append(f"  launches: not measured ({type(exc).__name__}: {exc})")
        results.append((k, md, mr, plain_gbs))
        assert cohort.rebuilds == 1
    del models, clients, cohort
    torch.cuda.empty_cache()
    line, copy_gbs = _copy_calibration(rounds)
    lines.append(line)
    for k, md, mr, gp in results:
        lines.append(f"K={k}: plain aggregate launch at {gp / copy_gbs:.2f} of the copy calibration's bandwidth; aggregate_dp is "
                     f"{'FASTER' if md < mr else 'NOT faster'} than dp_aggregate_reference ({md:.3f} ms against {mr:.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def fed_q8(out_path=None, reps=5, rounds=5, num_classes=101):
    """The compressed aggregation over VideoClassifier models at 112^2 that have each run one
    forward, K = 4 and K = 8 selected clients: FedCohort.aggregate_q8 (one launch plus the counter
    launch) without and with the payload, the plain FedCohort.aggregate, and the eager
    q8_aggregate_reference over state_dicts, alternating in one process.  The launch's own time
    comes from torch.profiler's trace of the same calls; GB/s against algorithmic bytes per
    quantised element, 4 + 8 K read (theta, K sources, K residuals) and 4 K + 4 x destinations
    written (K residuals, one destination), plus K x (1 + 4 / 256) for the payload ((K + 1) x 4 B
    per element for the plain aggregate and for the unquantised entries).  Ends with the 4.9 GB
    copy calibration; the ratio to it is recorded, the fused call must beat the eager reference."""
    import statistics
    from ssl_mae_amd.finetune import VideoClassifier
    lines = [f"device: {torch.cuda.get_device_name(0)}; VideoClassifier({num_classes}) at 112^2; {rounds} rounds of "
             f"{reps} aggregations (1 for the eager reference), median [min .. max]"]
    clip = torch.randn(1, 3, 1, 112, 112, device="cuda")
    models = []
    for s in range(9):
        torch.manual_seed(s)
        m = VideoClassifier(num_classes, img_size=112).cuda().eval()
        with torch.no_grad():
            m(clip)
        models.append(m)
    glob = models[0]
    results = []
    for k in (4, 8):
        clients = models[1:k + 1]
        sel = list(range(k))
        sizes = [100.0 + 10 * i for i in sel]
        cohort = F.FedCohort(glob, clients)
        state = glob.state_dict()
        n_all = sum(state[key].numel() for key in cohort.float_keys)
        n_q = sum(state[key].numel() for key, m in zip(cohort.float_keys, cohort._clip_modes) if m)
        params = {name for name, _ in glob.named_parameters()}
        residuals = [{} for _ in clients]

        def q8():
            cohort.aggregate_q8(sel, sizes)

        def q8_payload():
            cohort.aggregate_q8(sel, sizes, payload=True)

        def plain():
            cohort.aggregate(sel, sizes)

        def reference():
            states = [{n: v.detach() for n, v in c.state_dict().items()} for c in clients]
            F.q8_aggregate_reference(glob, states, sizes, residuals)

        for fn in (q8, q8_payload, plain, reference):
            fn()
        torch.cuda.synchronize()
        tq, ty, tp, tr = [], [], [], []
        for _ in range(rounds):                         # alternate the paths
            tq += _rounds(q8, reps, 1)
            ty += _rounds(q8_payload, reps, 1)
            tp += _rounds(plain, reps, 1)
            tr += _rounds(reference, 1, 1)
        mq, mr = statistics.median(tq), statistics.median(tr)
        gbq = ((4 + 8 * k + 4 * k + 4) * n_q + (k + 1) * 4 * (n_all - n_q)) / 1e9
        gby = gbq + k * (1 + 4 / 256) * n_q / 1e9
        gbp = (k + 1) * 4 * n_all / 1e9
        lines.append(f"K={k} selected clients, {len(cohort.float_keys)} fp32 entries ({sum(cohort._clip_modes)} quantised), "
                     f"{n_all} fp32 elements ({n_q} quantised) per model; one upload "
                     f"{F.q8_upload_bytes(state, params) / 2 ** 20:.2f} MiB against {F.model_size_bytes(state) / 2 ** 20:.2f} "
                     f"MiB in fp32:")
        lines.append(f"  FedCohort.aggregate_q8: {_fmt(tq)}")
        lines.append(f"  FedCohort.aggregate_q8, payload written: {_fmt(ty)}")
        lines.append(f"  FedCohort.aggregate (plain FedAvg): {_fmt(tp)}")
        lines.append(f"  q8_aggregate_reference (eager torch over state_dicts): {_fmt(tr)}  {mr / mq:.1f}x aggregate_q8")
        try:
            kq = _kernel_times(q8, reps, ("q8_exchange_kernel",))["q8_exchange_kernel"]
            ky = _kernel_times(q8_payload, reps, ("q8_exchange_kernel",))["q8_exchange_kernel"]
            kp = _kernel_times(plain, reps, ("fedavg_exchange_kernel",))["fedavg_exchange_kernel"]
            q8_gbs = gbq / max(kq, 1e-9) * 1e3
            lines.append(f"  launch of aggregate_q8: {kq:.3f} ms ({gbq:.3f} GB, {q8_gbs:.0f} GB/s); with the payload "
                         f"{ky:.3f} ms ({gby:.3f} GB, {gby / max(ky, 1e-9) * 1e3:.0f} GB/s)")
            lines.append(f"  launch of the plain aggregate: {kp:.3f} ms ({gbp:.3f} GB, {gbp / max(kp, 1e-9) * 1e3:.0f} GB/s)")
        except Exception as exc:  # the trace splits the total; the totals above are the measurement
            q8_gbs = float("nan")
            lines.append(f"  launches: not measured ({type(exc).__name__}: {exc})")
        results.append((k, mq, mr, q8_gbs))
        assert cohort.rebuilds == 1
    del models, clients, cohort, residuals
    torch.cuda.empty_cache()
    line, copy_gbs = _copy_calibration(rounds)
    lines.append(line)
    ok = True
    for k, mq, mr, gq in results:
        ok = ok and mq < mr
        lines.append(f"K={k}: aggregate_q8 launch at {gq / copy_gbs:.2f} of the copy calibration's bandwidth; aggregate_q8 is "
                     f"{'FASTER' if mq < mr else 'NOT faster'} than q8_aggregate_reference ({mq:.3f} ms against {mr:.3f} ms)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    if not ok:
        raise SystemExit("aggregate_q8 did not beat q8_aggregate_reference")


def _count_launches(fn):
    """Device kernels / memsets / copies of one call, from torch.profiler's trace."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))


def finetune(out_path=None, reps=10, rounds=7, num_classes=101):
    """The optimizer step of a full fine-tune of VideoClassifier(101) at 112^2, every parameter
    trainable, gradients from one training step: torch.optim.AdamW as finetune.build_optimizer
    makes it (the baseline), torch.optim.AdamW with one group per parameter (what layer-wise decay
    costs there), optim.GroupedAdamW with the head / backbone groups, and GroupedAdamW with
    layer_decay 0.75.  Only `step()` is timed, the four alternating within every round; GB/s at 28
    bytes per parameter element (p, g, m, v read; p, m, v written).  Then one training and one
    validation epoch of configs/finetune.yaml (synthetic clips; the second epoch of the process),
    and the 4.9 GB copy calibration."""
    import statistics
    import time
    from ssl_mae_amd import train_finetune as TF
    from ssl_mae_amd.finetune import VideoClassifier, build_optimizer, param_groups
    from ssl_mae_amd.optim import GroupedAdamW
    from ssl_mae_amd.utils import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = [f"device: {torch.cuda.get_device_name(0)}; VideoClassifier({num_classes}) at 112^2, all parameters "
             f"trainable; {rounds} rounds of {reps} optimizer steps, median [min .. max]"]
    torch.manual_seed(0)
    model = VideoClassifier(num_classes, img_size=112).cuda().train()
    clip = torch.randn(2, 3, 2, 112, 112, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(clip)
    torch.nn.CrossEntropyLoss()(logits.float(), torch.tensor([1, 7], device="cuda")).backward()
    elems = sum(p.numel() for p in model.parameters())

    def cfg(**tr):
        base = {"learning_rate": 1e-4, "weight_decay": 0.01, "head_lr": 1e-3, "backbone_lr": 1e-4}
        base.update(tr)
        return {"training": base}

    named = list(model.named_parameters())
    decay_groups = param_groups(model, cfg(layer_decay=0.75), "two_stage")
    opts = [
        ("torch.optim.AdamW, build_optimizer's groups (baseline)", build_optimizer(cfg(), model, "ft_ssl")),
        ("torch.optim.AdamW, one group per parameter",
         torch.optim.AdamW([{"params": [p], "lr": 1e-4, "weight_decay": 0.01} for _, p in named])),
        ("GroupedAdamW, 2 groups (head_lr / backbone_lr)", GroupedAdamW(param_groups(model, cfg(), "two_stage"))),
        (f"GroupedAdamW, layer_decay 0.75 ({len(decay_groups)} groups)", GroupedAdamW(decay_groups)),
    ]
    for _, o in opts:
        for _ in range(3):
            o.step()
    torch.cuda.synchronize()
    times = [[] for _ in opts]
    for _ in range(rounds):                             # alternate the four within every round
        for t, (_, o) in zip(times, opts):
            t += _rounds(o.step, reps, 1)
    gb = 28 * elems / 1e9
    lines.append(f"{len(named)} parameters, {elems} elements, {gb:.3f} GB per step at 28 bytes per element")
    med = [statistics.median(t) for t in times]
    for (name, o), t, m in zip(opts, times, med):
        extra = f"  {len(o.table_segments)} segments, table built {o.table_builds}x" if isinstance(o, GroupedAdamW) else ""
        lines.append(f"  {name}: {_fmt(t)}  {gb / m * 1e3:.0f} GB/s  {med[0] / m:.2f}x the baseline's speed{extra}")
    step_gbs = [gb / m * 1e3 for m in med]

    # one training and one validation epoch of the shipped config
    ft = TF.resolve_config(load_config(os.path.join(root, "configs", "finetune.yaml")))
    dev = torch.device("cuda")
    train_loader, val_loader = TF.build_loaders(ft, dev)
    torch.manual_seed(0)
    ft_model = VideoClassifier(int(ft["dataset"]["num_classes"]), img_size=int(ft["dataset"]["image_size"])).to(dev)
    opt = TF.build_optimizer(ft, ft_model)
    scaler = TF.GradScaler(enabled=bool(ft["training"]["amp"]))
    quiet = lambda msg: None  # noqa: E731
    epoch_t = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.time()
        TF.train_one_epoch(ft_model, train_loader, opt, scaler, dev, ft, quiet)
        torch.cuda.synchronize()
        t1 = time.time()
        TF.evaluate(ft_model, val_loader, dev, tuple(ft["evaluation"]["topk"]), quiet)
        torch.cuda.synchronize()
        epoch_t.append((t1 - t0, time.time() - t1))
    ds, tr = ft["dataset"], ft["training"]
    lines.append(f"configs/finetune.yaml (mode {ft['experiment']['mode']}, optimizer {ft['optimizer']['type']}, "
                 f"{ft['synthetic']['num_train']} + {ft['synthetic']['num_val']} synthetic clips of {ds['clip_len']} "
                 f"frames at {ds['image_size']}^2, batch {tr['batch_size']}, amp {tr['amp']}), second epoch of the "
                 f"process: training epoch {epoch_t[1][0]:.2f} s, validation epoch {epoch_t[1][1]:.2f} s "
                 f"(first epoch, with warm-up: {epoch_t[0][0]:.2f} s and {epoch_t[0][1]:.2f} s)")
    del ft_model, opt, train_loader, val_loader
    torch.cuda.empty_cache()
    line, copy_gbs = _copy_calibration(rounds)
    lines.append(line)
    lines.append("optimizer step against the copy calibration's bandwidth: " +
                 ", ".join(f"{g / copy_gbs:.2f}" for g in step_gbs) + " (the four configurations in order)")
    faster = med[2] <= med[0]
    lines.append(f"GroupedAdamW (2 groups) is {'not slower' if faster else 'SLOWER'} than the baseline: "
                 f"optimizer.type {'adamw' if faster else 'adamw_torch'} is the default to ship")

    def write():
        text = "\n".join(lines) + "\n"
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write(text)
        return text

    write()                                             # the timings are safe before the trace
    try:
        counts = [_count_launches(o.step) for _, o in opts]
        lines.append("device operations per step (kernels, memsets and copies in torch.profiler's trace of one step): " +
                     ", ".join(str(c) for c in counts) + "; sm_adamw_table enqueues 3 by construction (the flag's "
                     "reset, the flag pass, the update pass)")
    except Exception as exc:  # the trace is a cross-check, not the measurement
        lines.append(f"device operations per step: not measured ({type(exc).__name__}); sm_adamw_table enqueues 3 by "
                     "construction (the flag's reset, the flag pass, the update pass)")
    print(write(), end="")


def knn(out_path=None, rounds=5, D=576, num_classes=101, temperature=0.07):
    """The kNN evaluation (knn.knn_eval: two row-norm launches, the fused search, the vote and the
    metrics launch, one readback) against knn.knn_reference (eager mm, stable sort, scatter_add,
    chunked over the queries) on the same device in the same process, alternating, at k = 20,
    ks = [1, 5, 10, 20], cosine, standard-normal features: Nq = 3783 / Nb = 9537 (UCF101 split 1's
    test and train lists) and Nq = 16384 / Nb = 262144 (the eager path has to chunk).  The search
    alone (sm_knn_topk with its merge launch, norm vectors given) is event-timed too, its
    2 Nq Nb D FLOPs over that time next to the 157.3 TF fp32-matrix specification (a specification,
    not a measurement on this device); at the small shape also with splits = 1 against auto.  The
    two paths' idx are compared once per shape (a similarity is an fp32 sum in two different
    orders there, so a few near-tied neighbours may swap).  Ends with the 4.9 GB copy calibration.
    No speed-up is asserted: what is measured is written down."""
    import statistics
    from ssl_mae_amd import knn as KNN
    ks, k = [1, 5, 10, 20], 20
    lines = [f"device: {torch.cuda.get_device_name(0)}; D={D}, k={k}, ks={ks}, cosine, T={temperature}, "
             f"{num_classes} classes; {rounds} rounds, median [min .. max]"]
    for Nq, Nb, reps, ref_reps in ((3783, 9537, 20, 3), (16384, 262144, 2, 1)):
        g = torch.Generator(device="cuda").manual_seed(Nq)
        zq = torch.randn(Nq, D, device="cuda", generator=g)
        zb = torch.randn(Nb, D, device="cuda", generator=g)
        yq = torch.randint(0, num_classes, (Nq,), device="cuda", generator=g)
        yb = torch.randint(0, num_classes, (Nb,), device="cuda", generator=g)
        rq, rb = K.row_rnorm(zq), K.row_rnorm(zb)
        auto = max(1, K.query("sm_knn_topk_workspace_bytes", Nq, Nb, k, 0) // (Nq * k * 8))

        def fused():
            return KNN.knn_eval(zq, yq, zb, yb, ks, temperature, num_classes)

        def reference():
            return KNN.knn_reference(zq, yq, zb, yb, ks, temperature, num_classes)

        def search(splits=0):
            return K.knn_topk(zq, zb, rq, rb, k, -1, splits)

        a, b = fused(), reference()                     # warm-up of both paths, and the comparison
        search()
        search(1)
        torch.cuda.synchronize()
        same = (a["idx"] == b["idx"]).all(1).float().mean().item()
        tf, tr, ts, t1 = [], [], [], []
        for _ in range(rounds):                         # alternate the paths
            tf += _rounds(fused, reps, 1)
            tr += _rounds(reference, ref_reps, 1)
            ts += _rounds(search, reps, 1)
            if Nb < 100000:
                t1 += _rounds(lambda: search(1), reps, 1)
        mf, mr, ms = statistics.median(tf), statistics.median(tr), statistics.median(ts)
        flop = 2.0 * Nq * Nb * D
        lines.append(f"Nq={Nq} Nb={Nb} ({flop / 1e9:.1f} GFLOP of similarities, auto splits = {auto}):")
        lines.append(f"  knn_eval fused (norms + search + vote + metrics + readback): {_fmt(tf)}")
        lines.append(f"  knn_reference (eager torch, same device): {_fmt(tr)}  {mr / mf:.2f}x the fused path's time")
        lines.append(f"  sm_knn_topk alone (auto splits): {_fmt(ts)}  {flop / ms / 1e9:.1f} TFLOP/s fp32, "
                     f"{flop / ms / 1e9 / 157.3:.3f} of the 157.3 TF fp32-matrix specification")
        if t1:
            lines.append(f"  sm_knn_topk alone (splits = 1): {_fmt(t1)}  {statistics.median(t1) / ms:.2f}x auto")
        lines.append(f"  rows with identical idx in both paths: {same:.4f}; top1 fused {a['top1']} reference {b['top1']}")
        lines.append(f"  fused is {'FASTER' if mf < mr else 'NOT faster'} than the eager reference here")
        del zq, zb, rq, rb, a, b
        torch.cuda.empty_cache()
    lines.append(_copy_calibration(rounds)[0])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def blur(out_path=None, N=2048, reps=10, rounds=5):
    """sm_frames_box_blur at k = 15, 31, 51 on 2048 frames of 240x320 with one 96x96 box each, the
    same frames with no boxes (the launch then reserves no LDS) and with one box in frame 0 only (the
    same copy work under the blur tiles' LDS reservation), and 2048 frames of 112^2 with one 48x48 box; alternating in every
    round with a plain device copy of the same bytes (out.copy_(packed)) and with the same result
    from eager torch ops on the device (fp32 frames, reflect padding, separable conv2d, torch.where
    on a box mask, round, to uint8).  GB/s over bytes read plus written (2 x the packed bytes).  The
    statistics launch (memset + sm_box_region_stats) is timed as well.  Ends with the 4.9 GB copy
    calibration.  No target is asserted: what is measured is written down.  Agreement with
    OpenCV's own 8-bit GaussianBlur is NOT measured (no OpenCV here)."""
    import statistics
    import torch.nn.functional as Fn
    from ssl_mae_amd.visual_privacy import gaussian_weights
    dev = torch.device("cuda")
    lines = [f"device: {torch.cuda.get_device_name(0)}; N={N} frames; {rounds} rounds of {reps} launches, alternating, "
             "median [min .. max]; GB = bytes read + written = 2 x packed bytes"]
    print(lines[0], flush=True)

    def emit(line):                                     # every line as it is measured: a long run shows progress
        lines.append(line)
        print(line, flush=True)

    g = torch.Generator(device="cuda").manual_seed(0)
    # boxed: how many of the N frames own a box.  0 boxes: the launch reserves no LDS; 1 box (frame 0): the
    # same copy work with the blur tiles' LDS reserved, which isolates what that reservation costs the copy tiles
    for H, W, bs, boxed in ((240, 320, 96, N), (240, 320, 96, 0), (240, 320, 96, 1), (112, 112, 48, N)):
        src = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        packed = src.view(-1)
        out = torch.empty_like(packed)
        out2 = torch.empty_like(packed)
        desc = torch.tensor([[n * H * W * 3, H, W] for n in range(N)], device=dev)
        xy = [((37 * n) % (W - bs), (23 * n) % (H - bs)) for n in range(N)]
        xy = xy[:boxed]
        boxes = torch.tensor([[x, y, bs, bs] for x, y in xy], dtype=torch.int32, device=dev).view(-1, 4)
        start = torch.clamp(torch.arange(N + 1, dtype=torch.int32, device=dev), max=boxed)
        mask = torch.zeros((N, 1, H, W), dtype=torch.bool, device=dev)
        for n, (x, y) in enumerate(xy):
            mask[n, :, y:y + bs, x:x + bs] = True
        gb = 2 * packed.numel() / 1e9
        what = {N: f"one {bs}x{bs} box each", 0: "no boxes (no LDS reserved)",
                1: f"one {bs}x{bs} box in frame 0 only (LDS reserved, every other tile copies)"}[boxed]
        emit(f"{N} frames of {H}x{W}, {what} ({gb:.3f} GB per launch):")

        def k_copy():
            out2.copy_(packed)

        for k in (15, 31, 51):
            w = gaussian_weights(k)
            r = (k - 1) // 2
            wt = torch.from_numpy(w).to(dev)
            wh, wv = wt.view(1, 1, 1, k).repeat(3, 1, 1, 1), wt.view(1, 1, k, 1).repeat(3, 1, 1, 1)

            def k_blur():
                K.frames_box_blur(packed, desc, boxes, start, w, H, W, out=out)

            def eager(chunk=256):
                res = []
                for i in range(0, N, chunk):
                    x = src[i:i + chunk].permute(0, 3, 1, 2).float()
                    y = Fn.conv2d(Fn.pad(x, (r, r, 0, 0), mode="reflect"), wh, groups=3)
                    y = Fn.conv2d(Fn.pad(y, (0, 0, r, r), mode="reflect"), wv, groups=3)
                    y = torch.where(mask[i:i + chunk], y.round().clamp_(0, 255), x)
                    res.append(y.to(torch.uint8).permute(0, 2, 3, 1))
                return torch.cat(res)

            for fn in (k_blur, k_copy):                 # warm-up: code objects, allocator
                for _ in range(3):
                    fn()
            ref = eager()
            torch.cuda.synchronize()
            d = (ref.reshape(-1).int() - out.int()).abs()
            diff, frac = int(d.max()), float((d > 0).float().mean())
            del ref, d
            tb, tc, te = [], [], []
            for _ in range(rounds):                     # alternate the three paths
                tb += _rounds(k_blur, reps, 1)
                tc += _rounds(k_copy, reps, 1)
                te += _rounds(eager, 1, 1)
            mb, mc, me = statistics.median(tb), statistics.median(tc), statistics.median(te)
            emit(f"  k={k}: sm_frames_box_blur {_fmt(tb)}  {gb / mb * 1e3:.0f} GB/s; out.copy_(packed) {_fmt(tc)}  "
                         f"{gb / mc * 1e3:.0f} GB/s; blur / copy time: {mb / mc:.2f}")
            emit(f"        eager torch ops (float, pad, conv2d x 2, where, round, uint8): {_fmt(te)}  {me / mb:.1f}x "
                         f"the kernel; max |eager - kernel| = {diff} grey levels, {frac:.2e} of the bytes differ")
            torch.cuda.empty_cache()
        stats = torch.empty((N, 4), dtype=torch.int64, device=dev)

        def k_stats():
            K.box_region_stats(packed, out, desc, boxes, start, H, W, stats=stats)

        k_stats()
        ts = _rounds(k_stats, reps, rounds)
        emit(f"  sm_box_region_stats (memset + launch, original against the k=51 result): {_fmt(ts)}; "
                     f"box pixels per frame {stats[:, 0].float().mean().item():.0f}")
        del src, packed, out, out2, mask
        torch.cuda.empty_cache()
    emit(_copy_calibration(rounds)[0])
    emit("agreement with OpenCV's 8-bit cv2.GaussianBlur: NOT MEASURED (no OpenCV on this system)")
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def mix(out_path=None, B=256, T=8, reps=10, rounds=5, seed=0):
    """sm_clip_mix on a [B,3,T,S,S] fp32 batch at S = 112 and 224, with mae_loader.ClipMixer's draws at
    a fixed seed for all-Mixup pairs (cutmix_alpha 0) and all-CutMix pairs (mixup_alpha 0), out of
    place; alternating in every round with out.copy_(x) of the same tensor (the kernel moves the same
    bytes: every element read once and written once) and with the same result from eager torch ops
    on the device (x * lam + x.flip(0) * (1 - lam), then torch.where on the pairs' box mask).  GB =
    bytes read + written = 2 x the tensor.  Then the device operations one ClipMixer call adds to a
    training step, from torch.profiler's trace, and the 4.9 GB copy calibration.  No target is
    asserted: what is measured is written down."""
    import statistics
    from ssl_mae_amd.mae_loader import ClipMixer
    dev = torch.device("cuda")
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    emit(f"device: {torch.cuda.get_device_name(0)}; B={B} T={T}; draws: ClipMixer(seed={seed}); {rounds} rounds of "
         f"{reps} launches, alternating, median [min .. max]; GB = bytes read + written = 2 x the tensor")
    g = torch.Generator(device="cuda").manual_seed(0)
    P = B // 2
    for S in (112, 224):
        x = torch.randn((B, 3, T, S, S), device=dev, generator=g)
        out, out2 = torch.empty_like(x), torch.empty_like(x)
        gb = 2 * x.numel() * 4 / 1e9
        emit(f"[{B},3,{T},{S},{S}] fp32 ({gb:.3f} GB per launch):")

        def k_copy():
            out2.copy_(x)

        for what, kw in (("all Mixup", {"cutmix_alpha": 0.0}), ("all CutMix", {"mixup_alpha": 0.0})):
            lam_px, box, weight = ClipMixer(seed=seed, **kw).draw(B, S, S)
            lam_d, box_d = lam_px.to(dev), box.to(dev)
            lam_b = torch.cat([lam_px, lam_px.flip(0)]).to(dev).view(B, 1, 1, 1, 1)
            mask = torch.zeros((B, 1, 1, S, S), dtype=torch.bool, device=dev)
            for p, (y0, x0, h, w) in enumerate(box.tolist()):
                mask[p, ..., y0:y0 + h, x0:x0 + w] = True
                mask[B - 1 - p, ..., y0:y0 + h, x0:x0 + w] = True

            def k_mix():
                K.clip_mix(x, lam_d, box_d, out=out)

            def eager():
                xf = x.flip(0)
                return torch.where(mask, xf, x * lam_b + xf * (1 - lam_b))

            for fn in (k_mix, k_copy, eager):             # warm-up: code objects, allocator
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            diff = float((eager() - out).abs().max())
            tm, tc, te = [], [], []
            for _ in range(rounds):                       # alternate the three paths
                tm += _rounds(k_mix, reps, 1)
                tc += _rounds(k_copy, reps, 1)
                te += _rounds(eager, 2, 1)
            mm, mc, me = statistics.median(tm), statistics.median(tc), statistics.median(te)
            area = sum(h * w for _, _, h, w in box.tolist()) / max(P, 1) / (S * S)
            emit(f"  {what} (mean label weight {float(weight.mean()):.3f}, mean box {area:.3f} of the frame): sm_clip_mix "
                 f"{_fmt(tm)}  {gb / mm * 1e3:.0f} GB/s; out.copy_(x) {_fmt(tc)}  {gb / mc * 1e3:.0f} GB/s; "
                 f"mix / copy time: {mm / mc:.3f}")
            emit(f"      eager torch ops (flip, two products, sum, where): {_fmt(te)}  {me / mm:.1f}x the kernel; "
                 f"max |eager - kernel| = {diff:.2e}")
            torch.cuda.empty_cache()
        del x, out, out2
        torch.cuda.empty_cache()
    clip = torch.randn((8, 3, T, 112, 112), device=dev, generator=g)
    label = torch.arange(8, device=dev)
    mixer = ClipMixer(seed=seed)
    try:
        emit(f"device operations one ClipMixer call adds to a step (torch.profiler's trace: kernels, memsets, copies): "
             f"{_count_launches(lambda: mixer(clip, label))} = the table's upload, sm_clip_mix, and label.flip(0) for the "
             "partner labels")
    except Exception as exc:  # the trace is a cross-check, not the measurement
        emit(f"device operations one ClipMixer call adds to a step: not measured ({type(exc).__name__}); by construction "
             "the table's upload, sm_clip_mix, and label.flip(0) for the partner labels")
    emit(_copy_calibration(rounds)[0])
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("resize", "crop", "fedround", "finetune", "fed_dp", "fed_q8", "knn", "blur",
                                             "mix"):
        out = sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--out" else None
        {"resize": resize, "crop": crop, "fedround": fedround, "finetune": finetune, "fed_dp": fed_dp, "fed_q8": fed_q8,
         "knn": knn, "blur": blur, "mix": mix}[sys.argv[1]](out)
    else:
        main()
        frames()

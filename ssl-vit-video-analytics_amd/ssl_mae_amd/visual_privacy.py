"""Visual privacy: blur what lies inside given boxes of decoded frames on the GPU, and measure what
the blur removed there (the anonymisation half of the reference's src/run_privacy.py:118-226
run_visual_privacy and src/privacy/visual_anonymizer.py, MI355X-native).

The reference detects faces with YuNet and blurs each box with cv2.GaussianBlur on the host.  This
build takes the boxes from a file (detection is somebody else's model) and runs the pixel work as
two launches per batch of frames: sm_frames_box_blur and sm_box_region_stats
(csrc/anonymize.hip, specified in include/sm_api.h).  There is no OpenCV here and no download; PIL
reads and writes the files.

The blurred frames keep the packed layout mae_loader.collate_raw / ClipResizer consume (frame_desc
expands clip descriptors to frame rows), so an anonymised clip can go straight into
sm_frames_resize_normalize.

The reference's detector-dependent CSV columns (frames_with_face_after, avg_faces_after, the face
frame rates, flr_conditional, per_relative) are absent: no detector runs, so nothing can be detected
after the blur.  The columns here say how much was blurred (box_pixel_fraction), how far the boxes'
pixels moved (psnr_box_db) and how much local detail survived (detail_retained, the ratio of the
squared neighbour differences after / before inside the boxes).

Two deviations of the blur from the reference are documented in include/sm_api.h: boxes closer than
the kernel radius are blurred from the original frame (the reference's loop blurs already-blurred
pixels), and OpenCV's 8-bit Gaussian is fixed-point where this one is fp32; agreement with OpenCV's
own output is expected within one grey level and is not measured.
"""
import math
import random
from pathlib import Path

import numpy as np
import torch

from . import kernels as K
from ._lib import KernelError

IMAGE_EXTENSIONS = (".jpg", ".jpeg", ".png")
CSV_COLUMNS = ("frame_root", "total_frames", "frames_with_box", "avg_boxes", "box_pixel_fraction", "blur_kernel",
               "psnr_box_db", "detail_retained", "seconds", "overwrite_saved_root")
CSV_HEADER = ",".join(CSV_COLUMNS) + "\n"


def odd_kernel(ksize):
    """An even kernel becomes ksize + 1 (visual_anonymizer.py: blur_kernel | 1)."""
    k = int(ksize)
    return k + 1 if k % 2 == 0 else k


def gaussian_sigma(ksize):
    """OpenCV's rule for sigma <= 0: 0.3 ((ksize - 1) / 2 - 1) + 0.8."""
    return 0.3 * ((odd_kernel(ksize) - 1) * 0.5 - 1) + 0.8


def gaussian_weights(ksize):
    """-> fp32 [ksize]: w_i = exp(-(i - r)^2 / (2 sigma^2)) in float64, normalised to sum 1, then
    rounded to fp32 (cv2.getGaussianKernel(ksize, 0) for ksize above its small fixed tables)."""
    k = odd_kernel(ksize)
    if k < 1:
        raise ValueError(f"[ERROR] blur kernel {ksize} must be positive")
    r, sigma = (k - 1) // 2, gaussian_sigma(k)
    w = np.exp(-((np.arange(k, dtype=np.float64) - r) ** 2) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def read_boxes(path):
    """Text lines `relative/path.jpg,x,y,w,h` -> {relative posix path: [(x, y, w, h), ...]}.  Blank
    lines, `#` comments and an optional header line `path,x,y,w,h` are skipped; a malformed line
    raises ValueError naming its line number."""
    out = {}
    with open(path, encoding="utf-8") as f:
        for ln, line in enumerate(f, 1):
            s = line.strip()
            if not s or s.startswith("#"):
                continue
            parts = [p.strip() for p in s.split(",")]
            if [p.lower() for p in parts] == ["path", "x", "y", "w", "h"]:
                continue
            try:
                if len(parts) != 5 or not parts[0]:
                    raise ValueError
                box = tuple(int(p) for p in parts[1:])
                if any(abs(v) >= 2 ** 31 for v in box):
                    raise ValueError
            except ValueError:
                raise ValueError(f"[ERROR] {path}: line {ln} is not `path,x,y,w,h` with integer x, y, w, h: "
                                 f"{s!r}") from None
            out.setdefault(Path(parts[0].replace("\\", "/")).as_posix(), []).append(box)
    return out


def scan_images(root, max_images, seed):
    """The reference's rule (run_privacy.py scan_images): .jpg / .jpeg / .png below root, found
    recursively and sorted, then random.Random(seed).sample when there are more than max_images."""
    root = Path(root)
    if not root.exists():
        raise FileNotFoundError(f"[ERROR] frame_root not found: {root}")
    files = sorted(p for p in root.rglob("*") if p.is_file() and p.suffix.lower() in IMAGE_EXTENSIONS)
    if not files:
        raise RuntimeError(f"[ERROR] No image files found under: {root}")
    if len(files) > int(max_images):
        files = random.Random(int(seed)).sample(files, int(max_images))
    return files


def pack_frames(frames):
    """list of uint8 [H,W,3] (numpy or torch) -> (packed uint8 1-D, desc int64 [N,3] = {byte
    offset, H, W}), frames back to back."""
    desc = torch.zeros(len(frames), 3, dtype=torch.int64)
    parts, off = [], 0
    for n, fr in enumerate(frames):
        t = torch.as_tensor(np.ascontiguousarray(fr) if isinstance(fr, np.ndarray) else fr)
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3:
            raise ValueError(f"pack_frames takes uint8 [H,W,3] frames, got {t.dtype} {tuple(t.shape)}")
        desc[n] = torch.tensor([off, t.shape[0], t.shape[1]])
        parts.append(t.contiguous().view(-1))
        off += parts[-1].numel()
    packed = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8)
    return packed, desc


def frame_desc(desc_clips, T):
    """collate_raw's clip descriptors int64 [B,4] (or [B,8]) = {byte offset, Hs, Ws, flags, ...} ->
    per-frame rows int64 [B*T,3]: frame t of clip b starts Hs Ws 3 t bytes into the clip.  The
    frames of an invalid clip get H = W = 0 (no bytes; every consumer skips them)."""
    from .mae_loader import FLAG_INVALID
    if desc_clips.dtype != torch.int64 or desc_clips.dim() != 2 or desc_clips.shape[1] not in (4, 8):
        raise ValueError("frame_desc takes an int64 [B,4] or [B,8] clip descriptor")
    T = int(T)
    d = desc_clips[:, :4]
    ok = (d[:, 3] & FLAG_INVALID) == 0
    h, w = d[:, 1] * ok, d[:, 2] * ok
    t = torch.arange(T, dtype=torch.int64).view(1, T)
    off = d[:, 0:1] + (h * w * 3).view(-1, 1) * t
    return torch.stack([off, h.view(-1, 1).expand(-1, T), w.view(-1, 1).expand(-1, T)], dim=2).reshape(-1, 3)


def box_arrays(boxes_per_frame):
    """[[(x, y, w, h), ...] per frame] -> (boxes int32 [num_boxes,4], box_start int32 [N+1])."""
    flat, start = [], [0]
    for bs in boxes_per_frame:
        flat.extend(tuple(int(v) for v in b) for b in bs)
        start.append(len(flat))
    boxes = torch.tensor(flat, dtype=torch.int32).view(-1, 4)
    return boxes, torch.tensor(start, dtype=torch.int32)


def clip_box(box, H, W):
    """The kernel's clipping rule on the host -> (x0, y0, x1, y1) or None when empty."""
    x, y, w, h = box
    if w <= 0 or h <= 0:
        return None
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else None


class BoxBlur:
    """Packed host frames + boxes -> the blurred packed frames in HBM: one H2D copy of the pixels,
    one each of the descriptors and boxes, one launch (sm_frames_box_blur); `with_stats` adds
    sm_box_region_stats of (original, blurred).  More frames than one launch's grid takes
    (kernels.box_launch_max_frames) are split over several launches into the same output."""

    def __init__(self, ksize, device="cuda", max_frames_per_launch=None):
        self.ksize = odd_kernel(ksize)
        if not 3 <= self.ksize <= K.BOX_MAX_KSIZE:
            raise ValueError(f"[ERROR] blur kernel {ksize} is outside [3, {K.BOX_MAX_KSIZE}]")
        self.weights = gaussian_weights(self.ksize)
        self.device = torch.device(device)
        self.max_frames_per_launch = max_frames_per_launch

    @staticmethod
    def check(packed, desc, boxes_per_frame=None):
        """Host-side validation (the kernel bound-checks as well and skips the frame; a bad
        descriptor here is a caller's bug): sizes within limits, byte ranges inside the buffer,
        no two frames overlapping.  A row with H = W = 0 is an absent frame."""
        if packed.dtype != torch.uint8 or packed.dim() != 1:
            raise KernelError("packed must be a 1-D uint8 tensor")
        if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 3:
            raise KernelError("desc must be an int64 [N,3] tensor")
        if boxes_per_frame is not None and len(boxes_per_frame) != desc.shape[0]:
            raise KernelError(f"{len(boxes_per_frame)} box lists for {desc.shape[0]} frames")
        n, spans = packed.numel(), []
        for i, (off, h, w) in enumerate(desc.tolist()):
            if h == 0 and w == 0:
                continue
            if not (1 <= h <= K.BOX_MAX_SIDE and 1 <= w <= K.BOX_MAX_SIDE):
                raise KernelError(f"frame {i}: size {h}x{w} is outside [1, {K.BOX_MAX_SIDE}]")
            if off < 0 or off + h * w * 3 > n:
                raise KernelError(f"frame {i}: bytes [{off}, {off + h * w * 3}) leave the packed buffer of {n} bytes")
            spans.append((off, off + h * w * 3, i))
        spans.sort()
        for (_, e0, i0), (s1, _, i1) in zip(spans, spans[1:]):
            if s1 < e0:
                raise KernelError(f"frames {i0} and {i1} overlap in the packed buffer")

    def __call__(self, packed, desc, boxes_per_frame, with_stats=False):
        self.check(packed, desc, boxes_per_frame)
        N = desc.shape[0]
        p = packed.to(self.device, non_blocking=True).contiguous()
        out = torch.zeros_like(p)
        stats = torch.zeros((N, 4), dtype=torch.int64, device=self.device)
        if N:
            max_h, max_w = max(1, int(desc[:, 1].max())), max(1, int(desc[:, 2].max()))
            d = desc.to(self.device, non_blocking=True).contiguous()
            boxes, start = box_arrays(boxes_per_frame)
            boxes, start = boxes.to(self.device, non_blocking=True), start.to(self.device, non_blocking=True)
            step = int(self.max_frames_per_launch or K.box_launch_max_frames(max_h, max_w))
            for i in range(0, N, step):              # box_start holds absolute box indices: slices share `boxes`
                j = min(i + step, N)
                K.frames_box_blur(p, d[i:j], boxes, start[i:j + 1], self.weights, max_h, max_w, out=out)
                if with_stats:
                    K.box_region_stats(p, out, d[i:j], boxes, start[i:j + 1], max_h, max_w, stats=stats[i:j])
        return (out, stats) if with_stats else out


def summarise(stats, sizes, num_boxes):
    """stats rows (P, SSE, Ea, Eb), sizes (H, W) and the box count per frame -> the CSV's measured
    columns (unrounded; psnr_box_db is None without box pixels and inf without a difference)."""
    P = sum(int(s[0]) for s in stats)
    sse, ea, eb = (sum(int(s[k]) for s in stats) for k in (1, 2, 3))
    n = len(sizes)
    pixels = sum(int(h) * int(w) for h, w in sizes)
    if P == 0:
        psnr = None
    elif sse == 0:
        psnr = math.inf
    else:
        psnr = 10.0 * math.log10(255.0 ** 2 / (sse / (3.0 * P)))
    return {"total_frames": n, "frames_with_box": sum(1 for s in stats if int(s[0]) > 0),
            "avg_boxes": sum(int(b) for b in num_boxes) / max(1, n),
            "box_pixel_fraction": P / pixels if pixels else 0.0, "psnr_box_db": psnr,
            "detail_retained": eb / ea if ea else 0.0}


def format_row(row):
    """One CSV line: floats rounded to 6 places, a missing PSNR empty, an infinite one `inf`."""
    vals = []
    for c in CSV_COLUMNS:
        v = row[c]
        if v is None:
            vals.append("")
        elif isinstance(v, float):
            vals.append("inf" if math.isinf(v) else str(round(v, 6)))
        else:
            vals.append(str(v))
    return ",".join(vals) + "\n"


def synthetic_frames(count, seed, hw=(240, 320)):
    """`count` uint8 frames of `hw` from the seeded torch generator, with one or two deterministic
    boxes each: the stage runs without data, like every other driver."""
    g = torch.Generator().manual_seed(int(seed))
    H, W = hw
    frames = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).numpy() for _ in range(count)]
    boxes = []
    for i in range(count):
        bs = [((37 * i) % (W - 96), (23 * i) % (H - 96), 96, 96)]
        if i % 2:
            bs.append(((53 * i + 40) % (W - 48), (31 * i + 20) % (H - 48), 48, 48))
        boxes.append(bs)
    return frames, boxes


def example_grid(pairs, cols=4):
    """[(before, after) uint8 [H,W,3]] -> one uint8 image: rows of `cols` pairs, before above after,
    every frame resized with PIL to the first one's size (run_privacy.py save_visual_examples)."""
    from PIL import Image
    h, w = pairs[0][0].shape[:2]

    def fit(a):
        return a if a.shape[:2] == (h, w) else np.asarray(Image.fromarray(a).resize((w, h), Image.BILINEAR))

    rows = []
    for i in range(0, len(pairs), cols):
        chunk = [(fit(a), fit(b)) for a, b in pairs[i:i + cols]]
        chunk += [(np.zeros((h, w, 3), np.uint8),) * 2] * (cols - len(chunk) if rows else 0)
        rows.append(np.concatenate([np.concatenate([p[0] for p in chunk], axis=1),
                                    np.concatenate([p[1] for p in chunk], axis=1)], axis=0))
    return np.concatenate(rows, axis=0)

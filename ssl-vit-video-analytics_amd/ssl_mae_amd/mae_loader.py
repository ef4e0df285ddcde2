"""Clip loading and tube masking (reference: src/datasets/mae_loader.py).

LazyVideoMAEDataset (mae_loader.py:7-78) keeps the reference's constructor,
split-file parsing, sorted-*.jpg listing, frame-index rule (global numpy RNG),
black replacement frame for an unreadable file and zero clip for a missing or
empty directory.  What changes is where the per-pixel work runs:

  * transform=None (the MI355X path): __getitem__ returns the decoded uint8 frames
    [T,H,W,3] and a validity flag; `collate_frames` stacks a batch and
    `ClipNormalizer` ships it to HBM in ONE uint8 copy (1/4 of the fp32 bytes) and
    runs sm_frames_normalize, which applies the reference's transform
    (train_ssl_mae.py:137-141: /255, ImageNet mean/std) and its BGR channel swap
    (mae_loader.py:70-71) and lays the batch out as [B,3,T,H,W] fp32 — bit-identical
    to the reference's collated CPU clip;
  * transform=callable: the reference's behaviour verbatim (the callable runs per
    frame, then img[[2,1,0]] on tensors, stack, permute) — user code, on the host.

Frames that are not already `image_size` (a 112² frame store feeding a 224² model, a
dataset kept at its native 240x320) take `collate_raw` + `ClipResizer` instead of
`collate_frames` + `ClipNormalizer`: the batch is packed into one flat uint8 buffer with
a descriptor row {byte offset, Hs, Ws, flags} per clip, and sm_frames_resize_normalize
resizes (bilinear, align_corners=False, the rule of src/datasets/mae_dataset.py:84-90),
flips and normalises every clip in one launch.  A clip already at `image_size` comes out
bit-identical to the ClipNormalizer path, so the drivers use this path for every split.
`RandomResizedCropFlip` turns that launch into the training augmentation: it draws one source
window and one flip per clip on the host (every frame of a clip gets the same crop) and widens
the descriptor to {byte offset, Hs, Ws, flags, y0, x0, Hc, Wc}, which ClipResizer hands to
sm_frames_crop_resize_normalize: still one copy and one launch, the crop costs no pixel work on
the host.  The reference has no augmentation (src/datasets/transforms.py).
Deviation: the reference's supervised loaders resize with cv2.resize
(src/datasets/transforms.py:9-15), whose bilinear filter works in fixed-point uint8
arithmetic.  OpenCV is not available to pin that arithmetic against, so every loader here
gets the F.interpolate rule; the difference (cv2 rounds the interpolated value back to
uint8) has not been measured.

get_tube_mask (mae_loader.py:80-90) keeps the reference's signature and RNG stream:
the per-sample noise is drawn on the host from torch's global CPU generator exactly
as the reference draws it (B calls of torch.rand(L) == torch.rand(B, L)); the
ranking, the [B,T,L] expansion and the row-major compaction of masked token
indices run in one HIP kernel (sm_tube_mask).  The result is a bool tensor on the
GPU (the reference's `.to(device)` is then a no-op).  The kernel breaks ties in the
noise by lower index first, while the reference takes torch's CPU
`argsort(descending=True)`, which is not stable for L > 16.  The two can differ only
where equal noise values straddle the int(r*L) cut (~2e-5 per sample at L=784), and
the host removes exactly that case before the copy (`resolve_cut_ties`): one row sort
of the batch's noise in numpy (~0.5 ms at B=256, L=784) finds the samples whose
n_mask-th and (n_mask+1)-th largest values are equal, and for those samples only the
noise row is replaced by distinct values in the order of the reference's own
`torch.argsort(noise[b], descending=True)`.  The kernel's ranking then reproduces the
reference's selection by construction.
"""
import math
import os

import numpy as np
import torch

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class LazyVideoMAEDataset(torch.utils.data.Dataset):
    """mae_loader.py:7-78 (see the module docstring for the transform=None path)."""

    def __init__(self, split_file, clip_len=32, stride=2, image_size=112, transform=None):
        self.clip_len = clip_len
        self.stride = stride
        self.image_size = image_size
        self.transform = transform
        self.samples = []
        if not os.path.exists(split_file):
            raise FileNotFoundError(f"Index file not found: {split_file}")
        with open(split_file, "r") as f:
            for line in f:
                parts = line.strip().split()
                if parts:
                    self.samples.append(parts[0])

    def __len__(self):
        return len(self.samples)

    def _load_frame(self, frame_path):
        from PIL import Image
        try:
            return Image.open(frame_path).convert("RGB")
        except Exception:
            return Image.new("RGB", (self.image_size, self.image_size), (0, 0, 0))

    def _load_raw(self, video_dir, paths):
        """The transform=None clip: uint8 [T,Hs,Ws,3] at the frames' own size.  An unreadable
        frame is black at that size (image_size when no frame of the clip can be read), so it
        resizes to exactly the normalised black frame the reference substitutes."""
        from PIL import Image
        frames = []
        for p in paths:
            try:
                frames.append(np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8))
            except Exception:
                frames.append(None)
        shapes = sorted({f.shape for f in frames if f is not None})
        if len(shapes) > 1:
            raise ValueError(f"frames of {video_dir} differ in size ({', '.join(f'{h}x{w}' for h, w, _ in shapes)}): "
                             "one clip must have one frame size")
        shape = shapes[0] if shapes else (self.image_size, self.image_size, 3)
        black = np.zeros(shape, dtype=np.uint8)
        return torch.from_numpy(np.stack([black if f is None else f for f in frames]))

    def _indices(self, total):
        window = self.clip_len * self.stride
        if total < window:
            idx = np.linspace(0, total - 1, self.clip_len).astype(int)
        else:
            start = np.random.randint(0, total - window + 1)
            idx = np.arange(start, start + window, self.stride)
        return idx[:self.clip_len]

    def _empty(self):
        if self.transform is None:
            s = self.image_size
            return torch.zeros(self.clip_len, s, s, 3, dtype=torch.uint8), False
        return torch.zeros(3, self.clip_len, self.image_size, self.image_size)

    def __getitem__(self, index):
        video_dir = self.samples[index]
        if not os.path.exists(video_dir):
            return self._empty()
        names = sorted(f for f in os.listdir(video_dir) if f.endswith(".jpg"))
        if not names:
            return self._empty()
        paths = [os.path.join(video_dir, names[i]) for i in self._indices(len(names))]
        if self.transform is None:
            return self._load_raw(video_dir, paths), True
        imgs = [self._load_frame(p) for p in paths]
        clip = []
        for img in imgs:
            img = self.transform(img)
            if isinstance(img, torch.Tensor):
                img = img[[2, 1, 0], :, :]
            clip.append(img)
        return torch.stack(clip).permute(1, 0, 2, 3)


def collate_frames(batch):
    """DataLoader collate for transform=None items: (uint8 [B,T,H,W,3], bool [B])."""
    frames = torch.stack([f for f, _ in batch])
    valid = torch.tensor([bool(v) for _, v in batch], dtype=torch.bool)
    return frames, valid


class ClipNormalizer:
    """Host frames -> normalised fp32 clip [B,3,T,H,W] in HBM (sm_frames_normalize)."""

    def __init__(self, mean=IMAGENET_MEAN, std=IMAGENET_STD, bgr_swap=True, device="cuda"):
        self.mean, self.std, self.bgr_swap, self.device = tuple(mean), tuple(std), bgr_swap, torch.device(device)

    def __call__(self, frames, valid=None):
        f = frames.to(self.device, non_blocking=True)
        v = None if valid is None else valid.to(self.device, non_blocking=True)
        return K.frames_normalize(f.contiguous(), self.mean, self.std, self.bgr_swap, v)


FLAG_FLIP, FLAG_INVALID = 1, 2     # desc[b, 3] of sm_frames_resize_normalize
MAX_SOURCE_SIDE = 8192


def collate_raw(batch):
    """DataLoader collate for clips that keep their own frame size.  Items are
    (uint8 [T,Hs,Ws,3], valid) or (frames, valid, flip); returns (packed uint8 1-D, desc
    int64 [B,4] = {byte offset, Hs, Ws, flags}).  An invalid item contributes no bytes."""
    desc = torch.zeros(len(batch), 4, dtype=torch.int64)
    parts, off, clip_len = [], 0, None
    for b, item in enumerate(batch):
        frames, valid = item[0], item[1]
        flip = bool(item[2]) if len(item) > 2 else False
        desc[b, 0] = off
        if not valid:
            desc[b, 3] = FLAG_INVALID
            continue
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"collate_raw takes uint8 [T,H,W,3] frames, got {frames.dtype} {tuple(frames.shape)}")
        if clip_len is None:
            clip_len = frames.shape[0]
        elif frames.shape[0] != clip_len:
            raise ValueError(f"clips of one batch must have one length ({clip_len} and {frames.shape[0]} frames)")
        desc[b, 1], desc[b, 2], desc[b, 3] = frames.shape[1], frames.shape[2], FLAG_FLIP if flip else 0
        parts.append(frames.contiguous().view(-1))
        off += parts[-1].numel()
    packed = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8)
    return packed, desc


class RandomResizedCropFlip:
    """Clip-consistent random-resized crop and horizontal flip for ClipResizer: `windows` maps
    collate_raw's desc [B,4] to desc [B,8] = {byte offset, Hs, Ws, flags, y0, x0, Hc, Wc}, one
    window and one flip decision per clip.  A pure host function of the descriptor and of this
    object's own generator, called in the main process after collation, so a run does not depend
    on num_workers.

    The usual rule, per valid clip: up to TRIES tries of area = Hs * Ws * U(scale),
    ar = exp(U(log ratio[0], log ratio[1])), w = round(sqrt(area * ar)), h = round(sqrt(area / ar));
    the first try with 1 <= w <= Ws and 1 <= h <= Hs is taken and y0, x0 are uniform over the
    positions that keep the window inside the frame.  When no try fits, the window is the centred
    largest one whose aspect Ws / Hs is clamped to `ratio`.  FLAG_FLIP is set with probability
    `flip`.  An invalid clip keeps its flags and gets a zero window.

    Order of the draws: every call makes ONE draw, u = torch.rand(B, 2 * TRIES + 3, float64), from
    the generator; row b belongs to clip b whether or not it is valid and whatever it accepts, so
    the stream does not depend on the data.  u[b, 2 i] is try i's area, u[b, 2 i + 1] its aspect,
    then come y0 (floor(u * (Hs - h + 1))), x0 (floor(u * (Ws - w + 1))) and the flip (u < flip).
    `last_fallback` lists, for the last call, whether each clip took the fallback."""

    TRIES = 10

    def __init__(self, scale=(0.35, 1.0), ratio=(3 / 4, 4 / 3), flip=0.5, seed=0):
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        self.flip = float(flip)
        if not 0.0 < self.scale[0] <= self.scale[1] <= 1.0:
            raise ValueError(f"RandomResizedCropFlip needs 0 < scale[0] <= scale[1] <= 1, got {scale}")
        if not 0.0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError(f"RandomResizedCropFlip needs 0 < ratio[0] <= ratio[1], got {ratio}")
        if not 0.0 <= self.flip <= 1.0:
            raise ValueError(f"RandomResizedCropFlip needs flip within [0, 1], got {flip}")
        self.gen = torch.Generator().manual_seed(int(seed))
        self.last_fallback = []

    def _fallback(self, hs, ws):
        in_ratio = ws / hs
        h, w = hs, ws
        if in_ratio < self.ratio[0]:
            h = min(hs, max(1, math.floor(ws / self.ratio[0] + 0.5)))
        elif in_ratio > self.ratio[1]:
            w = min(ws, max(1, math.floor(hs * self.ratio[1] + 0.5)))
        return (hs - h) // 2, (ws - w) // 2, h, w

    def windows(self, desc):
        if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] != 4:
            raise ValueError("RandomResizedCropFlip.windows takes an int64 [B,4] descriptor")
        B = desc.shape[0]
        u = torch.rand(B, 2 * self.TRIES + 3, dtype=torch.float64, generator=self.gen).tolist()
        log_r = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        out = torch.zeros(B, 8, dtype=torch.int64)
        out[:, :4] = desc
        self.last_fallback = [False] * B
        for b, (_, hs, ws, flags) in enumerate(desc.tolist()):
            if flags & FLAG_INVALID or hs < 1 or ws < 1:
                continue
            ub, win = u[b], None
            for i in range(self.TRIES):
                area = hs * ws * (self.scale[0] + (self.scale[1] - self.scale[0]) * ub[2 * i])
                ar = math.exp(log_r[0] + (log_r[1] - log_r[0]) * ub[2 * i + 1])
                w, h = math.floor(math.sqrt(area * ar) + 0.5), math.floor(math.sqrt(area / ar) + 0.5)
                if 1 <= w <= ws and 1 <= h <= hs:
                    y0 = min(int(ub[2 * self.TRIES] * (hs - h + 1)), hs - h)
                    x0 = min(int(ub[2 * self.TRIES + 1] * (ws - w + 1)), ws - w)
                    win = (y0, x0, h, w)
                    break
            if win is None:
                win, self.last_fallback[b] = self._fallback(hs, ws), True
            out[b, 4:] = torch.tensor(win)
            if ub[2 * self.TRIES + 2] < self.flip:
                out[b, 3] = flags | FLAG_FLIP
        return out


class ClipResizer:
    """Packed host frames -> resized, flipped, normalised fp32 clip [B,3,T,S,S] in HBM: one
    H2D copy of the pixels, one of the descriptors, one launch (sm_frames_resize_normalize, or
    sm_frames_crop_resize_normalize when the descriptor has a window: 8 columns)."""

    def __init__(self, image_size, mean=IMAGENET_MEAN, std=IMAGENET_STD, bgr_swap=True, device="cuda"):
        hw = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        self.out_hw = (int(hw[0]), int(hw[1]))
        self.mean, self.std, self.bgr_swap, self.device = tuple(mean), tuple(std), bgr_swap, torch.device(device)

    @staticmethod
    def check(packed, desc, T):
        """Host-side validation of the descriptors against the packed buffer (the kernel
        bound-checks as well and writes zeros; a bad descriptor here is a loader bug)."""
        from ._lib import KernelError
        if packed.dtype != torch.uint8 or packed.dim() != 1:
            raise KernelError("packed must be a 1-D uint8 tensor")
        if desc.dtype != torch.int64 or desc.dim() != 2 or desc.shape[1] not in (4, 8):
            raise KernelError("desc must be an int64 [B,4] or [B,8] tensor")
        if int(T) < 0:
            raise KernelError("the clip length must not be negative")
        n = packed.numel()
        for b, (off, hs, ws, flags, *win) in enumerate(desc.tolist()):
            if flags & FLAG_INVALID:
                continue
            if not (1 <= hs <= MAX_SOURCE_SIDE and 1 <= ws <= MAX_SOURCE_SIDE):
                raise KernelError(f"clip {b}: frame size {hs}x{ws} is outside [1, {MAX_SOURCE_SIDE}]")
            if off < 0 or off + int(T) * hs * ws * 3 > n:
                raise KernelError(f"clip {b}: bytes [{off}, {off + int(T) * hs * ws * 3}) leave the packed buffer "
                                  f"of {n} bytes")
            if win:
                y0, x0, hc, wc = win
                if y0 < 0 or x0 < 0 or hc < 1 or wc < 1 or y0 + hc > hs or x0 + wc > ws:
                    raise KernelError(f"clip {b}: window rows [{y0}, {y0 + hc}) x columns [{x0}, {x0 + wc}) is "
                                      f"empty or leaves the {hs}x{ws} frame")

    def __call__(self, packed, desc, T):
        self.check(packed, desc, T)
        p = packed.to(self.device, non_blocking=True)
        d = desc.to(self.device, non_blocking=True)
        op = K.frames_crop_resize_normalize if desc.shape[1] == 8 else K.frames_resize_normalize
        return op(p.contiguous(), d.contiguous(), int(T), self.out_hw, self.mean, self.std, self.bgr_swap)


class ClipMixer:
    """Clip-consistent Mixup / CutMix of a training batch with its own flip (clip b with clip
    B-1-b, P = B // 2 pairs; the usual batch-flip rule, the reference has no augmentation).  A host
    sampler like RandomResizedCropFlip: `mixer(clip, label)` draws one decision per pair, uploads
    ONE small table and launches sm_clip_mix out of place; nothing is read back.

    Per pair, with probability `prob` it is mixed: by CutMix with probability `switch_prob` when
    both alphas are positive, otherwise by the one whose alpha is positive.
      Mixup   lam ~ Beta(a, a) rounded to fp32, no box, lam_px = lam, label weight lam
      CutMix  lam ~ Beta(a, a); r = sqrt(1 - lam), ch = int(H r), cw = int(W r); the centre (cy, cx)
              is uniform over the frame; y0 = clamp(cy - ch // 2, 0, H), y1 = clamp(cy + ch // 2, 0, H),
              the same for x; the box (y0, x0, y1 - y0, x1 - x0) holds the partner's pixels on every
              frame, lam_px = 1, label weight 1 - (y1 - y0) (x1 - x0) / (H W): the area actually kept
      none    lam_px = 1, no box, label weight 1
    Both clips of a pair share the box, lam_px and the weight: clip b's target is weight * label[b]
    + (1 - weight) * label[B-1-b].  The middle clip of an odd batch keeps weight 1.

    Order of the draws: every call makes TWO draws from the generator, whatever B > 1 pairs accept:
    u = torch.rand(P, 4, float64), row p = (mix?, CutMix?, cy, cx) of pair p, then one int64 that
    seeds a generator used for this call only, from which the gamma variates g [P, 2, 2] come
    (lam = g0 / (g0 + g1); g[p, 0] is the Mixup pair, g[p, 1] the CutMix pair, both always drawn).
    Gamma sampling rejects internally, so it gets a generator of its own: the main stream advances
    by the same amount per pair in every call and depends on neither the data nor the alphas.

    `last` keeps the last call's host-side draws: {"kind": ["none" | "mixup" | "cutmix"] per pair,
    "lam": the fp32 lam per pair (1.0 for none), "box": (y0, x0, h, w) per pair, "weight": the
    fp32 label weight per pair}."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, seed=0):
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        if self.mixup_alpha < 0.0 or self.cutmix_alpha < 0.0 or self.mixup_alpha + self.cutmix_alpha == 0.0:
            raise ValueError(f"ClipMixer needs alphas >= 0, not both zero, got {mixup_alpha}, {cutmix_alpha}")
        if not 0.0 <= self.prob <= 1.0 or not 0.0 <= self.switch_prob <= 1.0:
            raise ValueError(f"ClipMixer needs prob and switch_prob within [0, 1], got {prob}, {switch_prob}")
        self.gen = torch.Generator().manual_seed(int(seed))
        self.last = {"kind": [], "lam": [], "box": [], "weight": []}

    def draw(self, B, H, W):
        """The host half: -> (lam_px fp32 [P], box int32 [P,4], weight fp32 [B]) and `last`."""
        P = B // 2
        u = torch.rand(P, 4, dtype=torch.float64, generator=self.gen).tolist()
        sub = torch.Generator().manual_seed(int(torch.randint(0, 2 ** 62, (1,), generator=self.gen)))
        # an unused alpha (0) still draws, with shape 1, to keep the count fixed
        alphas = torch.tensor([self.mixup_alpha or 1.0, self.cutmix_alpha or 1.0], dtype=torch.float64)
        g = torch._standard_gamma(alphas.view(1, 2, 1).expand(P, 2, 2).contiguous(), generator=sub)
        lam_all = torch.where(g.sum(-1) > 0, g[..., 0] / g.sum(-1), torch.full((), 0.5, dtype=torch.float64))
        lam_all = lam_all.float()                                   # [P, 2] fp32: what the kernel gets
        kind, box = [], []
        lam_px, weight = torch.ones(P, dtype=torch.float32), torch.ones(B, dtype=torch.float32)
        for p, (u_mix, u_cut, u_cy, u_cx) in enumerate(u):
            k, bx = "none", (0, 0, 0, 0)
            if u_mix < self.prob:
                both = self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0
                k = "cutmix" if (u_cut < self.switch_prob if both else self.cutmix_alpha > 0.0) else "mixup"
            if k == "mixup":
                lam_px[p] = lam_all[p, 0]
                weight[p] = weight[B - 1 - p] = lam_all[p, 0]
            elif k == "cutmix":
                r = math.sqrt(1.0 - float(lam_all[p, 1]))
                ch, cw = int(H * r), int(W * r)
                cy, cx = min(int(u_cy * H), H - 1), min(int(u_cx * W), W - 1)
                y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
                x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
                bx = (y0, x0, y1 - y0, x1 - x0)
                weight[p] = weight[B - 1 - p] = 1.0 - (y1 - y0) * (x1 - x0) / (H * W)
            kind.append(k)
            box.append(bx)
        self.last = {"kind": kind, "lam": [float(lam_px[p]) if kind[p] == "mixup" else
                                           float(lam_all[p, 1]) if kind[p] == "cutmix" else 1.0 for p in range(P)],
                     "box": box, "weight": weight[:P].tolist()}
        return lam_px, torch.tensor(box, dtype=torch.int32).view(P, 4), weight

    def __call__(self, clip, label):
        """clip fp32 [B,3,T,H,W] and label int64 [B] on the device -> (mixed clip, labels_a = label,
        labels_b = label.flip(0), lam fp32 [B]: the weight of labels_a in each clip's target)."""
        from .kernels import mix_boxes_check
        B, H, W = clip.shape[0], clip.shape[-2], clip.shape[-1]
        P = B // 2
        lam_px, box, weight = self.draw(B, H, W)
        mix_boxes_check(box.tolist(), H, W)             # the table lives on the device: checked before it goes up
        table = torch.cat([box.view(-1), lam_px.view(torch.int32), weight.view(torch.int32)]).to(clip.device)
        mixed = K.clip_mix(clip.float().contiguous(), table[4 * P:5 * P].view(torch.float32), table[:4 * P].view(P, 4))
        return mixed, label, label.flip(0), table[5 * P:].view(torch.float32)


def resolve_cut_ties(noise, num_mask):
    """noise [B, L] fp32 (CPU): rows where equal values straddle the num_mask cut are
    replaced in place by distinct values ranked as the reference's
    torch.argsort(noise[b], descending=True) (mae_loader.py:86) ranks them; every other
    row is left untouched (the lower-index tie rule of sm_tube_mask cannot change
    which positions are selected there).  Returns the list of replaced rows."""
    B, L = noise.shape
    if num_mask <= 0 or num_mask >= L:
        return []
    s = np.sort(noise.numpy(), axis=1)
    rows = np.nonzero(s[:, L - num_mask] == s[:, L - num_mask - 1])[0].tolist()
    for b in rows:
        perm = torch.argsort(noise[b], descending=True)
        ranked = torch.empty(L, dtype=noise.dtype)
        ranked[perm] = torch.arange(L, 0, -1, dtype=noise.dtype)   # rank 0 -> largest
        noise[b] = ranked
    return rows


def tube_mask_from_noise(noise, num_frames, num_mask, device="cuda"):
    """noise [B, L] fp32 on the host -> (bool mask [B,T,L], int32 row-major index list) on
    `device`, selecting exactly the reference's argsort(descending)[:num_mask] per row."""
    noise = noise.clone()
    resolve_cut_ties(noise, num_mask)
    m8, idx = K.tube_mask(noise.to(device, non_blocking=True), num_frames, num_mask)
    return m8.view(torch.bool), idx


def tube_mask_with_index(batch_size, num_frames, num_patches, mask_ratio, device="cuda"):
    num_mask = int(mask_ratio * num_patches)
    noise = torch.rand(batch_size, num_patches)          # global CPU generator, reference order
    return tube_mask_from_noise(noise, num_frames, num_mask, device)


def get_tube_mask(batch_size, num_frames, num_patches, mask_ratio, device="cuda"):
    return tube_mask_with_index(batch_size, num_frames, num_patches, mask_ratio, device)[0]

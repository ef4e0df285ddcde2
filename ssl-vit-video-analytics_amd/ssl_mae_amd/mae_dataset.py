"""MAE dataset over frame-folder videos (reference: src/datasets/mae_dataset.py:20-138).

MAEVideoDataset keeps the reference's constructor, split-file parsing, LRU-cached sorted
frame listing (jpg / jpeg / png / bmp / webp), `max_start` and the clamped index rule, the
order of the draws from Python's global `random` (the start first, and only when
max_start > 0, then the flip draw; none with training=False) and the normalised zero clip
for a directory without frames.  Frames are decoded with PIL (torchvision.io.read_image
in the reference).

  * raw=False (default): the reference's item, computed on the host: u8 / 255 ->
    F.interpolate(bilinear, align_corners=False) -> clip-level horizontal flip ->
    (x - mean) / std -> fp32 [3,T,S,S], RGB order.
  * raw=True (the MI355X path): (uint8 frames [T,Hs,Ws,3], True, flip) for
    mae_loader.collate_raw; ClipResizer(image_size, mean, std, bgr_swap=False) then
    resizes, flips and normalises the whole batch in one launch
    (sm_frames_resize_normalize).  An unreadable frame is a black frame of the clip's own
    size and a directory without frames a black clip at image_size: both resize to exactly
    the (0 - mean) / std frame the reference substitutes.
"""
import os
import random
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp", ".webp")


class MAEVideoDataset(torch.utils.data.Dataset):
    """Split file: one `<frame directory> <label>` per line; the label is ignored."""

    def __init__(self, split_path, image_size=112, clip_len=32, stride=4, mean=(0.485, 0.456, 0.406),
                 std=(0.229, 0.224, 0.225), training=True, max_cache_videos=20000, raw=False):
        super().__init__()
        self.split_path = split_path
        self.image_size = int(image_size)
        self.clip_len = int(clip_len)
        self.stride = int(stride)
        self.mean = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        self.std = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        self.training = bool(training)
        self.raw = bool(raw)
        self.samples = []
        with open(split_path, "r", encoding="utf-8") as f:
            for line in f:
                parts = line.split()
                if parts:
                    self.samples.append(parts[0])
        self._list_frames = lru_cache(maxsize=max_cache_videos)(self._list_frames_uncached)

    def __len__(self):
        return len(self.samples)

    @staticmethod
    def _list_frames_uncached(vdir):
        if not os.path.isdir(vdir):
            return ()
        try:
            names = sorted(n for n in os.listdir(vdir) if n.lower().endswith(IMAGE_SUFFIXES))
        except OSError:
            return ()
        return tuple(os.path.join(vdir, n) for n in names)

    @staticmethod
    def _safe_read(path):
        """uint8 [H,W,3] RGB, or None for a file that cannot be decoded."""
        from PIL import Image
        try:
            return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        except Exception:
            return None

    def _resize_tensor(self, img_u8):
        """uint8 [H,W,3] -> fp32 [3,S,S] (mae_dataset.py:84-90)."""
        x = torch.from_numpy(np.ascontiguousarray(img_u8.transpose(2, 0, 1))).float().div_(255.0).unsqueeze(0)
        x = F.interpolate(x, size=(self.image_size, self.image_size), mode="bilinear", align_corners=False)
        return x.squeeze(0).contiguous()

    def _draw(self, n):
        """(frame indices, flip) with the reference's use of the global `random` stream."""
        max_start = max(0, n - (self.clip_len - 1) * self.stride - 1)
        start = random.randint(0, max_start) if self.training and max_start > 0 else 0
        indices = [min(start + i * self.stride, n - 1) for i in range(self.clip_len)]
        flip = self.training and random.random() < 0.5
        return indices, flip

    def __getitem__(self, idx):
        vdir = self.samples[idx]
        frames = self._list_frames(vdir)
        s = self.image_size
        if not frames:
            if self.raw:
                return torch.zeros(self.clip_len, s, s, 3, dtype=torch.uint8), True, False
            return (torch.zeros(3, self.clip_len, s, s) - self.mean.view(3, 1, 1, 1)) / self.std.view(3, 1, 1, 1)
        indices, flip = self._draw(len(frames))
        imgs = [self._safe_read(frames[j]) for j in indices]
        if self.raw:
            shapes = sorted({im.shape for im in imgs if im is not None})
            if len(shapes) > 1:
                raise ValueError(f"frames of {vdir} differ in size "
                                 f"({', '.join(f'{h}x{w}' for h, w, _ in shapes)}): one clip must have one frame size")
            black = np.zeros(shapes[0] if shapes else (s, s, 3), dtype=np.uint8)
            return torch.from_numpy(np.stack([black if im is None else im for im in imgs])), True, flip
        out = []
        for im in imgs:
            if im is None:
                x = torch.zeros(3, s, s)
            else:
                x = self._resize_tensor(im)
                if flip:
                    x = torch.flip(x, dims=[2])
            out.append((x - self.mean) / self.std)
        return torch.stack(out, dim=0).permute(1, 0, 2, 3).contiguous()

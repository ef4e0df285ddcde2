"""Generate tests/golden/mae_dataset.npz by RUNNING the reference's MAEVideoDataset.

Build container only (the reference never travels).  Loads src/datasets/mae_dataset.py by
file path.  torchvision is not installed, so `torchvision.io.read_image` / `ImageReadMode`
are replaced by a PIL stand-in of our own, placed in sys.modules before the import: it
returns the decoded RGB image as uint8 [3,H,W] and raises on a file PIL cannot decode, which
is all the reference asks of it (mae_dataset.py:76-82).

Trees (PNG, lossless): `long` 10 frames of 24x32 (random start), `short` 3 frames of 20x20
(clamped indices, no start draw), `corrupt` 6 frames of 16x16 with an undecodable 002.png
(zero frame) and a non-image file that must be ignored, `empty` (no frames).  image_size 16,
clip_len 4, stride 2; random.seed(7), then items 0..3 in order, once with training=True and
once (reseeded) with training=False.

The reference's item for the empty directory is `(zeros[3,T,S,S] - mean[3,1,1]) / std[3,1,1]`,
which broadcasts the channel vector against the T axis and raises unless clip_len is 1 or 3;
an item the reference could not produce is recorded by name in `raised` and has no clip.

Output (data only): the PNG bytes of every file, the directory names, the settings and the
clips the reference returned.

    python tests/golden/make_golden_mae_dataset.py
"""
import importlib.util
import io
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/datasets/mae_dataset.py"
MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]
SIZE, CLIP_LEN, STRIDE, SEED = 16, 4, 2, 7
DIRS = ["long", "short", "corrupt", "empty"]


def install_read_image():
    def read_image(path, mode=None):
        arr = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        return torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous()

    class ImageReadMode:
        RGB = "RGB"

    tv, tvio = types.ModuleType("torchvision"), types.ModuleType("torchvision.io")
    tvio.read_image, tvio.ImageReadMode = read_image, ImageReadMode
    tv.io = tvio
    sys.modules["torchvision"], sys.modules["torchvision.io"] = tv, tvio


def make_tree(root):
    rng = np.random.default_rng(11)
    files = {}

    def png(rel, h, w):
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(b, format="PNG")
        files[rel] = b.getvalue()

    for i in range(10):
        png(f"long/{i:05d}.png", 24, 32)
    for i in range(3):
        png(f"short/f{i}.png", 20, 20)
    for i in range(6):
        png(f"corrupt/{i:03d}.png", 16, 16)
    files["corrupt/002.png"] = b"not a png"
    files["corrupt/notes.txt"] = b"ignored"
    for rel, data in files.items():
        p = os.path.join(root, rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as f:
            f.write(data)
    os.makedirs(os.path.join(root, "empty"), exist_ok=True)
    return files


def main():
    install_read_image()
    spec = importlib.util.spec_from_file_location("ref_mae_dataset", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"dirs": np.array(DIRS), "seed": np.int64(SEED), "size": np.int64(SIZE), "clip_len": np.int64(CLIP_LEN),
           "stride": np.int64(STRIDE), "mean": np.array(MEAN, np.float32), "std": np.array(STD, np.float32)}
    raised = []
    with tempfile.TemporaryDirectory() as root:
        files = make_tree(root)
        split = os.path.join(root, "split.txt")
        with open(split, "w") as f:
            for d in DIRS:
                f.write(f"{os.path.join(root, d)} 1\n")
        for training in (True, False):
            ds = ref.MAEVideoDataset(split, image_size=SIZE, clip_len=CLIP_LEN, stride=STRIDE, mean=tuple(MEAN),
                                     std=tuple(STD), training=training)
            random.seed(SEED)
            for i in range(len(ds)):
                key = f"{'train' if training else 'eval'}{i}"
                try:
                    out[key] = ds[i].numpy()
                except RuntimeError as e:
                    raised.append(key)
                    print(key, "raised:", e)
    out["names"] = np.array(sorted(files))
    out["raised"] = np.array(raised)
    for i, name in enumerate(sorted(files)):
        out[f"file{i}"] = np.frombuffer(files[name], dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "mae_dataset.npz"), **out)
    print("wrote mae_dataset.npz; raised:", raised)


if __name__ == "__main__":
    main()

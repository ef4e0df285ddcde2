"""The resize arithmetic and the loader layer around sm_frames_resize_normalize, without a GPU:
tests/resize_mirror.py against the reference's ops (torch on the CPU) and against the
normalisation oracle, collate_raw's packing, LazyVideoMAEDataset's replacement frame, and
mae_dataset.MAEVideoDataset against clips the reference class returned
(tests/golden/mae_dataset.npz, make_golden_mae_dataset.py)."""
import io
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_mirror as M
from conftest import GOLDEN
from ssl_mae_amd import mae_dataset as MD
from ssl_mae_amd.mae_loader import ClipResizer, LazyVideoMAEDataset, collate_raw

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def torch_reference(frames_u8, out_hw, flip):
    """mae_dataset.py:84-90, :129-133 per frame: u8 / 255, F.interpolate, torch.flip, Normalize."""
    mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)
    frames = []
    for f in frames_u8:
        x = torch.from_numpy(f).permute(2, 0, 1).contiguous().float().div_(255.0).unsqueeze(0)
        x = F.interpolate(x, size=out_hw, mode="bilinear", align_corners=False).squeeze(0).contiguous()
        if flip:
            x = torch.flip(x, dims=[2])
        frames.append((x - mean) / std)
    return torch.stack(frames, dim=0).permute(1, 0, 2, 3).contiguous().numpy()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("hs,ws,ho,wo", [(240, 320, 112, 112), (112, 112, 224, 224), (112, 112, 96, 96),
                                         (112, 112, 128, 128), (7, 9, 8, 8), (5, 3, 16, 16), (33, 17, 8, 8),
                                         (1, 1, 4, 4)])
def test_mirror_matches_reference_ops(hs, ws, ho, wo, flip):
    rng = np.random.default_rng(hs * 1000 + ws)
    u8 = rng.integers(0, 256, (2, hs, ws, 3), dtype=np.uint8)
    got = M.resize_normalize(u8, (ho, wo), MEAN, STD, bgr_swap=False, flip=flip)
    ref = torch_reference(u8, (ho, wo), flip)
    err = float(np.abs(got - ref).max())
    print(f"{hs}x{ws}->{ho}x{wo} flip={flip}: max err {err:.3e}, bound {M.atol(hs, ws, STD):.3e}")
    assert got.shape == ref.shape == (3, 2, ho, wo)
    assert err <= M.atol(hs, ws, STD)


def test_bound_at_320_is_inside_fp32_parity():
    assert 2.6e-4 < M.atol(240, 320, STD) < 2.8e-4 < 1e-3


@pytest.mark.parametrize("h,w", [(112, 112), (8, 8)])
def test_identity_equals_normalisation_oracle(h, w):
    from oracle import loader_oracle as O
    u8 = np.random.default_rng(h).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    got = M.resize_normalize(u8, (h, w), MEAN, STD, bgr_swap=True, flip=False)
    assert np.array_equal(got, O.normalize_clip(u8, MEAN, STD))


def test_black_frame_is_exactly_normalised_zero():
    got = M.resize_normalize(np.zeros((1, 5, 7, 3), np.uint8), (16, 16), MEAN, STD, bgr_swap=False)
    for c in range(3):
        assert np.all(got[c] == (np.float32(0) - np.float32(MEAN[c])) / np.float32(STD[c]))


def test_collate_raw_packs_a_ragged_batch():
    rng = np.random.default_rng(3)
    a = torch.from_numpy(rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8))
    b = torch.from_numpy(rng.integers(0, 256, (2, 3, 4, 3), dtype=np.uint8))
    dead = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    c = torch.from_numpy(rng.integers(0, 256, (2, 1, 1, 3), dtype=np.uint8))
    packed, desc = collate_raw([(a, True, True), (dead, False, True), (b, True, False), (c, True)])
    na, nb = a.numel(), b.numel()
    assert packed.dtype == torch.uint8 and packed.dim() == 1 and packed.numel() == na + nb + c.numel()
    assert desc.dtype == torch.int64
    assert desc.tolist() == [[0, 5, 7, 1], [na, 0, 0, 2], [na, 3, 4, 0], [na + nb, 1, 1, 0]]
    assert torch.equal(packed[:na].view_as(a), a) and torch.equal(packed[na:na + nb].view_as(b), b)
    assert torch.equal(packed[na + nb:].view_as(c), c)
    ClipResizer.check(packed, desc, 2)                      # consistent: no error
    # the two-field items of LazyVideoMAEDataset; an all-invalid batch packs to nothing
    packed, desc = collate_raw([(dead, False), (dead, False)])
    assert packed.numel() == 0 and desc.tolist() == [[0, 0, 0, 2], [0, 0, 0, 2]]
    with pytest.raises(ValueError):
        collate_raw([(a, True), (torch.zeros(3, 5, 7, 3, dtype=torch.uint8), True)])


def test_resizer_validates_descriptors_on_the_host():
    from ssl_mae_amd._lib import KernelError
    packed = torch.zeros(2 * 4 * 4 * 3, dtype=torch.uint8)
    good = torch.tensor([[0, 4, 4, 0]])
    ClipResizer.check(packed, good, 2)
    for bad in ([[1, 4, 4, 0]], [[0, 4, 5, 0]], [[-1, 4, 4, 0]], [[0, 0, 4, 0]], [[0, 4, 8193, 0]]):
        with pytest.raises(KernelError):
            ClipResizer(16, device="cpu")(packed, torch.tensor(bad), 2)   # raises before any upload
    ClipResizer.check(packed, torch.tensor([[0, 0, 0, 2]]), 2)            # a flagged clip is not checked


def _png(arr):
    b = io.BytesIO()
    from PIL import Image
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _write_tree(root, name, frames):
    """frames: uint8 arrays (written lossless) or bytes (written as they are).  PNG data under
    the .jpg names LazyVideoMAEDataset lists: PIL decodes by content."""
    d = root / name
    d.mkdir()
    for i, f in enumerate(frames):
        (d / f"{i:04d}.jpg").write_bytes(f if isinstance(f, bytes) else _png(f))
    return str(d)


def test_lazy_dataset_replacement_frame_has_the_clip_size(tmp_path):
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (24, 32, 3), dtype=np.uint8) for _ in range(4)]
    tree = _write_tree(tmp_path, "v", [frames[0], b"broken", frames[2], frames[3]])
    dead = _write_tree(tmp_path, "dead", [b"broken"] * 4)
    mixed = _write_tree(tmp_path, "mixed", [frames[0], frames[1][:20], frames[2], frames[3]])
    split = tmp_path / "split.txt"
    split.write_text(f"{tree} 0\n{dead} 0\n{mixed} 0\n")
    ds = LazyVideoMAEDataset(str(split), clip_len=4, stride=1, image_size=16, transform=None)
    np.random.seed(0)
    clip, valid = ds[0]
    assert valid and clip.dtype == torch.uint8 and tuple(clip.shape) == (4, 24, 32, 3)
    assert not clip[1].any()                                     # black, at the clip's own size
    for i in (0, 2, 3):
        assert np.array_equal(clip[i].numpy(), frames[i])
    clip, valid = ds[1]                                          # nothing readable: image_size
    assert valid and tuple(clip.shape) == (4, 16, 16, 3) and not clip.any()
    with pytest.raises(ValueError, match="differ in size"):
        ds[2]


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    z = np.load(os.path.join(GOLDEN, "mae_dataset.npz"))
    root = tmp_path_factory.mktemp("mae_dataset")
    for d in z["dirs"]:
        (root / str(d)).mkdir()
    for i, name in enumerate(z["names"]):
        (root / str(name)).write_bytes(z[f"file{i}"].tobytes())
    split = root / "split.txt"
    split.write_text("".join(f"{root / str(d)} 1\n" for d in z["dirs"]))
    return z, str(split)


def _dataset(z, split, training, raw):
    return MD.MAEVideoDataset(split, image_size=int(z["size"]), clip_len=int(z["clip_len"]), stride=int(z["stride"]),
                              mean=tuple(z["mean"].tolist()), std=tuple(z["std"].tolist()), training=training,
                              raw=raw)


def _expected(z, key):
    """The reference's clip, or for the item its own broadcast error kept it from returning
    (the empty directory, see make_golden_mae_dataset.py) the clip it documents: black,
    normalised per channel."""
    if key in z["raised"]:
        assert key.endswith("3")
        black = (np.float32(0) - z["mean"]) / z["std"]
        S, T = int(z["size"]), int(z["clip_len"])
        return np.broadcast_to(black.reshape(3, 1, 1, 1), (3, T, S, S))
    return z[key]


SOURCE_SIDE = {"long": 32, "short": 20, "corrupt": 16, "empty": 16}


@pytest.mark.parametrize("training", [True, False])
def test_mae_dataset_host_path_matches_reference(golden, training):
    z, split = golden
    ds = _dataset(z, split, training, raw=False)
    random.seed(int(z["seed"]))
    for i, d in enumerate(z["dirs"]):
        clip = ds[i].numpy()
        exp = _expected(z, f"{'train' if training else 'eval'}{i}")
        assert clip.shape == exp.shape and clip.dtype == np.float32
        assert np.abs(clip - exp).max() <= M.atol(SOURCE_SIDE[str(d)], SOURCE_SIDE[str(d)], z["std"]), d


@pytest.mark.parametrize("training", [True, False])
def test_mae_dataset_raw_path_plus_mirror_matches_reference(golden, training):
    """raw=True items through collate_raw and the mirror of the device kernel: equal clips
    prove the frame indices, the flip draw and the replacement frames."""
    z, split = golden
    ds = _dataset(z, split, training, raw=True)
    random.seed(int(z["seed"]))
    items = [ds[i] for i in range(len(ds))]
    assert all(valid for _, valid, _ in items)
    if not training:
        assert not any(flip for _, _, flip in items)
    assert tuple(items[0][0].shape) == (int(z["clip_len"]), 24, 32, 3)
    packed, desc = collate_raw(items)
    S = int(z["size"])
    got = M.resize_normalize_batch(packed.numpy(), desc.numpy(), int(z["clip_len"]), (S, S), z["mean"], z["std"],
                                   bgr_swap=False)
    for i, d in enumerate(z["dirs"]):
        exp = _expected(z, f"{'train' if training else 'eval'}{i}")
        assert np.abs(got[i] - exp).max() <= M.atol(SOURCE_SIDE[str(d)], SOURCE_SIDE[str(d)], z["std"]), d


def test_golden_holds_a_flipped_and_an_unflipped_training_clip(golden):
    z, split = golden
    ds = _dataset(z, split, True, raw=True)
    random.seed(int(z["seed"]))
    flips = [ds[i][2] for i in range(3)]
    assert True in flips and False in flips, flips

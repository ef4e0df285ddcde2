"""The crop augmentation without a GPU: tests/crop_mirror.py (the window rule), the properties of
mae_loader.RandomResizedCropFlip, ClipResizer.check on windows, train_finetune's `augment`
section and what split_file_loader hands the resizer with and without an augmenter."""
import io
import math

import numpy as np
import pytest
import torch

import crop_mirror as CM
import resize_mirror as M
from ssl_mae_amd import mae_loader as ML
from ssl_mae_amd.mae_loader import ClipResizer, RandomResizedCropFlip

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
N = 2000
SIZES = [(240, 320), (112, 112), (5, 3)]


def _desc4(n, hs, ws, T=2):
    d = torch.zeros(n, 4, dtype=torch.int64)
    d[:, 0] = torch.arange(n) * (T * hs * ws * 3)
    d[:, 1], d[:, 2] = hs, ws
    return d


# ------------------------------------------------------------------ the window-rule mirror
def test_mirror_full_window_is_the_resize_mirror():
    u8 = np.random.default_rng(0).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    for flip in (False, True):
        assert np.array_equal(CM.crop_resize_normalize(u8, (0, 0, 9, 11), (8, 8), MEAN, STD, True, flip),
                              M.resize_normalize(u8, (8, 8), MEAN, STD, True, flip))


def test_mirror_ignores_pixels_outside_the_window():
    """The window clamp: changing every pixel outside the window leaves the result unchanged,
    and the top-left window differs from a frame-clamped interpolation of the same origin."""
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    win = (0, 0, 5, 4)
    other = rng.integers(0, 256, u8.shape, dtype=np.uint8)
    other[:, 0:5, 0:4] = u8[:, 0:5, 0:4]
    a = CM.crop_resize_normalize(u8, win, (8, 8), MEAN, STD)
    assert np.array_equal(a, CM.crop_resize_normalize(other, win, (8, 8), MEAN, STD))
    # the last output column / row sit on the window's last pixel alone (l1 applies to a clamped
    # neighbour, i1 == i0), whatever the frame holds to its right / below
    one = CM.crop_resize_normalize(u8[:, 4:5, 3:4], (0, 0, 1, 1), (1, 1), MEAN, STD)
    assert np.allclose(a[:, :, -1, -1], one[:, :, 0, 0], atol=2e-6)


def test_mirror_batch_rejects_bad_windows():
    u8 = np.random.default_rng(2).integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    packed = np.concatenate([u8.reshape(-1)] * 2)
    n = u8.size
    good = [0, 7, 9, 0, 1, 2, 5, 6]
    bad = [[n, 7, 9, 0, -1, 0, 3, 3], [n, 7, 9, 0, 0, -1, 3, 3], [n, 7, 9, 0, 0, 0, 0, 3], [n, 7, 9, 0, 0, 0, 3, 0],
           [n, 7, 9, 0, 3, 0, 5, 3], [n, 7, 9, 0, 0, 7, 3, 3], [n, 7, 9, 2, 0, 0, 7, 9], [n + 1, 7, 9, 0, 0, 0, 7, 9]]
    out = CM.crop_resize_normalize_batch(packed, np.asarray([good] + bad, np.int64), 2, (4, 4), MEAN, STD)
    assert out[0].any() and not out[1:].any()
    assert np.array_equal(out[0], CM.crop_resize_normalize(u8, (1, 2, 5, 6), (4, 4), MEAN, STD))


# ------------------------------------------------------------------ the sampler
@pytest.fixture(scope="module")
def drawn():
    """One draw of N clips per frame size with the default sampler (shared, never modified)."""
    out = {}
    for hs, ws in SIZES:
        aug = RandomResizedCropFlip(seed=3)
        d8 = aug.windows(_desc4(N, hs, ws))
        out[hs, ws] = (aug, d8, list(aug.last_fallback))
    return out


@pytest.mark.parametrize("hs,ws", SIZES)
def test_windows_lie_inside_their_frames(drawn, hs, ws):
    aug, d8, fb = drawn[hs, ws]
    assert d8.dtype == torch.int64 and tuple(d8.shape) == (N, 8) and len(fb) == N
    assert torch.equal(d8[:, :3], _desc4(N, hs, ws)[:, :3])
    y0, x0, hc, wc = d8[:, 4], d8[:, 5], d8[:, 6], d8[:, 7]
    assert bool(((hc >= 1) & (wc >= 1) & (y0 >= 0) & (x0 >= 0) & (y0 + hc <= hs) & (x0 + wc <= ws)).all())
    assert bool(((d8[:, 3] & ~1) == 0).all())
    ClipResizer.check(torch.zeros(N * 2 * hs * ws * 3, dtype=torch.uint8), d8, 2)


@pytest.mark.parametrize("hs,ws", SIZES)
def test_accepted_windows_have_the_drawn_area_and_aspect(drawn, hs, ws):
    """w = round(sqrt(area ar)), h = round(sqrt(area / ar)) = (a + dw, b + dh) with a b = area,
    a / b = ar, |dw|, |dh| <= 1/2: w h - area = w dh + h dw - dw dh, so |Hc Wc - area| <=
    (Hc + Wc) / 2 + 1/4 for an area within scale * Hs Ws, and (Wc - 1/2) / (Hc + 1/2) <= ar <=
    (Wc + 1/2) / (Hc - 1/2) for an ar within ratio."""
    aug, d8, fb = drawn[hs, ws]
    s0, s1 = aug.scale
    r0, r1 = aug.ratio
    n_acc = 0
    for (_, _, _, _, _, _, hc, wc), fell in zip(d8.tolist(), fb):
        if fell:
            continue
        n_acc += 1
        bound = 0.5 * (hc + wc) + 0.25
        assert s0 * hs * ws - bound <= hc * wc <= s1 * hs * ws + bound, (hc, wc)
        assert (wc + 0.5) / (hc - 0.5) >= r0 * (1 - 1e-12) and (wc - 0.5) / (hc + 0.5) <= r1 * (1 + 1e-12), (hc, wc)
    assert n_acc > N // 2
    if (hs, ws) != (5, 3):
        lo = min(h * w for _, _, _, _, _, _, h, w in d8.tolist())
        hi = max(h * w for _, _, _, _, _, _, h, w in d8.tolist())
        assert lo < 0.45 * hs * ws and hi > 0.9 * hs * ws            # the scale range is used
        assert len({(r[4], r[5]) for r in d8.tolist()}) > N // 4     # and so are the positions


@pytest.mark.parametrize("hs,ws", SIZES)
def test_flip_fraction_is_within_four_sigma(drawn, hs, ws):
    aug, d8, _ = drawn[hs, ws]
    frac = float((d8[:, 3] & ML.FLAG_FLIP).double().mean())
    sigma = math.sqrt(0.5 * 0.5 / N)
    print(f"{hs}x{ws}: flip fraction {frac:.4f}, 4 sigma {4 * sigma:.4f}")
    assert abs(frac - aug.flip) <= 4 * sigma


def test_flip_zero_and_one_are_exact():
    d4 = _desc4(N, 24, 32)
    assert not bool((RandomResizedCropFlip(flip=0.0, seed=1).windows(d4)[:, 3] & ML.FLAG_FLIP).any())
    assert bool((RandomResizedCropFlip(flip=1.0, seed=1).windows(d4)[:, 3] & ML.FLAG_FLIP).all())


def test_fallback_is_the_centred_window_of_clamped_aspect():
    aug = RandomResizedCropFlip(scale=(1, 1), ratio=(1, 1), flip=0.0, seed=0)
    d8 = aug.windows(_desc4(4, 5, 3))
    assert aug.last_fallback == [True] * 4
    assert d8[:, 4:].tolist() == [[1, 0, 3, 3]] * 4
    # a frame wider than ratio[1] allows: full height, centred
    aug = RandomResizedCropFlip(scale=(1, 1), ratio=(0.5, 2.0), flip=0.0, seed=0)
    assert aug.windows(_desc4(1, 4, 20))[0, 4:].tolist() == [0, 6, 4, 8] and aug.last_fallback == [True]


def test_seed_fixes_the_windows():
    d4 = _desc4(64, 24, 32)
    a = RandomResizedCropFlip(seed=7)
    b = RandomResizedCropFlip(seed=7)
    first = a.windows(d4)
    assert torch.equal(first, b.windows(d4))
    second = a.windows(d4)
    assert not torch.equal(first, second)                       # the stream moves on: fresh crops every batch
    assert torch.equal(second, b.windows(d4))
    assert not torch.equal(first, RandomResizedCropFlip(seed=8).windows(d4))


def test_invalid_clips_pass_through_and_do_not_shift_the_stream():
    d4 = _desc4(6, 24, 32)
    ref = RandomResizedCropFlip(seed=5).windows(d4)
    d4[2] = torch.tensor([int(d4[2, 0]), 0, 0, ML.FLAG_INVALID | ML.FLAG_FLIP])
    aug = RandomResizedCropFlip(seed=5)
    got = aug.windows(d4)
    assert got[2].tolist() == [int(d4[2, 0]), 0, 0, ML.FLAG_INVALID | ML.FLAG_FLIP, 0, 0, 0, 0]
    assert aug.last_fallback[2] is False
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(got[keep], ref[keep])
    ClipResizer.check(torch.zeros(6 * 2 * 24 * 32 * 3, dtype=torch.uint8), got, 2)


@pytest.mark.parametrize("hs,ws", SIZES)
def test_unit_scale_at_the_frame_aspect_is_the_full_frame(hs, ws):
    aug = RandomResizedCropFlip(scale=(1, 1), ratio=(ws / hs, ws / hs), flip=0.0, seed=2)
    d8 = aug.windows(_desc4(N, hs, ws))
    assert d8[:, 3:].tolist() == [[0, 0, 0, hs, ws]] * N and not any(aug.last_fallback)


def test_sampler_rejects_bad_settings_and_descriptors():
    for kw in ({"scale": (0.0, 1.0)}, {"scale": (0.5, 0.4)}, {"scale": (0.5, 1.1)}, {"ratio": (0.0, 1.0)},
               {"ratio": (2.0, 1.0)}, {"flip": -0.1}, {"flip": 1.1}):
        with pytest.raises(ValueError):
            RandomResizedCropFlip(**kw)
    with pytest.raises(ValueError):
        RandomResizedCropFlip().windows(torch.zeros(2, 8, dtype=torch.int64))


# ------------------------------------------------------------------ host checks
def test_resizer_validates_windows_on_the_host():
    from ssl_mae_amd._lib import KernelError
    packed = torch.zeros(2 * 4 * 6 * 3, dtype=torch.uint8)
    ClipResizer.check(packed, torch.tensor([[0, 4, 6, 0, 0, 0, 4, 6]]), 2)
    ClipResizer.check(packed, torch.tensor([[0, 4, 6, 1, 3, 5, 1, 1]]), 2)
    ClipResizer.check(packed, torch.tensor([[0, 0, 0, 2, -1, -1, 0, 0]]), 2)     # a flagged clip is not checked
    for win in ([-1, 0, 2, 2], [0, -1, 2, 2], [0, 0, 0, 2], [0, 0, 2, 0], [1, 0, 4, 2], [0, 1, 2, 6], [4, 0, 1, 1]):
        with pytest.raises(KernelError, match="clip 1"):
            ClipResizer(16, device="cpu")(packed, torch.tensor([[0, 4, 6, 0, 0, 0, 4, 6], [0, 4, 6, 0] + win]), 2)
    for bad in (torch.zeros(1, 5, dtype=torch.int64), torch.zeros(1, 8, dtype=torch.int32)):
        with pytest.raises(KernelError):
            ClipResizer.check(packed, bad, 2)
    with pytest.raises(KernelError):                             # the frame rules hold in the 8-column form
        ClipResizer.check(packed, torch.tensor([[1, 4, 6, 0, 0, 0, 4, 6]]), 2)


def _cfg(tmp_path, **augment):
    split = tmp_path / "split.txt"
    split.write_text("")
    return {"dataset": {"train_split": str(split), "val_split": str(split)}, "augment": augment}


def test_config_validation(tmp_path):
    from ssl_mae_amd import train_finetune as TF
    base = TF.resolve_config({})
    assert base["augment"] == {"enabled": False, "scale": [0.35, 1.0], "ratio": [0.75, 1.3333], "flip": 0.5}
    on = TF.resolve_config(_cfg(tmp_path, enabled=True, scale=[0.5, 0.5], flip=1.0))
    assert on["augment"] == {"enabled": True, "scale": [0.5, 0.5], "ratio": [0.75, 1.3333], "flip": 1.0}
    for bad in ({"scale": [0.0, 1.0]}, {"scale": [0.6, 0.5]}, {"scale": [0.5, 1.5]}, {"scale": [0.5]},
                {"ratio": [0.0, 1.0]}, {"ratio": [1.5, 1.0]}, {"ratio": 1.0}, {"flip": -0.01}, {"flip": 1.01},
                {"crop": True}):
        with pytest.raises(ValueError):
            TF.resolve_config(_cfg(tmp_path, **bad))
        with pytest.raises(ValueError):                          # out of range even when off
            TF.resolve_config({"augment": bad})
    with pytest.raises(ValueError, match="no source frames to crop"):
        TF.resolve_config({"augment": {"enabled": True}})


def test_shipped_config_has_the_section_switched_off():
    import os
    import yaml
    from conftest import ROOT
    from ssl_mae_amd import train_finetune as TF
    with open(os.path.join(ROOT, "configs", "finetune.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["augment"] == TF.DEFAULTS["augment"] and cfg["augment"]["enabled"] is False


# ------------------------------------------------------------------ the loader
def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _tree(root, n_videos=3, hw=(24, 32)):
    rng = np.random.default_rng(5)
    lines = []
    for v in range(n_videos):
        d = root / f"video_{v}"
        d.mkdir()
        for f in range(8):
            (d / f"{f:05d}.jpg").write_bytes(_png(rng.integers(0, 256, hw + (3,), dtype=np.uint8)))
        lines.append(f"{d} {v}")
    split = root / "split.txt"
    split.write_text("\n".join(lines) + "\n")
    return str(split)


class Recorder:
    """Stands in for ClipResizer: keeps every descriptor it is called with."""
    calls = []

    def __init__(self, image_size, **kw):
        self.image_size = image_size

    def __call__(self, packed, desc, T):
        ClipResizer.check(packed, desc, T)
        Recorder.calls.append(desc.clone())
        return torch.zeros(desc.shape[0], 3, T, self.image_size, self.image_size)


def test_split_file_loader_hands_the_resizer_windows_only_with_an_augmenter(tmp_path, monkeypatch):
    from ssl_mae_amd import driver
    monkeypatch.setattr(ML, "ClipResizer", Recorder)
    split = _tree(tmp_path)
    kw = dict(clip_len=4, stride=2, image_size=16, batch_size=2, num_workers=0, device="cpu")
    Recorder.calls = []
    out = list(driver.split_file_loader(split, **kw))
    assert [tuple(d.shape) for d in Recorder.calls] == [(2, 4), (1, 4)]
    assert [l.tolist() for _, l in out] == [[0, 1], [2]]
    plain = Recorder.calls
    Recorder.calls = []
    list(driver.split_file_loader(split, augment=None, **kw))
    assert all(torch.equal(a, b) for a, b in zip(plain, Recorder.calls)) and len(Recorder.calls) == 2
    Recorder.calls = []
    list(driver.split_file_loader(split, augment=RandomResizedCropFlip(seed=7), **kw))
    twin = RandomResizedCropFlip(seed=7)
    assert [tuple(d.shape) for d in Recorder.calls] == [(2, 8), (1, 8)]
    for got, d4 in zip(Recorder.calls, plain):
        assert torch.equal(got, twin.windows(d4))
    Recorder.calls = []
    list(driver.split_file_loader(split, labelled=False, augment=RandomResizedCropFlip(seed=7), **kw))
    assert [tuple(d.shape) for d in Recorder.calls] == [(2, 8), (1, 8)]

"""sm_frames_crop_resize_normalize on the GPU: bit for bit against tests/crop_mirror.py (the
window sliced out on the host, then the unchanged resize mirror) over the kernel's paths, against
sm_frames_resize_normalize for the full-frame window, the bounds rules, the argument checks, and
the augmented loader and fine-tuning driver on a small frame tree."""
import csv
import io

import numpy as np
import pytest
import torch
import yaml

import crop_mirror as CM
import resize_mirror as M

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PAD = 64          # bytes of 0xFF on either side of `packed`: a read outside it would change a result


def _pack(clips, flags, windows):
    """clips: uint8 [T,Hs,Ws,3] arrays or None (invalid); windows: (y0, x0, Hc, Wc) per clip."""
    desc, parts, off = [], [], 0
    for c, fl, w in zip(clips, flags, windows):
        if c is None:
            desc.append([off, 0, 0, fl | M.FLAG_INVALID] + list(w))
            continue
        desc.append([off, c.shape[1], c.shape[2], fl] + list(w))
        parts.append(c.reshape(-1))
        off += c.size
    return np.concatenate(parts), np.asarray(desc, np.int64)


def _run(packed, desc, T, out_hw, bgr, packed_shift=0, out_shift=0, full=False):
    from ssl_mae_amd import kernels as K
    buf = torch.full((PAD + packed_shift + packed.size + PAD,), 255, dtype=torch.uint8, device="cuda")
    view = buf[PAD + packed_shift:PAD + packed_shift + packed.size]
    view.copy_(torch.from_numpy(packed))
    out = None
    if out_shift:
        n = len(desc) * 3 * T * out_hw[0] * out_hw[1]
        flat = torch.full((n + out_shift,), float("nan"), device="cuda")
        out = flat[out_shift:].view(len(desc), 3, T, *out_hw)
    d = torch.from_numpy(np.ascontiguousarray(desc)).cuda()
    op = K.frames_resize_normalize if full else K.frames_crop_resize_normalize
    return op(view, d, T, out_hw, MEAN, STD, bgr, out=out).cpu().numpy()


def _rand(rng, T, hs, ws):
    return rng.integers(0, 256, (T, hs, ws, 3), dtype=np.uint8)


def _check(clips, flags, windows, T, out_hw, **kw):
    packed, desc = _pack(clips, flags, windows)
    for bgr in (True, False):
        exp = CM.crop_resize_normalize_batch(packed, desc, T, out_hw, MEAN, STD, bgr)
        got = _run(packed, desc, T, out_hw, bgr, **kw)
        assert got.shape == exp.shape
        assert np.array_equal(got, exp), (out_hw, bgr, float(np.abs(got - exp).max()))


# interior window with an odd byte start; the frame's bottom-right corner; the top-left corner
# (the right / bottom clamp is the window's while the frame has more pixels: a frame clamp fails
# here); full width (the contiguous staged range with a row offset); one pixel; identity scale;
# scalar stores with more than one row band
@pytest.mark.parametrize("hs,ws,win,ho,wo", [(9, 11, (2, 3, 5, 4), 8, 8), (9, 11, (4, 7, 5, 4), 8, 8),
                                             (9, 11, (0, 0, 5, 4), 8, 8), (9, 11, (3, 0, 4, 11), 6, 6),
                                             (7, 9, (6, 8, 1, 1), 4, 4), (12, 20, (1, 2, 8, 12), 8, 12),
                                             (12, 20, (1, 2, 8, 12), 19, 13)])
def test_kernel_equals_window_mirror(hs, ws, win, ho, wo):
    rng = np.random.default_rng(hs * 100 + ws)
    clips = [_rand(rng, 2, hs, ws), _rand(rng, 2, hs, ws)]
    _check(clips, [0, M.FLAG_FLIP], [win, win], 2, (ho, wo))


@pytest.mark.parametrize("hs,ws,s", [(7, 9, 8), (5, 3, 16)])
def test_full_frame_window_equals_the_resize_kernel(hs, ws, s):
    rng = np.random.default_rng(hs)
    clips = [_rand(rng, 2, hs, ws), _rand(rng, 2, hs, ws)]
    packed, desc = _pack(clips, [0, M.FLAG_FLIP], [(0, 0, hs, ws)] * 2)
    for bgr in (True, False):
        ref = _run(packed, desc[:, :4], 2, (s, s), bgr, full=True)
        assert np.array_equal(_run(packed, desc, 2, (s, s), bgr), ref)
        assert np.array_equal(ref, M.resize_normalize_batch(packed, desc[:, :4], 2, (s, s), MEAN, STD, bgr))


def test_ragged_batch_with_an_invalid_clip():
    rng = np.random.default_rng(1)
    clips = [_rand(rng, 3, 7, 9), None, _rand(rng, 3, 5, 3), _rand(rng, 3, 33, 17)]
    wins = [(1, 2, 5, 6), (0, 0, 2, 2), (2, 1, 3, 2), (4, 0, 29, 11)]
    _check(clips, [M.FLAG_FLIP, M.FLAG_FLIP, 0, M.FLAG_FLIP], wins, 3, (8, 8))
    _check(clips, [0, 0, M.FLAG_FLIP, 0], wins, 3, (6, 6))


@pytest.mark.parametrize("wo", [8, 6])
def test_unaligned_packed_and_out_give_the_same_bits(wo):
    """packed 1 and 3 bytes into its allocation, out 4 bytes in (scalar stores).  The last clip's
    window ends at the last byte of `packed`, so its last dword is assembled from in-range bytes
    (the bytes behind are 0xFF and would show)."""
    rng = np.random.default_rng(2)
    clips = [_rand(rng, 2, 7, 9), _rand(rng, 2, 9, 11)]
    wins = [(1, 1, 5, 7), (4, 7, 5, 4)]
    _check(clips, [0, M.FLAG_FLIP], wins, 2, (8, wo), packed_shift=1)
    _check(clips, [0, M.FLAG_FLIP], wins, 2, (8, wo), out_shift=1)
    _check(clips, [M.FLAG_FLIP, 0], wins, 2, (8, wo), packed_shift=3, out_shift=1)


def test_two_column_tiles_and_the_direct_gather():
    """3 x 700 source, 600-column window to 1028 and 1030 columns: two column tiles, each staging
    its own row segments, vector and scalar stores.  3 x 8192 source: two full-width rows (48 KiB)
    and three 8000-pixel segments both exceed the 24 KiB stage: the direct gather."""
    rng = np.random.default_rng(3)
    mid = [_rand(rng, 1, 3, 700), _rand(rng, 1, 3, 700)]
    _check(mid, [0, M.FLAG_FLIP], [(0, 50, 3, 600)] * 2, 1, (2, 1028))
    _check(mid, [M.FLAG_FLIP, 0], [(0, 50, 3, 600)] * 2, 1, (2, 1030))
    wide = [_rand(rng, 1, 3, 8192), _rand(rng, 1, 3, 8192)]
    _check(wide, [0, M.FLAG_FLIP], [(1, 0, 2, 8192)] * 2, 1, (3, 8))
    _check(wide, [M.FLAG_FLIP, 0], [(0, 100, 3, 8000)] * 2, 1, (2, 1030))


@pytest.mark.parametrize("hs,ws,win,s", [(240, 320, (20, 40, 180, 200), 112), (112, 112, (10, 10, 90, 90), 224)])
def test_workload_sizes(hs, ws, win, s):
    rng = np.random.default_rng(s)
    clips = [_rand(rng, 2, hs, ws), _rand(rng, 2, hs, ws)]
    _check(clips, [0, M.FLAG_FLIP], [win, win], 2, (s, s))


def test_bad_windows_and_descriptors_give_zero_clips():
    """Ordinary inputs the kernel must reject: a negative origin, an empty window, a window one
    row / column past its frame, and the sibling's bad descriptors in the 8-column form, each
    yield a zero clip between intact neighbours."""
    rng = np.random.default_rng(4)
    a, b = _rand(rng, 2, 7, 9), _rand(rng, 2, 5, 3)
    good_a, good_b = (1, 2, 5, 6), (1, 0, 3, 3)
    clips = [a, a, b, a, b, a, b, a, b, a, b, a, b]
    wins = [good_a, (-1, 2, 5, 6), good_b, (1, -1, 5, 6), good_b, (1, 2, 0, 6), good_b, (1, 2, 5, 0), good_b,
            (3, 2, 5, 6), good_b, (1, 4, 5, 6), good_b]                 # y0 + Hc = Hs + 1, x0 + Wc = Ws + 1
    packed, desc = _pack(clips, [0] * len(clips), wins)
    bad = [1, 3, 5, 7, 9, 11]
    extra = np.asarray([[packed.size - 10, 7, 9, 0, 0, 0, 7, 9],        # runs past the end of the buffer
                        [0, 0, 3, 0, 0, 0, 1, 1],                       # Hs = 0
                        [-4, 7, 9, 0, 0, 0, 7, 9],                      # starts before the buffer
                        [0, 1, 8193, 0, 0, 0, 1, 1],                    # a side above 8192
                        [0, 7, 9, M.FLAG_INVALID, 0, 0, 7, 9],          # flagged
                        [0, 7, 9, 0] + list(good_a)], np.int64)
    desc = np.concatenate([desc, extra])
    bad += [13, 14, 15, 16, 17]
    for bgr in (True, False):
        exp = CM.crop_resize_normalize_batch(packed, desc, 2, (8, 8), MEAN, STD, bgr)
        got = _run(packed, desc, 2, (8, 8), bgr)
        for i in range(len(desc)):
            if i in bad:
                assert not got[i].any(), (i, bgr)
            else:
                assert got[i].any() and np.array_equal(got[i], exp[i]), (i, bgr)


def test_argument_validation():
    import ctypes
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd._lib import KernelError, ptr, stream
    packed = torch.zeros(2 * 4 * 4 * 3, dtype=torch.uint8, device="cuda")
    desc = torch.tensor([[0, 4, 4, 0, 1, 1, 2, 3]], device="cuda")
    out = torch.full((1, 3, 2, 8, 8), 7.0, device="cuda")
    m = (ctypes.c_float * 3)(*MEAN)
    s = (ctypes.c_float * 3)(*STD)
    mp, sp = ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p)

    def raw(p=ptr(packed), d=ptr(desc), n=packed.numel(), B=1, T=2, Ho=8, Wo=8, mean=mp, std=sp, o=ptr(out)):
        return K.query("sm_frames_crop_resize_normalize", p, d, n, B, T, Ho, Wo, mean, std, 1, o, stream())

    assert raw(p=None) == -2 and raw(d=None) == -2 and raw(mean=None) == -2 and raw(std=None) == -2
    assert raw(o=None) == -2
    assert raw(B=-1) == -2 and raw(T=-1) == -2 and raw(Ho=-1) == -2 and raw(Wo=-1) == -2 and raw(n=-1) == -2
    assert raw(Ho=4097) == -2 and raw(Wo=4097) == -2
    assert raw(B=0) == 0 and raw(T=0) == 0 and raw(Ho=0, o=None) == 0          # empty output
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                            # nothing was launched
    assert raw() == 0
    assert np.array_equal(out.cpu().numpy(), CM.crop_resize_normalize_batch(np.zeros(96, np.uint8),
                                                                            desc.cpu().numpy(), 2, (8, 8), MEAN, STD))
    # the tensor-level wrapper
    f = K.frames_crop_resize_normalize
    for bad in (lambda: f(packed.float(), desc, 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc.int(), 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc.view(-1), 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc[:, :4].contiguous(), 2, (8, 8), MEAN, STD),
                lambda: f(packed.view(2, -1), desc, 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc.cpu(), 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc, -1, (8, 8), MEAN, STD),
                lambda: f(packed, desc, 2, (8, 4097), MEAN, STD),
                lambda: f(packed[::2], desc, 2, (8, 8), MEAN, STD),
                lambda: f(packed, desc, 2, (8, 8), MEAN, STD, out=out[:, :, :1]),
                lambda: K.frames_resize_normalize(packed, desc, 2, (8, 8), MEAN, STD)):
        with pytest.raises(KernelError):
            bad()
    assert f(packed, desc[:0], 2, (8, 8), MEAN, STD).shape == (0, 3, 2, 8, 8)


def test_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ssl_mae_amd import ops
    assert hasattr(torch.ops.ssl_mae, "frames_crop_resize_normalize")
    with FakeTensorMode():
        y = ops.frames_crop_resize_normalize(torch.empty(100, dtype=torch.uint8),
                                             torch.empty(3, 8, dtype=torch.int64), 2, (16, 12), MEAN, STD)
        assert y.shape == (3, 3, 2, 16, 12) and y.dtype == torch.float32


# ------------------------------------------------------------------ loader and driver
def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _frame_tree(root, n_videos=3, n_frames=8, hw=(24, 32)):
    """Lossless frames (PNG data under the .jpg names the dataset lists); every video has exactly
    clip_len * stride = 8 frames, so the one possible start index is 0."""
    rng = np.random.default_rng(5)
    videos, lines = [], []
    for v in range(n_videos):
        d = root / f"video_{v}"
        d.mkdir()
        frames = rng.integers(0, 256, (n_frames,) + hw + (3,), dtype=np.uint8)
        for f in range(n_frames):
            (d / f"{f:05d}.jpg").write_bytes(_png(frames[f]))
        videos.append(frames[0:8:2])
        lines.append(f"{d} {v}")
    split = root / "split.txt"
    split.write_text("\n".join(lines) + "\n")
    return split, videos


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _frame_tree(tmp_path_factory.mktemp("crop_tree"))


@pytest.mark.parametrize("workers", [0, 2])
def test_augmented_loader_equals_mirror_for_any_worker_count(tree, workers):
    from ssl_mae_amd import driver
    from ssl_mae_amd.mae_loader import RandomResizedCropFlip, collate_raw
    split, videos = tree
    loader = driver.split_file_loader(str(split), clip_len=4, stride=2, image_size=16, batch_size=2,
                                      num_workers=workers, device="cuda", augment=RandomResizedCropFlip(seed=7))
    out = list(loader)
    assert [tuple(c.shape) for c, _ in out] == [(2, 3, 4, 16, 16), (1, 3, 4, 16, 16)]
    assert torch.cat([l for _, l in out]).tolist() == [0, 1, 2]
    twin = RandomResizedCropFlip(seed=7)
    cropped = 0
    for (clip, _), ids in zip(out, ([0, 1], [2])):
        packed, d4 = collate_raw([(torch.from_numpy(videos[i]), True) for i in ids])
        d8 = twin.windows(d4)
        exp = CM.crop_resize_normalize_batch(packed.numpy(), d8.numpy(), 4, (16, 16), MEAN, STD, True)
        assert np.array_equal(clip.cpu().numpy(), exp)
        cropped += sum(r[4:] != [0, 0, 24, 32] for r in d8.tolist())
    assert cropped >= 2                                          # the windows were real crops


def test_loader_without_an_augmenter_gives_the_full_frames(tree):
    from ssl_mae_amd import driver
    split, videos = tree
    out = list(driver.split_file_loader(str(split), clip_len=4, stride=2, image_size=16, batch_size=3,
                                        num_workers=0, device="cuda", augment=None))
    assert len(out) == 1
    for i, frames in enumerate(videos):
        assert np.array_equal(out[0][0][i].cpu().numpy(), M.resize_normalize(frames, (16, 16), MEAN, STD, True)), i


def _summary(path):
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    cut = rows[0].index("seconds")
    return [r[:cut] + r[cut + 1:] for r in rows]


def _finetune(tmp_path, tree, name, augment, hooks=None):
    from ssl_mae_amd import train_finetune as TF
    split, _ = tree
    cfg = {"dataset": {"train_split": str(split), "val_split": str(split), "num_classes": 3, "clip_len": 4,
                       "stride": 2, "image_size": 112},
           "training": {"epochs": 2, "batch_size": 2, "amp": False, "log_interval": 100},
           "runtime": {"seed": 42, "num_workers": 0},
           "paths": {"save_dir": str(tmp_path / name), "log_dir": str(tmp_path / name / "logs")}}
    if augment is not None:
        cfg["augment"] = augment
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = TF.main(["--config", str(path), "--mode", "ft_random"], hooks=hooks)
    return res, _summary(tmp_path / name / "ft_random" / "finetune_summary.csv")


def test_driver_with_augmentation_trains_and_is_reproducible(tmp_path, tree, monkeypatch, capsys):
    from ssl_mae_amd import mae_loader as ML
    descs, first = [], {}
    call = ML.ClipResizer.__call__

    def recording(self, packed, desc, T):
        descs.append(desc.clone())
        return call(self, packed, desc, T)

    monkeypatch.setattr(ML.ClipResizer, "__call__", recording)

    def on_step(epoch, step, logits, label):
        if step == 0:
            first[epoch] = logits.float().cpu().clone()

    res, rows = _finetune(tmp_path, tree, "aug_a", {"enabled": True}, {"step": on_step})
    assert "[INFO] Augmentation:" in capsys.readouterr().out
    assert all(torch.isfinite(v).all() for v in res["model"].state_dict().values() if v.is_floating_point())
    assert res["checkpoints"] and all(p.exists() for p in res["checkpoints"])
    assert [r[0] for r in rows] == ["epoch", "1", "2"]
    # The step hook saw a first batch in both epochs.  That their logits differ would hold without
    # any augmentation (the weights and the shuffle change between epochs): the evidence for fresh
    # crops is the windows below, which the training loader alone received and which differ.
    assert sorted(first) == [1, 2] and not torch.equal(first[1], first[2])
    train = [d for d in descs if d.shape[1] == 8]
    val = [d for d in descs if d.shape[1] == 4]
    assert len(train) == 2 and len(val) == 4                    # 1 step, 2 validation batches per epoch
    assert not torch.equal(train[0][:, 3:], train[1][:, 3:])
    _, again = _finetune(tmp_path, tree, "aug_b", {"enabled": True})
    assert again == rows


def test_driver_with_augmentation_off_equals_a_config_without_the_section(tmp_path, tree, capsys):
    _, off = _finetune(tmp_path, tree, "off", {"enabled": False, "scale": [0.5, 0.9], "flip": 1.0})
    _, none = _finetune(tmp_path, tree, "none", None)
    assert "Augmentation" not in capsys.readouterr().out
    assert off == none and [r[0] for r in off] == ["epoch", "1", "2"]

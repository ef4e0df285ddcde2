"""sm_frames_resize_normalize on the GPU: bit-for-bit against tests/resize_mirror.py over the
kernel's paths (vector and scalar stores, staged and direct gather, more than one row band
and column tile, arbitrary byte offsets), the identity against sm_frames_normalize, the
bounds rules, the argument checks and the drivers' loader paths on frames that are not
`image_size`."""
import io

import numpy as np
import pytest
import torch
import yaml

import resize_mirror as M

pytestmark = pytest.mark.gpu

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _pack(clips, flags):
    """clips: uint8 [T,Hs,Ws,3] arrays or None (invalid) -> (packed, desc) numpy."""
    desc, parts, off = [], [], 0
    for c, fl in zip(clips, flags):
        if c is None:
            desc.append([off, 0, 0, fl | M.FLAG_INVALID])
            continue
        desc.append([off, c.shape[1], c.shape[2], fl])
        parts.append(c.reshape(-1))
        off += c.size
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return packed, np.asarray(desc, np.int64)


def _run(packed, desc, T, out_hw, bgr, packed_shift=0, out_shift=0):
    from ssl_mae_amd import kernels as K
    buf = torch.zeros(packed.size + packed_shift, dtype=torch.uint8, device="cuda")
    buf[packed_shift:].copy_(torch.from_numpy(packed))
    out = None
    if out_shift:
        n = len(desc) * 3 * T * out_hw[0] * out_hw[1]
        flat = torch.full((n + out_shift,), float("nan"), device="cuda")
        out = flat[out_shift:].view(len(desc), 3, T, *out_hw)
    got = K.frames_resize_normalize(buf[packed_shift:], torch.from_numpy(desc).cuda(), T, out_hw, MEAN, STD, bgr,
                                    out=out)
    return got.cpu().numpy()


def _rand(rng, T, hs, ws):
    return rng.integers(0, 256, (T, hs, ws, 3), dtype=np.uint8)


def _check(clips, flags, T, out_hw, **kw):
    packed, desc = _pack(clips, flags)
    for bgr in (True, False):
        exp = M.resize_normalize_batch(packed, desc, T, out_hw, MEAN, STD, bgr)
        got = _run(packed, desc, T, out_hw, bgr, **kw)
        assert got.shape == exp.shape
        assert np.array_equal(got, exp), (out_hw, bgr, float(np.abs(got - exp).max()))


# (Hs, Ws, Ho, Wo): non-integer downscale with odd Ws * 3; upscale with edge clamping; one
# pixel; Wo % 4 != 0 (scalar stores); Ho != Wo; more than one row band (Ho > 8)
@pytest.mark.parametrize("hs,ws,ho,wo", [(7, 9, 8, 8), (5, 3, 16, 16), (1, 1, 4, 4), (33, 17, 6, 6), (9, 11, 8, 12),
                                         (12, 20, 19, 13)])
def test_kernel_equals_mirror(hs, ws, ho, wo):
    rng = np.random.default_rng(hs * 100 + ws)
    clips = [_rand(rng, 2, hs, ws), _rand(rng, 2, hs, ws)]
    _check(clips, [0, M.FLAG_FLIP], 2, (ho, wo))


def test_ragged_batch_with_an_invalid_clip():
    rng = np.random.default_rng(1)
    clips = [_rand(rng, 3, 7, 9), None, _rand(rng, 3, 5, 3), _rand(rng, 3, 33, 17)]
    _check(clips, [M.FLAG_FLIP, M.FLAG_FLIP, 0, M.FLAG_FLIP], 3, (8, 8))
    _check(clips, [0, 0, M.FLAG_FLIP, 0], 3, (6, 6))


@pytest.mark.parametrize("wo", [8, 6])
def test_unaligned_packed_and_out_give_the_same_bits(wo):
    """packed 1 byte into its allocation (every staged row segment starts misaligned and the
    first dword straddles the start of the buffer); out 4 bytes in (scalar stores)."""
    rng = np.random.default_rng(2)
    clips = [_rand(rng, 2, 7, 9), _rand(rng, 2, 9, 11)]
    _check(clips, [0, M.FLAG_FLIP], 2, (8, wo), packed_shift=1)
    _check(clips, [0, M.FLAG_FLIP], 2, (8, wo), out_shift=1)
    _check(clips, [M.FLAG_FLIP, 0], 2, (8, wo), packed_shift=3, out_shift=1)


def test_rows_wider_than_the_staging_buffer_and_the_column_tile():
    """Two 8192-pixel source rows (48 KiB) exceed the 24 KiB the kernel stages: the direct
    gather.  1028 and 1030 output columns exceed the 1024-column tile: two column tiles, each
    staging its own row segments, with vector and with scalar stores."""
    rng = np.random.default_rng(3)
    wide = [_rand(rng, 1, 2, 8192), _rand(rng, 1, 2, 8192)]
    _check(wide, [0, M.FLAG_FLIP], 1, (3, 8))
    _check(wide, [M.FLAG_FLIP, 0], 1, (2, 1030))
    mid = [_rand(rng, 1, 3, 600), _rand(rng, 1, 3, 600)]
    _check(mid, [0, M.FLAG_FLIP], 1, (2, 1028))
    _check(mid, [M.FLAG_FLIP, 0], 1, (2, 1030))


@pytest.mark.parametrize("hs,ws,s", [(240, 320, 112), (112, 112, 224)])
def test_workload_sizes(hs, ws, s):
    rng = np.random.default_rng(s)
    clips = [_rand(rng, 2, hs, ws), _rand(rng, 2, hs, ws)]
    packed, desc = _pack(clips, [0, M.FLAG_FLIP])
    exp = M.resize_normalize_batch(packed, desc, 2, (s, s), MEAN, STD, True)
    assert np.array_equal(_run(packed, desc, 2, (s, s), True), exp)


@pytest.mark.parametrize("h,w", [(112, 112), (8, 12), (7, 9)])
def test_identity_equals_frames_normalize(h, w):
    from ssl_mae_amd import kernels as K
    rng = np.random.default_rng(h)
    u8 = rng.integers(0, 256, (3, 2, h, w, 3), dtype=np.uint8)
    packed, desc = _pack(list(u8), [0, 0, 0])
    for bgr in (True, False):
        ref = K.frames_normalize(torch.from_numpy(u8).cuda(), MEAN, STD, bgr).cpu().numpy()
        assert np.array_equal(_run(packed, desc, 2, (h, w), bgr), ref)


def test_out_of_range_descriptors_give_zero_clips():
    """Ordinary inputs the kernel must bound-check: a range past packed_bytes, a negative
    offset, Hs = 0 and a side above 8192 each yield a zero clip; their neighbours are intact."""
    rng = np.random.default_rng(4)
    a, b = _rand(rng, 2, 7, 9), _rand(rng, 2, 5, 3)
    packed, desc = _pack([a, a, b, b, a, b], [0] * 6)
    desc[1] = [packed.size - 10, 7, 9, 0]          # runs past the end of the buffer
    desc[3] = [desc[3][0], 0, 3, 0]                # Hs = 0
    desc[4] = [-4, 7, 9, 0]                        # starts before the buffer
    desc = np.concatenate([desc, [[0, 1, 8193, 0]]])
    exp = M.resize_normalize_batch(packed, desc, 2, (8, 8), MEAN, STD, True)
    got = _run(packed, desc, 2, (8, 8), True)
    for i in (1, 3, 4, 6):
        assert not got[i].any(), i
    for i in (0, 2, 5):
        assert got[i].any() and np.array_equal(got[i], exp[i]), i


def test_argument_validation():
    import ctypes
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd._lib import KernelError, ptr, stream
    packed = torch.zeros(2 * 4 * 4 * 3, dtype=torch.uint8, device="cuda")
    desc = torch.tensor([[0, 4, 4, 0]], device="cuda")
    out = torch.full((1, 3, 2, 8, 8), 7.0, device="cuda")
    m = (ctypes.c_float * 3)(*MEAN)
    s = (ctypes.c_float * 3)(*STD)
    mp, sp = ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p)

    def raw(p=ptr(packed), d=ptr(desc), n=packed.numel(), B=1, T=2, Ho=8, Wo=8, mean=mp, std=sp, o=ptr(out)):
        return K.query("sm_frames_resize_normalize", p, d, n, B, T, Ho, Wo, mean, std, 1, o, stream())

    assert raw(p=None) == -2 and raw(d=None) == -2 and raw(mean=None) == -2 and raw(std=None) == -2
    assert raw(o=None) == -2
    assert raw(B=-1) == -2 and raw(T=-1) == -2 and raw(Ho=-1) == -2 and raw(Wo=-1) == -2 and raw(n=-1) == -2
    assert raw(Ho=4097) == -2 and raw(Wo=4097) == -2
    assert raw(B=0) == 0 and raw(T=0) == 0 and raw(Ho=0, o=None) == 0          # empty output
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                            # nothing was launched
    assert raw() == 0
    assert np.array_equal(out.cpu().numpy(), M.resize_normalize_batch(np.zeros(96, np.uint8), desc.cpu().numpy(), 2,
                                                                      (8, 8), MEAN, STD, True))
    # the tensor-level wrapper
    for bad in (lambda: K.frames_resize_normalize(packed.float(), desc, 2, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed, desc.int(), 2, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed, desc.view(-1), 2, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed.view(2, -1), desc, 2, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed, desc.cpu(), 2, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed, desc, -1, (8, 8), MEAN, STD),
                lambda: K.frames_resize_normalize(packed, desc, 2, (8, 4097), MEAN, STD),
                lambda: K.frames_resize_normalize(packed[::2], desc, 2, (8, 8), MEAN, STD)):
        with pytest.raises(KernelError):
            bad()
    assert K.frames_resize_normalize(packed, desc[:0], 2, (8, 8), MEAN, STD).shape == (0, 3, 2, 8, 8)


def test_op_is_registered_with_a_fake():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ssl_mae_amd import ops
    with FakeTensorMode():
        y = ops.frames_resize_normalize(torch.empty(100, dtype=torch.uint8), torch.empty(3, 4, dtype=torch.int64), 2,
                                        (16, 12), MEAN, STD)
        assert y.shape == (3, 3, 2, 16, 12) and y.dtype == torch.float32


# ------------------------------------------------------------------ the drivers' loader paths
def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _frame_tree(root, n_videos=3, n_frames=8, hw=(24, 32)):
    """Lossless frames (PNG data under the .jpg names the dataset lists: PIL decodes by
    content) of `hw`; every video has exactly clip_len * stride = 8 frames, so the one
    possible start index is 0 and a clip does not depend on the order of the draws."""
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


def test_train_loader_path_resizes_to_image_size(tmp_path):
    from ssl_mae_amd import train_ssl_mae as TR
    from ssl_mae_amd.mae_loader import ClipResizer, LazyVideoMAEDataset
    split, videos = _frame_tree(tmp_path)
    ds = LazyVideoMAEDataset(str(split), clip_len=4, stride=2, image_size=16)
    loader = TR.make_loader(ds, batch_size=3, num_workers=0, shuffle=False)
    batches = [TR._to_clip(b, torch.device("cuda"), ClipResizer(16), 4) for b in loader]
    assert len(batches) == 1 and tuple(batches[0].shape) == (3, 3, 4, 16, 16)
    for i, frames in enumerate(videos):
        exp = M.resize_normalize(frames, (16, 16), MEAN, STD, bgr_swap=True)
        assert np.array_equal(batches[0][i].cpu().numpy(), exp), i


def test_temporal_and_dynamic_split_loaders_resize(tmp_path):
    from ssl_mae_amd import run_dynamic, temporal_ssl
    split, videos = _frame_tree(tmp_path)
    ds = {"split_root": "", "train_split": str(split), "split": str(split), "clip_len": 4, "stride": 2,
          "image_size": 16}
    exp = {bgr: [M.resize_normalize(f, (16, 16), MEAN, STD, bgr_swap=bgr) for f in videos] for bgr in (True, False)}
    clips = list(temporal_ssl.split_loader({"dataset": ds, "training": {"batch_size": 3, "num_workers": 0}}, "cuda"))
    assert len(clips) == 1 and tuple(clips[0].shape) == (3, 3, 4, 16, 16)
    got = clips[0].cpu().numpy()                    # shuffled: every clip is one of the expected, RGB order
    assert sorted(next(j for j in range(3) if np.array_equal(got[i], exp[False][j])) for i in range(3)) == [0, 1, 2]
    out = list(run_dynamic.split_loader({"dataset": ds, "runtime": {"batch_size": 2, "num_workers": 0}}, "cuda"))
    assert [tuple(c.shape) for c, _ in out] == [(2, 3, 4, 16, 16), (1, 3, 4, 16, 16)]
    assert torch.cat([l for _, l in out]).tolist() == [0, 1, 2]
    got = torch.cat([c for c, _ in out]).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[i], exp[True][i]), i


def test_main_trains_on_frames_that_are_not_image_size(tmp_path, monkeypatch):
    from ssl_mae_amd import train_ssl_mae as TR
    monkeypatch.chdir(tmp_path)
    split, _ = _frame_tree(tmp_path, n_videos=2, hw=(48, 80))
    cfg = {"dataset": {"train_split": str(split), "clip_len": 4, "stride": 2, "image_size": 64},
           "model": {"type": "tiny_vit_21m_variant", "decoder_embed_dim": 384, "decoder_depth": 2,
                     "decoder_num_heads": 6},
           "ssl": {"mask_ratio": 0.75, "mask_strategy": "tube", "norm_pix_loss": True},
           "training": {"epochs": 1, "batch_size": 2, "num_workers": 0, "lr": 5e-4, "weight_decay": 0.05,
                        "save_dir": str(tmp_path / "results" / "resize_test"), "log_interval": 20}}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    model = TR.main(["--config", str(p), "--max-steps", "1"])
    assert all(torch.isfinite(v).all() for v in model.state_dict().values() if v.is_floating_point())

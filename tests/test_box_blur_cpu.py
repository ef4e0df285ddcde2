"""The box blur's arithmetic and the host layers around sm_frames_box_blur / sm_box_region_stats,
without a GPU: the Gaussian weights, tests/blur_mirror.py against scipy's float64 correlation, the
reflect rule on frames smaller than the radius, the union semantics of the boxes, the statistics
on a hand-computed case, the box file, the image scan, the config rules and the CSV."""
import io
import math
import random

import numpy as np
import pytest
import torch

import blur_mirror as BM
from ssl_mae_amd import visual_privacy as V

KS = (3, 15, 31, 51, 63)


def test_gaussian_weights():
    for k, sigma in ((15, 2.6), (31, 5.0), (51, 8.0)):
        assert abs(V.gaussian_sigma(k) - sigma) < 1e-12
    for k in KS:
        w = V.gaussian_weights(k)
        assert w.dtype == np.float32 and w.shape == (k,)
        assert np.array_equal(w, w[::-1]) and w.argmax() == (k - 1) // 2
        s = np.float32(0)
        for x in w:
            s = s + x
        assert abs(float(s) - 1.0) <= 2.0 ** -20
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -20
    assert np.array_equal(V.gaussian_weights(30), V.gaussian_weights(31)) and V.odd_kernel(30) == 31
    assert V.odd_kernel(31) == 31


def _scipy_blur(u8, k):
    """float64 reference: correlate1d(mode="mirror") is reflect-101, periodic for short axes."""
    from scipy.ndimage import correlate1d
    w = V.gaussian_weights(k).astype(np.float64)
    x = u8.astype(np.float64)
    v = correlate1d(correlate1d(x, w, axis=1, mode="mirror"), w, axis=0, mode="mirror")
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("hw", [(40, 56), (120, 160)])
def test_mirror_against_scipy_float64(hw):
    """fp32 taps in a fixed order against float64: a pixel may land on the other side of a
    rounding boundary, never further than one grey level, and rarely (bounds set by the issue)."""
    u8 = np.random.default_rng(0).integers(0, 256, hw + (3,), dtype=np.uint8)
    for k in KS:
        got = BM.blur_frame(u8, V.gaussian_weights(k)).astype(np.int64)
        d = np.abs(got - _scipy_blur(u8, k).astype(np.int64))
        print(f"hw={hw} k={k}: max diff {int(d.max())}, fraction differing {float((d > 0).mean()):.2e}")
        assert d.max() <= 1, (hw, k)
        assert (d > 0).mean() <= 1e-3, (hw, k, float((d > 0).mean()))


def test_constant_frames_stay_constant():
    for val in (0, 1, 127, 200, 255):
        u8 = np.full((40, 56, 3), val, np.uint8)
        for k in KS:
            got = BM.blur_frame(u8, V.gaussian_weights(k)).astype(np.int64)
            d = np.abs(got - val)
            print(f"value={val} k={k}: max diff {int(d.max())}, fraction differing {float((d > 0).mean()):.2e}")
            assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (val, k)


def test_refl_on_short_axes():
    assert BM.refl(np.arange(-5, 6), 1).tolist() == [0] * 11
    assert BM.refl(np.arange(-5, 9), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert BM.refl(np.arange(-3, 8), 5).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert BM.refl(np.arange(-20, 21), 2).tolist() == [abs(i) % 2 for i in range(-20, 21)]
    rng = np.random.default_rng(1)
    for hw in ((1, 5), (7, 9)):                     # both axes shorter than r = 15
        u8 = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
        d = np.abs(BM.blur_frame(u8, V.gaussian_weights(31)).astype(np.int64) - _scipy_blur(u8, 31).astype(np.int64))
        assert d.max() <= 1, hw
    one = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)
    assert np.abs(BM.blur_frame(one, V.gaussian_weights(31)).astype(int) - one.astype(int)).max() <= 1


def _batch(frames):
    packed, desc = V.pack_frames(frames)
    return packed.numpy(), desc.numpy()


def _blur(frames, boxes_per_frame, k=15):
    packed, desc = _batch(frames)
    boxes, start = V.box_arrays(boxes_per_frame)
    mh, mw = max(f.shape[0] for f in frames), max(f.shape[1] for f in frames)
    return BM.box_blur_batch(packed, desc, boxes.numpy(), start.numpy(), V.gaussian_weights(k), mh, mw,
                             np.full(packed.size, 0xA5, np.uint8))


def test_union_semantics():
    rng = np.random.default_rng(2)
    fr = rng.integers(0, 256, (24, 30, 3), dtype=np.uint8)
    full = BM.blur_frame(fr, V.gaussian_weights(15))
    a, b = (3, 4, 10, 8), (9, 7, 12, 11)
    got = _blur([fr], [[a, b]]).reshape(24, 30, 3)
    m = BM.union_mask(np.asarray([a, b]), 24, 30)
    assert m.sum() == 10 * 8 + 12 * 11 - 4 * 5
    assert np.array_equal(got[~m], fr[~m]) and np.array_equal(got[m], full[m])
    for boxes in ([b, a], [a, b, a, a], [a, b, (0, 0, 0, 5), (2, 2, 5, -1), (40, 40, 3, 3), (-9, -9, 4, 4)]):
        assert np.array_equal(_blur([fr], [boxes]).reshape(24, 30, 3), got)
    # clipping: a negative origin keeps the part inside (the reference's slice would drop the box)
    got = _blur([fr], [[(-5, -3, 10, 8), (25, 20, 100, 100)]]).reshape(24, 30, 3)
    m = np.zeros((24, 30), bool)
    m[0:5, 0:5] = True
    m[20:24, 25:30] = True
    assert np.array_equal(BM.union_mask(np.asarray([(-5, -3, 10, 8), (25, 20, 100, 100)]), 24, 30), m)
    assert np.array_equal(got[~m], fr[~m]) and np.array_equal(got[m], full[m])
    # no boxes, only empty boxes: the frame itself
    for boxes in ([], [(3, 3, 0, 4), (3, 3, 4, 0), (-4, 0, 4, 4), (30, 0, 5, 5), (2 ** 31 - 1, 0, 2 ** 31 - 1, 5)]):
        assert np.array_equal(_blur([fr], [boxes]).reshape(24, 30, 3), fr)
    assert V.clip_box((-5, -3, 10, 8), 24, 30) == (0, 0, 5, 5) and V.clip_box((30, 0, 5, 5), 24, 30) is None


def test_invalid_frames_keep_the_prefill():
    rng = np.random.default_rng(3)
    fr = [rng.integers(0, 256, (5, 6, 3), dtype=np.uint8) for _ in range(3)]
    packed, desc = _batch(fr)
    desc[1] = [desc[1][0], 0, 6]
    desc[2] = [packed.size - 10, 5, 6]
    out = BM.box_blur_batch(packed, desc, np.zeros((0, 4)), np.zeros(4, np.int32), V.gaussian_weights(3), 5, 6,
                            np.full(packed.size, 0xA5, np.uint8))
    assert np.array_equal(out[:90], packed[:90]) and (out[90:] == 0xA5).all()
    out = BM.box_blur_batch(packed, desc, np.zeros((0, 4)), np.zeros(4, np.int32), V.gaussian_weights(3), 4, 6,
                            np.full(packed.size, 0xA5, np.uint8))
    assert (out == 0xA5).all()                       # H = 5 > max_h = 4


def test_region_stats_by_hand():
    a = np.zeros((3, 4, 3), np.uint8)
    b = np.zeros((3, 4, 3), np.uint8)
    a[..., 0] = [[1, 2, 4, 7], [0, 0, 0, 0], [5, 5, 5, 5]]
    b[..., 0] = [[1, 1, 1, 1], [0, 0, 0, 0], [5, 5, 5, 6]]
    a[..., 2] = 9
    # box x=2, y=0, w=5, h=2 -> clipped to columns 2..3, rows 0..1: P = 4
    boxes, start = np.asarray([[2, 0, 5, 2]]), np.asarray([0, 1])
    got = BM.region_stats(a.reshape(-1), b.reshape(-1), [[0, 3, 4]], boxes, start, 3, 4)
    # SSE: (4-1)^2 + (7-1)^2 + 4 pixels x 9^2 (channel 2)
    sse = 9 + 36 + 4 * 81
    # Ea, channel 0: (0,2): right (7-4)^2 = 9, down 16; (0,3): down 49; (1,2): down 25; (1,3): down 25; channel 2: flat
    ea = 9 + 16 + 49 + 25 + 25
    # Eb, channel 0: (0,2): down 1; (0,3): down 1; (1,2): down 25; (1,3): down 36
    eb = 1 + 1 + 25 + 36
    assert got.tolist() == [[4, sse, ea, eb]]
    assert BM.region_stats(a.reshape(-1), b.reshape(-1), [[0, 3, 4]], boxes, np.asarray([1, 0]), 3, 4).tolist() == [[0] * 4]
    s = V.summarise(got.tolist(), [(3, 4)], [1])
    assert s["frames_with_box"] == 1 and s["box_pixel_fraction"] == 4 / 12 and s["detail_retained"] == eb / ea
    assert s["psnr_box_db"] == 10 * math.log10(255.0 ** 2 / (sse / 12.0))


def test_pack_frames_frame_desc_and_check():
    from ssl_mae_amd._lib import KernelError
    from ssl_mae_amd.mae_loader import collate_raw
    rng = np.random.default_rng(4)
    a = torch.from_numpy(rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8))
    b = torch.from_numpy(rng.integers(0, 256, (2, 4, 3, 3), dtype=np.uint8))
    packed, dclip = collate_raw([(a, True), (a, False), (b, True)])
    d = V.frame_desc(dclip, 2)
    assert d.tolist() == [[0, 5, 7], [105, 5, 7], [210, 0, 0], [210, 0, 0], [210, 4, 3], [246, 4, 3]]
    V.BoxBlur.check(packed, d, [[]] * 6)
    p2, d2 = V.pack_frames([a[0].numpy(), b[1]])
    assert d2.tolist() == [[0, 5, 7], [105, 4, 3]] and torch.equal(p2, torch.cat([a[0].reshape(-1), b[1].reshape(-1)]))
    for bad in ([[0, 5, 7], [100, 5, 7]], [[0, 5, 7], [200, 5, 7]], [[-1, 5, 7]], [[0, 0, 7]], [[0, 1, 8193]]):
        with pytest.raises(KernelError):
            V.BoxBlur.check(packed, torch.tensor(bad), None)
    with pytest.raises(KernelError):
        V.BoxBlur.check(packed, d, [[]] * 5)
    with pytest.raises(KernelError):
        V.BoxBlur(31, device="cpu")(packed, torch.tensor([[0, 5, 7], [100, 5, 7]]), [[], []])   # before any upload
    with pytest.raises(Exception):                  # no CPU fallback: host tensors never reach a kernel
        V.BoxBlur(31, device="cpu")(packed, d, [[]] * 6)
    with pytest.raises(ValueError):
        V.BoxBlur(65)
    assert V.BoxBlur(30, device="cpu").ksize == 31


def test_read_boxes(tmp_path):
    f = tmp_path / "boxes.csv"
    f.write_text("# faces\npath,x,y,w,h\n\na/b.jpg,1,2,3,4\n  a/b.jpg , -5, 0, 7, 8\nc.png,0,0,1,1\n")
    assert V.read_boxes(f) == {"a/b.jpg": [(1, 2, 3, 4), (-5, 0, 7, 8)], "c.png": [(0, 0, 1, 1)]}
    for bad in ("a.jpg,1,2,3\n", "a.jpg,1,2,3,x\n", ",1,2,3,4\n", "a.jpg,1,2,3,4,5\n", "a.jpg,1,2,3,4.5\n"):
        f.write_text("# c\nok.jpg,1,1,1,1\n" + bad)
        with pytest.raises(ValueError, match="line 3"):
            V.read_boxes(f)


def test_scan_images(tmp_path):
    for name in ("b/2.jpg", "a/1.PNG", "a/0.jpeg", "a/x.txt", "c/d/3.jpg"):
        p = tmp_path / name
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"x")
    files = V.scan_images(tmp_path, 10, 42)
    assert [p.relative_to(tmp_path).as_posix() for p in files] == ["a/0.jpeg", "a/1.PNG", "b/2.jpg", "c/d/3.jpg"]
    assert V.scan_images(tmp_path, 2, 42) == random.Random(42).sample(files, 2)
    with pytest.raises(FileNotFoundError):
        V.scan_images(tmp_path / "missing", 10, 42)
    (tmp_path / "empty").mkdir()
    with pytest.raises(RuntimeError):
        V.scan_images(tmp_path / "empty", 10, 42)


def test_resolve_config_and_the_skipped_yunet_mode():
    import sys
    from ssl_mae_amd import run_privacy as RP
    vp = RP.resolve_config({})["visual_privacy"]
    assert vp["boxes_file"] is None and vp["batch_frames"] == 64 and vp["detector"] == "yunet" and not vp["enabled"]
    log = io.StringIO()
    assert RP.run_visual_privacy(RP.resolve_config({"visual_privacy": {"enabled": True}}), log) is None
    assert "OpenCV" in log.getvalue() and "skip" in log.getvalue() and "cv2" not in sys.modules
    # yunet mode validates as before: nothing about the method or the kernel is checked
    RP.resolve_config({"visual_privacy": {"enabled": True, "method": "pixelate", "blur_kernel": 101}})
    RP.resolve_config({"visual_privacy": {"enabled": False, "detector": "boxes", "method": "pixelate"}})
    ok = RP.resolve_config({"visual_privacy": {"enabled": True, "detector": "boxes", "blur_kernel": 30}})
    assert ok["visual_privacy"]["blur_kernel"] == 31
    assert RP.resolve_config({"visual_privacy": {"enabled": True, "detector": "boxes", "blur_kernel": 62}})[
        "visual_privacy"]["blur_kernel"] == 63
    for bad in ({"method": "pixelate"}, {"blur_kernel": 1}, {"blur_kernel": 2 - 2}, {"blur_kernel": 64},
                {"blur_kernel": 65}, {"batch_frames": 0}, {"frame_root": "frames"}, {"boxes": "x"}):
        with pytest.raises(ValueError):
            RP.resolve_config({"visual_privacy": dict({"enabled": True, "detector": "boxes"}, **bad)})


def test_csv_header_and_rounding():
    assert V.CSV_HEADER == ("frame_root,total_frames,frames_with_box,avg_boxes,box_pixel_fraction,blur_kernel,"
                            "psnr_box_db,detail_retained,seconds,overwrite_saved_root\n")
    row = {"frame_root": "data/frames", "total_frames": 6, "frames_with_box": 4, "avg_boxes": 4 / 3,
           "box_pixel_fraction": 0.123456789, "blur_kernel": 31, "psnr_box_db": 21.98765432, "detail_retained": 1 / 7,
           "seconds": 0.1234567, "overwrite_saved_root": ""}
    assert V.format_row(row) == "data/frames,6,4,1.333333,0.123457,31,21.987654,0.142857,0.123457,\n"
    row.update(psnr_box_db=math.inf, overwrite_saved_root="out")
    assert V.format_row(row).split(",")[6] == "inf" and V.format_row(row).endswith(",out\n")
    row.update(psnr_box_db=None)
    assert V.format_row(row).split(",")[6] == ""
    s = V.summarise([[0, 0, 0, 0]], [(4, 4)], [0])
    assert s["psnr_box_db"] is None and s["detail_retained"] == 0.0 and s["box_pixel_fraction"] == 0.0
    assert V.summarise([[4, 0, 8, 8]], [(4, 4)], [2])["psnr_box_db"] == math.inf


def test_synthetic_frames_are_deterministic():
    fa, ba = V.synthetic_frames(5, 7)
    fb, bb = V.synthetic_frames(5, 7)
    assert ba == bb and all(np.array_equal(x, y) for x, y in zip(fa, fb))
    assert all(f.shape == (240, 320, 3) for f in fa) and [len(b) for b in ba] == [1, 2, 1, 2, 1]
    assert all(V.clip_box(b, 240, 320) == (b[0], b[1], b[0] + b[2], b[1] + b[3]) for bs in ba for b in bs)

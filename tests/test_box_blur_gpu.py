"""sm_frames_box_blur and sm_box_region_stats on the GPU: bit for bit against tests/blur_mirror.py
on one batch that mixes frame sizes (smaller than the radius, odd byte offsets, several tiles per
axis) and box shapes, the validity rules, every copy width, determinism, the argument checks, the
torch.ops registration and BoxBlur in front of ClipResizer."""
import ctypes

import numpy as np
import pytest
import torch

import blur_mirror as BM
import resize_mirror as RM

pytestmark = pytest.mark.gpu

KS = (3, 15, 31, 63)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BIG = (70, 150)            # three 32 x 64 tiles on each axis, no multiple of either


def _weights(k):
    from ssl_mae_amd.visual_privacy import gaussian_weights
    return gaussian_weights(k)


def _mixed_batch():
    from ssl_mae_amd import visual_privacy as V
    rng = np.random.default_rng(11)
    sizes = [(1, 1), (1, 5), (7, 9), (40, 56), (33, 31), (33, 31), BIG, BIG, BIG, (40, 56)]
    frames = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes]
    boxes = [
        [(0, 0, 1, 1)],
        [(1, 0, 3, 1)],
        [(-2, -2, 5, 5), (6, 4, 10, 10)],
        [(-3, -3, 8, 8), (50, -2, 10, 6), (-4, 36, 9, 9), (52, 35, 20, 20)],     # partly outside at each corner
        [(0, 0, 31, 33)],                                                        # the whole frame
        [(5, 5, 0, 3), (5, 5, 3, -2), (10, 10, 4, 4), (12, 12, 6, 6)],           # w <= 0, h <= 0, two overlapping
        [],                                                                      # none
        [(0, 0, 150, 70)],                                                       # the whole frame, nine tiles
        [(60, 30, 10, 10), (100, 5, 1, 1), (5, 50, 20, 15), (30, 52, 20, 15),    # across a tile corner, 1 x 1, two
         (120, 60, 40, 20), (-10, -10, 20, 20), (126, 0, 4, 70)],                # closer than r, outside, a column strip
        [],
    ]
    packed, desc = V.pack_frames(frames)
    # 33 x 31 has rows of 93 bytes; one copy starts at an odd byte, the other on a multiple of 4
    assert desc[4, 0] % 2 == 1 and desc[5, 0] % 4 == 0
    b, s = V.box_arrays(boxes)
    return packed.numpy(), desc.numpy(), b.numpy(), s.numpy()


@pytest.fixture(scope="module")
def mixed():
    packed, desc, boxes, start = _mixed_batch()
    exp = {k: BM.box_blur_batch(packed, desc, boxes, start, _weights(k), 70, 150, np.full(packed.size, 0xA5, np.uint8))
           for k in KS}
    return packed, desc, boxes, start, exp


def _dev(a, shift=0, fill=0):
    """numpy 1-D uint8 -> device tensor that starts `shift` bytes into its allocation."""
    buf = torch.full((a.size + shift,), fill, dtype=torch.uint8, device="cuda")
    buf[shift:].copy_(torch.from_numpy(a))
    return buf[shift:]


def _run(packed, desc, boxes, start, k, max_h, max_w, packed_shift=0, out_shift=0):
    from ssl_mae_amd import kernels as K
    p = _dev(packed, packed_shift)
    out = _dev(np.full(packed.size, 0xA5, np.uint8), out_shift)
    d, b, s = (torch.from_numpy(x).cuda() for x in (desc, boxes.astype(np.int32), start.astype(np.int32)))
    got = K.frames_box_blur(p, d, b, s, _weights(k), max_h, max_w, out=out)
    assert got is out
    stats = K.box_region_stats(p, out, d, b, s, max_h, max_w)
    return out.cpu().numpy(), stats.cpu().numpy()


def _where(got, exp, desc):
    bad = np.nonzero(got != exp)[0]
    if bad.size == 0:
        return "equal"
    n = int(np.searchsorted(desc[:, 0], bad[0], side="right")) - 1
    return f"{bad.size} bytes differ, first at byte {bad[0]} (frame {n}), max |diff| {np.abs(got.astype(int) - exp).max()}"


@pytest.mark.parametrize("k", KS)
def test_kernel_equals_mirror(mixed, k):
    packed, desc, boxes, start, exp = mixed
    got, stats = _run(packed, desc, boxes, start, k, 70, 150)
    assert np.array_equal(got, exp[k]), (k, _where(got, exp[k], desc))
    again, stats2 = _run(packed, desc, boxes, start, k, 70, 150)
    assert np.array_equal(again, got) and np.array_equal(stats, stats2)          # two runs, the same bits
    want = BM.region_stats(packed, exp[k], desc, boxes, start, 70, 150)
    assert stats.dtype == np.int64 and np.array_equal(stats, want), (k, stats.tolist(), want.tolist())
    assert stats[6].tolist() == [0, 0, 0, 0] and stats[7, 0] == 70 * 150 and stats[0, 0] == 1


@pytest.mark.parametrize("packed_shift,out_shift", [(1, 1), (3, 19), (0, 4), (8, 4), (0, 1), (2, 5)])
def test_every_copy_width_gives_the_same_bits(mixed, packed_shift, out_shift):
    """packed and out congruent modulo 16 (16-byte copies from an unaligned base), modulo 4 only,
    and not at all (bytes); the blurred tiles' dword stores from an unaligned base."""
    packed, desc, boxes, start, exp = mixed
    got, stats = _run(packed, desc, boxes, start, 15, 70, 150, packed_shift, out_shift)
    assert np.array_equal(got, exp[15]), _where(got, exp[15], desc)
    assert np.array_equal(stats, BM.region_stats(packed, exp[15], desc, boxes, start, 70, 150))


def test_larger_bounds_and_box_order_do_not_change_the_bits(mixed):
    packed, desc, boxes, start, exp = mixed
    got, _ = _run(packed, desc, boxes, start, 31, 8192, 8192)
    assert np.array_equal(got, exp[31])
    rev = boxes.copy()
    for n in range(len(desc)):                       # every frame's boxes in reverse order
        rev[start[n]:start[n + 1]] = boxes[start[n]:start[n + 1]][::-1]
    got, _ = _run(packed, desc, rev, start, 31, 70, 150)
    assert np.array_equal(got, exp[31])


@pytest.mark.parametrize("packed_shift,out_shift", [(0, 0), (0, 4), (0, 1)])
def test_a_launch_without_boxes_is_a_copy(mixed, packed_shift, out_shift):
    """num_boxes == 0: the launch reserves no LDS and every tile takes the copy path."""
    packed, desc, _, start, _ = mixed
    got, stats = _run(packed, desc, np.zeros((0, 4), np.int32), np.zeros_like(start), 63, 70, 150, packed_shift,
                      out_shift)
    assert np.array_equal(got, packed) and not stats.any()


def test_validity_rules_keep_the_prefill_and_zero_stats(mixed):
    """Ordinary inputs the kernel must bound-check, the way test_resize_gpu.py checks its zero-clip
    rule: a range past packed_bytes, a negative offset, H = 0, a side above 8192 and a frame above
    max_h are not written (0xA5 stays) and have zero stats; out-of-range and reversed box_start
    entries behave as clamped."""
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in [(9, 12), (9, 12), (9, 12), (20, 12), (9, 12),
                                                                         (9, 12), (9, 12)]]
    from ssl_mae_amd import visual_privacy as V
    packed, desc = V.pack_frames(frames)
    packed, desc = packed.numpy(), desc.numpy()
    desc[1] = [packed.size - 10, 9, 12]              # runs past the end of the buffer
    desc[2] = [desc[2][0], 0, 12]                    # H = 0
    # frame 3 has H = 20 > max_h = 9
    desc[5] = [-4, 9, 12]                            # starts before the buffer
    desc = np.concatenate([desc, [[0, 1, 8193]]])
    boxes = np.asarray([[2, 2, 5, 5]] * 6 + [[0, 0, 3, 3], [4, 4, 8, 8]], np.int64)
    # frame 0: [-3, 2) -> [0, 2); 1: [2, 1) reversed; 2..3: own boxes; 4: [4, 99) -> [4, 8); 5: [99, 6) reversed;
    # 6: [6, 8); 7: [8, 8)
    start = np.asarray([-3, 2, 1, 3, 4, 99, 6, 8, 8], np.int64)
    w = _weights(15)
    exp = BM.box_blur_batch(packed, desc, boxes, start, w, 9, 12, np.full(packed.size, 0xA5, np.uint8))
    got, stats = _run(packed, desc, boxes, start, 15, 9, 12)
    assert np.array_equal(got, exp), _where(got, exp, desc[:7])
    want = BM.region_stats(packed, exp, desc, boxes, start, 9, 12)
    assert np.array_equal(stats, want)
    for n in (1, 2, 3, 5, 7):
        assert stats[n].tolist() == [0, 0, 0, 0], n
    for n, (off, h, wd) in ((2, (648, 9, 12)), (3, (972, 20, 12))):              # skipped: the prefill is intact
        assert (got[off:off + h * wd * 3] == 0xA5).all(), n
    # (4, 4, 8, 8) is clipped to 8 x 5 in the 9 x 12 frame; it shares 3 x 3 with (2, 2, 5, 5), which shares 1 with (0, 0, 3, 3)
    assert stats[0, 0] == 25 and stats[4, 0] == 25 + 9 + 40 - 1 - 9 and stats[6, 0] == 9 + 40
    assert np.array_equal(got[:324], exp[:324]) and not np.array_equal(got[:324], packed[:324])


def test_argument_validation():
    from ssl_mae_amd import kernels as K
    from ssl_mae_amd._lib import KernelError, ptr, stream
    packed = torch.zeros(4 * 4 * 3, dtype=torch.uint8, device="cuda")
    other = torch.zeros_like(packed)
    desc = torch.tensor([[0, 4, 4]], device="cuda")
    boxes = torch.tensor([[0, 0, 2, 2]], dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    out = torch.full_like(packed, 7)
    stats = torch.full((1, 4), 7, dtype=torch.int64, device="cuda")
    wv = (ctypes.c_float * 63)(*([1.0 / 3] * 63))
    wp = ctypes.cast(wv, ctypes.c_void_p)

    def blur(p=ptr(packed), d=ptr(desc), n=packed.numel(), N=1, mh=4, mw=4, b=ptr(boxes), s=ptr(start), nb=1, w=wp,
             k=3, o=ptr(out)):
        return K.query("sm_frames_box_blur", p, d, n, N, mh, mw, b, s, nb, w, k, o, stream())

    def st(a=ptr(packed), b2=ptr(other), d=ptr(desc), n=packed.numel(), N=1, mh=4, mw=4, b=ptr(boxes), s=ptr(start),
           nb=1, o=ptr(stats)):
        return K.query("sm_box_region_stats", a, b2, d, n, N, mh, mw, b, s, nb, o, stream())

    for null in ("p", "d", "b", "s", "w", "o"):
        assert blur(**{null: None}) == -2, null
    for null in ("a", "b2", "d", "b", "s", "o"):
        assert st(**{null: None}) == -2, null
    for f in (blur, st):
        assert f(N=-1) == -2 and f(nb=-1) == -2 and f(n=-1) == -2
        assert f(mh=0) == -2 and f(mw=0) == -2 and f(mh=8193) == -2 and f(mw=8193) == -2
        assert f(N=2 ** 31 - 1, mh=64, mw=64) == -2          # N x 2 x 1 tiles exceed 2^31 - 1 blocks
        assert f(N=0) == 0 and f(N=0, d=None, o=None) == 0
        assert f(b=None, nb=0) == 0                           # no boxes: the array may be absent
    for k in (1, 2, 4, 62, 64, 65, -3):
        assert blur(k=k) == -2, k
    assert blur(o=ptr(packed)) == -2                          # out == packed
    both = torch.zeros(96, dtype=torch.uint8, device="cuda")  # out a shifted view of packed's storage: -2 either way
    assert blur(p=ptr(both[:48]), o=ptr(both[16:64])) == -2 and blur(p=ptr(both[16:64]), o=ptr(both[:48])) == -2
    assert blur(p=ptr(both[:48]), o=ptr(both[47:95])) == -2
    torch.cuda.synchronize()
    assert bool((out == 0).all())                             # only the two valid no-box calls wrote: a copy
    assert stats.tolist() == [[0, 0, 0, 0]]
    out.fill_(7)
    assert blur(N=-1) == -2 and blur(k=4) == -2 and blur(o=None) == -2
    torch.cuda.synchronize()
    assert bool((out == 7).all())                             # nothing was launched
    assert K.box_launch_max_frames(64, 64) == (2 ** 31 - 1) // 2
    # the tensor-level wrappers
    w3 = [0.25, 0.5, 0.25]
    for bad in (lambda: K.frames_box_blur(packed.float(), desc, boxes, start, w3, 4, 4),
                lambda: K.frames_box_blur(packed, desc.int(), boxes, start, w3, 4, 4),
                lambda: K.frames_box_blur(packed, desc, boxes.long(), start, w3, 4, 4),
                lambda: K.frames_box_blur(packed, desc, boxes, start[:1], w3, 4, 4),
                lambda: K.frames_box_blur(packed, desc.cpu(), boxes, start, w3, 4, 4),
                lambda: K.frames_box_blur(packed, desc, boxes, start, w3 + [0.0], 4, 4),
                lambda: K.frames_box_blur(packed, desc, boxes, start, [1.0], 4, 4),
                lambda: K.frames_box_blur(packed, desc, boxes, start, w3, 0, 4),
                lambda: K.frames_box_blur(packed, desc, boxes, start, w3, 4, 4, out=packed),
                lambda: K.frames_box_blur(both[:48], desc, boxes, start, w3, 4, 4, out=both[40:88]),
                lambda: K.frames_box_blur(packed, desc, boxes, start, w3, 4, 4, out=out[:-1]),
                lambda: K.box_region_stats(packed, other[:-1], desc, boxes, start, 4, 4),
                lambda: K.box_region_stats(packed, other, desc, boxes, start, 4, 4, stats=stats.int())):
        with pytest.raises(KernelError):
            bad()
    got = K.frames_box_blur(packed[:0], desc[:0], boxes, start[:1], w3, 4, 4)
    assert got.numel() == 0 and K.box_region_stats(packed[:0], other[:0], desc[:0], boxes, start[:1], 4, 4).shape == (0, 4)


def test_ops_are_registered_with_fakes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ssl_mae_amd import ops
    assert hasattr(torch.ops.ssl_mae, "frames_box_blur") and hasattr(torch.ops.ssl_mae, "box_region_stats")
    with FakeTensorMode():
        p = torch.empty(100, dtype=torch.uint8)
        d, b, s = torch.empty(3, 3, dtype=torch.int64), torch.empty(5, 4, dtype=torch.int32), torch.empty(4, dtype=torch.int32)
        y = ops.frames_box_blur(p, d, b, s, [0.25, 0.5, 0.25], 8, 8)
        assert y.shape == (100,) and y.dtype == torch.uint8
        z = ops.box_region_stats(p, y, d, b, s, 8, 8)
        assert z.shape == (3, 4) and z.dtype == torch.int64
    packed = torch.arange(48, dtype=torch.uint8, device="cuda")
    desc = torch.tensor([[0, 4, 4]], device="cuda")
    boxes = torch.tensor([[1, 1, 2, 2]], dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    w3 = np.asarray([0.25, 0.5, 0.25], np.float32)
    y = ops.frames_box_blur(packed, desc, boxes, start, w3, 4, 4)
    exp = BM.box_blur_batch(packed.cpu().numpy(), [[0, 4, 4]], [[1, 1, 2, 2]], [0, 1], w3, 4, 4, np.zeros(48, np.uint8))
    assert np.array_equal(y.cpu().numpy(), exp)
    assert ops.box_region_stats(packed, y, desc, boxes, start, 4, 4).cpu().numpy().tolist() == \
        BM.region_stats(packed.cpu().numpy(), exp, [[0, 4, 4]], [[1, 1, 2, 2]], [0, 1], 4, 4).tolist()


def test_box_blur_then_clip_resizer():
    """An anonymised 2-clip collate_raw batch goes straight into sm_frames_resize_normalize: equal to
    the mirror blur followed by resize_mirror; more launches than one give the same bytes."""
    from ssl_mae_amd import visual_privacy as V
    from ssl_mae_amd.mae_loader import ClipResizer, collate_raw
    rng = np.random.default_rng(13)
    T = 2
    a = torch.from_numpy(rng.integers(0, 256, (T, 24, 32, 3), dtype=np.uint8))
    b = torch.from_numpy(rng.integers(0, 256, (T, 20, 70, 3), dtype=np.uint8))
    packed, dclip = collate_raw([(a, True), (b, True, True)])
    dframe = V.frame_desc(dclip, T)
    per_frame = [[(4, 4, 12, 10)], [], [(-3, 5, 40, 9), (60, 0, 20, 20)], [(10, 2, 5, 5)]]
    blur = V.BoxBlur(15)
    blurred = blur(packed, dframe, per_frame)
    assert blurred.is_cuda and blurred.dtype == torch.uint8 and blurred.shape == packed.shape
    boxes, start = V.box_arrays(per_frame)
    exp = BM.box_blur_batch(packed.numpy(), dframe.numpy(), boxes.numpy(), start.numpy(), blur.weights, 24, 70,
                            np.zeros(packed.numel(), np.uint8))
    assert np.array_equal(blurred.cpu().numpy(), exp)
    split, stats = V.BoxBlur(15, max_frames_per_launch=3)(packed, dframe, per_frame, with_stats=True)
    assert torch.equal(split, blurred)
    assert np.array_equal(stats.cpu().numpy(), BM.region_stats(packed.numpy(), exp, dframe.numpy(), boxes.numpy(),
                                                               start.numpy(), 24, 70))
    clip = ClipResizer(16)(blurred, dclip, T)
    want = RM.resize_normalize_batch(exp, dclip.numpy(), T, (16, 16), MEAN, STD, True)
    assert np.array_equal(clip.cpu().numpy(), want)

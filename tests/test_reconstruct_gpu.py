"""sm_mae_reconstruct / sm_recon_clip_metrics on the GPU against the fp64 mirror
(tests/recon_mirror.py), on random predictions (no model), and the visualiser end to end.

Tolerances.  token_err and clip_metrics: 1e-5 relative to the fp64 mirror, entry by entry (an entry
the mirror has as 0 must be 0), the project's tolerance for fused reductions (SURVEY.md §8(a) row
A3); n_masked is exact.  recon is held to 1e-5 of its largest magnitude, as the vector outputs in
tests/test_privacy_gpu.py are: its values cross zero (r = pred * sd + mu and v = r * std + mean
cancel), so an fp32 chain cannot hold 1e-5 of every single element whatever its order.

Bytes.  Each byte equals the mirror's, except where the mirror's v * 255 lies within 1e-3 of an
integer; there it may differ by one.  Eight fp32 roundings on magnitudes up to 10 give less than
3e-4 at scale 255 (a CPU fp32-against-fp64 run of the chain on 15.7 M values gave 53 mismatches,
all within 2.2e-5 of a boundary).  Every case also asserts that at least 99 % of its bytes were
compared exactly: the mirror alone leaves about 0.2 % of Gaussian inputs that close to a boundary."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import recon_mirror as RM

pytestmark = pytest.mark.gpu
DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHAPES = [(2, 2, 16, 16), (1, 1, 8, 8), (2, 3, 16, 24)]      # (B, T, H, W); hp != wp in the last
FLAGS = list(itertools.product((True, False), repeat=3))    # norm_pix, paste_visible, bgr_swap


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(shape, dtype=torch.float32, layout="contiguous", mask_kind="tube", scale=1.0, const_patch=False, seed=0):
    """-> pred (device, dtype), clip (device, fp32 [B,3,T,H,W]), mask uint8 [B,T,L] (device)."""
    B, T, H, W = shape
    L = (H // 8) * (W // 8)
    g = torch.Generator().manual_seed(1000 * seed + B * 131 + T * 17 + H + W)
    x = torch.randn(B, 3, T, H, W, generator=g) * scale
    if const_patch:                       # token (b=0, t=0, l=0): 3 * 0.5 is exact in fp32, so mu = 0.5, var = 0
        x[0, :, 0, :8, :8] = 0.5 * scale
    if layout == "contiguous":
        clip = x.to(DEV)
    else:                                 # every stride differs from the dense one, and an offset
        base = torch.zeros(B, T, H, W + 1, 4)
        base[:, :, :, 1:, 1:] = x.permute(0, 2, 3, 4, 1)
        clip = base.to(DEV).permute(0, 4, 1, 2, 3)[:, 1:, :, :, 1:]
        assert clip.shape == x.shape and clip.stride(1) == 1 and clip.stride(4) == 4
    pred = torch.randn(B, T * L, 192, generator=g).to(dtype).to(DEV)
    if mask_kind == "zeros":
        mask = torch.zeros(B, T, L, dtype=torch.uint8)
    elif mask_kind == "ones":
        mask = torch.ones(B, T, L, dtype=torch.uint8)
    else:
        keep = torch.rand(B, 1, L, generator=g)
        mask = (keep >= keep.median(dim=2, keepdim=True).values).expand(B, T, L).to(torch.uint8)
    return pred, clip, mask.contiguous().to(DEV)


def _check(pred, clip, mask, flags, what=""):
    from ssl_mae_amd import ops
    norm_pix, paste, bgr = flags
    panels, recon, te = ops.mae_reconstruct(pred, clip, mask, MEAN, STD, norm_pix, paste, bgr)
    cm = ops.recon_clip_metrics(te, mask)
    want = RM.reconstruct(pred.float(), clip, mask, MEAN, STD, norm_pix, paste, bgr)
    B, _, T, H, W = clip.shape
    assert panels.shape == (B, T, H, 3 * W, 3) and panels.dtype == torch.uint8
    assert recon.shape == (B, 3, T, H, W) and te.shape == (mask.numel(), 2) and cm.shape == (B, 4)
    te, recon, cm = te.double().cpu().reshape(B, -1, 2), recon.double().cpu(), cm.double().cpu()
    for j in range(2):
        w = want["token_err"][..., j]
        d = (te[..., j] - w).abs()
        e = float((d[w != 0] / w[w != 0]).max()) if bool((w != 0).any()) else 0.0
        print(f"{what} token_err[{j}] err {e:.3e}, smallest non-zero entry {float(w[w != 0].min()) if e else 0.0:.3e}")
        assert e <= 1e-5 and float(d[w == 0].max() if bool((w == 0).any()) else 0.0) == 0.0, (what, j, e)
    e = float((recon - want["recon"]).abs().max()) / float(want["recon"].abs().max())
    print(f"{what} recon err {e:.3e}")
    assert e <= 1e-5, (what, e)
    wcm = want["clip_metrics"]
    assert torch.equal(cm[:, 3], wcm[:, 3]), what
    for j in range(3):
        for b in range(B):
            g, w = float(cm[b, j]), float(wcm[b, j])
            print(f"{what} clip_metrics[{b}][{j}] {g!r} want {w!r}")
            assert (g == w) if np.isinf(w) else abs(g - w) <= 1e-5 * abs(w), (what, b, j, g, w)
    got = panels.cpu().to(torch.int16)
    diff = (got - want["panels"].to(torch.int16)).abs()
    near = want["near"]
    exact = float((~near).double().mean())
    print(f"{what} bytes: {exact:.4%} compared exactly, {int((diff > 0).sum())} differ")
    assert int(diff[~near].max() if (~near).any() else 0) == 0, (what, int((diff[~near] > 0).sum()))
    assert int(diff.max()) <= 1, what
    assert exact >= 0.99, (what, exact)
    return panels, recon, te, cm


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_flag_combination(shape, dtype):
    pred, clip, mask = _inputs(shape, dtype)
    for flags in FLAGS:
        _check(pred, clip, mask, flags, f"{shape} {dtype} {flags}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1, 16, 24), (1, 3, 8, 8), (3, 1, 8, 24)], ids=lambda s: "x".join(map(str, s)))
def test_partial_token_groups(shape, dtype):
    """A wave takes four consecutive tokens: 6, 3 and 9 tokens leave a last group of 2, 3 and 1,
    and the groups of the first and the last shape run across patch rows and clips."""
    pred, clip, mask = _inputs(shape, dtype, seed=8)
    for flags in ((True, True, True), (False, False, False)):
        _check(pred, clip, mask, flags, f"{shape} {dtype} {flags}")


@pytest.mark.parametrize("mask_kind", ["zeros", "ones", "tube"])
@pytest.mark.parametrize("layout", ["contiguous", "view"])
def test_clip_layouts_and_masks(layout, mask_kind):
    for dtype in (torch.float32, torch.bfloat16):
        pred, clip, mask = _inputs(SHAPES[2], dtype, layout, mask_kind, seed=1)
        for flags in ((True, True, True), (False, False, False)):
            _, _, _, cm = _check(pred, clip, mask, flags, f"{layout} {mask_kind} {dtype} {flags}")
            if mask_kind == "zeros":       # nothing masked: means 0, PSNR +inf
                assert float(cm[:, :2].abs().max()) == 0.0 and bool(torch.isinf(cm[:, 2]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_both_clamps_fire(dtype):
    pred, clip, mask = _inputs(SHAPES[2], dtype, scale=3.0, seed=2)
    for flags in ((True, True, True), (False, True, False)):
        panels, recon, _, _ = _check(pred, clip, mask, flags, f"x3 {dtype} {flags}")
        assert float(recon.min()) < -1.0 and float(recon.max()) > 2.0
        assert int(panels.min()) == 0 and int(panels.max()) == 255


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_constant_patch(dtype):
    """var = 0: the target is 0 and the reconstruction pred * 1e-3 + mu."""
    pred, clip, mask = _inputs(SHAPES[0], dtype, const_patch=True, seed=3)
    mask[0, :, 0] = 1
    _, recon, te, _ = _check(pred, clip, mask, (True, False, True), f"const {dtype}")
    p0 = pred[0, 0].double().cpu()
    assert abs(float(te[0, 0, 0]) - float((p0 ** 2).mean())) <= 1e-5 * float((p0 ** 2).mean())
    patch = recon[0, :, 0, :8, :8]
    want = (0.5 * torch.tensor(STD, dtype=torch.float64) + torch.tensor(MEAN, dtype=torch.float64)).view(3, 1, 1)
    assert float((patch - want).abs().max()) < 5e-3 * 0.3 and float(patch.std()) > 0


@pytest.mark.parametrize("T,L", [(1, 1), (3, 85), (1, 257)], ids=["TL1", "TL255", "TL257"])
def test_clip_metrics_token_counts(T, L):
    """sm_recon_clip_metrics on its own over T L = 1, 255 and 257 tokens per clip (a block's 256 strided
    sums hold one term, one term in all but the last thread, and two terms in thread 0) against the
    mirror's fp64 masked means, to the 1e-5 of _check; clip 0 all masked, clip 1 about half."""
    from ssl_mae_amd import ops
    B = 2
    g = torch.Generator().manual_seed(T * 1000 + L)
    te = torch.rand(B * T * L, 2, generator=g) * 0.5 + 0.01        # pixel error <= 0.51: PSNR >= 2.9 dB, away from 0
    mask = torch.ones(B, T, L, dtype=torch.uint8)
    mask[1] = (torch.rand(T, L, generator=g) < 0.5).to(torch.uint8)
    mask[1, 0, 0] = 1
    cm = ops.recon_clip_metrics(te.to(DEV), mask.to(DEV)).double().cpu()
    err, m = te.double().reshape(B, T * L, 2), mask.reshape(B, T * L).bool()
    for b in range(B):
        n = int(m[b].sum())
        en, mse = float(err[b, m[b], 0].sum() / n), float(err[b, m[b], 1].sum() / n)
        want = (en, mse, 10.0 * np.log10(1.0 / mse))
        print(f"T L = {T * L}, clip {b}: n {n}, got {cm[b].tolist()}, want {want}")
        assert float(cm[b, 3]) == n
        for j in range(3):
            assert abs(float(cm[b, j]) - want[j]) <= 1e-5 * abs(want[j]), (b, j)


def test_pixel_error_zero_gives_infinite_psnr():
    """norm_pix off and pred = patchify(clip): both errors are exactly 0 on masked tokens."""
    _, clip, mask = _inputs(SHAPES[2], mask_kind="ones", seed=4)
    pred = RM.patchify(clip.cpu()).to(DEV)
    _, _, te, cm = _check(pred, clip, mask, (False, True, True), "exact")
    assert float(te.abs().max()) == 0.0 and float(cm[:, :2].abs().max()) == 0.0 and bool(torch.isinf(cm[:, 2]).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_loss_map_is_consistent_with_the_training_loss(dtype):
    from ssl_mae_amd import ops
    for norm_pix in (True, False):
        pred, clip, mask = _inputs(SHAPES[2], dtype, seed=5)
        _, _, te = ops.mae_reconstruct(pred, clip, mask, MEAN, STD, norm_pix, True, True)
        loss = float(ops.mae_loss_fwd(pred, clip, mask, norm_pix)[0])
        m = mask.reshape(-1).double()
        mean = float((te[:, 0].double() * m).sum() / m.sum())
        print(f"{dtype} norm_pix={norm_pix}: masked mean {mean!r} loss {loss!r}")
        assert abs(mean - loss) <= 1e-5 * abs(loss)


def test_two_calls_are_bit_identical():
    from ssl_mae_amd import ops
    pred, clip, mask = _inputs(SHAPES[2], torch.bfloat16, seed=6)
    a = ops.mae_reconstruct(pred, clip, mask, MEAN, STD)
    b = ops.mae_reconstruct(pred, clip, mask, MEAN, STD)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(ops.recon_clip_metrics(a[2], mask).view(torch.int32),
                       ops.recon_clip_metrics(b[2], mask).view(torch.int32))
    assert ops.mae_reconstruct(pred, clip, mask, MEAN, STD, want_recon=False)[1].numel() == 0


def _raw(pred, clip, mask, panels, recon, te, flags=(1, 1, 1)):
    """The C entry point on caller-owned buffers; returns its status."""
    from ssl_mae_amd import _lib
    B, _, T, H, W = clip.shape
    m = (ctypes.c_float * 3)(*MEAN)
    s = (ctypes.c_float * 3)(*STD)
    return _lib.query("sm_mae_reconstruct", _lib.dt(pred), _lib.ptr(pred), _lib.ptr(clip), *clip.stride(),
                      _lib.ptr(mask), B, T, H, W, ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
                      *flags, _lib.ptr(panels), _lib.ptr(recon), _lib.ptr(te), _lib.stream())


def test_unaligned_panels_take_byte_stores_with_the_same_bits():
    """The packed-dword panel stores need a 4-byte aligned base; any other base, and a pred that
    starts on an odd bf16 element, give the same outputs."""
    from ssl_mae_amd import ops
    pred, clip, mask = _inputs(SHAPES[2], torch.bfloat16, seed=7)
    want = ops.mae_reconstruct(pred, clip, mask, MEAN, STD)
    shifted = torch.empty(pred.numel() + 1, dtype=torch.bfloat16, device=DEV)[1:].view(pred.shape)
    shifted.copy_(pred)
    assert shifted.data_ptr() % 4 == 2 and shifted.is_contiguous()
    got = ops.mae_reconstruct(shifted, clip, mask, MEAN, STD)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    raw = torch.full((want[0].numel() + 1,), 7, dtype=torch.uint8, device=DEV)
    panels = raw[1:].view(want[0].shape)
    assert panels.data_ptr() % 4 == 1
    recon, te = torch.empty_like(want[1]), torch.empty_like(want[2])
    assert _raw(pred, clip, mask, panels, recon, te) == 0
    assert torch.equal(panels, want[0]) and torch.equal(recon, want[1]) and torch.equal(te, want[2])
    assert int(raw[0]) == 7


def test_refused_arguments_launch_nothing():
    from ssl_mae_amd import _lib, kernels
    B, T, H, W = 1, 1, 12, 16
    L = (H // 8) * (W // 8)
    pred = torch.zeros(B, T * L, 192, device=DEV)
    clip = torch.zeros(B, 3, T, H, W, device=DEV)
    mask = torch.ones(B, T, L, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.KernelError, match="status -2"):
        kernels.mae_reconstruct(pred, clip, mask, MEAN, STD)
    panels = torch.full((B, T, H, 3 * W, 3), 7, dtype=torch.uint8, device=DEV)
    recon = torch.full((B, 3, T, H, W), -1.0, device=DEV)
    te = torch.full((B * T * L, 2), -1.0, device=DEV)
    assert _raw(pred, clip, mask, panels, recon, te) == -2
    clip8 = torch.zeros(B, 3, T, 16, 16, device=DEV)
    assert _raw(pred, clip8, mask, None, recon, te) == -2                       # a null output
    torch.cuda.synchronize()
    assert bool((panels == 7).all()) and bool((recon == -1).all()) and bool((te == -1).all())


# ------------------------------------------------------------------ end to end
def test_visualize_end_to_end(tmp_path):
    from PIL import Image
    from ssl_mae_amd import visualize_mae as V
    from ssl_mae_amd.checkpoint import save_training_state
    from ssl_mae_amd.train_ssl_mae import build_model
    B, T, S = 2, 2, 32                                                       # the step_b2_t2_s32 fixture's config
    cfg = {"dataset": {"clip_len": T, "image_size": S, "stride": 4, "train_split": "-"},
           "model": {"decoder_embed_dim": 384, "decoder_depth": 4, "decoder_num_heads": 6},
           "ssl": {"mask_ratio": 0.75, "norm_pix_loss": True}, "training": {"batch_size": B}}
    torch.manual_seed(11)
    model = build_model(cfg, "cpu")
    ckpt = tmp_path / "last_state.pth"
    save_training_state(ckpt, model, torch.optim.SGD(model.parameters(), lr=0.1), None, 1)
    frames_dir = tmp_path / "frames"
    frames_dir.mkdir()
    frames = np.random.default_rng(5).integers(0, 256, (B * T, S, S, 3), dtype=np.uint8)
    for i, f in enumerate(frames):
        Image.fromarray(f).save(frames_dir / f"img_{i:05d}.png")
    out = tmp_path / "out"
    rec = V.visualize(str(ckpt), str(frames_dir), str(out), config=cfg, mask_ratio=0.75, clips=B, sweep=True)
    assert rec.format == "training_state"
    L = (S // 8) ** 2
    assert rec.panels.shape == (B, T, S, 3 * S, 3) and rec.token_err.shape == (B, T, L, 2)
    panels = rec.panels.cpu().numpy()
    for i in range(T):
        assert np.array_equal(np.asarray(Image.open(out / f"frame_{i:02d}.png")), panels[0, i])
    assert not (out / f"frame_{T:02d}.png").exists()
    # the left panel is the input frame again: /255 -> normalise -> de-normalise -> floor has one level of slack
    left = panels[:, :, :, :S].astype(np.int16)
    assert int(np.abs(left - frames.reshape(B, T, S, S, 3).astype(np.int16)).max()) <= 1
    mask = rec.mask.cpu().numpy().astype(bool)
    up = np.repeat(np.repeat(mask.reshape(B, T, S // 8, S // 8), 8, axis=2), 8, axis=3)
    mid = panels[:, :, :, S:2 * S]
    assert np.array_equal(mid, panels[:, :, :, :S] * ~up[..., None])
    lines = (out / "reconstruction.csv").read_text().splitlines()
    assert lines[0] + "\n" == V.CSV_HEADER and len(lines) == 1 + B + 3
    cm = rec.clip_metrics.cpu().numpy()
    assert np.all(cm[:, 3] == T * int(0.75 * L))
    for b in range(B):
        cells = lines[1 + b].split(",")
        assert cells[0] == str(b) and float(cells[1]) == 0.75 and int(cells[2]) == int(cm[b, 3])
        assert [float(c) for c in cells[3:]] == [float(cm[b, 0]), float(cm[b, 1]), float(cm[b, 2])]
    for row, line, ratio in zip(rec.rows, lines[1 + B:], (0.5, 0.75, 0.9)):
        cells = line.split(",")
        assert cells[0] == "mean" and float(cells[1]) == ratio == row["mask_ratio"]
        assert float(cells[2]) == row["n_masked"] == T * int(ratio * L)
        assert np.isfinite(row["loss_norm"]) and row["mse_pix"] > 0 and np.isfinite(row["psnr_db"])
    err = np.load(out / "token_err.npy")
    assert err.shape == (B, T, L) and np.all(err[~mask] == 0) and np.all(err[mask] > 0)
    assert np.array_equal(err[mask], rec.token_err[..., 0].cpu().numpy()[mask])
    try:
        import matplotlib  # noqa: F401
        assert (out / "mask_grid.png").exists() and (out / "token_err.png").exists()
    except ImportError:
        assert not (out / "mask_grid.png").exists()

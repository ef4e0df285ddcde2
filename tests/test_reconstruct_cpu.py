"""CPU-side checks of the MAE reconstruction evaluation: the fp64 mirror the GPU tests compare
against (tests/recon_mirror.py) inverts the committed patchify fixture and obeys the header's
formulas on cases small enough to check by hand; checkpoint-format detection; fake-tensor shapes
of the two operators; the command line and the CSV.  Nothing here launches a kernel."""
import os
import warnings

import numpy as np
import pytest
import torch

import recon_mirror as RM
from conftest import GOLDEN

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------ mirror
def test_mirror_unpatchify_round_trips_the_patchify_fixture():
    fx = np.load(os.path.join(GOLDEN, "patchify.npz"))
    shape = tuple(int(v) for v in fx["patchify_in_shape"])
    B, C, T, H, W = shape
    x = torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(shape)
    want = torch.from_numpy(fx["patchify_out"])
    assert torch.equal(RM.patchify(x), want)
    assert torch.equal(RM.unpatchify(want, C, T, H, W), x)
    # the reference's 'bthwpqc->bcthpw' (q summed away) is not the inverse
    dropped = torch.einsum("bthwpqc->bcthpw", want.reshape(B, T, H // 8, W // 8, 8, 8, C))
    assert dropped.numel() != x.numel()


def _case(B=2, T=2, H=16, W=24, seed=0):
    g = torch.Generator().manual_seed(seed)
    L = (H // 8) * (W // 8)
    clip = torch.randn(B, 3, T, H, W, generator=g)
    pred = torch.randn(B, T * L, 192, generator=g)
    mask = torch.rand(B, 1, L, generator=g).expand(B, T, L) > 0.5
    return pred, clip, mask


def test_mirror_formulas():
    pred, clip, mask = _case()
    B, _, T, H, W = clip.shape
    # norm_pix = False and pred = patchify(clip): the reconstruction is the clip, both errors vanish
    exact = RM.patchify(clip)
    out = RM.reconstruct(exact, clip, mask, MEAN, STD, norm_pix=False, paste_visible=False, bgr_swap=False)
    assert float(out["token_err"].abs().max()) == 0.0
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1, 1)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1, 1)
    assert torch.allclose(out["recon"], clip.double() * std + mean, rtol=0, atol=1e-15)
    left, mid, right = out["panels"].split(W, dim=3)
    assert torch.equal(left, right)
    m_up = mask.reshape(B, T, H // 8, W // 8).repeat_interleave(8, 2).repeat_interleave(8, 3)
    assert torch.equal(mid, left * (~m_up)[..., None])
    assert bool(torch.isinf(out["clip_metrics"][:, 2]).all()) and float(out["clip_metrics"][:, :2].abs().max()) == 0
    assert torch.equal(out["clip_metrics"][:, 3], mask.reshape(B, -1).sum(1).double())
    # norm_pix: a prediction equal to the normalised target reconstructs the clip
    x = exact.double()
    mu = x.mean(-1, keepdim=True)
    sd = (x.var(-1, unbiased=True, keepdim=True) + 1e-6).sqrt()
    out = RM.reconstruct((x - mu) / sd, clip, mask, MEAN, STD, norm_pix=True, paste_visible=False, bgr_swap=True)
    assert float(out["token_err"].max()) < 1e-28
    # bgr_swap: clip channel c shows at RGB position 2 - c with that position's constants
    assert torch.allclose(out["recon"], clip.double().flip(1) * std + mean, rtol=0, atol=1e-13)
    # paste_visible: visible tokens show the clip whatever the prediction is; the errors do not change
    a = RM.reconstruct(pred, clip, mask, MEAN, STD, paste_visible=True)
    b = RM.reconstruct(pred, clip, mask, MEAN, STD, paste_visible=False)
    assert torch.equal(a["token_err"], b["token_err"])
    vis = ~m_up[:, None].expand(B, 3, T, H, W)
    assert torch.equal(a["recon"][vis], (clip.double().flip(1) * std + mean)[vis])
    assert torch.equal(a["recon"][~vis], b["recon"][~vis])
    # the loss map entry: its masked mean is the training loss (train_ssl_mae.py:81-84)
    tgt = (x - mu) / sd
    loss = (((pred.double() - tgt) ** 2).mean(-1) * mask.reshape(B, -1)).sum() / mask.sum()
    n = a["clip_metrics"][:, 3]
    assert abs(float((a["clip_metrics"][:, 0] * n).sum() / n.sum()) - float(loss)) < 1e-12
    # Gaussian inputs leave well under 1 % of the bytes near a level boundary
    assert float(a["near"].double().mean()) < 0.01


# ------------------------------------------------------------------ checkpoint formats
def _tiny_model(seed):
    from ssl_mae_amd.train_ssl_mae import build_model
    cfg = {"dataset": {"clip_len": 2, "image_size": 32, "stride": 4, "train_split": "-"},
           "model": {"decoder_embed_dim": 384, "decoder_depth": 4, "decoder_num_heads": 6},
           "ssl": {"mask_ratio": 0.75, "norm_pix_loss": True}, "training": {"batch_size": 2}}
    torch.manual_seed(seed)
    return build_model(cfg, "cpu")


def test_checkpoint_format_detection(tmp_path):
    from ssl_mae_amd.checkpoint import save_training_state
    from ssl_mae_amd.visualize_mae import FORMATS, load_mae_checkpoint
    src = _tiny_model(1)
    want = {k: v.clone() for k, v in src.state_dict().items()}
    save_training_state(tmp_path / "last_state.pth", src, torch.optim.SGD(src.parameters(), lr=0.1), None, 3)
    torch.save(src.state_dict(), tmp_path / "full.pth")
    torch.save(src.encoder.state_dict(), tmp_path / "encoder_ep10.pth")
    for name, fmt in (("last_state.pth", "training_state"), ("full.pth", "state_dict")):
        dst = _tiny_model(2)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            assert load_mae_checkpoint(dst, tmp_path / name) == fmt and fmt in FORMATS
        got = dst.state_dict()
        assert all(torch.equal(got[k], v) for k, v in want.items())
    dst = _tiny_model(2)
    before = dst.decoder_pred.weight.detach().clone()
    with pytest.warns(UserWarning, match="encoder only.*decoder"):
        assert load_mae_checkpoint(dst, tmp_path / "encoder_ep10.pth") == "encoder"
    got = dst.state_dict()
    assert all(torch.equal(got[k], v) for k, v in want.items() if k.startswith("encoder."))
    assert torch.equal(dst.decoder_pred.weight, before) and not torch.equal(before, want["decoder_pred.weight"])
    torch.save({"model": {}}, tmp_path / "empty.pth")
    with pytest.raises(ValueError):
        load_mae_checkpoint(dst, tmp_path / "empty.pth")


# ------------------------------------------------------------------ operators, CLI, CSV
def test_fake_tensor_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ssl_mae_amd import ops
    assert {"mae_reconstruct", "recon_clip_metrics"} <= set(ops.registered_ops())
    with FakeTensorMode():
        B, T, H, W = 2, 3, 16, 24
        L = (H // 8) * (W // 8)
        pred = torch.empty(B, T * L, 192, dtype=torch.bfloat16)
        clip = torch.empty(B, 3, T, H, W)
        mask = torch.empty(B, T, L, dtype=torch.uint8)
        panels, recon, te = ops.mae_reconstruct(pred, clip, mask, MEAN, STD)
        assert panels.shape == (B, T, H, 3 * W, 3) and panels.dtype == torch.uint8
        assert recon.shape == (B, 3, T, H, W) and recon.dtype == torch.float32
        assert te.shape == (B * T * L, 2) and te.dtype == torch.float32
        assert ops.mae_reconstruct(pred, clip, mask, MEAN, STD, want_recon=False)[1].numel() == 0
        cm = ops.recon_clip_metrics(te, mask)
        assert cm.shape == (B, 4) and cm.dtype == torch.float32


def test_no_cpu_fallback():
    from ssl_mae_amd import _lib, kernels
    pred, clip, mask = _case()
    with pytest.raises(_lib.KernelError, match="no CPU fallback"):
        kernels.mae_reconstruct(pred, clip, mask.to(torch.uint8).contiguous(), MEAN, STD)


def test_cli_parser():
    from ssl_mae_amd.visualize_mae import build_parser
    a = build_parser().parse_args([])
    assert (a.config, a.ckpt, a.frames, a.out, a.mask_ratio, a.clips, a.sweep) == (
        "configs/ssl_mae.yaml", None, None, "visual_results", 0.9, 1, False)
    a = build_parser().parse_args(["--config", "c.yaml", "--ckpt", "m.pth", "--frames", "d", "--out", "o",
                                   "--mask_ratio", "0.75", "--clips", "3", "--sweep"])
    assert (a.config, a.ckpt, a.frames, a.out, a.mask_ratio, a.clips, a.sweep) == (
        "c.yaml", "m.pth", "d", "o", 0.75, 3, True)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--clips", "x"])


def test_csv_header_and_rows(monkeypatch, tmp_path):
    from ssl_mae_amd import visualize_mae as V
    assert V.CSV_HEADER == "clip,mask_ratio,n_masked,loss_norm,mse_pix,psnr_db\n"
    vals = np.array([12.0, 0.1, 1e-3, 30.0], dtype=np.float32)          # n_masked, loss, mse, psnr
    line = V.format_row(0, 0.9, *vals)
    cells = line.rstrip("\n").split(",")
    assert cells[:3] == ["0", "0.9", "12"]
    assert [float(c) for c in cells[3:]] == [float(v) for v in vals[1:]]     # exact round trip
    assert V.format_row("mean", 0.5, 10.5, 1.0, 0.0, float("inf")) == "mean,0.5,10.5,1.0,0.0,inf\n"
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        V.visualize(None, None, str(tmp_path / "out"), config={})

"""Host side of Mixup / CutMix and label smoothing in fine-tuning: the numpy mirrors
(tests/mix_mirror.py) against the plain formulas, mae_loader.ClipMixer's draws, the config section
and the library's symbols.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from mix_mirror import batch_flip_reference, clip_mix_mirror, soft_ce_mirror, soft_target

H, W = 12, 20


# ------------------------------------------------------------------ the pixel mirror
def test_mirror_matches_the_batch_flip_formula():
    """fp32 mirror against x * lam + x[::-1] * (1 - lam) plus the slice paste in float64.  Each side
    makes at most four roundings of quantities bounded by max(|a|, |p|), each <= 2^-24 relative:
    2^-21 max(|a|, |p|) per element; exact where lam_px == 1 and inside the boxes."""
    rng = np.random.default_rng(0)
    for B in (1, 2, 5, 6):
        x = (rng.standard_normal((B, 6, 6, 8)) * 3).astype(np.float32)
        P = B // 2
        lam = np.array([0.3, 1.0, 0.0][:P], dtype=np.float32)
        box = np.array([[1, 3, 2, 3], [0, 0, 6, 4], [2, 2, 0, 0]][:P], dtype=np.int32).reshape(P, 4)
        got = clip_mix_mirror(x, lam, box)
        want = batch_flip_reference(x, lam, box)
        bound = 2.0 ** -21 * np.maximum(np.abs(x), np.abs(x[::-1])).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        print(f"B={B}: max error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert np.all(err <= bound)
        for p in range(P):
            y0, x0, h, w = box[p]
            for b in (p, B - 1 - p):
                assert np.array_equal(got[b][:, y0:y0 + h, x0:x0 + w], x[B - 1 - b][:, y0:y0 + h, x0:x0 + w])
                if lam[p] == 1.0:
                    keep = np.ones((6, 8), dtype=bool)
                    keep[y0:y0 + h, x0:x0 + w] = False
                    assert np.array_equal(got[b][:, keep], x[b][:, keep])
        if B % 2:
            assert np.array_equal(got[B // 2], x[B // 2])


def test_mirror_keeps_a_non_finite_partner_out_when_lam_is_one():
    x = np.ones((2, 3, 4, 4), dtype=np.float32)
    x[1, :, 0, 0], x[1, :, 3, 3] = np.nan, np.inf
    got = clip_mix_mirror(x, [1.0], [[1, 1, 2, 2]])
    assert np.array_equal(got[0], x[0])
    got = clip_mix_mirror(x, [0.5], [[1, 1, 2, 2]])
    assert np.isnan(got[0, 0, 0, 0]) and np.isinf(got[0, 0, 3, 3])


# ------------------------------------------------------------------ ClipMixer
def _mixer(**kw):
    from ssl_mae_amd.mae_loader import ClipMixer
    return ClipMixer(**kw)


def test_same_seed_same_draws_and_fixed_draw_count():
    a, b = _mixer(seed=7), _mixer(seed=7)
    for B in (8, 5, 8):
        ra, rb = a.draw(B, H, W), b.draw(B, H, W)
        assert all(torch.equal(s, t) for s, t in zip(ra, rb)) and a.last == b.last
    assert _mixer(seed=8).draw(8, H, W)[2].tolist() != _mixer(seed=7).draw(8, H, W)[2].tolist()
    # the generator's position after a call depends on the number of pairs alone: not on what was
    # accepted (prob, switch_prob) and not on the alphas
    ref = _mixer(seed=3)
    ref.draw(8, H, W)
    state = ref.gen.get_state()
    for kw in ({"prob": 0.0}, {"prob": 0.5, "switch_prob": 0.0}, {"switch_prob": 1.0}, {"mixup_alpha": 0.0},
               {"cutmix_alpha": 0.0, "mixup_alpha": 0.2}):
        other = _mixer(seed=3, **kw)
        other.draw(8, 2 * H, W)
        assert torch.equal(other.gen.get_state(), state), kw


def test_boxes_and_label_weights():
    m = _mixer(seed=1, prob=0.9)
    seen = set()
    for B in (16, 7):
        P = B // 2
        for _ in range(40):
            lam_px, box, weight = m.draw(B, H, W)
            assert lam_px.dtype == torch.float32 and box.dtype == torch.int32 and weight.dtype == torch.float32
            assert tuple(lam_px.shape) == (P,) and tuple(box.shape) == (P, 4) and tuple(weight.shape) == (B,)
            last = m.last
            for p in range(P):
                y0, x0, h, w = box[p].tolist()
                assert (y0, x0, h, w) == tuple(last["box"][p])
                assert 0 <= y0 and 0 <= x0 and h >= 0 and w >= 0 and y0 + h <= H and x0 + w <= W
                assert weight[p] == weight[B - 1 - p] and 0.0 <= float(weight[p]) <= 1.0
                assert float(weight[p]) == last["weight"][p]
                kind = last["kind"][p]
                seen.add(kind)
                if kind == "cutmix":
                    assert float(lam_px[p]) == 1.0
                    assert float(weight[p]) == float(np.float32(1.0 - h * w / (H * W)))
                    r = math.sqrt(1.0 - last["lam"][p])          # the box before clamping: at most ch x cw
                    assert h <= int(H * r) and w <= int(W * r)
                elif kind == "mixup":
                    assert (h, w) == (0, 0) and 0.0 <= float(lam_px[p]) <= 1.0
                    assert float(weight[p]) == float(lam_px[p]) == last["lam"][p]
                else:
                    assert kind == "none" and (h, w) == (0, 0) and float(lam_px[p]) == 1.0 and float(weight[p]) == 1.0
            if B % 2:
                assert float(weight[B // 2]) == 1.0
    assert seen == {"none", "mixup", "cutmix"}


def test_only_the_positive_alpha_is_used():
    m = _mixer(seed=2, cutmix_alpha=0.0, switch_prob=1.0)
    m.draw(64, H, W)
    assert set(m.last["kind"]) == {"mixup"}
    m = _mixer(seed=2, mixup_alpha=0.0, switch_prob=0.0)
    m.draw(64, H, W)
    assert set(m.last["kind"]) == {"cutmix"}
    for bad in ({"mixup_alpha": 0.0, "cutmix_alpha": 0.0}, {"mixup_alpha": -1.0}, {"prob": 1.5}, {"switch_prob": -0.1}):
        with pytest.raises(ValueError):
            _mixer(**bad)


def test_prob_and_switch_prob_are_honoured():
    """4000 pairs: the mixed share within 5 binomial standard deviations of prob, and the CutMix
    share of the mixed pairs within 5 of switch_prob."""
    n = 4000
    m = _mixer(seed=5, prob=0.3, switch_prob=0.7)
    m.draw(2 * n, H, W)
    kinds = m.last["kind"]
    mixed = sum(k != "none" for k in kinds)
    cut = sum(k == "cutmix" for k in kinds)
    print(f"mixed {mixed / n:.4f} (0.3), cutmix share of mixed {cut / mixed:.4f} (0.7)")
    assert abs(mixed / n - 0.3) <= 5 * math.sqrt(0.3 * 0.7 / n)
    assert abs(cut / mixed - 0.7) <= 5 * math.sqrt(0.7 * 0.3 / mixed)


def test_prob_zero_mixes_nothing():
    m = _mixer(seed=5, prob=0.0)
    lam_px, box, weight = m.draw(9, H, W)
    assert torch.all(lam_px == 1) and torch.all(weight == 1) and torch.all(box[:, 2:] == 0)
    assert set(m.last["kind"]) == {"none"}


def test_box_check_refuses_what_leaves_the_frame():
    from ssl_mae_amd import _lib, kernels
    kernels.mix_boxes_check([(0, 0, H, W), (H, W, 0, 0), (3, 4, 0, 5)], H, W)
    for bad in ((0, 0, H + 1, 1), (1, 0, H, 1), (0, W - 1, 1, 2), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1),
                (0, 0, 1, -1)):
        with pytest.raises(_lib.KernelError):
            kernels.mix_boxes_check([bad], H, W)


# ------------------------------------------------------------------ configuration
def test_config_section_and_validation():
    from ssl_mae_amd import train_finetune as TF
    base = TF.resolve_config({})
    assert base["mix"] == {"enabled": False, "mixup_alpha": 0.8, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5}
    assert base["training"]["label_smoothing"] == 0.0
    assert TF.build_mixer(base) is None
    on = TF.resolve_config({"mix": {"enabled": True, "cutmix_alpha": 0.0}, "training": {"label_smoothing": 0.1}})
    assert on["mix"]["enabled"] and on["mix"]["cutmix_alpha"] == 0.0 and on["training"]["label_smoothing"] == 0.1
    assert type(TF.build_mixer(on)).__name__ == "ClipMixer"        # synthetic clips: no train_split needed
    for bad in ({"mixup_alpha": -0.1}, {"cutmix_alpha": -1.0}, {"prob": -0.01}, {"prob": 1.01}, {"switch_prob": 2.0},
                {"switch_prob": -1.0}, {"alpha": 1.0}):
        with pytest.raises(ValueError):
            TF.resolve_config({"mix": bad})                          # out of range even when off
    with pytest.raises(ValueError):
        TF.resolve_config({"mix": {"enabled": True, "mixup_alpha": 0.0, "cutmix_alpha": 0.0}})
    TF.resolve_config({"mix": {"mixup_alpha": 0.0, "cutmix_alpha": 0.0}})       # both zero is fine while off
    for eps in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            TF.resolve_config({"training": {"label_smoothing": eps}})
    # the defaults are not written through
    assert TF.DEFAULTS["mix"]["enabled"] is False and TF.DEFAULTS["mix"]["cutmix_alpha"] == 1.0
    assert TF.DEFAULTS["training"]["label_smoothing"] == 0.0


def test_shipped_config_has_the_section_switched_off():
    import yaml
    from conftest import ROOT
    from ssl_mae_amd import train_finetune as TF
    with open(os.path.join(ROOT, "configs", "finetune.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["mix"] == TF.DEFAULTS["mix"] and cfg["mix"]["enabled"] is False
    assert cfg["training"]["label_smoothing"] == 0.0
    TF.resolve_config(cfg)


# ------------------------------------------------------------------ the soft loss mirror
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_soft_loss_mirror_against_torch(eps):
    g = torch.Generator().manual_seed(3)
    N, C = 9, 13
    l = torch.randn(N, C, generator=g) * 4
    ya, yb = torch.randint(0, C, (N,), generator=g), torch.randint(0, C, (N,), generator=g)
    yb[2] = ya[2]
    lam = torch.rand(N, generator=g)
    lam[0], lam[1] = 0.0, 1.0
    oh = torch.nn.functional.one_hot
    for b, w in ((yb, lam), (None, None)):
        lam64 = w.double()[:, None] if w is not None else torch.ones(N, 1, dtype=torch.float64)
        pb = oh(b if b is not None else ya, C).double()
        t = lam64 * ((1 - eps) * oh(ya, C).double() + eps / C) + (1 - lam64) * ((1 - eps) * pb + eps / C)
        l64 = l.double().requires_grad_()
        want = -(t * torch.log_softmax(l64, 1)).sum(1)
        want.sum().backward()
        wb, ww = (b.numpy(), w.numpy()) if b is not None else (None, None)
        loss, dl, hits = soft_ce_mirror(l.numpy(), ya.numpy(), wb, ww, eps)
        assert np.abs(soft_target(C, ya.numpy(), wb, ww, eps) - t.numpy()).max() <= 1e-15
        assert np.abs(loss - want.detach().numpy()).max() <= 1e-12
        assert np.abs(dl - l64.grad.numpy()).max() <= 1e-12
        assert hits == int((l.argmax(1) == ya).sum())


# ------------------------------------------------------------------ the library
def test_symbols_and_operators_exist():
    from ssl_mae_amd import _lib, ops
    for name in ("sm_clip_mix", "sm_soft_ce", "sm_soft_ce_workspace_bytes"):
        assert name in _lib._SIGS
    assert {"clip_mix", "soft_ce"} <= set(ops.registered_ops())
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(4, 3, 2, 8, 8)
        assert ops.clip_mix(x, torch.empty(2), torch.empty(2, 4, dtype=torch.int32)).shape == x.shape
        out = ops.soft_ce(torch.empty(4, 10), torch.empty(4, dtype=torch.int64))
        assert out.shape == (2,) and out.dtype == torch.float64
    with pytest.raises(Exception):                        # no CPU fallback
        ops.clip_mix(torch.zeros(2, 3, 4, 4), torch.ones(1), torch.zeros(1, 4, dtype=torch.int32))

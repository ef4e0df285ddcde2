"""CPU-side checks of the feature-privacy evaluation: the fixture (tests/golden/privacy.npz) is
pinned to its generators and, where the reference is present, to the reference; the host mirror
of the perturbation draws has the statistics the kernel is specified by; the driver's config /
CSV plumbing, the grid order and the per-configuration seeds behave.  Nothing here launches a
kernel."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_privacy as MGP  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "privacy.npz"))


# ------------------------------------------------------------------ fixture
def test_fixture_matches_generators(fx):
    for name, (N, C, _) in MGP.METRIC_CASES.items():
        logits, labels = MGP.metric_inputs(name)
        assert logits.shape == (N, C) and logits.dtype == np.float32 and labels.shape == (N,)
        assert MGP.metric_margin(logits, labels) >= 1e-3, name
        l64 = logits.astype(np.float64)
        z = l64 - l64.max(1, keepdims=True)
        lse = np.log(np.exp(z).sum(1))
        p = np.exp(z - lse[:, None])
        ly = l64[np.arange(N), labels]
        np.testing.assert_allclose(fx[f"metrics/{name}/loss64"], (lse + l64.max(1) - ly).mean(), rtol=1e-12)
        np.testing.assert_allclose(fx[f"metrics/{name}/entropy64"], (-(p * np.log(p + 1e-12)).sum(1)).mean(), rtol=1e-12)
        np.testing.assert_allclose(fx[f"metrics/{name}/entropy"], fx[f"metrics/{name}/entropy64"], rtol=1e-5)
        rank = (l64 > ly[:, None]).sum(1)
        np.testing.assert_allclose(fx[f"metrics/{name}/top1"], (rank < 1).mean(), rtol=1e-6)
        assert int(fx[f"metrics/{name}/topk_hits"]) == int((rank < MGP.topk_of(C)).sum())
    for name, (N, D, C, _, _) in MGP.ATTACKER_CASES.items():
        z, y = MGP.attacker_inputs(name)
        assert z.shape == (N, D) and z.dtype == np.float32 and y.shape == (N,)
        l64 = fx[f"attacker/{name}/logits64"]
        assert l64.shape == (N, C) and l64.dtype == np.float64
        assert MGP.logit_margin(l64) >= 1e-3, name
        assert 0 < float(fx[f"attacker/{name}/err32"]) < 1e-4
        assert float(fx[f"attacker/{name}/top1"]) == pytest.approx((l64.argmax(1) == y).mean(), abs=1e-6)
        assert name not in MGP.UNSATURATED or float(fx[f"attacker/{name}/top1"]) < 0.9


def test_fixture_matches_reference(fx):
    if not MGP.reference_present():
        pytest.skip("reference not on this machine")
    rec = MGP.build_fixture(MGP.import_reference())
    assert sorted(rec) == sorted(fx.files)
    for key, want in rec.items():
        got = fx[key]
        assert got.shape == np.shape(want) and got.dtype == np.asarray(want).dtype, key
        if key.endswith("/err32"):
            # the fp32 runs' rounding depends on the host BLAS's blocking: the same magnitude
            assert 0.25 * want <= got <= 4 * want, (key, got, want)
        elif got.dtype.kind in "iu":
            assert np.array_equal(got, want), key
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, err_msg=key)


def test_attacker_initial_weights_match_the_fixture(fx):
    """FeatureAttacker keeps the reference's parameter names and construction order, so the same
    torch seed draws the same initial weights."""
    from ssl_mae_amd.privacy import FeatureAttacker
    for name in MGP.ATTACKER_CASES:
        att = MGP.attacker_init(FeatureAttacker, name)
        assert list(att.state_dict()) == ["net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias"]
        rec = MGP.init_record(att.state_dict())
        assert sorted(f"attacker/{name}/init/{k}" for k in rec) == sorted(
            k for k in fx.files if k.startswith(f"attacker/{name}/init/"))
        for k, v in rec.items():
            assert np.array_equal(fx[f"attacker/{name}/init/{k}"], v), (name, k)


# ------------------------------------------------------------------ perturb_mirror
N_, D_ = 256, 576
SEED = 20240607


def test_mirror_noise_and_mask_statistics():
    from ssl_mae_amd import privacy as P
    n = N_ * D_
    z = np.zeros((N_, D_), dtype=np.float32)
    noise = P.perturb_mirror(z, 1.0, 0.0, SEED).ravel()
    assert abs(noise.mean()) < 5 / np.sqrt(n)
    assert abs(noise.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert np.abs(noise).max() <= np.sqrt(2 * np.log(2.0 ** 24)) + 1e-9
    ones = np.ones((N_, D_), dtype=np.float32)
    keeps = {}
    for r in (0.2, 0.4):
        keep = P.perturb_mirror(ones, 0.0, r, SEED).ravel()
        assert set(np.unique(keep)) == {0.0, 1.0}
        assert abs(keep.mean() - (1 - r)) < 5 * np.sqrt(r * (1 - r) / n)
        keeps[r] = keep
    assert np.all(keeps[0.4] <= keeps[0.2])                  # one draw per element: thresholds nest
    bound = 5 / np.sqrt(n)
    assert abs(np.corrcoef(noise, keeps[0.4])[0, 1]) < bound
    other = P.perturb_mirror(z, 1.0, 0.0, SEED + 1).ravel()
    assert abs(np.corrcoef(noise, other)[0, 1]) < bound
    assert abs(np.corrcoef(keeps[0.4], P.perturb_mirror(ones, 0.0, 0.4, SEED + 1).ravel())[0, 1]) < bound
    # neighbouring columns / rows are as independent as two seeds
    g = noise.reshape(N_, D_)
    assert abs(np.corrcoef(g[:, :-1].ravel(), g[:, 1:].ravel())[0, 1]) < bound
    assert abs(np.corrcoef(g[:-1].ravel(), g[1:].ravel())[0, 1]) < bound


def test_mirror_draws_have_no_duplicated_pairs():
    from ssl_mae_amd import privacy as P
    h0, h1, h2 = P.perturb_draws(SEED, N_, D_)
    for h in (h0, h1, h2):
        assert h.shape == (N_, D_) and int(h.max()) < 1 << 32
    pairs = (h0 << np.uint64(32)) | h1
    assert np.unique(pairs).size == pairs.size
    for h in (h0, h1, h2):                                   # the column round is a bijection within a row
        assert all(np.unique(row).size == D_ for row in h[:8])


def test_mirror_passthrough_and_full_mask():
    from ssl_mae_amd import privacy as P
    z = np.random.RandomState(3).standard_normal((5, 7)).astype(np.float32)
    for sigma, ratio in ((0.0, 0.0), (-1.0, -0.5)):
        out = P.perturb_mirror(z, sigma, ratio, SEED)
        assert out.dtype == np.float64 and np.array_equal(out, z.astype(np.float64))
    assert np.array_equal(P.perturb_mirror(z, 0.3, 1.0, SEED), np.zeros((5, 7)))
    assert np.array_equal(P.perturb_mirror(z, 0.0, 2.0, SEED), np.zeros((5, 7)))
    assert np.array_equal(P.perturb_mirror(torch.from_numpy(z), 0.1, 0.2, 9), P.perturb_mirror(z, 0.1, 0.2, 9))
    # noise first, then the mask, no 1 / keep rescale (feature_noise.py)
    noisy, keep = P.perturb_mirror(z, 0.1, 0.0, 9), P.perturb_mirror(np.ones_like(z), 0.0, 0.2, 9)
    assert np.array_equal(P.perturb_mirror(z, 0.1, 0.2, 9), noisy * keep)
    with pytest.raises(ValueError):
        P.perturb_mirror(np.zeros(4, dtype=np.float32), 0.1, 0.1, 1)


def test_mask_threshold_grid_order_and_seeds():
    from ssl_mae_amd import privacy as P
    from ssl_mae_amd.functions import splitmix64
    assert P.mask_threshold(0.0) == P.mask_threshold(-1.0) == 0
    assert P.mask_threshold(0.5) == 1 << 31 and P.mask_threshold(1.0) == P.mask_threshold(7.0) == 1 << 32
    for r in (0.2, 0.4, 1e-9, 0.999999):
        assert abs(P.mask_threshold(r) / 2.0 ** 32 - r) <= 2.4e-10
    cfgs = P.grid_configs([0.0, 0.1], [0.0, 0.2, 0.4], 42)
    assert [(s, r) for s, r, _ in cfgs] == [(0.0, 0.0), (0.0, 0.2), (0.0, 0.4), (0.1, 0.0), (0.1, 0.2), (0.1, 0.4)]
    assert [c[2] for c in cfgs] == [splitmix64(42 ^ splitmix64(g)) for g in range(6)]
    assert len({c[2] for c in cfgs}) == 6 and P.grid_configs([0.0, 0.1], [0.0, 0.2, 0.4], 43)[0][2] != cfgs[0][2]
    with pytest.raises(Exception):            # no CPU fallback: a host tensor never reaches a kernel
        P.perturb_grid(torch.zeros(4, 8), [0.1], [0.2], 1)
    with pytest.raises(ValueError):
        P.perturb_grid(torch.zeros(4, 8), [], [0.2], 1)
    z = torch.zeros(4, 8)
    assert P.add_gaussian_noise(z, 0.0) is z and P.apply_feature_mask(z, 0.0) is z      # feature_noise.py:5, :11


# ------------------------------------------------------------------ config and CSV
def test_driver_config_and_csv(fx, tmp_path, monkeypatch):
    from ssl_mae_amd import privacy as P
    from ssl_mae_amd import run_privacy as RP
    from ssl_mae_amd.utils import load_config
    cfg = RP.resolve_config(load_config(os.path.join(ROOT, "configs", "privacy.yaml")))
    assert set(cfg) == {"dataset", "model", "visual_privacy", "feature_privacy", "runtime", "output"}
    assert {"enabled", "noise_sigmas", "mask_ratios", "attacker_epochs", "attacker_lr"} == set(cfg["feature_privacy"])
    assert len(cfg["feature_privacy"]["noise_sigmas"]) * len(cfg["feature_privacy"]["mask_ratios"]) == 12
    assert cfg["feature_privacy"]["attacker_lr"] == 1e-3 and cfg["dataset"]["split"] is None
    got = RP.resolve_config({"feature_privacy": {"noise_sigmas": ["0.5", 1], "mask_ratios": (0,), "attacker_lr": "1e-3"}},
                            ckpt="x.pth", save_dir=str(tmp_path))
    assert got["feature_privacy"]["noise_sigmas"] == [0.5, 1.0] and got["feature_privacy"]["mask_ratios"] == [0.0]
    assert got["feature_privacy"]["attacker_lr"] == 1e-3
    assert got["model"]["finetune_ckpt"] == "x.pth" and got["output"]["save_dir"] == str(tmp_path)
    assert RP.resolve_config({"visual_privacy": {"enabled": True, "blur_kernel": 31}})["visual_privacy"]["enabled"]
    for bad in ({"feature_privacy": {"noise_sigmas": []}}, {"feature_privacy": {"mask_ratios": []}},
                {"feature_privacy": {"noise_sigma": [0.1]}}, {"feature_privasy": {}}, {"runtime": {"amp_dtype": "bf16"}},
                {"feature_privacy": {"noise_sigmas": 0.1}},
                {"feature_privacy": {"noise_sigmas": [0.1] * 9, "mask_ratios": [0.1] * 8}}):
        with pytest.raises(ValueError):
            RP.resolve_config(bad)
    # the reference's columns and rounding (run_privacy.py:329-346)
    assert RP.CSV_HEADER == "sigma,mask_ratio,top1,top5,entropy,attacker_top1,per_vs_clean\n"
    row = {"sigma": 0.05, "mask_ratio": 0.2, "top1": 1 / 3, "top5": 2 / 3, "entropy": 4.61512051684,
           "attacker_top1": 0.0104166667, "per_vs_clean": 0.03125}
    assert RP.format_row(row) == "0.05,0.2,0.333333,0.666667,4.615121,0.010417,0.03125\n"
    for (before, after), want in zip(fx["per/pairs"], fx["per/values"]):
        assert P.privacy_exposure_rate(float(before), float(after)) == want
    # an enabled visual stage is logged and skipped; cv2 is never imported
    import io
    log = io.StringIO()
    RP.run_visual_privacy(RP.resolve_config({"visual_privacy": {"enabled": True}}), log)
    assert "OpenCV" in log.getvalue() and "skip" in log.getvalue() and "cv2" not in sys.modules
    log = io.StringIO()
    RP.run_visual_privacy(RP.resolve_config({}), log)
    assert log.getvalue() == ""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg_file = tmp_path / "p.yaml"
    cfg_file.write_text("output:\n  save_dir: %s\n" % (tmp_path / "out"))
    with pytest.raises(RuntimeError, match="needs an MI355X"):
        RP.main(["--config", str(cfg_file)])

"""CPU-side checks of streaming dynamic inference: the fixture (tests/golden/dynamic.npz) is
pinned to the reference where the reference is present, its two sharpness conditions hold on
the stored arrays, and the driver's config / mode / CSV plumbing and the module's argument
validation behave.  Nothing here launches a kernel."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_dynamic as MGD  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "dynamic.npz"))


def test_fixture_matches_reference(fx):
    if not MGD.reference_present():
        pytest.skip("reference not on this machine")
    rec = MGD.build_fixture(MGD.import_reference())
    assert sorted(rec) == sorted(fx.files)
    for key, want in rec.items():
        got = fx[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        if want.dtype.kind in "iu":
            assert np.array_equal(got, want), key
        else:
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, err_msg=key)


def test_fixture_score_gaps(fx):
    for name, (B, T, S, *_rest) in MGD.MOTION_CASES.items():
        scores = fx[f"motion/{name}/scores"]
        assert scores.shape == (B, T) and np.all(scores[:, 0] == 0)
        assert MGD.score_gaps(scores).min() >= 1e-3, name
        for k in MGD.motion_ks(T):
            idx = fx[f"motion/{name}/idx_k{k}"]
            assert idx.shape == (B, min(k, T)) and np.all(np.diff(idx, axis=1) > 0)


def test_fixture_confidence_margin_and_spread(fx):
    E, w, bias = fx["ee/E"], fx["ee/w"], fx["ee/bias"]
    assert E.shape == (MGD.EE_B, MGD.EE_T, MGD.EE_D) and w.shape == (MGD.EE_K, MGD.EE_D)
    assert MGD.conf_margin(E, w, bias) >= 1e-3
    runs = MGD.ee_runs()
    used = fx["ee/used_frames"]
    assert used.shape == (len(runs), MGD.EE_B) and fx["ee/final_logits"].shape == (len(runs), MGD.EE_B, MGD.EE_K)
    # exit times differ within a batch (what makes compaction testable); the recorded counts
    # follow from the fp64 prefix confidences
    assert sum(len(set(u.tolist())) > 1 for u in used) >= len(runs) // 2
    for r, (thr, step, mn, mx) in enumerate(runs):
        conf = MGD.prefix_confidences(E, w, bias, step, mx)
        n = conf.shape[1]
        ok = (conf >= thr) & (np.arange(1, n + 1)[None, :] >= mn)
        want = np.where(ok.any(1), ok.argmax(1) + 1, n)
        assert np.array_equal(used[r], want), (r, used[r], want)
    clip = fx["ee/clip"]
    assert np.array_equal(clip[:, 0, :, 0, 0], np.arange(MGD.EE_B * MGD.EE_T).reshape(MGD.EE_B, MGD.EE_T))


def test_driver_config_modes_and_csv_headers(tmp_path):
    from ssl_mae_amd import run_dynamic as RD
    from ssl_mae_amd.utils import load_config
    cfg = RD.resolve_config(load_config(os.path.join(ROOT, "configs", "dynamic.yaml")))
    assert set(cfg) == {"dataset", "model", "dynamic", "runtime", "output"}
    assert set(cfg["dynamic"]) == {"mode", "confidence_thresholds", "min_frames", "max_frames", "frame_step",
                                   "gating_topk_list", "gating_score"}
    assert {"num_warmup", "num_measure"} <= set(cfg["runtime"]) and set(cfg["output"]) == {"save_dir", "save_csv"}
    assert cfg["dynamic"]["mode"] in RD.MODES and set(RD.RUNNERS) == set(RD.MODES)
    assert RD.resolve_config({}, mode="hybrid", ckpt="x.pth", save_dir=str(tmp_path))["dynamic"]["mode"] == "hybrid"
    assert RD.resolve_config({}, ckpt="x.pth")["model"]["finetune_ckpt"] == "x.pth"
    assert RD.resolve_config({"dynamic": {"confidence_thresholds": ["0.5", 1]}})["dynamic"]["confidence_thresholds"] \
        == [0.5, 1.0]
    for bad in ({"dynamic": {"mode": "late_exit"}}, {"dynamic": {"gating_score": "entropy"}},
                {"dynamic": {"gating_topk_list": []}}, {"dynamic": {"gating_topk_list": [0]}},
                {"dynamic": {"threshold": 0.5}}, {"dinamic": {}}):
        with pytest.raises(ValueError):
            RD.resolve_config(bad)
    with pytest.raises(ValueError):
        RD.resolve_config({}, mode="gating")
    # the reference's CSV columns (run_dynamic.py:89, :179, :259)
    assert RD.EARLY_EXIT_HEADER == "threshold,top1,top5,avg_frames,avg_conf,avg_latency_ms,throughput_fps\n"
    assert RD.FRAME_GATING_HEADER == "k,top1,top5,avg_latency_ms,throughput_clips_per_s\n"
    assert RD.HYBRID_HEADER == "k,threshold,top1,top5,avg_used_frames,avg_conf,avg_latency_ms\n"
    with pytest.raises(RuntimeError):
        RD.load_finetune_ckpt(torch.nn.Linear(2, 2), str(tmp_path / "missing.pth"))


def test_argument_validation_without_a_kernel():
    from ssl_mae_amd import dynamic_infer as DI
    clip = torch.zeros(2, 3, 4, 8, 8)
    with pytest.raises(ValueError):
        DI.select_topk_frames(clip, 2, score_type="entropy")
    with pytest.raises(ValueError):
        DI.select_topk_frames(clip, 0)
    with pytest.raises(ValueError):
        DI.motion_scores_l1(torch.zeros(3, 4, 8, 8))
    # the reference's clamping rules: frame_step, min_frames >= 1; max_frames truncates
    assert DI.frame_order(6) == [0, 1, 2, 3, 4, 5]
    assert DI.frame_order(6, frame_step=0) == DI.frame_order(6, frame_step=-3) == [0, 1, 2, 3, 4, 5]
    assert DI.frame_order(7, frame_step=2) == [0, 1, 3, 5]
    assert DI.frame_order(7, max_frames=3, frame_step=2) == [0, 1]
    assert DI.frame_order(4, max_frames=9) == [0, 1, 2, 3] and DI.frame_order(1) == [0]
    bb = torch.nn.Linear(2, 2).train()
    with pytest.raises(RuntimeError):
        DI.streaming_early_exit(bb, torch.nn.Linear(2, 2), clip, 0.5)
    with pytest.raises(Exception):            # no CPU fallback: a host clip never reaches a kernel
        DI.motion_scores_l1(clip)
    s = DI.EarlyExitStats(used_frames=torch.zeros(2, dtype=torch.long), final_conf=torch.zeros(2))
    assert s.used_frames.dtype == torch.int64 and s.final_conf.shape == (2,)

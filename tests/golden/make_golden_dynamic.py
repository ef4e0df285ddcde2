"""Golden fixture for streaming dynamic inference (tests/golden/dynamic.npz) by RUNNING the
reference's src/models/dynamic_infer.py on the CPU in the build container.

The reference module needs only torch, so it is loaded by file path (the rest of the import
machinery of make_golden.py::_import_reference is not needed).  This file also holds the
deterministic input generators, which the tests import (the motion clips are too large to
store; numpy's RandomState stream is stable across machines), and asserts the conditions
that make the fixture a sharp test when it writes it:

Motion clips  clip[b, :, t] = base[b] + a[b, t] * noise[b, t], amplitudes a permutation of
  a0 + spacing * rank per sample.  Recorded: the reference's scores and, for
  k in {1, 3, T-1, T, T+2}, its select_topk_frames indices.
  Condition: per sample the sorted scores of frames 1..T-1 differ pairwise by >= 1e-3
  relative, so no top-k choice hangs on rounding (torch.topk's tie order never matters).

Early exit     an embedding table E [6, 12, 576], a head with 11 classes, and a clip
  [6, 3, 12, 2, 2] whose pixel (0, 0, 0) carries b * T + t; the stub backbone looks E up by
  that id, so it also serves a compacted batch.  E = noise + ramp[b] * t * dirs[class_b],
  head weight 0.05 * dirs: confidence grows with the prefix at a per-sample rate, so the
  samples of one batch exit at different frames.  Recorded for thresholds {0.3, 0.5, 0.7,
  0.9} x frame_step {1, 2} x min_frames {1, 3} x max_frames {None, 5}: final_logits,
  used_frames, final_conf.
  Condition: at every confidence check of every run |conf - threshold| >= 1e-3 (prefix
  confidences recomputed here in fp64).

Run:  python tests/golden/make_golden_dynamic.py
"""
import importlib.util
import itertools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_FILE = "/root/reference/src/models/dynamic_infer.py"
OUT = os.path.join(HERE, "dynamic.npz")

# name -> (B, T, S, parent width, first column of the view, a0, spacing, seed)
MOTION_CASES = {
    "b3_t8_s32": (3, 8, 32, 32, 0, 0.05, 0.05, 101),
    "b5_t7_s24": (5, 7, 24, 24, 0, 0.05, 0.05, 102),       # W % 4 == 0, 7 frames
    "b2_t6_s30_sliced": (2, 6, 30, 34, 2, 0.05, 0.05, 103),   # W-sliced view: scalar path
    "b2_t16_s112": (2, 16, 112, 112, 0, 0.05, 0.15, 104),
}
THRESHOLDS = (0.3, 0.5, 0.7, 0.9)
FRAME_STEPS = (1, 2)
MIN_FRAMES = (1, 3)
MAX_FRAMES = (None, 5)
EE_B, EE_T, EE_D, EE_K = 6, 12, 576, 11


def reference_present():
    return os.path.isfile(REF_FILE)


def import_reference():
    spec = importlib.util.spec_from_file_location("ref_dynamic_infer", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    import sys
    sys.modules["ref_dynamic_infer"] = mod      # dataclass needs the module registered
    spec.loader.exec_module(mod)
    return mod


def motion_ks(T):
    return (1, 3, T - 1, T, T + 2)


def motion_parent(name):
    """-> (parent fp32 [B,3,T,S,Wp] torch CPU tensor, w0, W): the clip is parent[..., w0:w0+W]."""
    B, T, S, Wp, w0, a0, spacing, seed = MOTION_CASES[name]
    rng = np.random.RandomState(seed)
    base = rng.standard_normal((B, 3, 1, S, Wp))
    noise = rng.standard_normal((B, 3, T, S, Wp))
    amp = np.stack([a0 + spacing * rng.permutation(T) for _ in range(B)])          # [B,T]
    clip = base + amp[:, None, :, None, None] * noise
    return torch.from_numpy(clip.astype(np.float32)), w0, S


def motion_clip(name):
    parent, w0, W = motion_parent(name)
    return parent[..., w0:w0 + W]


def early_exit_inputs():
    """-> E [B,T,D], head weight [K,D], head bias [K], clip [B,3,T,2,2] (fp32 numpy)."""
    rng = np.random.RandomState(785)
    B, T, D, K = EE_B, EE_T, EE_D, EE_K
    dirs = rng.standard_normal((K, D))
    cls = rng.permutation(K)[:B]
    ramp = 0.012 + 0.007 * rng.permutation(B)                                       # per-sample rate
    E = 0.5 * rng.standard_normal((B, T, D)) + (ramp[:, None] * np.arange(T)[None, :])[:, :, None] * dirs[cls][:, None, :]
    w = 0.05 * dirs
    bias = 0.01 * rng.standard_normal(K)
    clip = np.zeros((B, 3, T, 2, 2))
    clip[:, 0, :, 0, 0] = np.arange(B * T).reshape(B, T)
    return tuple(a.astype(np.float32) for a in (E, w, bias, clip))


class TableBackbone:
    """frames [n,3,2,2] -> (None, E[id]) with id = pixel (0,0,0); counts what it is asked for."""

    def __init__(self, E):
        self.table = E.reshape(-1, E.shape[-1])
        self.calls = []           # per call: the ids seen (a CPU int64 tensor)

    def __call__(self, frames):
        ids = frames[:, 0, 0, 0].round().long()
        self.calls.append(ids.cpu())
        return None, self.table[ids]


def ee_runs():
    return list(itertools.product(THRESHOLDS, FRAME_STEPS, MIN_FRAMES, MAX_FRAMES))


def prefix_confidences(E, w, bias, step, max_frames):
    """fp64 max-softmax of the head over the running mean after each processed frame:
    -> conf [B, n_processed] for the order 0, 1, 1 + step, ... below min(T, max_frames)."""
    T = E.shape[1] if max_frames is None else min(E.shape[1], max_frames)
    order = [0] + list(range(1, T, step))
    e = E.astype(np.float64)[:, order]
    mean = np.cumsum(e, axis=1) / np.arange(1, len(order) + 1)[None, :, None]
    logits = mean @ w.astype(np.float64).T + bias.astype(np.float64)
    z = logits - logits.max(-1, keepdims=True)
    return 1.0 / np.exp(z).sum(-1)


def score_gaps(scores):
    """Smallest relative gap between neighbouring sorted scores of frames 1..T-1, per sample."""
    s = np.sort(np.asarray(scores, dtype=np.float64)[:, 1:], axis=1)
    if s.shape[1] < 2:
        return np.full(s.shape[0], np.inf)
    return ((s[:, 1:] - s[:, :-1]) / s[:, 1:]).min(axis=1)


def conf_margin(E, w, bias):
    """Smallest |prefix confidence - threshold| over every run's checks."""
    m = np.inf
    for step, mx in itertools.product(FRAME_STEPS, MAX_FRAMES):
        c = prefix_confidences(E, w, bias, step, mx)
        for thr in THRESHOLDS:
            m = min(m, np.abs(c - thr).min())
    return m


def build_fixture(ref):
    torch.set_num_threads(8)
    rec = {}
    for name in MOTION_CASES:
        clip = motion_clip(name)
        T = clip.shape[2]
        scores = ref.motion_scores_l1(clip).numpy()
        gap = score_gaps(scores).min()
        assert gap >= 1e-3, (name, gap)
        rec[f"motion/{name}/scores"] = scores
        for k in motion_ks(T):
            sel, idx = ref.select_topk_frames(clip, k)
            assert sel.shape[2] == min(k, T)
            rec[f"motion/{name}/idx_k{k}"] = idx.numpy().astype(np.int64)
    E, w, bias, clip = early_exit_inputs()
    margin = conf_margin(E, w, bias)
    assert margin >= 1e-3, margin
    rec.update({"ee/E": E, "ee/w": w, "ee/bias": bias, "ee/clip": clip})
    head = torch.nn.Linear(EE_D, EE_K)
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(w))
        head.bias.copy_(torch.from_numpy(bias))
    logits, used, conf = [], [], []
    for thr, step, mn, mx in ee_runs():
        fl, stats = ref.streaming_early_exit(TableBackbone(torch.from_numpy(E)), head, torch.from_numpy(clip), thr,
                                             min_frames=mn, max_frames=mx, frame_step=step)
        logits.append(fl.numpy())
        used.append(stats.used_frames.numpy())
        conf.append(stats.final_conf.numpy())
    rec["ee/final_logits"] = np.stack(logits)
    rec["ee/used_frames"] = np.stack(used).astype(np.int64)
    rec["ee/final_conf"] = np.stack(conf)
    return rec


def main():
    rec = build_fixture(import_reference())
    np.savez_compressed(OUT, **rec)
    used = rec["ee/used_frames"]
    spread = [(int(u.min()), int(u.max())) for u in used]
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); used-frame range per run: {spread}")
    for name in MOTION_CASES:
        print(name, "min relative score gap", score_gaps(rec[f'motion/{name}/scores']).min())
    print("confidence margin", conf_margin(rec["ee/E"], rec["ee/w"], rec["ee/bias"]))


if __name__ == "__main__":
    main()

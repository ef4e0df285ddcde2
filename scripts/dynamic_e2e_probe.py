"""Measures the two figures tests/test_dynamic_gpu.py gates its end-to-end check with (the
test's own model, clip and expectation): the embeddings of a compacted batch against those
of the full B*T batch, and the streamed logits against the dense expectation.
Run on the GPU:  python scripts/dynamic_e2e_probe.py > profiles/dynamic_e2e_probe.txt"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ssl-vit-video-analytics_amd"), ROOT):
    sys.path.insert(0, p)
import test_dynamic_gpu as TD  # noqa: E402
from ssl_mae_amd import dynamic_infer as DI, ops  # noqa: E402


def main():
    model, clip, emb = TD._e2e_setup()
    B, T = emb.shape[:2]
    scale = float(emb.abs().max())
    print(f"dense embeddings [B={B}, T={T}, D={emb.shape[2]}]: max |emb| {scale:.4f}, "
          f"mean |emb[:, t] - emb[:, 0]| {float((emb - emb[:, :1]).abs().mean()):.4f}")
    worst = 0.0
    with torch.no_grad():
        for rows in ([0, 1, 2, 3, 4], [0, 2, 4], [1, 3], [4], [2]):
            act = torch.tensor(rows, dtype=torch.int32, device="cuda")
            for t in (0, T // 2, T - 1):
                e = model.backbone(ops.gather_frames(clip, act, None, len(rows), t_fixed=t))[1]
                d = float((e - emb[rows, t]).abs().max()) / scale
                worst = max(worst, d)
                print(f"  batch {rows} frame {t}: max |emb - dense| / max |emb| = {d:.3e}")
    print(f"E2E_EMB_MEASURED = {worst:.3e}")
    worst_l = 0.0
    for step, mn in ((1, 1), (1, 3), (2, 2)):
        order = DI.frame_order(T, None, step)
        conf = TD._dense_expectation(emb, model.classifier, 2.0, mn, order)[2]
        c = conf.cpu().numpy().reshape(-1)
        print(f"step {step} min_frames {mn}: dense prefix confidences " + " ".join(f"{v:.4f}" for v in sorted(c)))
        for thr in sorted(set([float(v) + 1e-3 for v in c] + [2.0])):
            want_used, want_logits, _ = TD._dense_expectation(emb, model.classifier, thr, mn, order)
            logits, stats = DI.streaming_early_exit(model.backbone, model.classifier, clip, thr, min_frames=mn,
                                                    frame_step=step)
            err = float((logits.double() - want_logits).abs().max() / want_logits.abs().max())
            worst_l = max(worst_l, err)
    print(f"E2E_LOGIT_MEASURED = {worst_l:.3e}  (max over every threshold just above a dense prefix confidence)")


if __name__ == "__main__":
    main()

"""The fine-tuning driver with `mix.enabled` and `training.label_smoothing` on synthetic clips
(the shapes of test_train_finetune_gpu.py): the Mixing line, the "mix" hook, the soft loss in the
summary CSV, validation untouched, and the draws' reproducibility."""
import csv

import numpy as np
import pytest
import torch
import yaml

from mix_mirror import soft_ce_mirror

pytestmark = pytest.mark.gpu

NC, T, S = 4, 2, 112
N_TRAIN, N_VAL, BATCH = 6, 2, 2
EPS = 0.1


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(tmp_path, name):
    from ssl_mae_amd import train_finetune as TF
    cfg = {"dataset": {"num_classes": NC, "clip_len": T, "image_size": S},
           "training": {"epochs": 1, "batch_size": BATCH, "amp": False, "log_interval": 100, "label_smoothing": EPS},
           "mix": {"enabled": True},
           "synthetic": {"num_train": N_TRAIN, "num_val": N_VAL},
           "paths": {"save_dir": str(tmp_path / name), "log_dir": str(tmp_path / name / "logs")}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    steps, mixes = [], []

    def on_step(epoch, step, logits, label):
        steps.append((epoch, step, logits.float().cpu().numpy(), label.cpu().numpy()))

    def on_mix(epoch, step, info):
        assert set(info) == {"labels_b", "lam", "draws"}
        mixes.append((epoch, step, info["labels_b"].cpu().numpy(), info["lam"].cpu().numpy(),
                      {k: list(v) for k, v in info["draws"].items()}))

    TF.main(["--config", str(path)], hooks={"step": on_step, "mix": on_mix})
    return tmp_path / name, steps, mixes


def test_mixed_smoothed_run(tmp_path):
    out, steps, mixes = _run(tmp_path, "mix")
    log = (out / "logs" / "finetune_ft_random.log").read_text()
    assert log.count("[INFO] Mixing:") == 1
    n_steps = N_TRAIN // BATCH
    assert len(steps) == len(mixes) == n_steps
    losses = []
    for (e, s, logits, label), (e2, s2, lb, lam, draws) in zip(steps, mixes):
        assert (e, s) == (e2, s2) == (1, len(losses))
        assert lam.shape == (BATCH,) and np.all((lam >= 0) & (lam <= 1)) and lam[0] == lam[1]
        assert np.array_equal(lb, label[::-1])                           # the step hook has the batch's own labels
        assert len(draws["kind"]) == 1 and lam[0] == np.float32(draws["weight"][0])
        losses.append(soft_ce_mirror(logits, label, lb, lam, EPS)[0].mean())
    with open(out / "ft_random" / "finetune_summary.csv", newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["epoch", "train_loss", "val_top1", "val_topk", "lr", "seconds"] and len(rows) == 2
    want = float(np.mean(losses))
    print(f"train_loss {rows[1][1]}, mean fp64 soft loss {want!r}, draws {[m[4]['kind'] for m in mixes]}")
    assert abs(float(rows[1][1]) - want) <= 1e-5
    assert 0.0 <= float(rows[1][2]) <= float(rows[1][3]) <= 1.0         # validation: plain top-k accuracies

    # the same seed: the same draws
    _, _, again = _run(tmp_path, "mix_again")
    assert [m[4] for m in again] == [m[4] for m in mixes]
    assert all(np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]) for a, b in zip(again, mixes))

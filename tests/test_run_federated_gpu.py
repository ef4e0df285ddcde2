"""The federated driver on the GPU (ssl_mae_amd.run_federated): client_update against
nn.CrossEntropyLoss and the finetune.train_one_epoch step, evaluate_topk against
finetune.accuracy_topk, and `main` on synthetic clips with both exchange paths."""
import copy
import csv
import io

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NC, B, T, S = 4, 2, 2, 112
N_TRAIN, N_VAL = 6, 2          # synthetic clips of the `main` runs: a handful of steps per run


@pytest.fixture(scope="module")
def fresh():
    """(a never-run VideoClassifier(4, 112^2), two batches of B=2, T=2 clips with labels); tests
    work on deep copies."""
    from ssl_mae_amd.finetune import VideoClassifier
    from ssl_mae_amd.init_rule import synthetic_clip
    torch.manual_seed(5)
    model = VideoClassifier(NC, img_size=S).to(DEV)
    batches = [(torch.from_numpy(synthetic_clip(B, T, S, seed=70 + i)).to(DEV), torch.tensor(y, device=DEV))
               for i, y in enumerate(([1, 3], [0, 2]))]
    return model, batches


def test_client_update_loss_and_step_match_finetune(fresh):
    """fp32 mode (amp=False), one step.  Loss: nn.CrossEntropyLoss on the same logits, to 1e-5.
    Parameters after the step: those of the finetune.train_one_epoch step on an identically
    seeded model, with the step tolerance of tests/test_finetune_gpu.py (rtol 1e-5, atol 2e-6
    at lr 1e-3; entries whose gradient is below 1e-5 may move by up to 2.1 lr, since Adam
    normalises g / (|g| + eps))."""
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.finetune import train_one_epoch
    model0, batches = fresh
    loader = batches[:1]
    lr, wd = 1e-3, 0.01
    ours, theirs, probe = (copy.deepcopy(model0) for _ in range(3))

    probe.train()
    logits = probe(loader[0][0])
    want_loss = torch.nn.CrossEntropyLoss()(logits.float(), loader[0][1]).item()
    got_loss = R.client_update(ours, loader, DEV, epochs=1, lr=lr, weight_decay=wd, amp=False)
    print(f"client_update loss {got_loss!r}, CrossEntropyLoss {want_loss!r}")
    assert isinstance(got_loss, float) and abs(got_loss - want_loss) <= 1e-5

    opt = torch.optim.AdamW(theirs.parameters(), lr=lr, weight_decay=wd)
    ref_loss = train_one_epoch(theirs, loader, opt, None, DEV, {"training": {"amp": False, "log_interval": 100}},
                               io.StringIO())
    assert abs(ref_loss - want_loss) <= 1e-5
    assert ours.training and theirs.training
    worst = 0.0
    for (name, p), (_, q) in zip(ours.named_parameters(), theirs.named_parameters()):
        a, b, g = p.detach().cpu().numpy(), q.detach().cpu().numpy(), q.grad.detach().cpu().numpy()
        atol = np.where(np.abs(g) < 1e-5, 2.1 * lr, 2e-6)
        err = np.abs(a - b)
        worst = max(worst, float(err.max()))
        assert np.all(err <= atol + 1e-5 * np.abs(b)), (name, float(err.max()))
    print(f"largest parameter difference after one step {worst:.3e}")
    for (name, x), (_, y) in zip(ours.named_buffers(), theirs.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(x) == int(y) >= T, name       # T per-frame calls (checkpointed stages count twice)
    # a second call builds a fresh optimizer and returns the average over epochs x samples
    two = R.client_update(copy.deepcopy(model0), fresh[1], DEV, epochs=2, lr=lr, weight_decay=wd, amp=True)
    assert np.isfinite(two) and 0.0 < two < 10.0
    assert R.client_update(copy.deepcopy(model0), [], DEV) == 0.0


def test_evaluate_topk_matches_accuracy_topk(fresh):
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.finetune import accuracy_topk
    model0, batches = fresh
    model = copy.deepcopy(model0).eval()
    with torch.no_grad():
        logits = torch.cat([model(clip) for clip, _ in batches]).float()
    srt = logits.sort(dim=1).values
    assert bool((srt[:, 1:] - srt[:, :-1] > 0).all())             # no ties
    labels = torch.cat([y for _, y in batches])
    labels[0] = logits[0].argmax()                                 # at least one top-1 hit and one miss
    labels[1] = logits[1].argmin()
    loader = [(batches[0][0], labels[:B]), (batches[1][0], labels[B:])]
    got = R.evaluate_topk(model, loader, DEV)
    want = accuracy_topk(logits, labels, topk=(1, min(5, NC)))
    assert got == (want[1], want[min(5, NC)])
    assert 0.0 < got[0] < 1.0 and got[1] == 1.0                   # k = min(5, 4 classes) covers every class
    assert not model.training
    assert R.evaluate_topk(model, [], DEV) == (0.0, 0.0)


def test_shared_evaluate_caps_k_at_the_class_count(fresh):
    """driver.evaluate over three batches of 2 clips with topk=(1, 3, 5) against
    finetune.accuracy_topk with (1, 3, 4), batch-weighted, to 1e-12: with 4 classes key 5 holds
    the k = 4 value.  Labels by rank, so that every k has hits and k = 1, 3 have misses."""
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.driver import evaluate
    from ssl_mae_amd.finetune import accuracy_topk
    from ssl_mae_amd.init_rule import synthetic_clip
    model0, batches = fresh
    model = copy.deepcopy(model0).eval()
    clips = [clip for clip, _ in batches] + [torch.from_numpy(synthetic_clip(B, T, S, seed=72)).to(DEV)]
    with torch.no_grad():
        logits = [model(clip).float() for clip in clips]
    srt = torch.cat(logits).sort(dim=1).values
    assert bool((srt[:, 1:] - srt[:, :-1] > 0).all())             # no ties
    order = torch.cat(logits).argsort(dim=1, descending=True)
    labels = order[torch.arange(3 * B), torch.tensor([0, 3, 2, 1, 3, 0], device=DEV)]   # the label's rank per clip
    loader = [(clip, labels[i * B:(i + 1) * B]) for i, clip in enumerate(clips)]
    got = evaluate(model, loader, DEV, topk=(1, 3, 5))
    want = {k: 0.0 for k in (1, 3, 4)}
    for lg, (_, y) in zip(logits, loader):
        acc = accuracy_topk(lg, y, topk=(1, 3, 4))
        for k in want:
            want[k] += acc[k] * y.size(0)
    want = {k: v / (3 * B) for k, v in want.items()}
    print(f"driver.evaluate {got}, accuracy_topk {want}")
    assert sorted(got) == [1, 3, 5]
    assert abs(got[1] - want[1]) <= 1e-12 and abs(got[3] - want[3]) <= 1e-12 and abs(got[5] - want[4]) <= 1e-12
    assert (want[1], want[3], want[4]) == (2 / 6, 4 / 6, 1.0)
    assert R.evaluate_topk(model, loader, DEV) == (got[1], got[5])
    assert not model.training


def _config(tmp_path, name, exchange):
    cfg = {"dataset": {"num_classes": NC, "clip_len": T, "image_size": S},
           "federated": {"num_clients": 3, "rounds": 2, "local_epochs": 1, "batch_size": 2, "exchange": exchange,
                         "non_iid": {"shards_per_client": 1, "min_samples_per_client": 2}},
           "centralized": {"epochs": 1},
           "synthetic": {"num_train": N_TRAIN, "num_val": N_VAL},
           "output": {"save_dir": str(tmp_path / name)}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), tmp_path / name


def _rows(path):
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_main_on_synthetic_clips_both_exchanges(tmp_path):
    """3 clients, 2 rounds, 1 local epoch, batch 2, T=2, 112^2, 4 classes, 1 centralized epoch.
    The fused and the reference exchange give identical fed_summary.csv rows: the exchange paths
    are bit-identical and a run is deterministic for a seed (DropPath seeds come from the device
    generator's seed and per-model forward counters)."""
    from ssl_mae_amd import run_federated as R
    from ssl_mae_amd.federated import estimate_comm_mb_per_round
    from ssl_mae_amd.finetune import VideoClassifier
    cfg_fused, dir_fused = _config(tmp_path, "fused", "fused")
    cfg_ref, dir_ref = _config(tmp_path, "reference", "reference")
    out = R.main(["--config", cfg_fused])
    assert out["save_dir"] == dir_fused
    head, rows = _rows(dir_fused / "fed_summary.csv")
    assert head == list(R.FED_COLUMNS) and [r[0] for r in rows] == ["1", "2"]
    comm, model_mb = estimate_comm_mb_per_round(VideoClassifier(NC, img_size=S).state_dict(), 3)
    for i, r in enumerate(rows):
        assert r[4] == "3" and float(r[5]) == round(model_mb, 6) and float(r[6]) == round(comm, 6)
        assert float(r[7]) == round(comm * (i + 1), 6)
        assert 0.0 <= float(r[1]) <= float(r[2]) <= 1.0 and float(r[3]) > 0.0
    head, cen = _rows(dir_fused / "centralized_summary.csv")
    assert head == list(R.CENTRALIZED_COLUMNS) and len(cen) == 1 and cen[0][0] == "1" and float(cen[0][1]) > 0.0
    head, sysrow = _rows(dir_fused / "system_privacy_summary.csv")
    assert head == list(R.SYSTEM_COLUMNS) and len(sysrow) == 1
    raw = N_TRAIN * 3 * T * S * S / 2 ** 20
    assert float(sysrow[0][0]) == round(raw, 6) and float(sysrow[0][1]) == round(2 * comm, 6)
    assert float(sysrow[0][2]) == round(2 * comm / raw, 6)
    head, stats = _rows(dir_fused / "fed_client_stats.csv")
    assert head == R.CLIENT_STATS_HEADER.strip().split(",") and [s[0] for s in stats] == ["0", "1", "2"]
    assert sum(int(s[1]) for s in stats) == N_TRAIN
    for i, s in enumerate(stats):
        assert len(R.read_split(dir_fused / "splits" / f"fed_client_{i}_train.txt")) == int(s[1])
    assert "selected_clients=" in (dir_fused / "federated.log").read_text()

    R.main(["--config", cfg_ref])
    for name in ("fed_summary.csv", "centralized_summary.csv", "fed_client_stats.csv", "system_privacy_summary.csv"):
        assert (dir_ref / name).read_text() == (dir_fused / name).read_text(), name

"""The fine-tuning driver on the GPU (ssl_mae_amd.train_finetune.main) on synthetic clips: the
two_stage schedule, the checkpoint run_dynamic.load_finetune_ckpt reads, the summary CSV, and
the fused optimizer against torch.optim.AdamW."""
import csv

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NC, T, S = 4, 2, 112
N_TRAIN, N_VAL, BATCH = 6, 2, 2
UNFREEZE = "[INFO] two_stage: unfreeze backbone and rebuild optimizer"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _config(tmp_path, name, **training):
    tr = {"epochs": 2, "batch_size": BATCH, "amp": False, "log_interval": 100}
    tr.update(training)
    cfg = {"dataset": {"num_classes": NC, "clip_len": T, "image_size": S},
           "training": tr,
           "synthetic": {"num_train": N_TRAIN, "num_val": N_VAL},
           "paths": {"save_dir": str(tmp_path / name), "log_dir": str(tmp_path / name / "logs")}}
    path = tmp_path / f"{name}.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), tmp_path / name


def test_two_stage_run(tmp_path):
    from ssl_mae_amd import train_finetune as TF
    from ssl_mae_amd.finetune import VideoClassifier
    from ssl_mae_amd.run_dynamic import load_finetune_ckpt
    from ssl_mae_amd.run_federated import SyntheticClips
    torch.manual_seed(11)
    ssl_state = VideoClassifier(NC, img_size=S).backbone.state_dict()      # an encoder-only SSL file
    ssl_path = tmp_path / "encoder.pth"
    torch.save(ssl_state, ssl_path)
    path, out = _config(tmp_path, "two_stage", stage1_epochs=1, head_lr=1e-3, backbone_lr=1e-4)
    probe = SyntheticClips({"dataset": {"num_classes": NC, "clip_len": T, "image_size": S}}, 1, 77, DEV).clips

    step_losses, backbones, eval_logits = {}, {}, {}
    ce = torch.nn.CrossEntropyLoss()

    def on_step(epoch, step, logits, label):
        step_losses.setdefault(epoch, []).append(ce(logits.float(), label).item())

    def on_epoch(epoch, model, optimizer):
        backbones[epoch] = {n: p.detach().cpu().clone() for n, p in model.backbone.named_parameters()}
        model.eval()
        with torch.no_grad():
            eval_logits[epoch] = model(probe).float().cpu().clone()

    res = TF.main(["--config", path, "--mode", "two_stage", "--pretrained_ssl", str(ssl_path)],
                  hooks={"step": on_step, "epoch": on_epoch})

    log = (out / "logs" / "finetune_two_stage.log").read_text()
    assert log.count(UNFREEZE) == 1
    assert log.index("[INFO] Epoch 1/2 started") < log.index(UNFREEZE) < log.index("[INFO] Epoch 2/2 started")
    assert len(step_losses[1]) == len(step_losses[2]) == N_TRAIN // BATCH
    # stage 1: the backbone keeps the SSL file's bits; stage 2: it trains
    assert all(torch.equal(backbones[1][n], ssl_state[n]) for n in backbones[1])
    assert any(not torch.equal(backbones[2][n], ssl_state[n]) for n in backbones[2])
    assert type(res["optimizer"]).__name__ == "GroupedAdamW" and len(res["optimizer"].param_groups) == 2

    # the checkpoint: model.state_dict(), read unchanged by load_finetune_ckpt
    assert res["checkpoints"] and all(p.exists() for p in res["checkpoints"])
    ckpt = res["checkpoints"][-1]
    assert ckpt.parent == out / "two_stage"
    epoch = int(ckpt.name.split("_")[2])
    assert ckpt.name.startswith(f"finetune_epoch_{epoch}_top1_") and ckpt.suffix == ".pth"
    fresh = VideoClassifier(NC, img_size=S)
    state = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert list(state) == list(fresh.state_dict())
    load_finetune_ckpt(fresh, str(ckpt))
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        got = fresh(probe).float().cpu()
    assert torch.equal(got, eval_logits[epoch])

    # the summary
    with open(out / "two_stage" / "finetune_summary.csv", newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["epoch", "train_loss", "val_top1", "val_topk", "lr", "seconds"]
    assert len(rows) == 3 and [r[0] for r in rows[1:]] == ["1", "2"]
    want = float(np.mean(step_losses[1]))
    print(f"epoch 1 train_loss {rows[1][1]}, CrossEntropyLoss mean {want!r}")
    assert abs(float(rows[1][1]) - want) <= 1e-5
    assert all(0.0 <= float(r[2]) <= float(r[3]) <= 1.0 for r in rows[1:])
    assert float(rows[1][4]) == 1e-3


def test_fused_and_torch_optimizers_agree_after_one_step(tmp_path):
    from ssl_mae_amd import train_finetune as TF
    lr = 1e-3
    models = {}
    for name in ("torch", "fused"):
        path, _ = _config(tmp_path, name, epochs=1, learning_rate=lr, weight_decay=0.01)
        cfg = yaml.safe_load(open(path))
        cfg["synthetic"]["num_train"] = BATCH                      # one step
        open(path, "w").write(yaml.safe_dump(cfg))
        res = TF.main(["--config", path, "--optimizer", name])
        assert type(res["optimizer"]).__name__ == {"torch": "AdamW", "fused": "GroupedAdamW"}[name]
        models[name] = res["model"]
    worst = 0.0
    for (n, p), (_, q) in zip(models["fused"].named_parameters(), models["torch"].named_parameters()):
        a, b, g = p.detach().cpu().numpy(), q.detach().cpu().numpy(), q.grad.detach().cpu().numpy()
        atol = np.where(np.abs(g) < 1e-5, 2.1 * lr, 2e-6)
        err = np.abs(a - b)
        worst = max(worst, float(err.max()))
        assert np.all(err <= atol + 1e-5 * np.abs(b)), (n, float(err.max()))
    print(f"largest parameter difference after one step {worst:.3e}")

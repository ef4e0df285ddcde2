"""The kNN evaluation driver end to end on the GPU (ssl_mae_amd/run_knn.py): synthetic clips, two
batches of 4, through the backbone, the fused search, the vote and the metrics launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = ("dataset: {clip_len: 2, image_size: 112}\n"             # the synthetic default, shrunk
       "knn: {ks: [1, 5]%s}\n"
       "runtime: {batch_size: 4, num_batches: 2}\n")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rows(path):
    from ssl_mae_amd import run_knn as R
    lines = path.read_text().splitlines()
    assert lines[0] + "\n" == R.CSV_HEADER
    return [ln.split(",") for ln in lines[1:]]


def test_run_knn_main_synthetic(tmp_path):
    from ssl_mae_amd import run_knn as R
    cfg = tmp_path / "knn.yaml"
    cfg.write_text(CFG % "")
    res = R.main(["--config", str(cfg), "--save_dir", str(tmp_path / "a")])
    rows = _rows(tmp_path / "a" / "knn_eval.csv")
    assert [r[:2] for r in rows] == [["none", "1"], ["none", "5"]] and all(r[4:] == ["8", "8"] for r in rows)
    assert float(rows[0][2]) == 1.0 == res["rows"][0]["top1"]          # bank = queries: k = 1 finds the query itself
    assert np.array_equal(res["results"][0]["idx"][:, 0].cpu().numpy(), np.arange(8))
    for r in rows:
        assert 0.0 <= float(r[2]) <= float(r[3]) <= 1.0
    log = (tmp_path / "a" / "knn.log").read_text()
    assert "only show chance" in log and "against itself" in log and "kNN evaluation finished" in log
    # the eager reference writes the same file on this input
    R.main(["--config", str(cfg), "--save_dir", str(tmp_path / "b"), "--impl", "reference"])
    assert (tmp_path / "b" / "knn_eval.csv").read_text() == (tmp_path / "a" / "knn_eval.csv").read_text()


def test_run_knn_leave_one_out(tmp_path):
    from ssl_mae_amd import run_knn as R
    cfg = tmp_path / "knn.yaml"
    cfg.write_text(CFG % ", leave_one_out: true")
    res = R.main(["--config", str(cfg), "--save_dir", str(tmp_path / "out")])
    idx = res["results"][0]["idx"].cpu().numpy()
    assert idx.shape == (8, 5) and np.all(idx >= 0) and not np.any(idx == np.arange(8)[:, None])
    assert len(_rows(tmp_path / "out" / "knn_eval.csv")) == 2
    assert "leave-one-out" in (tmp_path / "out" / "knn.log").read_text()


def test_run_knn_two_checkpoints(tmp_path):
    from ssl_mae_amd import run_knn as R
    from ssl_mae_amd.finetune import VideoClassifier
    from ssl_mae_amd.init_rule import apply_rule
    model = VideoClassifier(101, img_size=112)
    apply_rule(model)
    paths = [str(tmp_path / "a.pth"), str(tmp_path / "b.pth")]
    torch.save(model.state_dict(), paths[0])
    g = torch.Generator().manual_seed(3)
    state = {k: v + 0.02 * torch.randn(v.shape, generator=g) if v.is_floating_point() and "running_var" not in k
             else v for k, v in model.state_dict().items()}
    torch.save(state, paths[1])
    cfg = tmp_path / "knn.yaml"
    cfg.write_text(CFG % ", leave_one_out: true")
    res = R.main(["--config", str(cfg), "--save_dir", str(tmp_path / "out"), "--ckpt"] + paths)
    rows = _rows(tmp_path / "out" / "knn_eval.csv")
    assert [r[:2] for r in rows] == [[paths[0], "1"], [paths[0], "5"], [paths[1], "1"], [paths[1], "5"]]
    assert len(res["results"]) == 2
    assert not torch.equal(res["results"][0]["sim"], res["results"][1]["sim"])   # two different encoders were embedded

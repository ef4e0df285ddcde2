"""CPU-side checks of temporal SSL pretraining (ssl_mae_amd/temporal_ssl.py): the host draws and
permutation indices against the fixture the reference recorded (tests/golden/temporal_ssl.npz,
tests/golden/make_golden_temporal.py), the fp64 mirror against the reference's losses, the
config, the checkpoint bridge and the operator registration.  No kernel runs here."""
import os

import numpy as np
import pytest
import torch

import temporal_mirror as TM
from conftest import ROOT
from ssl_mae_amd import temporal_ssl as TS


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "temporal_ssl.npz"))


@pytest.mark.parametrize("T", [3, 4, 8, 16])
@pytest.mark.parametrize("label", [0, 1, 2, 3])
def test_perm_index_4way(gold, T, label):
    idx = TS._perm_index_4way(T, label).numpy()
    assert np.array_equal(idx, gold[f"perm/T{T}_l{label}"])
    assert sorted(idx.tolist()) == list(range(T))
    if T == 3 and label == 3:
        assert idx.tolist() == [0, 1, 2]           # T < 4: the identity fallback


@pytest.mark.parametrize("B,T,ratio,n", [(3, 5, 0.75, 3), (2, 4, 0.75, 3), (4, 16, 0.75, 12), (2, 3, 0.1, 1)])
def test_build_mask_counts(B, T, ratio, n):
    m = TS.build_mask(B, T, ratio, "cpu")
    assert m.shape == (B, T) and m.dtype == torch.bool
    assert m.sum(dim=1).tolist() == [n] * B


@pytest.mark.parametrize("tag,sub", [("a/", 0.7), ("b/", 1.0)])
def test_host_draws_reproduce_the_reference(gold, tag, sub):
    """Same seed, same calls in the same order on the CPU generator: randperm(T) per sample,
    randperm(B)[:k] when subsampling, randint(0, 4, (k,))."""
    B, T = int(gold[tag + "B"]), int(gold[tag + "T"])
    torch.manual_seed(int(gold[tag + "seed"]))
    assert np.array_equal(TS.build_mask(B, T, 0.75, "cpu").numpy(), gold[tag + "mask"])
    k = B
    if sub < 1.0:
        k = max(2, int(B * sub))
        torch.randperm(B)[:k]
    assert k == int(gold[tag + "top_batch"])
    assert np.array_equal(torch.randint(0, 4, (k,)).numpy(), gold[tag + "labels"])


def test_mirror_reproduces_the_reference_losses(gold):
    mask = torch.from_numpy(gold["a/mask"]).reshape(-1)
    idx = mask.nonzero().reshape(-1)
    pred = torch.from_numpy(gold["a/pred"])
    teacher = torch.from_numpy(gold["a/ctx_t"]).reshape(pred.shape)
    mfm, var, sigma = TM.mfm_terms(pred, teacher, idx, 1.0, 1e-4)
    assert abs(float(mfm) - float(gold["a/mfm64"])) < 1e-12
    assert abs(float(var) - float(gold["a/var64"])) < 1e-12
    # the step itself ran in fp32
    assert abs(float(mfm) - float(gold["a/mfm"])) < 1e-5 and abs(float(var) - float(gold["a/var"])) < 1e-5
    losses, dpred, _ = TM.mfm_loss_and_grad(pred, teacher, idx, 1.0, 25.0, 1.0, 1e-4)
    assert abs(float(losses[2]) - (float(mfm) + 25.0 * float(var))) < 1e-12
    assert bool((dpred[~mask] == 0).all()) and bool((dpred[mask].abs().sum(dim=1) > 0).all())


def test_config_loads():
    from ssl_mae_amd.utils import load_config
    cfg = TS.resolve_config(load_config(os.path.join(ROOT, "configs", "ssl_train.yaml")))
    assert cfg["model"] == {"backbone": "tiny_vit_21m_variant", "embed_dim": 576, "temporal_layers": 4,
                            "temporal_heads": 9}
    assert cfg["training"]["clip_grad_norm"] == 1.0 and cfg["training"]["batch_size"] == 48
    ssl = cfg["ssl_objectives"]
    assert (ssl["mask_ratio"], ssl["ema_momentum"], ssl["var_weight"], ssl["top_every"], ssl["top_subsample"]) == \
        (0.75, 0.996, 25.0, 2, 0.5)
    assert cfg["dataset"]["clip_len"] == 16 and cfg["dataset"]["image_size"] == 112


def test_head_dim_is_refused():
    with pytest.raises(ValueError, match="head dim"):
        TS.TemporalSSL(embed_dim=256, layers=1, heads=2, clip_len=4, encoder=TM.StandInEncoder(256))
    with pytest.raises(ValueError, match="head dim"):
        TS.TemporalSSL(embed_dim=64, layers=1, heads=3, clip_len=4, encoder=TM.StandInEncoder(64))


def _small():
    return TS.TemporalSSL(embed_dim=64, layers=2, heads=2, clip_len=5, encoder=TM.StandInEncoder(64))


def test_parameter_tree():
    keys = set(_small().state_dict())
    for k in ("pos", "mask_token", "encoder.w", "temporal.layers.0.self_attn.in_proj_weight",
              "temporal.layers.1.linear2.bias", "temporal.layers.0.norm2.weight", "predictor_fc1.weight",
              "predictor_bn1.running_var", "predictor_bn1.num_batches_tracked", "predictor_fc2.bias",
              "top_head.weight"):
        assert k in keys, k
    assert not any(k.startswith("temporal.norm") for k in keys)        # no final norm
    full = TS.TemporalSSL(embed_dim=576, layers=1, heads=9, clip_len=4)
    assert "encoder.stages.3.2.mlp.fc2.weight" in full.state_dict()
    assert full.top_head.weight.shape == (4, 576) and full.pos.shape == (1, 4, 576)


def test_checkpoint_keys_and_finetune_bridge(tmp_path):
    """ssl_ep{N}.pth has the reference's keys; load_pretrained_ssl takes the student's encoder.*
    from it, and loads the forms it accepted before exactly as before."""
    import copy
    from ssl_mae_amd.finetune import VideoClassifier, load_pretrained_ssl
    from ssl_mae_amd.optim import FusedAdamW
    model = TS.TemporalSSL(embed_dim=576, layers=1, heads=9, clip_len=4)
    ema = copy.deepcopy(model)
    with torch.no_grad():
        for p in ema.parameters():
            p.add_(1.0)                                # the teacher must not be what is loaded
    opt = FusedAdamW(model.parameters(), lr=5e-4, weight_decay=0.05)
    state = TS.checkpoint_state(3, model, ema, opt)
    assert list(state) == ["epoch", "student", "ema", "opt"] and state["epoch"] == 3
    assert set(state["student"]) == set(model.state_dict()) == set(state["ema"])
    path = str(tmp_path / "ssl_ep3.pth")
    torch.save(state, path)
    clf = VideoClassifier(7)
    assert load_pretrained_ssl(clf, path)
    enc = model.encoder.state_dict()
    got = clf.backbone.state_dict()
    assert set(got) == set(enc)
    for k, v in enc.items():
        assert torch.equal(got[k], v), k
    # earlier forms: a full state with the encoder. prefix (bare or under "model"), a bare encoder state
    for form in ({"encoder." + k: v + 2 for k, v in enc.items()},
                 {"model": {"encoder." + k: v + 3 for k, v in enc.items()}},
                 {k: v + 4 for k, v in enc.items()}):
        p2 = str(tmp_path / "other.pth")
        torch.save(form, p2)
        clf2 = VideoClassifier(7)
        assert load_pretrained_ssl(clf2, p2)
        inner = form.get("model", form)
        want = {k[len("encoder."):] if k.startswith("encoder.") else k: v for k, v in inner.items()}
        for k, v in clf2.backbone.state_dict().items():
            assert torch.equal(v, want[k]), k
    assert not load_pretrained_ssl(VideoClassifier(7), str(tmp_path / "missing.pth"))


def test_train_ssl_module_is_an_alias():
    from ssl_mae_amd import train_ssl
    assert train_ssl.main is TS.main and train_ssl.TemporalSSL is TS.TemporalSSL


def test_operators_and_fakes_registered():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ssl_mae_amd import ops
    names = ("mfm_loss_fwd", "mfm_loss_bwd", "ema_update", "grad_clip", "relu_dropout_fwd", "relu_dropout_bwd")
    registered = set(ops.registered_ops())
    for n in names:
        assert n in registered, n
        assert str(getattr(torch.ops.ssl_mae, n).default._schema).startswith("ssl_mae::" + n)
    with FakeTensorMode():
        pred = torch.empty(15, 40, dtype=torch.bfloat16)
        teacher = torch.empty(15, 40)
        idx = torch.empty(11, dtype=torch.int32)
        out, stats = ops.mfm_loss_fwd(pred, teacher, idx, 1.0, 25.0, 1.0, 1e-4)
        assert out.shape == (3,) and out.dtype == torch.float32 and stats.shape == (3 * 11 + 2 * 40,)
        g = torch.empty(1)
        assert ops.mfm_loss_bwd(pred, teacher, idx, stats, g).dtype == torch.bfloat16
        assert ops.mfm_loss_bwd(pred, teacher, idx, stats, g, out_dtype=torch.float32).shape == (15, 40)
        x = torch.empty(6, 64, dtype=torch.bfloat16)
        y = ops.relu_dropout_fwd(x, 0.1, 2 ** 63 + 5)
        assert y.shape == x.shape and y.dtype == x.dtype
        assert ops.relu_dropout_bwd(y, x, 0.1, 2 ** 63 + 5).shape == x.shape
        buf = torch.empty(100)
        assert ops.ema_update(buf, torch.empty(100), 0.996) is buf
        assert ops.grad_clip(buf, [(0, 40), (48, 100)], 1.0).shape == (1,)


def test_no_cpu_fallback():
    from ssl_mae_amd import _lib, kernels
    pred, idx = torch.zeros(4, 8), torch.arange(2, dtype=torch.int32)
    for call in (lambda: kernels.ema_update(torch.zeros(8), torch.zeros(8), 0.5),
                 lambda: kernels.relu_dropout_fwd(torch.zeros(2, 8)),
                 lambda: kernels.relu_dropout_bwd(torch.zeros(2, 8), torch.zeros(2, 8)),
                 lambda: kernels.grad_clip(torch.zeros(8), [(0, 8)], 1.0),
                 lambda: kernels.mfm_loss_fwd(pred, pred, idx),
                 lambda: kernels.mfm_loss_bwd(pred, pred, idx, torch.zeros(22), torch.ones(1))):
        with pytest.raises(_lib.KernelError, match="no CPU fallback"):
            call()

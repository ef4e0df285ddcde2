"""Host-side pieces of the fine-tuning driver (no GPU): the AdamW segment table's layout,
train_finetune.resolve_config, finetune.layer_ids / param_groups / epoch_lr_mult."""
import math

import numpy as np
import pytest
import torch

LENS = [0, 1, 3, 4, 5, 2047, 2048, 2049, 4099]
GROUPS = [0, 1, 0, 1, 0, 1, 0, 1, 0]


# ------------------------------------------------------------------ adamw_table_layout
def test_adamw_table_layout_matches_the_documented_format():
    from ssl_mae_amd import kernels as K
    chunk = K.ADAMW_CHUNK_ELEMS
    assert chunk == 2048 and chunk % 4 == 0
    S = len(LENS)
    addrs = [(0x1000 * (4 * s + 1) + 4 * (s % 2), 0x1000 * (4 * s + 2), 0x1000 * (4 * s + 3) + 8, 0x1000 * (4 * s + 4))
             for s in range(S)]
    raw = K.adamw_table_layout(addrs, LENS, GROUPS)
    assert raw.dtype == np.uint8
    C = sum((n + chunk - 1) // chunk for n in LENS)
    total = (64 + 44 * S + 12 * C + 15) // 16 * 16
    assert raw.size == total == K.adamw_table_bytes(S, C)
    assert K.adamw_table_counts(raw) == (S, C)
    buf = raw.tobytes()
    header = np.frombuffer(buf, dtype=np.int64, count=8)
    assert header.tolist() == [K.ADAMW_TABLE_MAGIC, S, C, chunk, total, 0, 0, 0]
    assert K.ADAMW_TABLE_MAGIC.to_bytes(8, "little") == b"ADAMWTB1"
    off = 64
    addr = np.frombuffer(buf, dtype=np.uint64, count=4 * S, offset=off).reshape(4, S)
    off += 32 * S
    assert addr.T.tolist() == [list(a) for a in addrs]
    seg_len = np.frombuffer(buf, dtype=np.int64, count=S, offset=off)
    off += 8 * S
    assert seg_len.tolist() == LENS
    chunk_off = np.frombuffer(buf, dtype=np.int64, count=C, offset=off)
    off += 8 * C
    chunk_seg = np.frombuffer(buf, dtype=np.int32, count=C, offset=off)
    off += 4 * C
    seg_group = np.frombuffer(buf, dtype=np.int32, count=S, offset=off)
    off += 4 * S
    assert seg_group.tolist() == GROUPS
    assert set(buf[off:]) <= {0} and total - off < 16
    # the chunks cover every element of every segment exactly once
    assert (chunk_off % chunk == 0).all()
    cover = [np.zeros(n, dtype=np.int32) for n in LENS]
    for o, s in zip(chunk_off.tolist(), chunk_seg.tolist()):
        assert 0 <= s < S and 0 <= o < LENS[s]
        cover[s][o:min(o + chunk, LENS[s])] += 1
    assert all((c == 1).all() for c in cover)
    assert 0 not in chunk_seg.tolist()            # the zero-length segment has no chunk


def test_adamw_table_layout_rejects_bad_segments():
    from ssl_mae_amd import _lib, kernels as K
    ok = [(16, 32, 48, 64)]
    with pytest.raises(_lib.KernelError):
        K.adamw_table_layout([(18, 32, 48, 64)], [4], [0])          # address not a multiple of 4
    with pytest.raises(_lib.KernelError):
        K.adamw_table_layout(ok, [-1], [0])
    with pytest.raises(_lib.KernelError):
        K.adamw_table_layout(ok, [4], [K.ADAMW_MAX_GROUPS])
    with pytest.raises(_lib.KernelError):
        K.adamw_table_layout(ok, [4, 4], [0, 0])
    raw = K.adamw_table_layout(ok, [4], [0]).copy()
    raw[8] ^= 1                                                      # num_segments no longer fits the size
    with pytest.raises(_lib.KernelError):
        K.adamw_table_counts(raw)
    assert K.adamw_table_layout([], [], []).size == 64


# ------------------------------------------------------------------ resolve_config
def test_resolve_config_rules(tmp_path):
    from ssl_mae_amd import train_finetune as TF
    cfg = TF.resolve_config({})
    assert cfg["experiment"]["mode"] == "ft_random" and cfg["optimizer"]["type"] in TF.OPTIMIZERS
    assert cfg["training"]["layer_decay"] == 1.0 and cfg["training"]["no_decay_1d"] is False
    assert cfg["training"]["schedule"] == "constant" and cfg["model"]["embed_dim"] == 576
    with pytest.raises(ValueError, match="Unknown config section"):
        TF.resolve_config({"trainin": {}})
    with pytest.raises(ValueError, match="Unknown keys in training"):
        TF.resolve_config({"training": {"lr": 1.0}})
    with pytest.raises(ValueError, match="Unknown mode"):
        TF.resolve_config({"experiment": {"mode": "finetune"}})
    with pytest.raises(ValueError, match="Unknown mode"):
        TF.resolve_config({}, mode="probe")
    ckpt = tmp_path / "ssl.pth"
    torch.save({}, ckpt)
    with pytest.raises(ValueError, match="stage1_epochs"):
        TF.resolve_config({"training": {"stage1_epochs": 0}, "model": {"pretrained_ssl": str(ckpt)}}, mode="two_stage")
    for mode in ("linear_probe", "ft_ssl", "two_stage"):
        with pytest.raises(RuntimeError, match="pretrained_ssl checkpoint not found"):
            TF.resolve_config({"training": {"stage1_epochs": 1}}, mode=mode)
        with pytest.raises(RuntimeError, match="pretrained_ssl checkpoint not found"):
            TF.resolve_config({"training": {"stage1_epochs": 1}}, mode=mode, pretrained_ssl=str(tmp_path / "no.pth"))
        assert TF.resolve_config({"training": {"stage1_epochs": 1}}, mode=mode,
                                 pretrained_ssl=str(ckpt))["experiment"]["mode"] == mode
    # command line over file over defaults
    got = TF.resolve_config({"training": {"epochs": 7, "batch_size": 3}, "optimizer": {"type": "adamw_torch"}},
                            epochs=2, save_dir="out", optimizer="fused")
    assert got["training"]["epochs"] == 2 and got["training"]["batch_size"] == 3
    assert got["paths"]["save_dir"] == "out" and got["optimizer"]["type"] == "adamw"
    assert TF.resolve_config({}, optimizer="torch")["optimizer"]["type"] == "adamw_torch"
    with pytest.raises(ValueError):
        TF.resolve_config({}, optimizer="sgd")
    with pytest.raises(ValueError):
        TF.resolve_config({"optimizer": {"type": "sgd"}})
    with pytest.raises(ValueError):
        TF.resolve_config({"training": {"schedule": "step"}})


def test_shipped_config_resolves_and_cli_help(capsys):
    import os
    from conftest import ROOT
    from ssl_mae_amd import train_finetune as TF
    from ssl_mae_amd.utils import load_config
    cfg = TF.resolve_config(load_config(os.path.join(ROOT, "configs", "finetune.yaml")))
    assert cfg["experiment"]["mode"] == "ft_random" and not cfg["dataset"]["train_split"]
    with pytest.raises(SystemExit) as e:
        TF.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--config", "--mode", "--pretrained_ssl", "--epochs", "--batch_size", "--save_dir", "--optimizer"):
        assert flag in out


# ------------------------------------------------------------------ layer ids / groups / schedule
@pytest.fixture(scope="module")
def model():
    from ssl_mae_amd.finetune import VideoClassifier
    torch.manual_seed(0)
    return VideoClassifier(4, img_size=112)


def test_layer_ids(model):
    from ssl_mae_amd.finetune import layer_ids
    ids = layer_ids(model)
    names = [n for n, _ in model.named_parameters()]
    assert set(ids) == set(names)
    L = sum(len(stage) for stage in model.backbone.stages)
    assert L == 15
    stem = [n for n in names if n.startswith("backbone.patch_embed.")]
    assert stem and all(ids[n] == 0 for n in stem)
    assert all(ids[n] == L + 1 for n in names if n.startswith("classifier."))
    seq = [ids[n] for n in names]                       # named_parameters is forward order
    assert seq == sorted(seq)
    bb = [ids[n] for n in names if n.startswith("backbone.")]
    assert max(bb) == L and sorted(set(bb)) == list(range(L + 1))
    first_of_stage1 = next(n for n in names if n.startswith("backbone.stages.1.0."))
    assert ids[first_of_stage1] == 1 + len(model.backbone.stages[0])


def _cfg(**training):
    tr = {"learning_rate": 3e-4, "weight_decay": 0.05, "head_lr": 1e-3, "backbone_lr": 1e-4, "layer_decay": 1.0,
          "no_decay_1d": False}
    tr.update(training)
    return {"training": tr}


def _same_groups(ours, opt):
    theirs = opt.param_groups
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        assert [id(p) for p in a["params"]] == [id(p) for p in b["params"]]
        assert a["lr"] == b["lr"] and a["weight_decay"] == b["weight_decay"]


def test_param_groups_equal_build_optimizer_without_decay(model):
    from ssl_mae_amd.finetune import build_optimizer, param_groups, set_requires_grad
    cfg = _cfg()
    try:
        for mode in ("ft_random", "linear_probe", "ft_ssl", "two_stage"):
            for frozen in (True, False):               # before and after unfreezing
                set_requires_grad(model.backbone, not frozen)
                groups = param_groups(model, cfg, mode)
                _same_groups(groups, build_optimizer(cfg, model, mode))
                assert all(len(g["names"]) == len(g["params"]) for g in groups)
                assert all(p.requires_grad for g in groups for p in g["params"])
    finally:
        set_requires_grad(model.backbone, True)


def test_param_groups_layer_decay_and_no_decay_1d(model):
    from ssl_mae_amd.finetune import param_groups
    for mode in ("ft_ssl", "two_stage"):
        cfg = _cfg(layer_decay=0.75, no_decay_1d=True)
        groups = param_groups(model, cfg, mode)
        got = {}
        for g in groups:
            for n, p in zip(g["names"], g["params"]):
                assert n not in got
                got[n] = (g["lr"], g["weight_decay"], p)
        assert len({(g["lr"], g["weight_decay"]) for g in groups}) == len(groups)      # equal pairs merged
        params = dict(model.named_parameters())
        assert set(got) == set(params)
        sizes = [len(s) for s in model.backbone.stages]
        for n, p in params.items():
            # the expected pair, worked out from the name alone
            parts = n.split(".")
            if parts[0] == "classifier":
                depth, base = 0, (1e-3 if mode == "two_stage" else 3e-4)
            else:
                base = 1e-4 if mode == "two_stage" else 3e-4
                if parts[1] == "patch_embed":
                    depth = 16
                else:
                    depth = 16 - (1 + sum(sizes[:int(parts[2])]) + int(parts[3]))
            want_lr = base * 0.75 ** depth
            want_wd = 0.0 if p.ndim <= 1 else 0.05
            assert got[n][2] is p
            assert got[n][0] == pytest.approx(want_lr, rel=1e-12) and got[n][1] == want_wd, n
        assert any(wd == 0.0 for _, wd, _ in got.values()) and any(wd == 0.05 for _, wd, _ in got.values())
        assert len(groups) <= 64


def test_epoch_lr_mult():
    from ssl_mae_amd.finetune import epoch_lr_mult
    const = {"training": {"schedule": "constant", "epochs": 10, "learning_rate": 1e-3}}
    assert all(epoch_lr_mult(e, const) == 1.0 for e in range(10))
    assert epoch_lr_mult(3, {"training": {"epochs": 10, "learning_rate": 1e-3}}) == 1.0
    cfg = {"training": {"schedule": "cosine", "epochs": 20, "warmup_epochs": 4, "min_lr": 1e-5,
                        "learning_rate": 1e-3}}
    assert [epoch_lr_mult(e, cfg) for e in range(4)] == [0.25, 0.5, 0.75, 1.0]          # linear warmup
    assert epoch_lr_mult(4, cfg) == 1.0                                                 # first cosine epoch
    floor = 1e-5 / 1e-3
    for e in range(4, 20):
        want = floor + 0.5 * (1 - floor) * (1 + math.cos(math.pi * (e - 4) / 16))
        assert epoch_lr_mult(e, cfg) == pytest.approx(want, rel=1e-12)
    seq = [epoch_lr_mult(e, cfg) for e in range(4, 20)]
    assert all(a > b for a, b in zip(seq, seq[1:]))
    long = dict(cfg["training"], epochs=2000)
    assert epoch_lr_mult(1999, {"training": long}) == pytest.approx(floor, abs=1e-5)    # approaches min_lr / base
    assert epoch_lr_mult(1999, {"training": long}) > floor
    with pytest.raises(ValueError):
        epoch_lr_mult(0, {"training": {"schedule": "step", "epochs": 1, "learning_rate": 1.0}})

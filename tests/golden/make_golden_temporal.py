"""Golden fixture for temporal SSL pretraining (tests/golden/temporal_ssl.npz) by RUNNING the
reference's own TemporalSSL and train_one_epoch (src/train_ssl.py) on the CPU, in the build
container.  The reference is imported the way make_golden.py does it, plus an empty `cv2`
module (datasets/loader.py and transforms.py import it at module scope and the step never
touches it) and the `datasets` package routed to the reference's directory.  No reference code
is copied: the step is the reference's function, observed through wrappers around the helpers
it calls (build_mask, permute_frames_4way, cosine_loss, variance_loss, F.cross_entropy,
clip_grad_norm_, forward_tokens, predictor).

(a) `a/*`  head only: build_mobilevit_s replaced by tests/temporal_mirror.StandInEncoder (a fixed
    linear map of the pooled frame, no parameters); D = 64, 2 heads, 1 layer, B = 3, T = 5, 32x32
    frames, dropout 0, TOP on with top_subsample 0.7 (k = 2), clip_grad_norm 1.0.
(b) `b/*`  one real step: the reference TinyViT (tiny_vit_21m_variant, embedding = pooled stage-4
    map, as make_golden_finetune.py) as encoder, D = 576, 9 heads, 2 layers, B = 2, T = 4,
    112x112, DropPath and dropout 0, fp32, TOP on (every sample), clip_grad_norm 1.0.
Weights: ssl_mae_amd.init_rule on the whole model (student; the teacher is its deepcopy).
Both also hold `perm/T{T}_l{label}` = _perm_index_4way(T, label) for T in {3, 4, 8, 16}.

Run:  python tests/golden/make_golden_temporal.py
"""
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import temporal_mirror as TM  # noqa: E402
from ssl_mae_amd.init_rule import apply_rule, synthetic_clip  # noqa: E402


def import_train_ssl():
    MG._install_stubs()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, MG.REF_SRC)
    saved = {k: v for k, v in sys.modules.items() if k == "datasets" or k.startswith("datasets.")}
    for k in saved:
        del sys.modules[k]
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(MG.REF_SRC, "datasets")]
    sys.modules["datasets"] = pkg
    import train_ssl
    import models.tiny_vit as tiny_vit
    for k in [k for k in sys.modules if k == "datasets" or k.startswith("datasets.")]:
        del sys.modules[k]
    sys.modules.update(saved)
    return train_ssl, tiny_vit


class _FProxy:
    """torch.nn.functional with cross_entropy's result recorded."""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(F, name)

    def cross_entropy(self, *a, **k):
        out = F.cross_entropy(*a, **k)
        self._log["top"] = float(out.detach())
        return out


def run_step(train_ssl, model, cfg, clip, seed):
    """One reference step (epoch 1, step 1) -> the record of everything observed."""
    log = {}
    ema = copy.deepcopy(model)
    for p in ema.parameters():
        p.requires_grad_(False)
    opt = torch.optim.AdamW(model.parameters(), lr=float(cfg["training"]["learning_rate"]),
                            weight_decay=float(cfg["training"]["weight_decay"]))
    scaler = torch.cuda.amp.GradScaler(enabled=False)
    orig = {n: getattr(train_ssl, n) for n in ("build_mask", "permute_frames_4way", "cosine_loss", "variance_loss", "F")}
    orig_clip = torch.nn.utils.clip_grad_norm_

    def build_mask(*a, **k):
        log["mask"] = orig["build_mask"](*a, **k)
        return log["mask"]

    def permute(clip_src):
        out, labels = orig["permute_frames_4way"](clip_src)
        log["labels"] = labels
        log["top_batch"] = clip_src.shape[0]
        return out, labels

    def cosine(p, z):
        out = orig["cosine_loss"](p, z)
        log["mfm"] = float(out.detach())
        return out

    def variance(z, *a, **k):
        out = orig["variance_loss"](z, *a, **k)
        log["var"] = float(out.detach())
        return out

    def clip_norm(params, max_norm, *a, **k):
        out = orig_clip(params, max_norm, *a, **k)
        log["norm"] = float(out)
        return out

    fwd, pred = model.forward_tokens, model.predictor

    def forward_tokens(c, mask=None):
        out = fwd(c, mask=mask)
        if mask is not None:
            log["ctx"] = out.detach().clone()
        else:
            log["ctx_top"] = out.detach().clone()
        return out

    def predictor(x):
        out = pred(x)
        log["pred"] = out.detach().clone()
        return out

    ema_fwd = ema.forward_tokens

    def teacher_tokens(c, mask=None):
        log["ctx_t"] = ema_fwd(c, mask=mask).detach().clone()
        return log["ctx_t"]

    ema.forward_tokens = teacher_tokens
    model.forward_tokens, model.predictor = forward_tokens, predictor
    train_ssl.build_mask, train_ssl.permute_frames_4way = build_mask, permute
    train_ssl.cosine_loss, train_ssl.variance_loss, train_ssl.F = cosine, variance, _FProxy(log)
    torch.nn.utils.clip_grad_norm_ = clip_norm
    try:
        torch.manual_seed(seed)
        train_ssl.train_one_epoch(model, ema, [clip], opt, scaler, None, torch.device("cpu"), cfg, 1)
    finally:
        for n, v in orig.items():
            setattr(train_ssl, n, v)
        torch.nn.utils.clip_grad_norm_ = orig_clip
        del model.forward_tokens, model.predictor, ema.forward_tokens
    # the two losses once more by the reference's functions on the recorded tensors in fp64
    # (train_ssl.py:205-219 line for line): what the fp64 mirror must reproduce to rounding
    m = log["mask"]
    z_t = F.normalize(log["ctx_t"].double()[m], dim=-1)
    z_s = F.normalize(log["pred"].double().reshape(m.shape + (-1,))[m], dim=-1)
    ssl = cfg["ssl_objectives"]
    log["mfm64"] = float(train_ssl.cosine_loss(z_s, z_t))
    log["var64"] = float(train_ssl.variance_loss(z_s, ssl["var_target_std"], ssl["var_eps"]))
    return log, ema


def cfg_for(top_subsample):
    return {"training": {"amp": False, "clip_grad_norm": 1.0, "log_interval": 1000, "learning_rate": 5e-4,
                         "weight_decay": 0.05},
            "ssl_objectives": {"mask_ratio": 0.75, "mfm_weight": 1.0, "ema_momentum": 0.996, "var_weight": 25.0,
                               "var_eps": 1e-4, "var_target_std": 1.0, "top_weight": 1.0, "top_start_epoch": 1,
                               "top_every": 1, "top_subsample": top_subsample, "top_detach_backbone": False}}


def record(rec, tag, log, model, ema, full_grads, tol):
    rec[tag + "mask"] = log["mask"].numpy()
    rec[tag + "labels"] = log["labels"].numpy()
    rec[tag + "top_batch"] = np.int64(log["top_batch"])
    for k in ("mfm", "var", "top", "norm", "mfm64", "var64"):
        rec[tag + k] = np.float64(log[k])
    if full_grads:
        rec[tag + "ctx"] = log["ctx"].numpy()
        rec[tag + "ctx_t"] = log["ctx_t"].numpy()
        rec[tag + "pred"] = log["pred"].numpy()
    # per parameter with a gradient, in `names` order: rows of (sum, L2, first 8 values, zero
    # padded) for the clipped gradient, the student after AdamW and the teacher after the EMA
    # update; (a) also the gradients in full, concatenated
    # `cond`: how far one AdamW step can move when the gradient is off by delta = tol max|g| (tol
    # the gradient tolerance of the case's GPU test), in units of lr.  The first step is
    # lr g / (|g| + 1e-8), whose slope is 1e-8 / (|g| + 1e-8)^2: e_i = min(2, delta 1e-8 /
    # (max(|g_i| - delta, 0) + 1e-8)^2) -- negligible for |g_i| >> delta, a full step of either sign
    # below it.  Row = (sum e, L2 e, e of the first 8).
    # (TM.adam_step_slack).  (a) holds the after-step student and teacher in full as well.
    names, rows, full = [], {"g": [], "after": [], "ema": [], "cond": []}, {"grads": [], "after_full": [], "ema_full": []}
    teacher = dict(ema.named_parameters())
    for n, p in model.named_parameters():
        if p.grad is None:
            continue
        names.append(n)
        if full_grads:
            for key, t in (("grads", p.grad), ("after_full", p), ("ema_full", teacher[n])):
                full[key].append(t.detach().reshape(-1).numpy().copy())
        e = TM.adam_step_slack(p.grad, tol)
        head = e[:8].numpy()
        rows["cond"].append(np.concatenate([[float(e.sum()), float(e.norm())], head, np.zeros(8 - head.size)]))
        for kind, t in (("g", p.grad), ("after", p), ("ema", teacher[n])):
            s, l2, head = TM.summary(t)
            rows[kind].append(np.concatenate([[s, l2], head, np.zeros(8 - head.size)]))
    rec[tag + "names"] = np.array(names)
    for kind, r in rows.items():
        rec[tag + kind] = np.stack(r)
    if full_grads:
        for key, parts in full.items():
            rec[tag + key] = np.concatenate(parts)
    # BatchNorm buffers: the predictor's in full, the encoder's as (sum, L2) in `bufnames` order
    bufnames, bufrows = [], []
    for n, b in model.named_buffers():
        if not n.endswith(("running_mean", "running_var", "num_batches_tracked")):
            continue
        if n.startswith("predictor"):
            rec[tag + "buf/" + n] = b.detach().numpy().copy()
        else:
            bufnames.append(n)
            v = b.detach().double().reshape(-1)
            bufrows.append([float(v.sum()), float(v.norm())])
    if bufnames:
        rec[tag + "bufnames"] = np.array(bufnames)
        rec[tag + "bufstats"] = np.array(bufrows)
    ebuf = {n: b for n, b in ema.named_buffers()}
    rec[tag + "ema_bn_tracked_max"] = np.int64(max([int(b) for n, b in ebuf.items()
                                                    if n.endswith("num_batches_tracked")] or [0]))


def parity_mode(model):
    MG._parity_mode(model)


def main():
    train_ssl, tiny_vit = import_train_ssl()
    torch.set_num_threads(8)
    rec = {}
    for T in (3, 4, 8, 16):
        for label in range(4):
            rec[f"perm/T{T}_l{label}"] = train_ssl._perm_index_4way(T, label).numpy()

    # (a) head only
    B, T, S, D = 3, 5, 32, 64
    orig_build = train_ssl.build_mobilevit_s
    train_ssl.build_mobilevit_s = lambda embed_dim=256: TM.StandInEncoder(embed_dim)
    model = train_ssl.TemporalSSL(embed_dim=D, layers=1, heads=2, clip_len=T)
    apply_rule(model)
    parity_mode(model)
    clip = torch.from_numpy(synthetic_clip(B, T, S, seed=97531))
    log, ema = run_step(train_ssl, model, cfg_for(0.7), clip, seed=2024)
    rec.update({"a/B": B, "a/T": T, "a/S": S, "a/D": D, "a/seed": 2024, "a/clip_seed": 97531})
    record(rec, "a/", log, model, ema, full_grads=True, tol=1e-5)
    print(f"(a) mfm {log['mfm']:.6f} var {log['var']:.6f} top {log['top']:.6f} norm {log['norm']:.6f}")

    # (b) one real step
    class RefBackbone(tiny_vit.TinyViT):
        def forward(self, x):
            feat = super().forward(x)
            return feat, F.adaptive_avg_pool2d(feat, 1).flatten(1)

    B, T, S, D = 2, 4, 112, 576
    train_ssl.build_mobilevit_s = lambda embed_dim=256: RefBackbone(
        img_size=S, embed_dims=[96, 192, 384, 576], depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 18], use_checkpoint=True)
    model = train_ssl.TemporalSSL(embed_dim=D, layers=2, heads=9, clip_len=T)
    train_ssl.build_mobilevit_s = orig_build
    apply_rule(model)
    parity_mode(model)
    clip = torch.from_numpy(synthetic_clip(B, T, S, seed=86420))
    log, ema = run_step(train_ssl, model, cfg_for(1.0), clip, seed=777)
    rec.update({"b/B": B, "b/T": T, "b/S": S, "b/D": D, "b/seed": 777, "b/clip_seed": 86420})
    record(rec, "b/", log, model, ema, full_grads=False, tol=1e-3)
    print(f"(b) mfm {log['mfm']:.6f} var {log['var']:.6f} top {log['top']:.6f} norm {log['norm']:.6f}")

    out = os.path.join(HERE, "temporal_ssl.npz")
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()

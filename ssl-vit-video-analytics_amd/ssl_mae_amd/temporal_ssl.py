"""Temporal SSL pretraining (reference: src/train_ssl.py), MI355X-native.

`TemporalSSL` does masked-frame modelling against an EMA teacher with a VICReg-style
variance term and a 4-way temporal-order-prediction (TOP) head.  Names, signatures,
parameter tree and arithmetic are the reference's; as in the fine-tune row the
MobileViT backbone is replaced by the MAE's TinyViT (`finetune.tiny_vit_backbone`,
576-d embedding).  The torch modules are parameter containers (same classes and init
calls as train_ssl.py:97-126); the computation runs on the HIP Functions:

    encoder      all B*T frames as ONE batch (train_ssl.py:145-149: BatchNorm statistics over
                 B*T frames), read from the 5-D clip through its strides
    pos / token  sm_pos_blend_fwd/bwd with L = 1 and a zero spatial table: a masked frame
                 carries the bare token, without position (train_ssl.py:151-155)
    temporal     BlockFn on an fp32 residual stream, ReLU feed-forward (st.relu), dropout
                 0.1 in train mode, no final norm
    predictor    fc1 -> train-mode BatchNorm over the B*T rows fused with GELU -> fc2
    objective    sm_mfm_loss_fwd/bwd over the masked rows of pred and the teacher's tokens
    TOP          sm_gather_frames (index arithmetic on (b, t), no clone of the clip) ->
                 encoder -> temporal layers -> segment mean -> head -> sm_logits_metrics
    step         backward, sm_grad_clip, FusedAdamW, sm_ema_update over the flat buffers

Host draws come from torch's CPU generator in the reference's calls and order
(randperm(T) per sample, randperm(B)[:k], randint(0, 4, (B,))), so a fixture recorded by
the reference on the CPU reproduces them.  The teacher is a deepcopy taken before the
first forward, kept in eval(): update_ema covers parameters only (train_ssl.py:36-39), so
its BatchNorm buffers keep their values from construction -- reproduced here.
The reference calls the teacher outside its autocast block (fp32); fp32 is this
project's parity path, so the driver runs the teacher in the student's precision
unless `training.teacher_amp: false` asks for the reference's fp32 teacher.

    PYTHONPATH=ssl-vit-video-analytics_amd python -m ssl_mae_amd.train_ssl --config configs/ssl_train.yaml
"""
import argparse
import copy
import os
from pathlib import Path
from typing import Tuple

import torch
import torch.nn as nn

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher
from .driver import SyntheticBatches as SyntheticClips    # drawn per batch: pixels, gain; no labels
from .driver import split_file_loader, start
from .finetune import SegMeanFn, TopCEFn, tiny_vit_backbone
from .functions import BlockFn, G, Mode, W, _bn_params, _done, _touch, _train_bn_only
from .mae_vit_adapter import _St, ensure_flat, make_flat, next_seed_base
from .optim import FusedAdamW, GradScaler
from .utils import load_config


# ============================================================ autograd Functions
class MFMLossFn(torch.autograd.Function):
    """pred [R,D], teacher fp32 [R,D], idx int32 [N] ascending -> fp32 [3] = (mfm, var,
    w_mfm mfm + w_var var); only element 2 carries a gradient (to pred)."""

    @staticmethod
    def forward(ctx, pred, teacher, idx, w_mfm, w_var, target_std, eps):
        pred = pred.contiguous()
        out, stats = K.mfm_loss_fwd(pred, teacher, idx, w_mfm, w_var, target_std, eps)
        ctx.w = (w_mfm, w_var)
        ctx.save_for_backward(pred, teacher, idx, stats)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, teacher, idx, stats = ctx.saved_tensors
        dpred = K.mfm_loss_bwd(pred, teacher, idx, stats, g.float()[2:3].contiguous(), ctx.w[0], ctx.w[1])
        return dpred, None, None, None, None, None, None


class FlatLinearFn(torch.autograd.Function):
    """nn.Linear on the fp32 GEMM (as finetune.HeadLinearFn) whose gradients go to the flat
    buffer: the root's parameters all live there, for FusedAdamW."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = x.float().contiguous()
        ctx.params = (w, b)
        ctx.save_for_backward(x)
        return K.linear(x, w.detach(), b.detach())

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        w, b = ctx.params
        _touch(w, b)
        dy = dy.float().contiguous()
        M, N = dy.shape
        K.linear_dw(dy, x, G(w))
        ones = K.fill_(torch.empty(M, dtype=torch.float32, device=dy.device), 1.0)
        K.gemm(ones, dy, G(b), 1, N, M, 0, 1, M, N, N, beta=1.0)          # db += 1^T dy
        dx = K.linear_dx(dy, w.detach()) if ctx.needs_input_grad[0] else None
        _done(w, b)
        return dx, None, None


class PosTokenFn(torch.autograd.Function):
    """f + pos[:, :T], then f[mask] = mask_token (train_ssl.py:151-155): emb fp32 [B*T, D] ->
    fp32 [B*T, D] by the MAE's position / mask-token blend with one token per frame."""

    @staticmethod
    def forward(ctx, emb, mask_u8, st, pos, tok):
        B, T, D = st.B, st.T, st.D
        emb = emb.float().contiguous()
        spos = torch.zeros((1, D), dtype=torch.float32, device=emb.device)
        x = K.pos_blend(emb, pos.detach().reshape(-1, D)[:T], spos, tok.detach().reshape(D), mask_u8, B, T, 1, D,
                        torch.float32)
        ctx.st = st
        ctx.params = (pos, tok)
        ctx.save_for_backward(mask_u8)
        return x

    @staticmethod
    def backward(ctx, dx):
        mask_u8, = ctx.saved_tensors
        pos, tok = ctx.params
        B, T, D = ctx.st.B, ctx.st.T, ctx.st.D
        _touch(pos, tok)
        dx = dx.float().contiguous()
        sink = torch.zeros((1, D), dtype=torch.float32, device=dx.device)     # the spatial table has no parameter
        dy = K.pos_blend_bwd(dx, mask_u8, torch.float32, G(pos).reshape(-1, D)[:T], sink, G(tok).reshape(D), B, T,
                             1, D)
        _done(pos, tok)
        return dy, None, None, None, None


class PredictorFn(torch.autograd.Function):
    """fc1 -> BatchNorm1d (batch statistics over all rows in train mode, running statistics
    updated as nn.BatchNorm1d updates them) fused with exact GELU -> fc2 (train_ssl.py:128-136)."""

    @staticmethod
    def forward(ctx, x, st, w1, b1, g, beta, w2, b2):
        mode = st.mode
        xa = x.contiguous() if x.dtype == mode.act else K.cast(x.contiguous(), mode.act)
        a = K.linear(xa, W(w1, mode), b1.detach())
        mean, rstd = _bn_params(a, st.bn)
        h = K.bn_apply(a, mean, rstd, g.detach(), beta.detach(), gelu=True)
        y = K.linear(h, W(w2, mode), b2.detach())
        ctx.st = st
        ctx.params = (w1, b1, g, beta, w2, b2)
        ctx.x_dtype = x.dtype
        ctx.save_for_backward(xa, a, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        _train_bn_only(ctx, ctx.st.bn)
        xa, a, mean, rstd = ctx.saved_tensors
        w1, b1, g, beta, w2, b2 = ctx.params
        mode = ctx.st.mode
        _touch(*ctx.params)
        dy = dy.contiguous()
        if dy.dtype != mode.act:
            dy = K.cast(dy, mode.act)
        h = K.bn_apply(a, mean, rstd, g.detach(), beta.detach(), gelu=True)
        K.linear_dw_bias(dy, h, G(w2), G(b2))
        del h
        dh = K.linear_dx(dy, W(w2, mode))
        da = K.bn_bwd(dh, a, mean, rstd, g.detach(), beta.detach(), True, G(g), G(beta))
        del dh
        K.linear_dw_bias(da, xa, G(w1), G(b1))
        dx = K.linear_dx(da, W(w1, mode), out_dtype=ctx.x_dtype)
        _done(*ctx.params)
        return (dx,) + (None,) * 7


# ============================================================ loss helpers
def _rows(n, device):
    return torch.arange(n, dtype=torch.int32, device=device)


def cosine_loss(p: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """train_ssl.py:26-29 over all rows of p, z [N, D] (device tensors)."""
    return MFMLossFn.apply(p, z.detach().float().contiguous(), _rows(p.shape[0], p.device), 1.0, 0.0, 1.0, 1e-4)[2]


def variance_loss(z: torch.Tensor, target_std: float = 1.0, eps: float = 1e-4) -> torch.Tensor:
    """train_ssl.py:31-34 of the row-normalised z [N, D] (what the step passes: z_s is normalised
    at train_ssl.py:216 before both losses)."""
    return MFMLossFn.apply(z, z.detach().float().contiguous(), _rows(z.shape[0], z.device), 0.0, 1.0,
                           float(target_std), float(eps))[2]


def _flat_of(root):
    params = list(root.parameters())
    flat = getattr(params[0], "_sm_flat", None)
    if flat is None or any(getattr(p, "_sm_flat", None) is not flat for p in params):
        if params[0].device.type != "cuda":
            raise RuntimeError("ssl_mae_amd models run on the GPU only (move the model with .to('cuda'))")
        flat = make_flat(root, params[0].device)
    return flat


@torch.no_grad()
def update_ema(ema: nn.Module, model: nn.Module, m: float):
    """train_ssl.py:36-39 as one launch over the two flat parameter buffers (parameters only:
    the teacher's buffers are never touched)."""
    fe, fs = _flat_of(ema), _flat_of(model)
    if fe.names != fs.names or fe.offsets != fs.offsets or fe.total != fs.total:
        raise RuntimeError("update_ema: teacher and student do not share a parameter layout")
    K.ema_update(fe.data, fs.data, float(m))


def _host_mask(B: int, T: int, ratio: float) -> torch.Tensor:
    n = max(1, int(T * ratio))
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(T)[:n]] = True                  # CPU generator, one draw per sample
    return mask


def build_mask(B: int, T: int, ratio: float, device) -> torch.Tensor:
    """train_ssl.py:41-47; the draws come from the CPU generator whatever the device."""
    return _host_mask(B, T, ratio).to(device)


# ============================================================ TOP permutation: 4-way
def _perm_index_4way(T: int, label: int) -> torch.Tensor:
    """train_ssl.py:54-74: 0 identity, 1 reverse, 2 swap halves, 3 rotate quarters (identity
    when T < 4)."""
    frames = torch.arange(T)
    if label == 1:
        return frames.flip(0)
    # the other three are rotations to the left: by nothing, by half the clip, by a quarter of it
    # (a quarter of fewer than 4 frames is 0 frames: the identity)
    shift = {0: 0, 2: T // 2}.get(label, T // 4)
    return torch.roll(frames, -shift)


def _top_frames(clip, idx_b, labels):
    """Frames [b'*T, C, H, W] of the permuted clips: frame (i, t) = clip[idx_b[i], :, perm_i[t]]
    (sm_gather_frames)."""
    T = clip.shape[2]
    n = labels.numel()
    src = torch.arange(n) if idx_b is None else idx_b
    t_idx = torch.stack([_perm_index_4way(T, int(labels[i])) for i in range(n)]).reshape(-1)
    b_idx = src.reshape(-1, 1).expand(n, T).reshape(-1)
    dev = clip.device
    return K.gather_frames(clip if clip.dtype == torch.float32 else clip.float(),
                           b_idx.to(torch.int32).to(dev), t_idx.to(torch.int32).to(dev), n * T)


def permute_frames_4way(clip: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """train_ssl.py:76-90.  clip [B,C,T,H,W] on the device -> (clip_top, labels): clip_top is a
    [B,C,T,H,W] view of the gathered frames (stored frame-major, the layout the backbone reads),
    labels int64 [B] on the device, drawn from the CPU generator."""
    B, C, T, H, W = clip.shape
    labels = torch.randint(0, 4, (B,))
    frames = _top_frames(clip, None, labels)
    return frames.view(B, T, C, H, W).permute(0, 2, 1, 3, 4), labels.to(clip.device)


# ============================================================ Model
class TemporalSSL(nn.Module):
    """train_ssl.py:97-158 with `encoder = tiny_vit_backbone(img_size)`; state-dict keys
    `encoder.*`, `pos`, `mask_token`, `temporal.layers.N.*`, `predictor_fc1/bn1/fc2`, `top_head`.
    `encoder` may be any module with `embed(x, mode) -> (emb fp32 [N, embed_dim], _)` for a clip
    [B,3,T,H,W] or frames [N,3,H,W]."""

    def __init__(self, embed_dim: int, layers: int, heads: int, clip_len: int, img_size: int = 112, encoder=None):
        super().__init__()
        if embed_dim % heads or embed_dim // heads not in (32, 64):
            raise ValueError(f"TemporalSSL: head dim {embed_dim}/{heads} is not 32 or 64 (the attention kernels' "
                             "head sizes); e.g. embed_dim 576 with 9 or 18 heads")
        self.embed_dim = embed_dim
        self.clip_len = clip_len
        self.heads = heads
        self.encoder = encoder if encoder is not None else tiny_vit_backbone(img_size=img_size)
        enc_dim = getattr(self.encoder, "embed_dims", [embed_dim])[-1]
        if enc_dim != embed_dim:
            raise ValueError(f"TemporalSSL: embed_dim {embed_dim} but the encoder embeds to {enc_dim}")

        self.pos = nn.Parameter(torch.zeros(1, clip_len, embed_dim))
        nn.init.trunc_normal_(self.pos, std=0.02)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        nn.init.trunc_normal_(self.mask_token, std=0.02)

        enc = nn.TransformerEncoderLayer(d_model=embed_dim, nhead=heads, dim_feedforward=embed_dim * 4,
                                         batch_first=True, norm_first=True)
        self.temporal = nn.TransformerEncoder(enc, layers, enable_nested_tensor=False)

        self.predictor_fc1 = nn.Linear(embed_dim, embed_dim)
        self.predictor_bn1 = nn.BatchNorm1d(embed_dim)
        self.predictor_fc2 = nn.Linear(embed_dim, embed_dim)
        self.top_head = nn.Linear(embed_dim, 4)
        from .tiny_vit import index_modules
        index_modules(self)
        self._sm_mode = None

    def _begin(self):
        mode = Mode(torch.is_autocast_enabled("cuda"), next_seed_base(self))
        ensure_flat(self, mode)
        self._sm_mode = mode
        return mode

    def predictor(self, x_bt_d: torch.Tensor) -> torch.Tensor:
        """x_bt_d [B*T, D] -> [B*T, D] (bf16 under autocast)."""
        mode = self._sm_mode
        if mode is None or mode.bf16 != torch.is_autocast_enabled("cuda"):
            mode = self._begin()
        st = _St(mode=mode, bn=self.predictor_bn1)
        return PredictorFn.apply(x_bt_d, st, self.predictor_fc1.weight, self.predictor_fc1.bias,
                                 self.predictor_bn1.weight, self.predictor_bn1.bias, self.predictor_fc2.weight,
                                 self.predictor_fc2.bias)

    def top_logits(self, feat: torch.Tensor) -> torch.Tensor:
        return FlatLinearFn.apply(feat, self.top_head.weight, self.top_head.bias)

    def forward_tokens(self, clip: torch.Tensor, mask: torch.Tensor = None) -> torch.Tensor:
        """clip [B,C,T,H,W] (any strides), mask bool [B,T] or None -> ctx fp32 [B,T,D]."""
        B, C, T, H, W = clip.shape
        if T > self.clip_len:
            raise ValueError(f"clip has {T} frames, pos covers {self.clip_len}")
        mode = self._begin()
        dev = self.pos.device
        if clip.device != dev:
            clip = clip.to(dev, non_blocking=True)
        if clip.dtype != torch.float32:
            clip = clip.float()
        D = self.embed_dim
        emb = self.encoder.embed(clip, mode)[0]                  # [B*T, D]: frames b*T + t, one batch
        if mask is None:
            m8 = torch.zeros((B, T, 1), dtype=torch.uint8, device=dev)
        else:
            m8 = mask.to(device=dev, dtype=torch.uint8).reshape(B, T, 1).contiguous()
        x = PosTokenFn.apply(emb.reshape(B * T, D), m8, _St(B=B, T=T, D=D), self.pos, self.mask_token)
        tr = self.training
        for layer in self.temporal.layers:
            sa = layer.self_attn
            idx = getattr(layer, "_sm_index", 0)
            st = _St(mode=mode, N=B, L=T, heads=self.heads, head_dim=D // self.heads, eps=layer.norm1.eps, relu=True,
                     attn_drop=sa.dropout if tr else 0.0, seed_attn=mode.seed(idx, 0),
                     drop1=layer.dropout1.p if tr else 0.0, seed1=mode.seed(idx, 1),
                     drop_ff=layer.dropout.p if tr else 0.0, seed_ff=mode.seed(idx, 2),
                     drop2=layer.dropout2.p if tr else 0.0, seed2=mode.seed(idx, 3), dp1=None, dp2=None)
            x = BlockFn.apply(x, st, layer.norm1.weight, layer.norm1.bias, sa.in_proj_weight, sa.in_proj_bias,
                              sa.out_proj.weight, sa.out_proj.bias, layer.norm2.weight, layer.norm2.bias,
                              layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias)
        return x.view(B, T, D)


# ============================================================ Train step
def clip_grad_norm_(model: nn.Module, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) over the gradient ranges the
    backward touched; the total norm stays on the device."""
    flat = _flat_of(model)
    return K.grad_clip(flat.grad, flat.touched_ranges(), float(max_norm))


def ssl_step(model, ema, clip, cfg, epoch, step, opt=None, amp=True):
    """One step of train_ssl.py:195-265 on a device clip: teacher target, masked student, the
    optional TOP pass, backward, clip, optimizer, EMA.  Returns the device scalars
    {mfm, var, top (or None), norm (or None)}, the host draws {mask, labels, idx_b} and the tokens
    {ctx, pred, ctx_t}.  The teacher runs in the student's precision unless training.teacher_amp
    says otherwise (false: fp32, where the reference's call outside its autocast block puts it)."""
    ssl, tr = cfg["ssl_objectives"], cfg["training"]
    B, C, T, H, W = clip.shape
    dev = clip.device
    mask = _host_mask(B, T, ssl["mask_ratio"])
    idx = mask.reshape(-1).nonzero().reshape(-1).to(torch.int32).to(dev)

    def autocast(on=amp):
        return torch.autocast("cuda", dtype=torch.bfloat16, enabled=on)

    with torch.no_grad(), autocast(bool(tr.get("teacher_amp", amp)) and amp):
        ctx_t = ema.forward_tokens(clip, mask=None).reshape(B * T, -1)
    with autocast():
        ctx_s = model.forward_tokens(clip, mask=mask)
        pred = model.predictor(ctx_s.reshape(B * T, -1))
        out = MFMLossFn.apply(pred, ctx_t, idx, float(ssl["mfm_weight"]), float(ssl["var_weight"]),
                              float(ssl["var_target_std"]), float(ssl["var_eps"]))
        loss = out[2]

    loss_top = labels = idx_b = None
    top_on = epoch >= int(ssl["top_start_epoch"]) and step % int(ssl.get("top_every", 1)) == 0 \
        and ssl["top_weight"] > 0
    if top_on:
        sub = float(ssl.get("top_subsample", 1.0))
        if sub < 1.0:
            idx_b = torch.randperm(B)[:max(2, int(B * sub))]
        nb = B if idx_b is None else idx_b.numel()
        labels = torch.randint(0, 4, (nb,))
        frames = _top_frames(clip, idx_b, labels)
        clip_top = frames.view(nb, T, C, H, W).permute(0, 2, 1, 3, 4)
        detach = bool(ssl.get("top_detach_backbone", False))
        with autocast():
            if detach:     # feat.detach(): nothing upstream of the head is differentiated
                with torch.no_grad():
                    ctx_top = model.forward_tokens(clip_top, mask=None)
            else:
                ctx_top = model.forward_tokens(clip_top, mask=None)
            feat = SegMeanFn.apply(ctx_top.reshape(nb * T, -1), nb, T)
            loss_top = TopCEFn.apply(model.top_logits(feat), labels.to(dev))
            loss = loss + ssl["top_weight"] * loss_top

    norm = None
    if opt is not None:
        opt.zero_grad(set_to_none=True)
    loss.backward()
    if tr.get("clip_grad_norm", None) is not None:
        norm = clip_grad_norm_(model, tr["clip_grad_norm"])
    if opt is not None:
        opt.step()
        update_ema(ema, model, ssl["ema_momentum"])
    return {"mfm": out[0].detach(), "var": out[1].detach(), "top": None if loss_top is None else loss_top.detach(),
            "norm": norm, "mask": mask, "labels": labels, "idx_b": idx_b, "ctx": ctx_s.detach(), "pred": pred.detach(),
            "ctx_t": ctx_t}


def train_one_epoch(model, ema, loader, opt, scaler, sch, device, cfg, epoch):
    """train_ssl.py:165-295.  The loss scalars accumulate on the device and are read back every
    log_interval steps; bf16 needs no loss scaling (`scaler` is the optim.GradScaler shim)."""
    model.train()
    ema.eval()
    ssl, tr = cfg["ssl_objectives"], cfg["training"]
    use_amp = bool(tr.get("amp", True))
    top_enabled = epoch >= int(ssl["top_start_epoch"])
    running = None
    n = 0
    avg = (0.0, 0.0, 0.0)
    for step, clip in enumerate(loader, start=1):
        clip = clip.to(device, non_blocking=True)
        r = ssl_step(model, ema, clip, cfg, epoch, step, opt=opt, amp=use_amp)
        if sch is not None:
            sch.step()
        if running is None:
            running = torch.zeros(3, dtype=torch.float32, device=clip.device)
        running[0] += r["mfm"]
        running[1] += r["var"]
        if r["top"] is not None:
            running[2] += r["top"]
        n += 1
        if step % int(tr["log_interval"]) == 0:
            avg = tuple(v / n for v in running.tolist())
            top_note = (f"TOP every {int(ssl.get('top_every', 1))} steps on {float(ssl.get('top_subsample', 1.0)):g} "
                        "of the batch") if top_enabled else "TOP off"
            print(f"[INFO] epoch {epoch} step {step}/{len(loader)}: running means mfm {avg[0]:.4f}, var {avg[1]:.4f}, "
                  f"top {avg[2]:.4f} ({top_note})")
    if running is not None:
        avg = tuple(v / max(1, n) for v in running.tolist())
    print(f"[INFO] epoch {epoch} finished after {n} steps: mean mfm {avg[0]:.4f}, var {avg[1]:.4f}, top {avg[2]:.4f}")
    return {"mfm": avg[0], "var": avg[1], "top": avg[2]}


# ============================================================ Main
def split_loader(cfg, device):
    """Lines of `<frame directory> ...` under `split_root` through driver.split_file_loader:
    unlabelled, shuffled, RGB order (ClipResizer(bgr_swap=False))."""
    ds, tr = cfg["dataset"], cfg["training"]
    return split_file_loader(os.path.join(ds.get("split_root", ""), ds["train_split"]), clip_len=ds["clip_len"],
                             stride=ds["stride"], image_size=ds["image_size"], batch_size=tr["batch_size"],
                             num_workers=tr.get("num_workers", 4), device=device, labelled=False, bgr_swap=False,
                             shuffle=True, drop_last=True, pin_memory=True)


DATASET_DEFAULTS = {"clip_len": 16, "stride": 2, "image_size": 112, "train_split": None, "split_root": "data/splits",
                    "synthetic_steps": 4}


def resolve_config(cfg):
    """The file's values with the dataset keys the reference reads from configs/base.yaml."""
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in (cfg or {}).items()}
    ds = dict(DATASET_DEFAULTS)
    ds.update(cfg.get("dataset") or {})
    cfg["dataset"] = ds
    for sec in ("training", "model", "ssl_objectives"):
        if sec not in cfg:
            raise ValueError(f"[ERROR] config section missing: {sec}")
    return cfg


def build_model(cfg, device):
    m, ds = cfg["model"], cfg["dataset"]
    model = TemporalSSL(embed_dim=int(m["embed_dim"]), layers=int(m["temporal_layers"]),
                        heads=int(m["temporal_heads"]), clip_len=int(ds["clip_len"]),
                        img_size=int(ds["image_size"])).to(device)
    ema = copy.deepcopy(model).to(device)        # before the first forward
    for p in ema.parameters():
        p.requires_grad_(False)
    ema.eval()
    return model, ema


def checkpoint_state(epoch, model, ema, opt):
    """train_ssl.py:355-360: keys epoch, student, ema, opt (tensors cloned off the flat buffers)."""
    return {"epoch": epoch,
            "student": {k: v.detach().clone() for k, v in model.state_dict().items()},
            "ema": {k: v.detach().clone() for k, v in ema.state_dict().items()},
            "opt": opt.state_dict()}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Temporal SSL pretraining (masked-frame teacher-student + TOP).")
    ap.add_argument("--config", default="configs/ssl_train.yaml")
    ap.add_argument("--epochs", type=int, default=None, help="override training.epochs")
    ap.add_argument("--batch_size", type=int, default=None, help="override training.batch_size")
    ap.add_argument("--save_every", type=int, default=None, help="override training.save_every")
    ap.add_argument("--save_dir", default=None, help="override training.save_dir")
    ap.add_argument("--synthetic_steps", type=int, default=None, help="batches per epoch without a split")
    args = ap.parse_args(argv)
    cfg = resolve_config(load_config(args.config))
    tr = cfg["training"]
    for key in ("epochs", "batch_size", "save_every", "save_dir"):
        if getattr(args, key) is not None:
            tr[key] = getattr(args, key)
    if args.synthetic_steps is not None:
        cfg["dataset"]["synthetic_steps"] = args.synthetic_steps
    device = start("train_ssl", cfg.get("seed", 42))
    ds = cfg["dataset"]
    split = ds.get("train_split")
    if split and os.path.isfile(os.path.join(ds.get("split_root", ""), split)):
        loader = split_loader(cfg, device)
    else:
        print("[INFO] No split file: synthetic clips")
        loader = SyntheticClips(ds["synthetic_steps"], tr["batch_size"], ds["clip_len"], ds["image_size"], device,
                                seed=cfg.get("seed", 42))
    model, ema = build_model(cfg, device)
    opt = FusedAdamW(model.parameters(), lr=float(tr["learning_rate"]), weight_decay=float(tr["weight_decay"]))
    scaler = GradScaler(enabled=bool(tr.get("amp", True)))
    sch = None                                    # as the reference (train_ssl.py:345-346)
    save_dir = Path(tr["save_dir"])
    save_dir.mkdir(parents=True, exist_ok=True)
    for ep in range(1, int(tr["epochs"]) + 1):
        train_one_epoch(model, ema, loader, opt, scaler, sch, device, cfg, ep)
        if ep % int(tr["save_every"]) == 0:
            torch.save(checkpoint_state(ep, model, ema, opt), save_dir / f"ssl_ep{ep}.pth")
            print(f"[INFO] Saved checkpoint: {save_dir / f'ssl_ep{ep}.pth'}")


if __name__ == "__main__":
    main()

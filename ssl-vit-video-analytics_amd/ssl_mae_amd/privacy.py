"""Feature-privacy evaluation of the video embeddings (reference src/privacy/feature_noise.py,
metrics_privacy.py, attacker.py and run_privacy.py:229-348), MI355X-native.

Perturbation   add_gaussian_noise, apply_feature_mask and perturb_grid run sm_privacy_perturb:
  counter-based draws, a pure function of (seed, row, column), so a rerun reproduces every
  number (the reference draws from the global torch RNG).  perturb_mirror states the same
  draws on the host in numpy / fp64: it is the specification the kernel is tested against.
Metrics        prediction_entropy, top1_accuracy, privacy_exposure_rate with the reference's
  formulas; logits_metrics gives loss / entropy / top-1 / top-k for S stacked copies of a
  label vector in one launch (sm_logits_metrics).
Attacker       FeatureAttacker keeps the reference's net.0 / net.2 parameters; its Linears
  run on the fp32 GEMM, its ReLU on sm_relu_fwd / sm_relu_bias_bwd.  train_attacker is the
  reference's full-batch Adam loop (run_privacy.py:310-320) on one flat buffer with sm_adamw,
  the cross-entropy gradient from sm_logits_metrics; nothing is read back inside the loop.
Embeddings     video_embeddings is the [B, D] eval-mode mean embedding
  (run_privacy.py:45-53 extract_video_embedding) on VideoClassifier.forward's path.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops as K
from .finetune import HeadLinearFn, SegMeanFn
from .functions import Mode, splitmix64
from .mae_vit_adapter import ensure_flat, next_seed_base

_M32 = 0xFFFFFFFF
_ROW_MUL, _COL_MUL = 0x9E3779B1, 0x7FEB352D
_STREAMS = (0x68E31DA4, 0xB5297A4D, 0x1B56C4E9)


# ------------------------------------------------------------------ draw specification (host)
def mask_threshold(mask_ratio):
    """Integer keep threshold T = min(round(ratio * 2^32), 2^32): an element is kept iff its
    32-bit mask draw is >= T, so the drop probability is T / 2^32 (within 2^-33 of the ratio).
    ratio <= 0 keeps everything, ratio >= 1 drops everything."""
    r = float(mask_ratio)
    if not r > 0.0:
        return 0
    return min(int(round(r * 4294967296.0)), 1 << 32)


def config_seed(seed, g):
    """Seed of grid configuration g: splitmix64(seed ^ splitmix64(g))."""
    return splitmix64((int(seed) & ((1 << 64) - 1)) ^ splitmix64(int(g)))


def grid_configs(sigmas, mask_ratios, seed):
    """[(sigma, mask_ratio, seed_g)] in the reference's loop order (run_privacy.py:294-295:
    sigma outer, mask inner)."""
    out = []
    for s in sigmas:
        for r in mask_ratios:
            out.append((float(s), float(r), config_seed(seed, len(out))))
    return out


def _fmix32(h):
    h = h & _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    h ^= h >> 16
    return h


def perturb_draws(seed, N, D):
    """The three 32-bit streams (h0, h1, h2), each uint64-typed [N, D] numpy, of sm_privacy_perturb
    (include/sm_api.h): the row and the column are mixed in separate fmix32 rounds."""
    seed = int(seed) & ((1 << 64) - 1)
    s32 = (seed & _M32) ^ (seed >> 32)
    rows = np.arange(N, dtype=np.uint64)[:, None]
    cols = np.arange(D, dtype=np.uint64)[None, :]
    rb = _fmix32(np.uint64(s32) + rows * np.uint64(_ROW_MUL))
    cm = (cols * np.uint64(_COL_MUL)) & np.uint64(_M32)
    return tuple(_fmix32(_fmix32(rb + np.uint64(k)) + cm) for k in _STREAMS)


def gaussian_from_draws(h0, h1):
    """fp64 Box-Muller cosine branch: u1 = ((h0 >> 8) + 1) 2^-24, u2 = (h1 >> 8) 2^-24."""
    u1 = ((h0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (h1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def perturb_mirror(z, sigma, mask_ratio, seed):
    """Host statement of one configuration: (z + sigma n) keep in fp64 for z [N, D]; sigma is
    rounded to fp32 first, as the kernel receives it.  sigma <= 0 and mask_ratio <= 0 return z's
    values unchanged."""
    z = np.asarray(z.detach().cpu().numpy() if isinstance(z, torch.Tensor) else z)
    if z.ndim != 2:
        raise ValueError("perturb_mirror takes z [N, D]")
    N, D = z.shape
    out = z.astype(np.float64)
    h0, h1, h2 = perturb_draws(seed, N, D)
    sig = float(np.float32(sigma))
    if sig > 0.0:
        out = out + sig * gaussian_from_draws(h0, h1)
    thr = mask_threshold(mask_ratio)
    if thr:
        out = out * (h2 >= np.uint64(thr)).astype(np.float64)
    return out


# ------------------------------------------------------------------ perturbation (device)
def _fresh_seed():
    return int(torch.randint(0, 1 << 62, (1,)).item())


def _z2d(z):
    if z.dim() != 2:
        raise ValueError("feature perturbation takes embeddings [N, D]")
    return z.float().contiguous()


def add_gaussian_noise(z, sigma, seed=None):
    """feature_noise.py:4-7; sigma <= 0 returns z itself."""
    if float(sigma) <= 0:
        return z
    return K.privacy_perturb(_z2d(z), [float(sigma)], [0], [_fresh_seed() if seed is None else seed])[0]


def apply_feature_mask(z, mask_ratio, seed=None):
    """feature_noise.py:10-15 (0/1 mask, no rescale); mask_ratio <= 0 returns z itself."""
    if float(mask_ratio) <= 0:
        return z
    return K.privacy_perturb(_z2d(z), [0.0], [mask_threshold(mask_ratio)],
                             [_fresh_seed() if seed is None else seed])[0]


def perturb_grid(z, sigmas, mask_ratios, seed):
    """-> fp32 [G, N, D], configuration g = grid_configs(...)[g], one launch that reads z once."""
    cfgs = grid_configs(sigmas, mask_ratios, seed)
    if not cfgs:
        raise ValueError("perturb_grid needs at least one sigma and one mask ratio")
    return K.privacy_perturb(_z2d(z), [c[0] for c in cfgs], [mask_threshold(c[1]) for c in cfgs],
                             [c[2] for c in cfgs])


# ------------------------------------------------------------------ metrics
def logits_metrics(logits, labels, k, segments=1):
    """logits [S*N, C], labels [N] -> (loss, entropy, top1, topk): fp64 [S] per-segment means."""
    out = K.logits_metrics(logits.float().contiguous(), labels.long().contiguous(), k, segments)
    out = out / float(labels.numel())
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def prediction_entropy(logits):
    """metrics_privacy.py:5-8: mean over rows of -sum p log(p + 1e-12)."""
    labels = torch.zeros(logits.shape[0], dtype=torch.int64, device=logits.device)
    return logits_metrics(logits, labels, 1)[1].item()


def top1_accuracy(logits, labels):
    """metrics_privacy.py:15-16."""
    return logits_metrics(logits, labels, 1)[2].item()


def privacy_exposure_rate(before, after):
    """metrics_privacy.py:11-12."""
    return after / max(before, 1e-6)


# ------------------------------------------------------------------ attacker
class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre):
        h = K.relu_fwd(pre.contiguous())
        ctx.save_for_backward(h)
        return h

    @staticmethod
    def backward(ctx, dh):
        (h,) = ctx.saved_tensors
        db = torch.empty(h.shape[-1], dtype=torch.float32, device=h.device)
        return K.relu_bias_bwd(dh.float().contiguous().view(-1, h.shape[-1]), h.view(-1, h.shape[-1]), db).view_as(h)


class FeatureAttacker(nn.Module):
    """attacker.py:5-18 (Linear - ReLU - Linear, parameters net.0.* / net.2.*: the same draws
    under the same torch seed), forward on the fp32 GEMM and the ReLU kernel."""

    def __init__(self, dim, num_classes):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, num_classes))

    def forward(self, z):
        z = z.float().contiguous()
        h = ReluFn.apply(HeadLinearFn.apply(z, self.net[0].weight, self.net[0].bias))
        return HeadLinearFn.apply(h, self.net[2].weight, self.net[2].bias)


def _flatten_attacker(attacker):
    """Move the four parameters into one flat fp32 buffer (each segment padded to 16 bytes; the
    padding has zero gradient, which Adam leaves at zero) -> (flat, parameter views)."""
    params = [attacker.net[0].weight, attacker.net[0].bias, attacker.net[2].weight, attacker.net[2].bias]
    sizes = [(p.numel() + 3) // 4 * 4 for p in params]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=params[0].device)
    views, off = [], 0
    for p, n in zip(params, sizes):
        v = flat[off:off + p.numel()].view(p.shape)
        v.copy_(p.detach())
        p.data = v
        views.append(v)
        off += n
    return flat, views


def train_attacker(attacker, z_priv, y, epochs, lr):
    """run_privacy.py:310-320: `epochs` full-batch steps of Adam(lr) (betas 0.9 / 0.999, eps 1e-8,
    no weight decay) on the mean cross-entropy of attacker(z_priv) against y.  Forward, backward
    and the update are kernel launches only; returns the attacker (trained in place)."""
    z = z_priv.detach().float().contiguous()
    y = y.long().contiguous()
    if not z.is_cuda:
        raise RuntimeError("train_attacker needs device tensors (no CPU fallback)")
    N, D = z.shape
    attacker.to(z.device)
    flat, (w1, b1, w2, b2) = _flatten_attacker(attacker)
    grad = torch.zeros_like(flat)
    gw1, gb1, gw2, gb2 = [], [], [], []
    off = 0
    for p, dst in ((w1, gw1), (b1, gb1), (w2, gw2), (b2, gb2)):
        dst.append(grad[off:off + p.numel()].view(p.shape))
        off += (p.numel() + 3) // 4 * 4
    gw1, gb1, gw2, gb2 = gw1[0], gb1[0], gw2[0], gb2[0]
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    step = torch.zeros(1, dtype=torch.int64, device=z.device)
    C = w2.shape[0]
    ones = K.fill_(torch.empty(N, dtype=torch.float32, device=z.device), 1.0)
    dlogits = torch.empty((N, C), dtype=torch.float32, device=z.device)
    for _ in range(int(epochs)):
        h = K.relu_fwd(K.linear(z, w1, b1))
        logits = K.linear(h, w2, b2)
        K.logits_metrics(logits, y, 1, 1, dlogits, 1.0 / N)          # d mean-CE / d logits
        K.linear_dw(dlogits, h, gw2, accumulate=False)
        K.gemm(ones, dlogits, gb2, 1, C, N, 0, 1, N, C, C)           # db2 = 1^T dlogits (any class count)
        dpre = K.relu_bias_bwd(K.linear_dx(dlogits, w2), h, gb1)
        K.linear_dw(dpre, z, gw1, accumulate=False)
        K.adamw(flat, grad, m, v, float(lr), 0.9, 0.999, 1e-8, 0.0, None, step)
    return attacker


# ------------------------------------------------------------------ embeddings and head
class HeadLinear(nn.Linear):
    """nn.Linear whose forward is finetune.HeadLinearFn, the fp32 GEMM VideoClassifier.forward
    applies its head with (same parameters, same state_dict keys)."""

    def forward(self, x):
        return HeadLinearFn.apply(x.float().contiguous(), self.weight, self.bias)


def route_head(model):
    """Make `model.classifier(z)` -- the call the reference's driver makes on embeddings
    (run_privacy.py:272, :304) -- run on the GEMM that `model(clip)` uses for its head instead of
    torch's eager Linear, whose sums come in another order: the module's class becomes
    HeadLinear, nothing else changes.  Idempotent; returns the model."""
    if type(model.classifier) is nn.Linear:
        model.classifier.__class__ = HeadLinear
    return model


@torch.no_grad()
def video_embeddings(model, clip):
    """clip [B, C, T, H, W] -> fp32 [B, D]: the temporal mean of the per-frame embeddings of an
    eval-mode finetune.VideoClassifier, computed exactly as VideoClassifier.forward does before
    its head (all B * T frames in one batch).  The model's head is routed through the project's
    GEMM (route_head), so model.classifier(video_embeddings(model, clip)) equals model(clip) bit
    for bit."""
    bb = model.backbone
    if bb.training:
        raise RuntimeError("video_embeddings needs model.eval(): it is the eval-mode embedding")
    route_head(model)
    B, C, T, H, W = clip.shape
    if clip.dtype != torch.float32:
        clip = clip.float()
    mode = Mode(torch.is_autocast_enabled("cuda"), next_seed_base(bb))
    ensure_flat(bb, mode)
    feats = bb.embed(clip, mode)[0].view(B, T, -1)
    return SegMeanFn.apply(feats.reshape(B * T, -1), B, T)

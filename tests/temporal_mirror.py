"""fp64 torch statement of the temporal-SSL formulas (reference src/train_ssl.py:26-34,
:205-220), gradients by autograd, and the stand-in encoder shared by the fixture generator
(tests/golden/make_golden_temporal.py) and the GPU test.  No HIP here."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def mfm_terms(pred, teacher, idx, target_std, eps):
    """pred, teacher [R, D] (any float dtype, taken to fp64), idx long [N] ->
    (mfm, var, sigma [D]) as the reference's step forms them: both row sets normalised
    (train_ssl.py:206, :216), cosine_loss normalising a second time (:27-28), variance_loss
    on the normalised student rows (:33-34)."""
    z_t = F.normalize(teacher.double()[idx], dim=-1)
    z_s = F.normalize(pred.double()[idx], dim=-1)
    p, z = F.normalize(z_s, dim=-1), F.normalize(z_t, dim=-1)
    mfm = 2.0 - 2.0 * (p * z).sum(dim=-1).mean()
    sigma = torch.sqrt(z_s.var(dim=0, unbiased=False) + eps)
    var = torch.mean(F.relu(target_std - sigma))
    return mfm, var, sigma


def mfm_loss_and_grad(pred, teacher, idx, w_mfm, w_var, target_std, eps, upstream=1.0):
    """-> (fp64 [3] losses, fp64 dpred [R, D], sigma [D])."""
    p = pred.detach().double().clone().requires_grad_(True)
    mfm, var, sigma = mfm_terms(p, teacher, idx, target_std, eps)
    total = w_mfm * mfm + w_var * var
    (total * upstream).backward()
    return torch.stack([mfm, var, total]).detach(), p.grad.detach(), sigma.detach()


def midpoint_target(sigma):
    """The midpoint of two adjacent sorted sigma: the widest gap among the pairs that leave at
    least a quarter of the columns on each side of the hinge."""
    s = torch.sort(sigma.double()).values
    n = s.numel()
    lo, hi = (n + 3) // 4, n - (n + 3) // 4
    gaps = (s[lo:hi + 1] - s[lo - 1:hi]) / s[lo:hi + 1]
    k = lo + int(torch.argmax(gaps))
    return float((s[k - 1] + s[k]) / 2)


def ema_fp64(dst, src, m):
    """(fp64 value, the bound 2^-23 (|m e| + |(1 - m) p|)) with m, 1 - m rounded as torch rounds
    them for an fp32 tensor (1.0 - m formed in double)."""
    mf = float(torch.tensor(m, dtype=torch.float32))
    af = float(torch.tensor(1.0 - m, dtype=torch.float32))
    a, b = mf * dst.double(), af * src.double()
    return a + b, 2.0 ** -23 * (a.abs() + b.abs())


def drop_scale(p):
    """csrc/common.h drop_scale16 / drop_thr16 -> (scale, thr): 16-bit threshold."""
    thr = int(p * 65536.0 + 0.5)
    return 0.0 if thr >= 65536 else 65536.0 / (65536 - thr), thr


class StandInEncoder(nn.Module):
    """A fixed linear map of the frame pooled to 4x4 (48 values) to `embed_dim`: no parameters,
    one buffer.  `forward` has the reference backbone's contract (x [N,3,H,W] -> (None, emb));
    `embed` the HIP model's (clip [B,3,T,H,W] or frames -> (emb fp32 [N, D], None))."""

    def __init__(self, embed_dim):
        super().__init__()
        self.embed_dims = [embed_dim]
        d = torch.arange(embed_dim, dtype=torch.float64).reshape(-1, 1)
        k = torch.arange(48, dtype=torch.float64).reshape(1, -1)
        self.register_buffer("w", (torch.sin(0.37 * d + 1.3 * k + 0.11 * d * k) / math.sqrt(48.0) * 6.0).float())

    def forward(self, x):
        pooled = F.adaptive_avg_pool2d(x.float(), 4).flatten(1)
        return None, pooled @ self.w.t()

    def embed(self, x, mode=None):
        if x.dim() == 5:
            B, C, T, H, W = x.shape
            x = x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
        return self.forward(x)[1], None


def adam_step_slack(grad, tol, whole_noise=False):
    """Per element, in units of lr: how far one AdamW step can move when the gradient is off by
    delta = tol max|g|.  The first step is lr g / (|g| + 1e-8), whose slope is 1e-8 / (|g| + 1e-8)^2:
    e_i = min(2, delta 1e-8 / (max(|g_i| - delta, 0) + 1e-8)^2) -- nothing for |g_i| >> delta, a full
    step of either sign below it.  whole_noise: the whole gradient is rounding noise (analytically
    zero), every element may take a full step of either sign."""
    g = grad.detach().double().reshape(-1).abs().cpu()
    if whole_noise:
        return torch.full_like(g, 2.0)
    delta = tol * float(g.max())
    return torch.clamp(delta * 1e-8 / (torch.clamp(g - delta, min=0.0) + 1e-8) ** 2, max=2.0)


def summary(t):
    """(sum, L2, first 8) in fp64: the ft_ssl fixture's per-parameter form."""
    v = t.detach().double().reshape(-1).cpu()
    return float(v.sum()), float(v.norm()), v[:8].numpy().copy()

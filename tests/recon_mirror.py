"""fp64 torch mirror of sm_mae_reconstruct / sm_recon_clip_metrics (include/sm_api.h), shared by
tests/test_reconstruct_cpu.py and tests/test_reconstruct_gpu.py.  Plain tensor ops on the host:
patchify, the norm_pix statistics, the blends, the clamp and the byte cast, each as the header
states it; the inputs are taken as given (a bf16 pred is widened exactly)."""
import torch

NEAR = 1e-3      # |v * 255 - integer| below this: the byte may differ by one (tests' docstring)


def patchify(x, p=8):
    """[B,C,T,H,W] -> [B, T*hp*wp, p*p*C], token (t,h,w), feature (pi,qi,c) (train_ssl_mae.py:26-31)."""
    B, C, T, H, W = x.shape
    hp, wp = H // p, W // p
    x = x.reshape(B, C, T, hp, p, wp, p)
    return torch.einsum("bcthpwq->bthwpqc", x).reshape(B, T * hp * wp, p * p * C)


def unpatchify(tok, C, T, H, W, p=8):
    """The exact inverse: 'bthwpqc->bcthpwq' (the reference's visualize_mae.py:30 drops q)."""
    B = tok.shape[0]
    hp, wp = H // p, W // p
    x = tok.reshape(B, T, hp, wp, p, p, C)
    return torch.einsum("bthwpqc->bcthpwq", x).reshape(B, C, T, H, W)


def reconstruct(pred, clip, mask, mean, std, norm_pix=True, paste_visible=True, bgr_swap=True):
    """-> dict: panels uint8 [B,T,H,3W,3], level fp64 (the clamped v * 255 behind each byte),
    near bool (bytes that may differ by one), recon fp64 [B,3,T,H,W], token_err fp64 [B,T*L,2],
    clip_metrics fp64 [B,4]."""
    B, C, T, H, W = clip.shape
    L = (H // 8) * (W // 8)
    x = patchify(clip.detach().cpu().double())
    pr = pred.detach().cpu().double().reshape(B, T * L, 192)
    m = mask.detach().cpu().reshape(B, T * L).bool()
    src = [2 - c if bgr_swap else c for c in range(3)]                 # source channel of clip channel c
    mean_f = torch.tensor([mean[s] for s in src], dtype=torch.float64).repeat(64)   # feature f: c = f % 3
    std_f = torch.tensor([std[s] for s in src], dtype=torch.float64).repeat(64)
    if norm_pix:
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).sum(-1, keepdim=True) / 191.0
        sd = (var + 1e-6).sqrt()
        tgt, r = (x - mu) / sd, pr * sd + mu
    else:
        tgt, r = x, pr
    v_x, v_r = x * std_f + mean_f, r * std_f + mean_f
    err = torch.stack([((pr - tgt) ** 2).mean(-1),
                       ((v_r.clamp(0, 1) - v_x.clamp(0, 1)) ** 2).mean(-1)], dim=-1)
    v_out = torch.where(~m[..., None], v_x, v_r) if paste_visible else v_r

    def rgb(tokens):                                                   # -> [B,3,T,H,W], RGB order
        img = unpatchify(tokens, 3, T, H, W)
        return img.flip(1) if bgr_swap else img

    orig, out = rgb(v_x), rgb(v_out)
    m_up = rgb(m[..., None].expand(-1, -1, 192).double())              # 1 on the pixels of masked patches
    hwc = [t.permute(0, 2, 3, 4, 1) for t in (orig, orig, out)]
    v = torch.cat(hwc, dim=3)                                          # [B,T,H,3W,3]
    zero = torch.cat([torch.zeros_like(m_up), m_up, torch.zeros_like(m_up)], dim=4).permute(0, 2, 3, 4, 1) > 0
    t255 = v * 255.0
    level = (v.clamp(0, 1) * 255.0).masked_fill(zero, 0.0)
    tc = t255.clamp(-0.5, 255.5)                                       # far outside [0, 1]: the clamp decides
    near = ((tc - tc.round()).abs() < NEAR) & ~zero
    cm = torch.zeros(B, 4, dtype=torch.float64)
    for b in range(B):
        n = int(m[b].sum())
        cm[b, 3] = n
        if n:
            cm[b, 0] = err[b, m[b], 0].sum() / n
            cm[b, 1] = err[b, m[b], 1].sum() / n
        cm[b, 2] = 10.0 * torch.log10(1.0 / cm[b, 1]) if cm[b, 1] > 0 else float("inf")
    return {"panels": level.floor().to(torch.uint8), "level": level, "near": near, "recon": out,
            "token_err": err, "clip_metrics": cm}

"""Streaming dynamic inference for the fine-tuned VideoClassifier, MI355X-native.

Reference: src/models/dynamic_infer.py -- `motion_scores_l1` (:34-49),
`select_topk_frames` (:53-82), `EarlyExitStats` (:85-89) and
`streaming_early_exit` (:93-189), with the reference's names and signatures.

Execution (all HIP, csrc/dynamic.hip): the motion scores are one pass over the
strided clip; the top-k selection, the frame gather, the per-frame
running-mean / head / max-softmax / exit decision and the compaction of the
still-undecided samples are one kernel each.  No torch compute op runs inside the
loop.

Where this departs from the reference, on purpose: the reference keeps encoding
all B samples until every one has exited (:175 encodes clip[:, :, t] whole and
masks afterwards).  Here each step gathers frame t of the *active* samples only
into one dense batch, so a decided sample is never encoded again.  With an
eval-mode backbone (BatchNorm on running statistics) frames are independent and
the outputs are those of the reference; a training-mode backbone would see other
batch statistics after compaction, so it is refused.

Host traffic of the loop: the count of active samples, 4 bytes per processed
frame, which sizes the next step's launches (`readbacks()` counts them).
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import ops as K

_readbacks = 0


def readbacks():
    """Device-to-host count readbacks issued by streaming_early_exit so far (one per
    processed frame)."""
    return _readbacks


def _read_count(count):
    global _readbacks
    _readbacks += 1
    return int(count.item())


def _f32(clip):
    if clip.dim() != 5:
        raise ValueError(f"clip must be [B,C,T,H,W], got {tuple(clip.shape)}")
    return clip if clip.dtype == torch.float32 else clip.float()


@torch.no_grad()
def motion_scores_l1(clip: torch.Tensor) -> torch.Tensor:
    """clip [B,C,T,H,W] -> scores [B,T]: mean |frame t - frame t-1|, 0 for t = 0."""
    return K.motion_scores(_f32(clip))


@torch.no_grad()
def select_topk_frames(clip: torch.Tensor, k: int, score_type: str = "motion") -> Tuple[torch.Tensor, torch.Tensor]:
    """Keep k frames per sample: -> (clip_sel [B,C,k,H,W], idx [B,k] int64, ascending).

    "motion": the k frames with the highest motion score (ties: the lower frame index
    first -- the reference leaves them to torch.topk).  "random": k sorted distinct frames
    per sample drawn from the torch CPU generator.

    clip_sel is a permuted view of the dense [B,k,C,H,W] gather output, not a
    contiguous [B,C,k,H,W] tensor: every consumer here (the stem, the gather of
    streaming_early_exit, motion_scores_l1) reads a clip through its strides."""
    if score_type not in ("motion", "random"):
        raise ValueError(f"Unknown score_type: {score_type}")
    clip = _f32(clip)
    B, C, T, H, W = clip.shape
    k_eff = min(int(k), T)
    if k_eff < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if score_type == "motion":
        idx32 = K.topk_frames(K.motion_scores(clip), k_eff)
    else:
        idx32 = torch.stack([torch.randperm(T)[:k_eff].sort()[0] for _ in range(B)], dim=0).to(
            device=clip.device, dtype=torch.int32)
    dense = K.gather_frames(clip, None, idx32.reshape(-1), B * k_eff, rows_per_b=k_eff)
    return dense.view(B, k_eff, C, H, W).permute(0, 2, 1, 3, 4), idx32.long()


@dataclass
class EarlyExitStats:
    """Statistics returned by streaming early-exit."""
    used_frames: torch.Tensor  # [B] int64
    final_conf: torch.Tensor   # [B] float


def frame_order(T, max_frames=None, frame_step=1):
    """The frames streaming_early_exit encodes, in order: 0, then 1, 1 + step, ...
    below min(T, max_frames) (dynamic_infer.py:121-124, :144, :171)."""
    if max_frames is not None:
        T = min(T, int(max_frames))
    return [0] + list(range(1, T, max(int(frame_step), 1)))


@torch.no_grad()
def streaming_early_exit(backbone, classifier, clip: torch.Tensor, threshold: float, min_frames: int = 4,
                         max_frames: Optional[int] = None, frame_step: int = 1
                         ) -> Tuple[torch.Tensor, EarlyExitStats]:
    """Streaming confidence-based temporal early-exit; each frame is encoded at most once and
    only for the samples still undecided.

    backbone: frames [n,C,H,W] -> (feat, emb [n,D]) (TinyViTBackbone.forward); an nn.Module
    must be in eval mode.  classifier: nn.Linear D -> K.  Returns (final_logits [B,K],
    EarlyExitStats(used_frames [B], final_conf [B]))."""
    if isinstance(backbone, nn.Module) and backbone.training:
        raise RuntimeError("streaming_early_exit needs an eval-mode backbone: dropping decided samples from the "
                           "batch would change train-mode BatchNorm statistics")
    clip = _f32(clip)
    B = clip.shape[0]
    order = frame_order(clip.shape[2], max_frames, frame_step)
    min_frames = max(int(min_frames), 1)
    dev = clip.device
    w = classifier.weight.detach().float().contiguous()
    bias = classifier.bias.detach().float().contiguous()
    nclass = w.shape[0]

    # every state array is a slice of one zeroed fp32 buffer (all-zero bits are 0 / 0.0 / False),
    # cut on the first step once the embedding width is known
    st = {}

    def cut(D):
        sizes = [B * D, B * nclass, B, B, B, 4, (B + 3) // 4 + 3]
        buf = K.fill_(torch.empty(sum(sizes), dtype=torch.float32, device=dev), 0.0)
        parts = torch.split(buf, sizes)
        st.update(sum=parts[0].view(B, D), logits=parts[1].view(B, nclass), conf=parts[2],
                     cnt=parts[3].view(torch.int32), used=parts[4].view(torch.int32),
                     count=parts[5].view(torch.int32)[:1], decided=parts[6].view(torch.uint8)[:B])

    active = None
    n = B
    for t in order:
        # first step: every sample, b = i; afterwards the compacted active list
        frames = K.gather_frames(clip, active, None, n, rows_per_b=1, t_fixed=t)
        out = backbone(frames)
        if not isinstance(out, (tuple, list)) or len(out) < 2:
            raise TypeError("backbone must return (feat, emb)")
        emb = out[1]
        if emb.dtype != torch.float32 or not emb.is_contiguous():
            emb = emb.float().contiguous()
        if active is None:
            cut(emb.shape[-1])
            active = torch.empty((B,), dtype=torch.int32, device=dev)
            K.active_compact(st["decided"], active, st["count"])          # 0 .. B-1
        K.exit_step(emb, active, n, w, bias, threshold, min_frames, False, st["sum"], st["cnt"], st["decided"],
                    st["logits"], st["used"], st["conf"])
        K.active_compact(st["decided"], active, st["count"])
        n = _read_count(st["count"])
        if n == 0:
            break
    if n > 0:   # the closing pass over the samples that never crossed the threshold
        K.exit_step(None, active, n, w, bias, threshold, min_frames, True, st["sum"], st["cnt"], st["decided"],
                    st["logits"], st["used"], st["conf"])
    return st["logits"], EarlyExitStats(used_frames=st["used"].long(), final_conf=st["conf"])

"""What the drivers (temporal_ssl, train_finetune, run_dynamic, run_privacy, run_federated, run_knn) share:
the config merge, start-up, the classifier they all build, the synthetic and split-file clip
sources, and the supervised pass and top-k evaluation of the two training drivers.  No driver
imports another; they meet here and in the library modules (the log line and the CSV writer are
in utils, TopCEFn and load_finetune_ckpt in finetune).
"""
import torch

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher
from .finetune import SoftCEFn, TopCEFn, VideoClassifier, load_finetune_ckpt
from .utils import set_seed


def _merge_section(defaults, vals, where):
    out = {k: _merge_section(v, None, k) if isinstance(v, dict) else v for k, v in defaults.items()}
    vals = vals or {}
    unknown = set(vals) - set(out)
    if unknown:
        raise ValueError(f"[ERROR] Unknown keys in {where}: {sorted(unknown)}")
    for key, val in vals.items():
        out[key] = _merge_section(defaults[key], val, f"{where}.{key}") if isinstance(defaults[key], dict) else val
    return out


def merge_config(defaults, cfg):
    """A copy of `defaults` (no dict shared with it) with the loaded file's values over it.  An
    unknown section or key raises; None for a section counts as empty; a section's nested dict
    (federated.non_iid) merges by the same rule."""
    out = {sec: _merge_section(vals, None, sec) for sec, vals in defaults.items()}
    for sec, vals in (cfg or {}).items():
        if sec not in out:
            raise ValueError(f"[ERROR] Unknown config section: {sec}")
        out[sec] = _merge_section(defaults[sec], vals, sec)
    return out


def start(name, seed):
    """Seeds, the check for a GPU and the kernel build that every driver's main begins with;
    returns the device."""
    set_seed(seed)
    if not torch.cuda.is_available():
        raise RuntimeError(f"[ERROR] {name} needs an MI355X: the HIP kernels have no CPU fallback")
    from .build import build
    build()
    return torch.device("cuda")


def build_classifier(cfg, ckpt, device, load=load_finetune_ckpt):
    """The VideoClassifier of `dataset.num_classes` / `model.embed_dim` / `dataset.image_size` on
    the device, after `load(model, ckpt)` (None: as constructed)."""
    model = VideoClassifier(int(cfg["dataset"]["num_classes"]), embed_dim=int(cfg["model"]["embed_dim"]),
                            img_size=int(cfg["dataset"]["image_size"]))
    if load is not None:
        load(model, ckpt)
    return model.to(device)


# ------------------------------------------------------------------ synthetic clips
def synthetic_pixels(g, n, T, S):
    """n uniform-noise clips [n, 3, T, S, S] whose frames differ in gain: two draws from `g`."""
    pixels = torch.rand(n, 3, T, S, S, generator=g)
    return (pixels - 0.45) / 0.226 * (0.3 + 1.4 * torch.rand(n, 1, T, 1, 1, generator=g))


class SyntheticBatches:
    """`steps` fixed batches on the device, drawn batch by batch: pixels, gain and, with
    `num_classes`, random labels (the batches are then (clip, label) pairs)."""

    def __init__(self, steps, batch_size, clip_len, image_size, device, seed=42, num_classes=None):
        g = torch.Generator().manual_seed(int(seed))
        self.batch_size = int(batch_size)
        self.batches = []
        for _ in range(max(1, int(steps))):
            clip = synthetic_pixels(g, self.batch_size, int(clip_len), int(image_size)).to(device)
            if num_classes is not None:
                clip = (clip, torch.randint(0, int(num_classes), (self.batch_size,), generator=g).to(device))
            self.batches.append(clip)

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


class SyntheticClips:
    """`n` labelled clips on the device, drawn at once (pixels, gain, labels) and named
    `synthetic/<index>` in split files, so the class-shard rule partitions them like real ones."""

    def __init__(self, cfg, n, seed, device):
        ds = cfg["dataset"]
        g = torch.Generator().manual_seed(int(seed))
        self.clips = synthetic_pixels(g, n, int(ds["clip_len"]), int(ds["image_size"])).to(device)
        self.labels = torch.randint(0, int(ds["num_classes"]), (n,), generator=g)

    def items(self):
        return [(f"synthetic/{i}", int(y)) for i, y in enumerate(self.labels.tolist())]

    def loader(self, items, batch_size, shuffle, seed):
        idx = torch.tensor([int(p.split("/")[1]) for p, _ in items], dtype=torch.long)
        return ClipSetLoader(self.clips, self.labels, idx, batch_size, shuffle, seed)


class ClipSetLoader:
    """(clip, label) batches of the rows `idx` of a clip set; shuffle implies drop_last
    (utils_fed.build_loader) and a fresh permutation per pass from one seeded generator."""

    def __init__(self, clips, labels, idx, batch_size, shuffle, seed):
        self.clips, self.labels, self.idx = clips, labels, idx
        self.batch_size, self.shuffle = int(batch_size), bool(shuffle)
        self.gen = torch.Generator().manual_seed(int(seed))

    def __len__(self):
        n = len(self.idx)
        return n // self.batch_size if self.shuffle else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        idx = self.idx[torch.randperm(len(self.idx), generator=self.gen)] if self.shuffle else self.idx
        labels = self.labels.to(self.clips.device)
        for b in range(len(self)):
            sel = idx[b * self.batch_size:(b + 1) * self.batch_size].to(self.clips.device)
            yield self.clips[sel], labels[sel]


# ------------------------------------------------------------------ split files
def split_file_loader(split, *, clip_len, stride, image_size, batch_size, num_workers, device, labelled=True,
                      bgr_swap=True, shuffle=False, drop_last=False, seed=None, pin_memory=False, augment=None):
    """Clips of a split file (lines of `<frame directory> [<label>]`): frames decoded on the host
    at their own size, resized to `image_size` and normalised on the device
    (mae_loader.ClipResizer).  `labelled` yields (clip, label) with the label from the second
    column, otherwise the clip alone.  `shuffle` draws its order from a generator seeded with
    `seed`, or from torch's global one when `seed` is None.  `augment` (a
    mae_loader.RandomResizedCropFlip) gives every clip of a batch a source window and a flip
    decision, drawn here in the main process after collation."""
    from .mae_loader import ClipResizer, LazyVideoMAEDataset, collate_raw
    data = LazyVideoMAEDataset(split, clip_len=int(clip_len), stride=int(stride), image_size=int(image_size))
    norm = ClipResizer(int(image_size), bgr_swap=bgr_swap, device=device)
    collate = collate_raw
    if labelled:
        frames = data
        with open(split) as f:
            labels = [int(line.split()[1]) for line in f if line.strip()]

        class Labelled(torch.utils.data.Dataset):
            def __len__(self):
                return len(frames)

            def __getitem__(self, i):
                return frames[i] + (labels[i],)

        def collate(batch):
            return collate_raw([b[:2] for b in batch]) + (torch.tensor([b[2] for b in batch]),)

        data = Labelled()
    gen = torch.Generator().manual_seed(int(seed)) if seed is not None else None
    loader = torch.utils.data.DataLoader(data, batch_size=int(batch_size), shuffle=bool(shuffle),
                                         drop_last=bool(drop_last), generator=gen, num_workers=int(num_workers),
                                         pin_memory=bool(pin_memory), collate_fn=collate)

    class Normalised:
        batch_size = loader.batch_size

        def __iter__(self):
            for packed, desc, *label in loader:
                if augment is not None:
                    desc = augment.windows(desc)
                clip = norm(packed, desc, int(clip_len))
                yield (clip, label[0].to(device)) if labelled else clip

    if not labelled:     # the labelled loader stays unsized: train_finetune's step line prints `/?` for it
        Normalised.__len__ = lambda self: len(loader)
    return Normalised()


# ------------------------------------------------------------------ supervised pass / evaluation
def train_pass(model, loader, opt, device, amp, sums, scaler=None, on_step=None, *, mixer=None, label_smoothing=0.0,
               on_mix=None):
    """One supervised pass over `loader`: bf16 autocast when `amp`, the cross-entropy through
    sm_logits_metrics (TopCEFn), backward and the optimizer step (through `scaler` when given).
    Adds (loss, loss * batch) of every step to the float64 device pair `sums`, so the caller
    reads back once, whenever it wants; returns (steps, samples).  `on_step(step, loss, logits,
    label)` runs after every optimizer step with detached device tensors.

    `mixer` (a mae_loader.ClipMixer) mixes every batch with its own flip before the forward pass
    and `label_smoothing` in (0, 1) smooths the target; with either the loss is the soft
    cross-entropy of sm_soft_ce (SoftCEFn) against the mixed, smoothed target, and `loss` is that
    value.  `on_step` still gets the batch's own labels; `on_mix(step, labels_b, lam)` runs right
    after the mix with the partner labels and the labels' weights (device tensors).  With both at
    their defaults the step is the one above, untouched."""
    soft = mixer is not None or float(label_smoothing) != 0.0
    steps = samples = 0
    for step, (clip, label) in enumerate(loader):
        clip = clip.to(device, non_blocking=True)
        label = label.to(device, non_blocking=True).long()
        opt.zero_grad(set_to_none=True)
        labels_b = lam = None
        if mixer is not None:
            clip, _, labels_b, lam = mixer(clip, label)
            if on_mix is not None:
                on_mix(step, labels_b, lam)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(amp)):
            logits = model(clip)
        if soft:
            loss = SoftCEFn.apply(logits, label, labels_b, lam, float(label_smoothing))
        else:
            loss = TopCEFn.apply(logits, label)
        if scaler is not None:
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        else:
            loss.backward()
            opt.step()
        bs = int(label.size(0))
        loss64 = loss.detach().double()
        sums[0] += loss64
        sums[1] += loss64 * bs
        steps, samples = steps + 1, samples + bs
        if on_step is not None:
            on_step(step, loss.detach(), logits.detach(), label)
    return steps, samples


@torch.no_grad()
def evaluate(model, loader, device, topk=(1, 5)):
    """-> {k: accuracy} for k = 1 and every k of `topk`; hits counted on the device by
    sm_logits_metrics (its tie rule: kernels.logits_metrics), each k capped at the class count,
    read back once per pass.  An empty loader gives zeros."""
    model.eval()
    ks = [k for k in dict.fromkeys(topk) if k != 1]
    hits = torch.zeros(1 + len(ks), dtype=torch.float64, device=device)
    total = 0
    for clip, label in loader:
        clip = clip.to(device, non_blocking=True)
        label = label.to(device, non_blocking=True).long()
        logits = model(clip).float().contiguous()
        nc = logits.shape[1]
        if ks:
            for i, k in enumerate(ks):
                m = K.logits_metrics(logits, label, min(k, nc))
                hits[1 + i] += m[0, 3]
            hits[0] += m[0, 2]
        else:
            hits[0] += K.logits_metrics(logits, label, 1)[0, 2]
        total += int(label.size(0))
    counts = hits.cpu().tolist()
    acc = {1: counts[0] / max(1, total)}
    for i, k in enumerate(ks):
        acc[k] = counts[1 + i] / max(1, total)
    return acc

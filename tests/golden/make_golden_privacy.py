"""Golden fixture for the feature-privacy evaluation (tests/golden/privacy.npz) by RUNNING the
reference's src/privacy/{feature_noise,metrics_privacy,attacker}.py on the CPU in the build
container.

The three reference modules need only torch, so they are loaded by file path (as
make_golden_dynamic.py loads its module).  This file also holds the deterministic input
generators, which the tests import (numpy's RandomState stream is stable across machines), and
asserts the conditions that make the fixture a sharp test when it writes it:

Metrics cases  logits [N, C] = 2 * noise with the label's logit raised by 0 / 1.5 / 4 in turn, so
  top-1 and top-5 both land between chance and 1.  Recorded: the reference's prediction_entropy and
  top1_accuracy (fp32, as the reference computes them), torch's top-min(5, C) hit count, and the
  mean cross-entropy and mean entropy in fp64.
  Condition: in every row the label's logit is >= 1e-3 relative away from the k-th largest of
  the other logits for k in {1, min(5, C)} (where the row has that many), so no hit hangs on
  rounding and torch.topk's unspecified tie order cannot matter.

Attacker cases z = class directions + noise through privacy.perturb_mirror (sigma 0.1, mask
  ratio 0.2), initial weights from the reference's FeatureAttacker under torch.manual_seed.
  Recorded: the initial weights (init_record), the final logits of the reference loop (run_privacy.py:310-325,
  10 epochs of Adam, lr 1e-3) in fp64, its top-1, and err32 = the largest deviation from those
  logits, relative to their largest magnitude, over three fp32 runs of the same loop: as is, with
  torch.set_num_threads(1), and with the D features of z and the matching columns of
  net.0.weight permuted consistently (the same problem in another summation order: err32 measures
  Adam's sensitivity to fp32 reordering).
  Condition: in every row the top-1 margin of the fp64 logits is >= 1e-3 of the largest logit
  magnitude; the first case's attacker accuracy is not saturated (< 0.9; the second has more
  features than samples and fits its training set in 10 steps).

Run:  python tests/golden/make_golden_privacy.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = "/root/reference/src/privacy"
REF_MODULES = ("feature_noise", "metrics_privacy", "attacker")
OUT = os.path.join(HERE, "privacy.npz")

# name -> (N, C, seed)
METRIC_CASES = {"n1_c3": (1, 3, 211), "n5_c7": (5, 7, 212), "n257_c101": (257, 101, 213), "n64_c1000": (64, 1000, 214)}
# name -> (N, D, C, data seed, torch init seed)
ATTACKER_CASES = {"n192_d64_c7": (192, 64, 7, 311, 1311), "n320_d576_c11": (320, 576, 11, 312, 1312)}
UNSATURATED = ("n192_d64_c7",)      # with D > N the second case fits its training set whatever the signal
ATTACKER_EPOCHS, ATTACKER_LR = 10, 1e-3
ATTACKER_SIGMA, ATTACKER_MASK, ATTACKER_PERTURB_SEED = 0.1, 0.2, 977
PER_PAIRS = ((0.5, 0.25), (0.0, 0.3), (1e-7, 1e-7), (0.6715, 0.1), (1.0, 1.0))


def reference_present():
    return all(os.path.isfile(os.path.join(REF_DIR, m + ".py")) for m in REF_MODULES)


def import_reference():
    """-> {name: module} of the three reference files."""
    mods = {}
    for name in REF_MODULES:
        spec = importlib.util.spec_from_file_location("ref_privacy_" + name, os.path.join(REF_DIR, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["ref_privacy_" + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def topk_of(C):
    return min(5, C)


def metric_inputs(name):
    """-> (logits fp32 [N, C], labels int64 [N]) numpy."""
    N, C, seed = METRIC_CASES[name]
    rng = np.random.RandomState(seed)
    logits = 2.0 * rng.standard_normal((N, C))
    labels = rng.randint(0, C, size=N)
    logits[np.arange(N), labels] += np.array([0.0, 1.5, 4.0])[np.arange(N) % 3]
    return logits.astype(np.float32), labels.astype(np.int64)


def metric_margin(logits, labels):
    """Smallest relative distance of a label's logit from the k-th largest other logit of its
    row, k in {1, min(5, C)}."""
    N, C = logits.shape
    l64 = logits.astype(np.float64)
    m = np.inf
    for i in range(N):
        ly = l64[i, labels[i]]
        others = np.sort(np.delete(l64[i], labels[i]))[::-1]
        for k in {1, topk_of(C)}:
            if k <= others.size:
                o = others[k - 1]
                m = min(m, abs(ly - o) / max(abs(ly), abs(o)))
    return m


def attacker_inputs(name):
    """-> (z_priv fp32 [N, D], y int64 [N]) numpy: class directions plus noise, perturbed by the
    host mirror of the project's draws."""
    from ssl_mae_amd.privacy import perturb_mirror
    N, D, C, seed, _ = ATTACKER_CASES[name]
    rng = np.random.RandomState(seed)
    dirs = rng.standard_normal((C, D))
    y = rng.randint(0, C, size=N)
    z = 0.35 * dirs[y] + rng.standard_normal((N, D))
    z_priv = perturb_mirror(z.astype(np.float32), ATTACKER_SIGMA, ATTACKER_MASK, ATTACKER_PERTURB_SEED)
    return z_priv.astype(np.float32), y.astype(np.int64)


def attacker_init(attacker_cls, name):
    """A fresh attacker of `attacker_cls` under the case's torch seed (the global RNG state is
    restored afterwards)."""
    N, D, C, _, tseed = ATTACKER_CASES[name]
    state = torch.get_rng_state()
    torch.manual_seed(tseed)
    att = attacker_cls(D, C)
    torch.set_rng_state(state)
    return att


def init_record(state_dict):
    """What the fixture keeps of an attacker's initial weights: every tensor in full, except
    that a matrix of more than 65536 entries is kept as every 8th row plus the fp64 sum of all
    its entries (the second case's [576, 576] matrix alone would exceed the size limit of a
    committed file)."""
    rec = {}
    for k, v in state_dict.items():
        a = v.detach().cpu().numpy()
        if a.size > 65536:
            rec[k + "/rows8"] = a[::8].copy()
            rec[k + "/sum64"] = np.float64(a.astype(np.float64).sum())
        else:
            rec[k] = a.copy()
    return rec


def reference_loop(attacker, z, y, epochs=ATTACKER_EPOCHS, lr=ATTACKER_LR):
    """run_privacy.py:310-325 on the CPU -> final logits."""
    opt = torch.optim.Adam(attacker.parameters(), lr=lr)
    ce = torch.nn.CrossEntropyLoss()
    attacker.train()
    for _ in range(epochs):
        opt.zero_grad()
        loss = ce(attacker(z.detach()), y)
        loss.backward()
        opt.step()
    attacker.eval()
    with torch.no_grad():
        return attacker(z)


def logit_margin(logits):
    """Smallest top-1 margin over the rows, relative to the largest logit magnitude."""
    s = np.sort(np.asarray(logits, dtype=np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min() / np.abs(s).max())


def _attacker_case(ref, name):
    import copy
    N, D, C, _, _ = ATTACKER_CASES[name]
    z_np, y_np = attacker_inputs(name)
    z, y = torch.from_numpy(z_np), torch.from_numpy(y_np)
    init = attacker_init(ref["attacker"].FeatureAttacker, name)
    rec = {f"attacker/{name}/init/{k}": v for k, v in init_record(init.state_dict()).items()}
    l64 = reference_loop(copy.deepcopy(init).double(), z.double(), y).numpy()
    runs = [reference_loop(copy.deepcopy(init), z, y).numpy()]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    runs.append(reference_loop(copy.deepcopy(init), z, y).numpy())
    torch.set_num_threads(threads)
    perm = np.random.RandomState(5).permutation(D)
    att_p = copy.deepcopy(init)
    with torch.no_grad():
        att_p.net[0].weight.copy_(init.net[0].weight[:, torch.from_numpy(perm)])
    runs.append(reference_loop(att_p, z[:, torch.from_numpy(perm)].contiguous(), y).numpy())
    scale = np.abs(l64).max()
    err32 = max(float(np.abs(r.astype(np.float64) - l64).max() / scale) for r in runs)
    top1 = ref["metrics_privacy"].top1_accuracy(torch.from_numpy(l64), y)
    margin = logit_margin(l64)
    assert margin >= 1e-3, (name, margin)
    assert name not in UNSATURATED or top1 < 0.9, (name, top1)
    rec[f"attacker/{name}/logits64"] = l64
    rec[f"attacker/{name}/err32"] = np.float64(err32)
    rec[f"attacker/{name}/top1"] = np.float64(top1)
    return rec


def build_fixture(ref):
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    rec = {}
    mp = ref["metrics_privacy"]
    for name in METRIC_CASES:
        logits_np, labels_np = metric_inputs(name)
        margin = metric_margin(logits_np, labels_np)
        assert margin >= 1e-3, (name, margin)
        logits, labels = torch.from_numpy(logits_np), torch.from_numpy(labels_np)
        k = topk_of(logits.shape[1])
        rec[f"metrics/{name}/entropy"] = np.float64(mp.prediction_entropy(logits))
        rec[f"metrics/{name}/top1"] = np.float64(mp.top1_accuracy(logits, labels))
        rec[f"metrics/{name}/topk_hits"] = np.int64((logits.topk(k, dim=1).indices == labels.view(-1, 1)).any(1).sum())
        l64 = logits.double()
        rec[f"metrics/{name}/loss64"] = np.float64(torch.nn.functional.cross_entropy(l64, labels).item())
        p = torch.softmax(l64, dim=1)
        rec[f"metrics/{name}/entropy64"] = np.float64((-(p * (p + 1e-12).log()).sum(1)).mean().item())
    for name in ATTACKER_CASES:
        rec.update(_attacker_case(ref, name))
    rec["per/pairs"] = np.array(PER_PAIRS, dtype=np.float64)
    rec["per/values"] = np.array([mp.privacy_exposure_rate(b, a) for b, a in PER_PAIRS], dtype=np.float64)
    torch.set_num_threads(threads)
    return rec


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "ssl-vit-video-analytics_amd"))
    rec = build_fixture(import_reference())
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    for name in METRIC_CASES:
        lg, lb = metric_inputs(name)
        print(name, "margin", metric_margin(lg, lb), "top1", rec[f"metrics/{name}/top1"], "topk hits",
              rec[f"metrics/{name}/topk_hits"], "entropy", rec[f"metrics/{name}/entropy"])
    for name in ATTACKER_CASES:
        print(name, "err32", rec[f"attacker/{name}/err32"], "margin", logit_margin(rec[f"attacker/{name}/logits64"]),
              "top1", rec[f"attacker/{name}/top1"], "max |logit|", np.abs(rec[f"attacker/{name}/logits64"]).max())


if __name__ == "__main__":
    main()

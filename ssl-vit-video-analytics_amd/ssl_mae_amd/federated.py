"""FedAvg aggregation on MI355X (reference: src/federated/fed_loop.py, comm_cost.py).

Same API as the reference module: `fedavg_aggregate(global_model, client_states,
client_weights)`, `run_fedavg(...)`, `estimate_comm_mb_per_round(state, n)`,
`model_size_bytes`, `bytes_to_mb`, with the same error conditions and the same
per-key rules (fed_loop.py:38-58):

  * floating-point entries: weighted average, accumulated in client order with
    separately rounded products and sums — one HIP launch over ONE flat fp32
    buffer per client (sm_fedavg_weighted_sum), bit-identical to the reference;
  * `num_batches_tracked`: elementwise max over clients (sm_fedavg_counters_max);
  * other integer entries: copied from the first client;
  * a key missing from any client: the global model's value.

Difference from the reference: it aggregates on the CPU "to avoid GPU memory
spikes" (fed_loop.py:22); here the model is ~80 MiB and HBM is 288 GB, so the
client states are staged into device buffers and the result stays on the global
model's device.  The flattening (one torch.cat per client) is data movement; the
arithmetic is the HIP kernel — there is no CPU arithmetic path.

DP-FedAvg (not in the reference): `FedCohort.aggregate_dp` clips every client's update over the
global model's parameters, averages the clipped updates and adds Gaussian noise in three launches
(sm_fedavg_dp_exchange); `dp_aggregate_reference` is the same in eager torch, `dp_aggregate_mirror`
the numpy statement the tests compare bits with, `dp_epsilon` the RDP accountant's estimate.
BatchNorm running statistics keep plain FedAvg and are outside the guarantee.

Compressed uploads (not in the reference): `FedCohort.aggregate_q8` quantises every client's update
over the global model's parameters to int8 with one fp32 scale per 256 elements and keeps the
quantisation error as the client's residual for its next update (error feedback), in one launch
(sm_fedavg_q8_exchange); `q8_aggregate_reference` is the same in eager torch, `q8_aggregate_mirror`
the numpy statement the tests compare bits with, `q8_upload_bytes` the wire size of one upload.

Multi-GPU (BASELINE config C5, 4 clients on 4 GPUs): `fedavg_allgather` makes
every rank one client.  Each rank's flat fp32 state is all-gathered over RCCL
(one collective per round, (N-1) x 80 MiB per rank over xGMI ~ 2 ms at N=4),
then every rank runs the same weighted-sum kernel in rank order, so every
replica holds exactly the reference's aggregate (an all-reduce SUM would be
cheaper but its ring order breaks bit-exactness, and the exchange happens once
per round).  Counters take a MAX all-reduce; other integer buffers come from
rank 0 (the "first client").
"""
import functools
import math
import random

import numpy as np
import torch
import torch.distributed as dist

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher
from .privacy import _COL_MUL, _ROW_MUL, _STREAMS, config_seed
from .utils import log_line


def _is_float_tensor(t):
    return torch.is_tensor(t) and torch.is_floating_point(t)


def _check(client_states, client_weights):
    # fed_loop.py:24-31
    if len(client_states) == 0:
        raise RuntimeError("[ERROR] No client states provided for aggregation.")
    if len(client_states) != len(client_weights):
        raise RuntimeError("[ERROR] client_states and client_weights length mismatch.")
    total_w = float(sum(client_weights))
    if total_w <= 0:
        raise RuntimeError("[ERROR] total client weight must be > 0.")
    return total_w


def _norm_weights(client_weights, total_w):
    # torch multiplies an fp32 tensor by the Python double w / total_w in fp32
    # (the scalar is rounded to fp32 first): the kernel takes those fp32 values.
    return [float(torch.tensor(float(w) / total_w, dtype=torch.float32)) for w in client_weights]


def _device_of(global_model, global_state):
    for v in global_state.values():
        if torch.is_tensor(v):
            return v.device
    return next(global_model.parameters()).device


def _flat(tensors, device, dtype):
    return torch.cat([t.detach().reshape(-1).to(device=device, dtype=dtype) for t in tensors])


def fedavg_aggregate(global_model, client_states, client_weights):
    """fed_loop.py:14-62.  Aggregates, loads the result into `global_model`
    (strict) and returns the new state dict (tensors on the model's device)."""
    total_w = _check(client_states, client_weights)
    global_state = global_model.state_dict()
    device = _device_of(global_model, global_state)
    if device.type != "cuda":
        raise RuntimeError("ssl_mae_amd FedAvg runs on the GPU only (move the global model with .to('cuda'))")

    new_state = {}
    float_keys, count_keys = [], []
    norm = _norm_weights(client_weights, total_w)
    for k, g in global_state.items():
        if any(k not in cs for cs in client_states):
            new_state[k] = g.detach().clone()
        elif _is_float_tensor(g):
            if g.dtype == torch.float32:
                float_keys.append(k)
            else:
                # fp16 / bf16 / fp64 entries (not produced by the MAE models): the
                # reference's per-key accumulation in the entry's own dtype
                # (fed_loop.py:46-49), as device tensor ops on the global model's GPU.
                acc = torch.zeros_like(g.detach())
                for cs, w in zip(client_states, client_weights):
                    acc += cs[k].detach().to(device=device, dtype=acc.dtype) * (float(w) / total_w)
                new_state[k] = acc
        elif "num_batches_tracked" in k:
            count_keys.append(k)
        else:
            new_state[k] = client_states[0][k].detach().to(device).clone()

    if float_keys:
        bufs = [_flat([cs[k] for k in float_keys], device, torch.float32) for cs in client_states]
        out = K.fedavg_weighted_sum(bufs, norm)
        _unflat(out, float_keys, global_state, new_state)
    if count_keys:
        bufs = [_flat([cs[k] for k in count_keys], device, torch.int64) for cs in client_states]
        out = K.fedavg_counters_max(bufs)
        _unflat(out, count_keys, global_state, new_state)

    new_state = {k: new_state[k] for k in global_state}   # reference key order
    global_model.load_state_dict(new_state, strict=True)
    return new_state


def _unflat(flat, keys, like, dst):
    off = 0
    for k in keys:
        n = like[k].numel()
        dst[k] = flat[off:off + n].view(like[k].shape)
        off += n


# ------------------------------------------------------------------ one-launch round exchange
def _state_slots(model):
    """[(state_dict key, the owning module's parameter or buffer dict, name)]: where the tensors
    state_dict() returns live.  Reading them from there skips building the OrderedDict and its
    detached aliases, and the module walk, on every exchange (a few hundred entries per
    VideoClassifier, looked up twice per round per model)."""
    out = []
    for prefix, mod in model.named_modules():
        pre = prefix + "." if prefix else ""
        out += [(pre + name, mod._parameters, name) for name, p in mod._parameters.items() if p is not None]
        out += [(pre + name, mod._buffers, name) for name, b in mod._buffers.items()
                if b is not None and name not in mod._non_persistent_buffers_set]
    return out


class FedCohort:
    """A global model and its client models on one GPU, exchanged in place: `broadcast` and
    `aggregate` each take one sm_fedavg_exchange launch over the fp32 entries (plus one
    sm_fedavg_exchange_counters launch over the num_batches_tracked entries) that reads the
    source models' tensors where they live and writes into the destination models' tensors,
    instead of run_fedavg's load_state_dict copies, torch.cat gathers and un-flatten.  The
    arithmetic and its order are fedavg_aggregate's, so the states agree bit for bit.

    Table model 0 is the global model, model c + 1 is client c.  The tables hold device
    addresses; parameter storage moves (the first forward re-homes the backbone's parameters
    into its flat buffer, `.to()` moves everything), so every exchange compares the
    participating tensors' addresses against the tables' host copy and rebuilds on a mismatch.
    It follows tensors that move, not sub-modules that are replaced: build a new cohort then."""

    def __init__(self, global_model, client_models):
        self.global_model = global_model
        self.client_models = list(client_models)
        self.models = [global_model] + self.client_models
        if not 1 <= len(self.client_models) <= K.FEDAVG_MAX_CLIENTS:
            raise RuntimeError(f"[ERROR] FedCohort takes 1..{K.FEDAVG_MAX_CLIENTS} client models, "
                               f"got {len(self.client_models)}")
        states = [m.state_dict() for m in self.models]
        ref = states[0]
        for i, st in enumerate(states):
            if list(st) != list(ref):
                raise RuntimeError(f"[ERROR] FedCohort: client {i - 1} state_dict keys differ from the global model's")
            for k, v in st.items():
                if v.device.type != "cuda" or v.device != next(iter(ref.values())).device:
                    raise RuntimeError("[ERROR] FedCohort needs every model on one cuda device "
                                       f"({k} of model {i} is on {v.device})")
                if v.shape != ref[k].shape or v.dtype != ref[k].dtype:
                    raise RuntimeError(f"[ERROR] FedCohort: {k} of client {i - 1} is {tuple(v.shape)} {v.dtype}, "
                                       f"the global model's is {tuple(ref[k].shape)} {ref[k].dtype}")
        self.float_keys, self.count_keys, self.other_keys = [], [], []
        for k, v in ref.items():
            if _is_float_tensor(v):
                if v.dtype != torch.float32:
                    raise RuntimeError(f"FedCohort exchanges fp32 state only; {k} is {v.dtype} "
                                       "(use fedavg_aggregate, which follows the reference for any float dtype)")
                self.float_keys.append(k)
            elif "num_batches_tracked" in k:
                if v.dtype != torch.int64:
                    raise RuntimeError(f"FedCohort: counter {k} is {v.dtype}, expected int64")
                self.count_keys.append(k)
            else:
                self.other_keys.append(k)
        self._slots = [_state_slots(m) for m in self.models]
        if any([k for k, _, _ in sl] != list(ref) for sl in self._slots):
            raise RuntimeError("[ERROR] FedCohort: a model's state_dict() is not its modules' parameters and "
                               "persistent buffers (state_dict hooks are not supported)")
        # the DP exchange clips the global model's parameters; float buffers (BatchNorm running
        # statistics) keep plain FedAvg
        params = {k for k, _ in global_model.named_parameters(remove_duplicate=False)}
        self._clip_modes = [1 if k in params else 0 for k in self.float_keys]
        self._float_chunks = sum(-(-ref[k].numel() // K.FEDAVG_CHUNK_ELEMS) for k in self.float_keys)
        self.rebuilds = 0
        self._resid = None        # aggregate_q8's residuals, one row per client
        self._build()

    def _entries(self, p):
        return {k: d[name] for k, d, name in self._slots[p]}

    def _build(self):
        ents = [self._entries(p) for p in range(len(self.models))]
        self._float_table, self._float_addr = K.fedavg_exchange_table(
            [[e[k].detach() for k in self.float_keys] for e in ents], torch.float32)
        self._count_table, self._count_addr = K.fedavg_exchange_table(
            [[e[k].detach() for k in self.count_keys] for e in ents], torch.int64)
        self._seg_clip = torch.tensor(self._clip_modes, dtype=torch.uint8).to(self._float_table.device)
        self.rebuilds += 1

    def _fresh(self, p, ents):
        nf, nc = len(self.float_keys), len(self.count_keys)
        return (all(ents[k].data_ptr() == a for k, a in zip(self.float_keys, self._float_addr[p * nf:(p + 1) * nf]))
                and all(ents[k].data_ptr() == a
                        for k, a in zip(self.count_keys, self._count_addr[p * nc:(p + 1) * nc])))

    @torch.no_grad()
    def exchange(self, src, weights, dst, copy_only=False, dp=None, q8=None):
        """Table-model indices: sources (in accumulation order), their normalised fp32 weights,
        destinations.  dp = (clip_norm, noise_std, seed): the fp32 entries go through
        sm_fedavg_dp_exchange against the global model (table model 0) instead, and the device
        `stats` tensor (the sources' update norms, then their clip scales) is returned.
        q8 = (codes, scales), either None: they go through sm_fedavg_q8_exchange with the cohort's
        residuals instead, and the device `part` tensor is returned."""
        ents = {p: self._entries(p) for p in dict.fromkeys(list(src) + list(dst) + ([0] if dp or q8 else []))}
        if not all(self._fresh(p, e) for p, e in ents.items()):
            self._build()
        stats = None
        if dp is not None:
            if not self.float_keys:
                raise RuntimeError("[ERROR] FedCohort: DP-FedAvg needs fp32 state entries")
            clip_norm, noise_std, seed = dp
            stats = K.fedavg_dp_exchange([ents[p][k].detach() for p in dst for k in self.float_keys], src, weights, 0,
                                         dst, self._float_table, self._float_chunks, self._seg_clip, clip_norm,
                                         noise_std, seed)
        elif q8 is not None:
            if not self.float_keys:
                raise RuntimeError("[ERROR] FedCohort: compressed FedAvg needs fp32 state entries")
            stats = K.fedavg_q8_exchange([ents[p][k].detach() for p in dst for k in self.float_keys], src, weights, 0,
                                         dst, self._float_table, self._float_chunks, self._seg_clip,
                                         self._residuals(), q8[0], q8[1])
        elif self.float_keys:
            K.fedavg_exchange([ents[p][k].detach() for p in dst for k in self.float_keys], src, weights, dst,
                              self._float_table, copy_only)
        if self.count_keys:
            K.fedavg_exchange_counters([ents[p][k].detach() for p in dst for k in self.count_keys], src, dst,
                                       self._count_table)
        for k in self.other_keys:        # the reference's "first client" rule (fed_loop.py:56-58)
            for p in dst:
                if p != src[0]:
                    ents[p][k].copy_(ents[src[0]][k])
        return stats

    def aggregate_dp(self, selected, client_weights, clip_norm, noise_multiplier, seed, also=()):
        """DP-FedAvg (McMahan et al. 2018) of the clients `selected` into the global model and the
        clients `also`: each client's update x_c - theta over the global model's parameters is
        clipped to the L2 bound `clip_norm`, the clipped updates are averaged onto theta with the
        normalised weights, and noise_multiplier * clip_norm * max(weight) -- the noise multiplier
        times one client's sensitivity of the weighted sum -- times a standard Gaussian of (seed,
        entry, element) is added, in three launches (sm_fedavg_dp_exchange).  Float buffers, the
        BatchNorm running statistics, keep plain FedAvg and are OUTSIDE the guarantee, as are the
        integer entries (num_batches_tracked: max; others: the first client's).
        -> the device tensor fp32 [2 * len(selected)]: the update norms, then the clip scales."""
        total_w = _check(selected, client_weights)
        norm = _norm_weights(client_weights, total_w)
        return self.exchange(self._clients(selected), norm, [0] + self._clients(also),
                             dp=(float(clip_norm), dp_noise_std(norm, clip_norm, noise_multiplier), int(seed)))

    def _residuals(self):
        device = self._float_table.device
        if self._resid is None:
            self._resid = torch.zeros((len(self.client_models), self._float_chunks * K.FEDAVG_CHUNK_ELEMS),
                                      dtype=torch.float32, device=device)
        elif self._resid.device != device:          # the cohort moved: the residuals follow it
            self._resid = self._resid.to(device)
        return self._resid

    def reset_residuals(self):
        """Zeroes every client's quantisation residual."""
        if self._resid is not None:
            self._resid.zero_()

    def aggregate_q8(self, selected, client_weights, also=(), payload=False):
        """Compressed FedAvg of the clients `selected` into the global model and the clients `also`:
        over the global model's parameters each client's update x_c - theta plus its residual is
        quantised to int8 with one fp32 scale per 256 elements, the dequantised updates are
        averaged onto theta with the normalised weights, and the quantisation error becomes the
        client's residual (one row per client, owned by the cohort, zero at first, indexed by
        chunk so it survives a table rebuild), in one launch (sm_fedavg_q8_exchange).  Float
        buffers, the BatchNorm running statistics, keep plain FedAvg in fp32, as do the integer
        entries' rules.
        -> the device tensor fp64 [len(selected), chunks, 2]: per chunk, max |update + residual| and
        the sum of squares of the new residual; with payload=True (part, (codes, scales)), what the
        clients upload: int8 [len(selected), chunks, 2048] and fp32 [len(selected), chunks, 8]."""
        total_w = _check(selected, client_weights)
        norm = _norm_weights(client_weights, total_w)
        q8 = (None, None)
        if payload:
            device, k, C = self._float_table.device, len(selected), self._float_chunks
            q8 = (torch.empty((k, C, K.FEDAVG_CHUNK_ELEMS), dtype=torch.int8, device=device),
                  torch.empty((k, C, K.FEDAVG_CHUNK_ELEMS // Q8_BLOCK), dtype=torch.float32, device=device))
        part = self.exchange(self._clients(selected), norm, [0] + self._clients(also), q8=q8)
        return (part, q8) if payload else part

    def aggregate(self, selected, client_weights, also=()):
        """FedAvg of the clients `selected` (in that order) into the global model and into the
        clients `also`, which may be among `selected`."""
        total_w = _check(selected, client_weights)
        norm = _norm_weights(client_weights, total_w)
        self.exchange(self._clients(selected), norm, [0] + self._clients(also))

    def broadcast(self, selected):
        """The global model's state, bit for bit, into the clients `selected`."""
        if len(selected):
            self.exchange([0], [1.0], self._clients(selected), copy_only=True)

    def _clients(self, ids):
        for c in ids:
            if not 0 <= int(c) < len(self.client_models):
                raise RuntimeError(f"[ERROR] FedCohort: no client {c} (clients 0..{len(self.client_models) - 1})")
        return [int(c) + 1 for c in ids]


# ------------------------------------------------------------------ DP-FedAvg (not in the reference)
def dp_round_seed(seed, r):
    """The noise seed of round r: privacy.config_seed(seed, r)."""
    return config_seed(seed, r)


def dp_noise_std(norm_weights, clip_norm, noise_multiplier):
    """noise_multiplier x the L2 sensitivity of the weighted sum to one client, max(weight) x
    clip_norm, formed on the host."""
    return float(noise_multiplier) * float(clip_norm) * max(float(w) for w in norm_weights)


def _dp_check(clip_norm, noise_multiplier):
    if not float(clip_norm) > 0.0:
        raise ValueError(f"[ERROR] DP-FedAvg: clip_norm must be > 0, got {clip_norm}")
    if not float(noise_multiplier) >= 0.0:
        raise ValueError(f"[ERROR] DP-FedAvg: noise_multiplier must be >= 0, got {noise_multiplier}")


def _fmix32_t(h):
    h = h & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def dp_noise(seed, seg, n, device):
    """The standard Gaussian of sm_privacy_perturb for row `seg`, columns 0..n-1, as fp64 torch
    ops on `device` (privacy.perturb_draws / gaussian_from_draws, one row)."""
    seed = int(seed) & ((1 << 64) - 1)
    s32 = (seed & 0xFFFFFFFF) ^ (seed >> 32)
    rb = _fmix32_t(torch.tensor((s32 + int(seg) * _ROW_MUL) & 0xFFFFFFFF, dtype=torch.int64, device=device))
    cm = (torch.arange(n, dtype=torch.int64, device=device) * _COL_MUL) & 0xFFFFFFFF
    h0, h1 = (_fmix32_t(_fmix32_t(rb + k) + cm) for k in _STREAMS[:2])
    u1 = ((h0 >> 8) + 1).double() * 2.0 ** -24
    u2 = (h1 >> 8).double() * 2.0 ** -24
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2.0 * math.pi * u2)


def dp_aggregate_reference(global_model, client_states, client_weights, clip_norm, noise_multiplier, seed):
    """DP-FedAvg in eager torch over state_dicts, the mathematics of FedCohort.aggregate_dp entry
    by entry: the global model's float parameters are clipped and noised (the noise is the same
    function of (seed, index among the float entries, element), added in fp64 and rounded once),
    float buffers take fedavg_aggregate's weighted sum, num_batches_tracked the max, other integer
    entries the first client's value.  Loads the result into `global_model` (strict) and returns
    (the new state dict, the fp32 [2 K] tensor of update norms then clip scales).  It serves
    `federated.exchange: reference` and is the baseline the fused exchange is timed against."""
    _dp_check(clip_norm, noise_multiplier)
    total_w = _check(client_states, client_weights)
    norm = _norm_weights(client_weights, total_w)
    noise_std = dp_noise_std(norm, clip_norm, noise_multiplier)
    global_state = global_model.state_dict()
    device = _device_of(global_model, global_state)
    params = {k for k, _ in global_model.named_parameters(remove_duplicate=False)}
    float_keys = [k for k, v in global_state.items() if _is_float_tensor(v)]
    for k in float_keys:
        if global_state[k].dtype != torch.float32 or any(k not in cs for cs in client_states):
            raise RuntimeError(f"[ERROR] DP-FedAvg needs {k} as fp32 in every client state")
    clipped = [k for k in float_keys if k in params]

    sq = torch.zeros(len(client_states), dtype=torch.float64, device=device)
    for c, cs in enumerate(client_states):
        for k in clipped:
            sq[c] += (cs[k].detach().to(device) - global_state[k].detach()).double().pow(2).sum()
    norms = sq.sqrt().float()
    scales = torch.clamp(float(clip_norm) / (norms + 1e-6), max=1.0)          # a NaN norm stays a NaN
    ws = torch.tensor(norm, dtype=torch.float32, device=device) * scales

    new_state = {}
    for k, g in global_state.items():
        if k in params and _is_float_tensor(g):
            theta = g.detach()
            acc = theta.clone()
            for c, cs in enumerate(client_states):
                acc += ws[c] * (cs[k].detach().to(device) - theta)
            if noise_std > 0.0:
                n = dp_noise(seed, float_keys.index(k), acc.numel(), device).view(acc.shape)
                acc = (acc.double() + noise_std * n).float()
            new_state[k] = acc
        elif _is_float_tensor(g):
            acc = torch.zeros_like(g.detach())
            for cs, w in zip(client_states, norm):
                acc += cs[k].detach().to(device) * w
            new_state[k] = acc
        elif any(k not in cs for cs in client_states):
            new_state[k] = g.detach().clone()
        elif "num_batches_tracked" in k:
            new_state[k] = torch.stack([cs[k].detach().to(device) for cs in client_states]).max(dim=0).values
        else:
            new_state[k] = client_states[0][k].detach().to(device).clone()
    global_model.load_state_dict(new_state, strict=True)
    return new_state, torch.cat([norms, scales])


def dp_aggregate_mirror(theta, sources, norm_weights, seg_clip, clip_norm, scales=None):
    """Host mirror (numpy) of sm_fedavg_dp_exchange without its noise.  theta: S fp32 arrays;
    sources: K lists of S fp32 arrays; norm_weights: the K normalised fp32 weights; seg_clip: S
    modes.  -> (the S result arrays, the K update norms in fp64).  The update repeats the kernel's
    pass 2 one operation at a time in np.float32 (add, subtract and multiply are correctly
    rounded), with the clip `scales` it is given (fp32 [K], e.g. the device's own); None forms them
    from the fp64 norms in fp32, min(1, clip_norm / (norm + 1e-6))."""
    f32 = np.float32
    theta = [np.asarray(t, dtype=f32) for t in theta]
    sources = [[np.asarray(x, dtype=f32) for x in src] for src in sources]
    norms = np.array([math.sqrt(sum(float(np.sum((x.astype(np.float64) - t.astype(np.float64)) ** 2))
                                    for x, t, m in zip(src, theta, seg_clip) if m)) for src in sources])
    if scales is None:
        with np.errstate(invalid="ignore"):
            scales = np.minimum(f32(1.0), f32(clip_norm) / (norms.astype(f32) + f32(1e-6)))
    scales = np.asarray(scales, dtype=f32)
    w = [f32(x) for x in norm_weights]
    ws = [w[c] * scales[c] for c in range(len(sources))]
    out = []
    for s, (t, m) in enumerate(zip(theta, seg_clip)):
        if m:
            acc = t.copy()
            for c, src in enumerate(sources):
                acc = acc + ws[c] * (src[s] - t)
        else:
            acc = np.zeros_like(t)
            for c, src in enumerate(sources):
                acc = acc + src[s] * w[c]
        out.append(acc)
    return out, norms


def dp_epsilon(noise_multiplier, sample_rate, rounds, delta, orders=range(2, 256)):
    """An ESTIMATE of the (epsilon, delta) budget spent by `rounds` rounds of DP-FedAvg: the
    Renyi-DP accountant of the sampled Gaussian mechanism at integer orders (Mironov, Talwar,
    Zhang 2019, "Renyi Differential Privacy of the Sampled Gaussian Mechanism", eq. for integer
    alpha), with z = noise_multiplier and q = sample_rate:

        A_alpha = sum_{k=0..alpha} C(alpha, k) (1 - q)^(alpha - k) q^k exp((k^2 - k) / (2 z^2))
        RDP_alpha = log(A_alpha) / (alpha - 1)
        epsilon = min_alpha (rounds * RDP_alpha + log(1 / delta) / (alpha - 1))

    in log space (lgamma, log-sum-exp).  inf for noise_multiplier == 0, 0 for rounds == 0.
    What it assumes, and the driver does not strictly provide: clients are sampled independently
    with probability q (Poisson sampling; the driver draws a fixed-size sample of
    q = selected / num_clients), one client changes the weighted sum by at most max(weight) x
    clip_norm (the weights come from the clients' sample counts, which are themselves data), and
    only the clipped parameters count: the BatchNorm running statistics and the integer entries
    are exchanged without clipping or noise and are outside the guarantee."""
    z, q, T, delta = float(noise_multiplier), float(sample_rate), int(rounds), float(delta)
    if z < 0.0 or not 0.0 <= q <= 1.0 or T < 0 or not 0.0 < delta < 1.0:
        raise ValueError("[ERROR] dp_epsilon: noise_multiplier >= 0, 0 <= sample_rate <= 1, rounds >= 0, "
                         "0 < delta < 1")
    if T == 0:
        return 0.0
    if z == 0.0:
        return math.inf
    best = math.inf
    for a in orders:
        a = int(a)
        terms = []
        for k in range(a + 1):
            if (q == 0.0 and k > 0) or (q == 1.0 and k < a):
                continue                                   # a zero-probability term
            t = math.lgamma(a + 1) - math.lgamma(k + 1) - math.lgamma(a - k + 1) + (k * k - k) / (2.0 * z * z)
            if a - k:
                t += (a - k) * math.log1p(-q)
            if k:
                t += k * math.log(q)
            terms.append(t)
        m = max(terms)
        log_a = m + math.log(sum(math.exp(t - m) for t in terms))
        best = min(best, T * log_a / (a - 1) + math.log(1.0 / delta) / (a - 1))
    return best


# ------------------------------------------------------------------ compressed uploads (not in the reference)
Q8_BLOCK = K.FEDAVG_Q8_BLOCK    # elements per scale
_Q8_LIVE = 1e-30          # a block whose largest |v| is below this (or not finite) is not quantised


def q8_upload_bytes(state, params):
    """The wire size of one client's compressed upload: an entry named in `params` (the quantised
    ones, the global model's parameters) takes one byte per element plus one fp32 scale per block
    of 256; every other entry goes as it is."""
    total = 0
    for k, v in state.items():
        if not torch.is_tensor(v):
            continue
        n = v.numel()
        total += n + 4 * (-(-n // Q8_BLOCK)) if k in params and _is_float_tensor(v) else n * v.element_size()
    return int(total)


def _q8_check(compress, dp):
    if compress is None:
        return
    if dp is not None:
        raise ValueError("[ERROR] FedAvg: dp and compress are exclusive (quantising a clipped, noised aggregate "
                         "changes the sensitivity analysis)")
    if compress.get("method") != "q8":
        raise ValueError(f"[ERROR] FedAvg: unknown compression method {compress.get('method')!r} (q8)")


def _q8_chunk_part(m_blocks, e_new, n):
    """The kernel's chunk statistics of one entry from its block maxima and new residual (flat,
    n elements), in the kernel's order: a lane's 8 squares in fp32, ascending; the 64 lanes of a
    wave by the xor butterfly and the 4 waves in order in fp64.  -> fp64 [chunks, 2]."""
    chunk = K.FEDAVG_CHUNK_ELEMS
    C = -(-n // chunk)
    per = chunk // Q8_BLOCK
    mx = torch.nn.functional.pad(m_blocks, (0, C * per - m_blocks.numel())).view(C, per).max(dim=1).values
    E = torch.nn.functional.pad(e_new, (0, C * chunk - n)).view(C, chunk // 1024, 256, 4)
    sq = E * E
    s = torch.zeros((C, 256), dtype=torch.float32, device=e_new.device)
    for u in range(chunk // 1024):
        for i in range(4):
            s = s + sq[:, u, :, i]
    sd = s.double().view(C, 4, 64)
    lanes = torch.arange(64, device=e_new.device)
    for o in (32, 16, 8, 4, 2, 1):
        sd = sd + sd[:, :, lanes ^ o]
    w = sd[:, :, 0]
    return torch.stack([mx.double(), ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]], dim=1)


def q8_aggregate_reference(global_model, client_states, client_weights, residuals):
    """Compressed FedAvg in eager torch over state_dicts, the mathematics of FedCohort.aggregate_q8
    entry by entry with one individually rounded torch op per kernel operation: the global model's
    float parameters are quantised in blocks of 256 (an entry is padded with zeros to whole blocks
    for the block maximum), float buffers take fedavg_aggregate's weighted sum, num_batches_tracked
    the max, other integer entries the first client's value.  `residuals` is a list of per-client
    dicts {key: fp32 tensor}, one per client state, updated in place (a missing key starts at
    zero).  Loads the result into `global_model` (strict) and returns (the new state dict, the fp64
    [K, chunks, 2] tensor FedCohort.aggregate_q8 returns).  It serves `federated.exchange:
    reference` and is the baseline the fused exchange is timed against."""
    total_w = _check(client_states, client_weights)
    if len(residuals) != len(client_states):
        raise RuntimeError("[ERROR] q8_aggregate_reference: one residual dict per client state")
    norm = _norm_weights(client_weights, total_w)
    global_state = global_model.state_dict()
    device = _device_of(global_model, global_state)
    params = {k for k, _ in global_model.named_parameters(remove_duplicate=False)}
    float_keys = [k for k, v in global_state.items() if _is_float_tensor(v)]
    for k in float_keys:
        if global_state[k].dtype != torch.float32 or any(k not in cs for cs in client_states):
            raise RuntimeError(f"[ERROR] compressed FedAvg needs {k} as fp32 in every client state")
    f32 = dict(dtype=torch.float32, device=device)
    live_min = torch.tensor(_Q8_LIVE, **f32)
    c127 = torch.tensor(127.0, dtype=torch.float64, device=device)      # a device tensor: a true division
    zero = torch.zeros((), **f32)
    chunk = K.FEDAVG_CHUNK_ELEMS

    new_state, parts = {}, [[] for _ in client_states]
    for k, g in global_state.items():
        if k in params and _is_float_tensor(g):
            theta = g.detach().reshape(-1)
            n = theta.numel()
            nb = -(-n // Q8_BLOCK)
            acc = theta.clone()
            for c, cs in enumerate(client_states):
                if k not in residuals[c]:
                    residuals[c][k] = torch.zeros_like(g.detach())
                e = residuals[c][k]
                v = (cs[k].detach().to(device).reshape(-1) - theta) + e.reshape(-1)
                vb = torch.nn.functional.pad(v, (0, nb * Q8_BLOCK - n)).view(nb, Q8_BLOCK)
                m = vb.abs().max(dim=1).values                         # a NaN in a block makes m NaN
                live = (m >= live_min) & torch.isfinite(m)
                # an fp32 quotient formed in fp64 and rounded once more is the correctly rounded fp32
                # quotient (53 >= 2 * 24 + 2 bits), whatever the backend's fp32 division does
                s = torch.where(live, (m.double() / c127).float(), zero)
                inv = torch.where(live, (c127 / m.double()).float(), zero)
                q = torch.where(live[:, None], torch.clamp(torch.round(vb * inv[:, None]), -127.0, 127.0), zero)
                d = q * s[:, None]
                e_new = (vb - d).reshape(-1)[:n]
                acc = acc + (d.reshape(-1)[:n] * norm[c])
                e.copy_(e_new.view(e.shape))
                parts[c].append(_q8_chunk_part(m, e_new, n))
            new_state[k] = acc.view(g.shape)
        elif _is_float_tensor(g):
            acc = torch.zeros_like(g.detach())
            for cs, w in zip(client_states, norm):
                acc += cs[k].detach().to(device) * w
            new_state[k] = acc
            for p in parts:
                p.append(torch.zeros((-(-g.numel() // chunk), 2), dtype=torch.float64, device=device))
        elif any(k not in cs for cs in client_states):
            new_state[k] = g.detach().clone()
        elif "num_batches_tracked" in k:
            new_state[k] = torch.stack([cs[k].detach().to(device) for cs in client_states]).max(dim=0).values
        else:
            new_state[k] = client_states[0][k].detach().to(device).clone()
    global_model.load_state_dict(new_state, strict=True)
    return new_state, torch.stack([torch.cat(p) for p in parts])


def q8_aggregate_mirror(theta, sources, residuals, norm_weights, seg_modes, with_part=False):
    """Host mirror (numpy) of sm_fedavg_q8_exchange, one operation at a time in np.float32 (add,
    subtract, multiply and divide are correctly rounded, np.rint rounds half to even).  theta: S
    fp32 arrays; sources and residuals: K lists of S fp32 arrays; norm_weights: the K normalised
    fp32 weights; seg_modes: S modes.  -> (the S result arrays, the K lists of S new residuals, the
    K lists of S int8 code arrays, the K lists of S fp32 scale arrays, one scale per block of 256);
    a mode-0 segment keeps its residual and has codes and scales of zeros.  with_part adds the
    kernel's `part`, fp64 [K, chunks, 2]."""
    f32 = np.float32
    chunk = K.FEDAVG_CHUNK_ELEMS
    theta = [np.asarray(t, dtype=f32) for t in theta]
    w = [f32(x) for x in norm_weights]
    out, new_res, codes, scales = [], [[] for _ in sources], [[] for _ in sources], [[] for _ in sources]
    parts = [[] for _ in sources]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for s, (t, mode) in enumerate(zip(theta, seg_modes)):
            n = t.size
            nb, C = -(-n // Q8_BLOCK), -(-n // chunk)
            if not mode:
                acc = np.zeros_like(t)
                for c, src in enumerate(sources):
                    acc = acc + np.asarray(src[s], dtype=f32) * w[c]
                    new_res[c].append(np.asarray(residuals[c][s], dtype=f32).copy())
                    codes[c].append(np.zeros(n, dtype=np.int8))
                    scales[c].append(np.zeros(nb, dtype=f32))
                    parts[c].append(np.zeros((C, 2)))
                out.append(acc)
                continue
            acc = t.copy()
            for c, src in enumerate(sources):
                v = (np.asarray(src[s], dtype=f32) - t) + np.asarray(residuals[c][s], dtype=f32)
                vb = np.zeros(nb * Q8_BLOCK, dtype=f32)
                vb[:n] = v
                vb = vb.reshape(nb, Q8_BLOCK)
                m = np.max(np.abs(vb), axis=1)                      # np.max propagates a NaN
                live = (m >= f32(_Q8_LIVE)) & np.isfinite(m)
                safe = np.where(live, m, f32(1.0))
                sc = np.where(live, safe / f32(127.0), f32(0.0)).astype(f32)
                inv = np.where(live, f32(127.0) / safe, f32(0.0)).astype(f32)
                q = np.where(live[:, None], np.clip(np.rint(vb * inv[:, None]), f32(-127.0), f32(127.0)), f32(0.0))
                q = q.astype(f32)
                d = q * sc[:, None]
                e_new = (vb - d).reshape(-1)
                acc = acc + w[c] * d.reshape(-1)[:n]
                new_res[c].append(e_new[:n].copy())
                codes[c].append(q.reshape(-1)[:n].astype(np.int8))
                scales[c].append(sc)
                if with_part:
                    parts[c].append(_q8_chunk_part_np(m, e_new, n))
            out.append(acc)
    if with_part:
        return out, new_res, codes, scales, np.stack([np.concatenate(p) for p in parts])
    return out, new_res, codes, scales


def _q8_chunk_part_np(m_blocks, e_new, n):
    """_q8_chunk_part in numpy: e_new is the entry's new residual padded with zeros to whole blocks."""
    f32 = np.float32
    chunk = K.FEDAVG_CHUNK_ELEMS
    C, per = -(-n // chunk), chunk // Q8_BLOCK
    mb = np.zeros(C * per, dtype=f32)
    mb[:m_blocks.size] = m_blocks
    E = np.zeros(C * chunk, dtype=f32)
    E[:e_new.size] = e_new
    E = E.reshape(C, chunk // 1024, 256, 4)
    sq = E * E
    s = np.zeros((C, 256), dtype=f32)
    for u in range(chunk // 1024):
        for i in range(4):
            s = s + sq[:, u, :, i]
    sd = s.astype(np.float64).reshape(C, 4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        sd = sd + sd[:, :, lanes ^ o]
    wv = sd[:, :, 0]
    return np.stack([np.max(mb.reshape(C, per), axis=1).astype(np.float64),
                     ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]], axis=1)


# ------------------------------------------------------------------ multi-GPU (C5)
def fedavg_allgather(model, weight, group=None, combine=None):
    """Every rank is one client: replace `model`'s state on every rank with the
    FedAvg of all ranks' states (rank order = client order), in place.

    `combine(bufs, norm_weights) -> flat` is the weighted sum; it defaults to the
    HIP kernel (device tensors required).  Returns the total client weight."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    state = model.state_dict()
    device = _device_of(model, state)
    float_keys = [k for k, v in state.items() if _is_float_tensor(v)]
    count_keys = [k for k, v in state.items() if not _is_float_tensor(v) and "num_batches_tracked" in k]
    other_keys = [k for k, v in state.items() if not _is_float_tensor(v) and "num_batches_tracked" not in k]
    for k in float_keys:
        if state[k].dtype != torch.float32:
            raise RuntimeError(f"fedavg_allgather aggregates fp32 state only; {k} is {state[k].dtype} "
                               "(use fedavg_aggregate, which follows the reference for any float dtype)")

    w = torch.tensor([float(weight)], dtype=torch.float64, device=device)
    ws = [torch.empty_like(w) for _ in range(world)]
    if world > 1:
        dist.all_gather(ws, w, group=group)
    else:
        ws = [w]
    client_weights = [float(x.item()) for x in ws]
    total_w = _check([None] * world, client_weights)
    norm = _norm_weights(client_weights, total_w)

    if combine is None:
        combine = K.fedavg_weighted_sum
    new_state = {}
    if float_keys:
        mine = _flat([state[k] for k in float_keys], device, torch.float32)
        if world > 1:
            bufs = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(bufs, mine, group=group)
        else:
            bufs = [mine]
        _unflat(combine(bufs, norm), float_keys, state, new_state)
    if count_keys:
        cnt = _flat([state[k] for k in count_keys], device, torch.int64)
        if world > 1:
            dist.all_reduce(cnt, op=dist.ReduceOp.MAX, group=group)
        _unflat(cnt, count_keys, state, new_state)
    if other_keys:
        oth = [state[k].detach().clone() for k in other_keys]
        if world > 1:
            src = dist.get_global_rank(group, 0) if group is not None else 0
            for t in oth:
                dist.broadcast(t, src=src, group=group)
        new_state.update(dict(zip(other_keys, oth)))
    model.load_state_dict({k: new_state[k] for k in state}, strict=True)
    return total_w


# ------------------------------------------------------------------ comm accounting (comm_cost.py)
def model_size_bytes(state_dict):
    """comm_cost.py:4-10."""
    return int(sum(v.numel() * v.element_size() for v in state_dict.values() if torch.is_tensor(v)))


def bytes_to_mb(x):
    """comm_cost.py:13-14."""
    return float(x) / (1024.0 * 1024.0)


def estimate_comm_mb_per_round(global_state, num_clients_participating):
    """comm_cost.py:17-26: broadcast + upload = 2 N model bytes."""
    size_b = model_size_bytes(global_state)
    return bytes_to_mb(int(2 * int(num_clients_participating) * size_b)), bytes_to_mb(size_b)


# ------------------------------------------------------------------ host loop (fed_loop.py:65-150)
def _round_record(log, r, selected, losses, global_state, top1, top5):
    """fed_loop.py:125-147: the round's record and its log line."""
    comm_total_mb, model_mb = estimate_comm_mb_per_round(global_state, num_clients_participating=len(selected))
    rec = {"round": r, "val_top1": float(top1), "val_top5": float(top5),
           "avg_local_loss": float(sum(losses) / max(1, len(losses))), "clients": int(len(selected)),
           "model_mb": float(model_mb), "comm_mb_round": float(comm_total_mb)}
    log(f"[INFO] Round {r} val_top1={top1:.4f} val_top5={top5:.4f} "
        f"avg_local_loss={rec['avg_local_loss']:.4f} comm_mb={comm_total_mb:.2f}")
    return rec


def _dp_round(log, r, rec, stats, selected, weights, dp):
    """One read-back of the round's DP statistics: a non-finite update norm raises, naming the
    client; the record gains dp_clipped / dp_norm_mean / dp_norm_max / dp_noise_std and the log one
    line."""
    vals = [float(x) for x in stats.tolist()]
    k = len(selected)
    norms, scales = vals[:k], vals[k:]
    for cid, n in zip(selected, norms):
        if not math.isfinite(n):
            raise RuntimeError(f"[ERROR] Round {r}: the update of client {cid} has a non-finite norm ({n})")
    rec["dp_clipped"] = int(sum(1 for s in scales if s < 1.0))
    rec["dp_norm_mean"] = float(sum(norms) / k)
    rec["dp_norm_max"] = float(max(norms))
    rec["dp_noise_std"] = dp_noise_std(_norm_weights(weights, float(sum(weights))), dp["clip_norm"],
                                       dp["noise_multiplier"])
    log(f"[INFO] Round {r} dp_clipped={rec['dp_clipped']}/{k} dp_norm_mean={rec['dp_norm_mean']:.4f} "
        f"dp_norm_max={rec['dp_norm_max']:.4f} dp_noise_std={rec['dp_noise_std']:.6f}")
    return rec


def _q8_round(log, r, rec, part, selected, global_model, global_state):
    """One read-back of the round's compression statistics (per client, the largest chunk maximum
    and the sum of the chunks' residual squares, reduced on `part`'s device): a non-finite maximum
    raises, naming the client; comm_mb_round becomes the fp32 broadcast plus the compressed upload,
    and the record gains upload_mb_fp32 / upload_mb_q8 / q8_absmax / q8_resid_norm and the log one
    line."""
    mx, sq = torch.stack([part[:, :, 0].amax(dim=1), part[:, :, 1].sum(dim=1)]).tolist()
    for cid, m in zip(selected, mx):
        if not math.isfinite(m):
            raise RuntimeError(f"[ERROR] Round {r}: the update of client {cid} has a non-finite element "
                               f"(largest |update + residual| = {m})")
    k = len(selected)
    params = {name for name, _ in global_model.named_parameters(remove_duplicate=False)}
    fp32_mb = bytes_to_mb(k * model_size_bytes(global_state))
    rec["upload_mb_fp32"] = float(fp32_mb)
    rec["upload_mb_q8"] = float(bytes_to_mb(k * q8_upload_bytes(global_state, params)))
    rec["comm_mb_round"] = float(fp32_mb + rec["upload_mb_q8"])
    rec["q8_absmax"] = float(max(mx))
    rec["q8_resid_norm"] = float(math.sqrt(sum(sq)))
    log(f"[INFO] Round {r} upload_mb_q8={rec['upload_mb_q8']:.2f} upload_mb_fp32={fp32_mb:.2f} "
        f"comm_mb={rec['comm_mb_round']:.2f} q8_absmax={rec['q8_absmax']:.6f} "
        f"q8_resid_norm={rec['q8_resid_norm']:.6f}")
    return rec


def run_fedavg(global_model, client_models, client_loaders, client_sizes, evaluate_fn, device, rounds=10,
               client_fraction=1.0, amp=True, log_f=None, dp=None, compress=None):
    """fed_loop.py:65-150: each round samples clients with random.Random(42),
    broadcasts the global weights, runs client_loaders[cid]["update_fn"](model),
    aggregates with fedavg_aggregate and evaluates.  Returns the per-round records.
    dp = {"clip_norm", "noise_multiplier", "seed"}: the round aggregates with
    dp_aggregate_reference under dp_round_seed(seed, r) instead, and its record and log carry the
    DP statistics (_dp_round).
    compress = {"method": "q8", "error_feedback": bool}: the round aggregates with
    q8_aggregate_reference over per-client residuals kept here (zeroed before every round when
    error_feedback is false), and its record carries the compressed upload (_q8_round).  dp and
    compress together raise ValueError."""
    _q8_check(compress, dp)
    if dp is not None:
        _dp_check(dp["clip_norm"], dp["noise_multiplier"])
    num_clients = len(client_models)
    rng = random.Random(42)
    records = []
    log = functools.partial(log_line, log_f)
    residuals = [{} for _ in range(num_clients)]

    for r in range(1, int(rounds) + 1):
        m = max(1, int(num_clients * float(client_fraction)))
        selected = rng.sample(list(range(num_clients)), m)
        log(f"[INFO] Round {r}/{rounds} selected_clients={selected}")
        g = {k: v.detach().clone() for k, v in global_model.state_dict().items()}
        for cid in selected:
            client_models[cid].load_state_dict(g, strict=True)
        states, weights, losses = [], [], []
        for cid in selected:
            losses.append(float(client_loaders[cid]["update_fn"](client_models[cid])))
            states.append({k: v.detach() for k, v in client_models[cid].state_dict().items()})
            weights.append(float(client_sizes[cid]))
        if compress is not None:
            if not compress.get("error_feedback", True):
                for res in residuals:
                    res.clear()
            new_state, part = q8_aggregate_reference(global_model, states, weights, [residuals[cid] for cid in selected])
        elif dp is None:
            new_state = fedavg_aggregate(global_model, states, weights)
        else:
            new_state, stats = dp_aggregate_reference(global_model, states, weights, dp["clip_norm"],
                                                      dp["noise_multiplier"], dp_round_seed(dp["seed"], r))
        top1, top5 = evaluate_fn(global_model)
        records.append(_round_record(log, r, selected, losses, new_state, top1, top5))
        if dp is not None:
            _dp_round(log, r, records[-1], stats, selected, weights, dp)
        if compress is not None:
            _q8_round(log, r, records[-1], part, selected, global_model, new_state)
    return records


def run_fedavg_fused(global_model, client_models, client_loaders, client_sizes, evaluate_fn, device, rounds=10,
                     client_fraction=1.0, amp=True, log_f=None, dp=None, compress=None):
    """run_fedavg with the round's exchange through a FedCohort: the same sampled clients, log
    lines and records, and bit-identical model states, with one broadcast launch and one
    aggregation launch per round in place of the state_dict copies.  With `dp` (as run_fedavg's)
    the aggregation is FedCohort.aggregate_dp, with `compress` FedCohort.aggregate_q8 over the
    cohort's residuals."""
    _q8_check(compress, dp)
    if dp is not None:
        _dp_check(dp["clip_norm"], dp["noise_multiplier"])
    num_clients = len(client_models)
    rng = random.Random(42)
    records = []
    cohort = FedCohort(global_model, client_models)
    log = functools.partial(log_line, log_f)

    for r in range(1, int(rounds) + 1):
        m = max(1, int(num_clients * float(client_fraction)))
        selected = rng.sample(list(range(num_clients)), m)
        log(f"[INFO] Round {r}/{rounds} selected_clients={selected}")
        cohort.broadcast(selected)
        losses = [float(client_loaders[cid]["update_fn"](client_models[cid])) for cid in selected]
        weights = [float(client_sizes[cid]) for cid in selected]
        if compress is not None:
            if not compress.get("error_feedback", True):
                cohort.reset_residuals()
            part = cohort.aggregate_q8(selected, weights)
        elif dp is None:
            cohort.aggregate(selected, weights)
        else:
            stats = cohort.aggregate_dp(selected, weights, dp["clip_norm"], dp["noise_multiplier"],
                                        dp_round_seed(dp["seed"], r))
        top1, top5 = evaluate_fn(global_model)
        records.append(_round_record(log, r, selected, losses, global_model.state_dict(), top1, top5))
        if dp is not None:
            _dp_round(log, r, records[-1], stats, selected, weights, dp)
        if compress is not None:
            _q8_round(log, r, records[-1], part, selected, global_model, global_model.state_dict())
    return records

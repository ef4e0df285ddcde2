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
import random

import torch
import torch.distributed as dist

from . import ops as K    # every kernel launch through the torch.ops.ssl_mae dispatcher
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
        self.rebuilds = 0
        self._build()

    def _entries(self, p):
        return {k: d[name] for k, d, name in self._slots[p]}

    def _build(self):
        ents = [self._entries(p) for p in range(len(self.models))]
        self._float_table, self._float_addr = K.fedavg_exchange_table(
            [[e[k].detach() for k in self.float_keys] for e in ents], torch.float32)
        self._count_table, self._count_addr = K.fedavg_exchange_table(
            [[e[k].detach() for k in self.count_keys] for e in ents], torch.int64)
        self.rebuilds += 1

    def _fresh(self, p, ents):
        nf, nc = len(self.float_keys), len(self.count_keys)
        return (all(ents[k].data_ptr() == a for k, a in zip(self.float_keys, self._float_addr[p * nf:(p + 1) * nf]))
                and all(ents[k].data_ptr() == a
                        for k, a in zip(self.count_keys, self._count_addr[p * nc:(p + 1) * nc])))

    @torch.no_grad()
    def exchange(self, src, weights, dst, copy_only=False):
        """Table-model indices: sources (in accumulation order), their normalised fp32 weights,
        destinations."""
        ents = {p: self._entries(p) for p in dict.fromkeys(list(src) + list(dst))}
        if not all(self._fresh(p, e) for p, e in ents.items()):
            self._build()
        if self.float_keys:
            K.fedavg_exchange([ents[p][k].detach() for p in dst for k in self.float_keys], src, weights, dst,
                              self._float_table, copy_only)
        if self.count_keys:
            K.fedavg_exchange_counters([ents[p][k].detach() for p in dst for k in self.count_keys], src, dst,
                                       self._count_table)
        for k in self.other_keys:        # the reference's "first client" rule (fed_loop.py:56-58)
            for p in dst:
                if p != src[0]:
                    ents[p][k].copy_(ents[src[0]][k])

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


def run_fedavg(global_model, client_models, client_loaders, client_sizes, evaluate_fn, device, rounds=10,
               client_fraction=1.0, amp=True, log_f=None):
    """fed_loop.py:65-150: each round samples clients with random.Random(42),
    broadcasts the global weights, runs client_loaders[cid]["update_fn"](model),
    aggregates with fedavg_aggregate and evaluates.  Returns the per-round records."""
    num_clients = len(client_models)
    rng = random.Random(42)
    records = []
    log = functools.partial(log_line, log_f)

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
        new_state = fedavg_aggregate(global_model, states, weights)
        top1, top5 = evaluate_fn(global_model)
        records.append(_round_record(log, r, selected, losses, new_state, top1, top5))
    return records


def run_fedavg_fused(global_model, client_models, client_loaders, client_sizes, evaluate_fn, device, rounds=10,
                     client_fraction=1.0, amp=True, log_f=None):
    """run_fedavg with the round's exchange through a FedCohort: the same sampled clients, log
    lines and records, and bit-identical model states, with one broadcast launch and one
    aggregation launch per round in place of the state_dict copies."""
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
        cohort.aggregate(selected, [float(client_sizes[cid]) for cid in selected])
        top1, top5 = evaluate_fn(global_model)
        records.append(_round_record(log, r, selected, losses, global_model.state_dict(), top1, top5))
    return records

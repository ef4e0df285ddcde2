// FedAvg aggregation on the GPU (reference: src/federated/fed_loop.py:14-62).
//
// The reference averages client state_dicts on the CPU, key by key:
//   acc = zeros; for (state, w) in clients: acc += state[k].to(f32) * (w / total_w)
// (fed_loop.py:46-49) and takes the max over clients for num_batches_tracked
// (:52-55).  Here every floating-point entry of a state_dict lives in one flat fp32
// buffer per client (same key order), so one launch aggregates the whole model:
// each element is read once from each client and written once — (K + 1) * 4 B per
// parameter, HBM-bound.  The accumulation order and rounding are the reference's:
// acc starts at +0, then for each client in list order acc = acc + (x * w) with
// the product and the sum rounded separately (no FMA contraction), w the fp32
// rounding of w_i / total_w.  The result is therefore bit-identical to
// fedavg_aggregate's.
#include "common.h"
#include "fed_table.h"
#include "sm_api.h"

using namespace fedtab;   // the table view, the launch helpers and the argument check, shared with fed_dp.hip and fed_q8.hip

// The reference rounds x * w and acc + (x * w) separately: this file is compiled
// with -ffp-contract=off (build.py FILE_FLAGS) so no FMA is formed.

namespace {

struct ClientPtrs {
  const float* p[kMaxClients];
  float w[kMaxClients];
};

struct ClientCounters {
  const int64_t* p[kMaxClients];
};

// 16 B per lane per client; grid-stride over float4 groups.  KC > 0: client count
// known at compile time, so all KC loads of an element group are issued before the
// first multiply-add (KC x 16 B in flight per lane); KC == 0: runtime count.
template <int KC>
__global__ void __launch_bounds__(256) fedavg_sum4_kernel(ClientPtrs c, int k, int64_t n4, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KC > 0) {
      f32x4 x[KC];
#pragma unroll
      for (int j = 0; j < KC; ++j) x[j] = __builtin_nontemporal_load((const f32x4*)c.p[j] + i);
#pragma unroll
      for (int j = 0; j < KC; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(x[j][e], c.w[j]));
    } else {
      for (int j = 0; j < k; ++j) {
        const f32x4 x = __builtin_nontemporal_load((const f32x4*)c.p[j] + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(x[e], c.w[j]));
      }
    }
    __builtin_nontemporal_store(acc, (f32x4*)out + i);
  }
}

__global__ void fedavg_sum1_kernel(ClientPtrs c, int k, int64_t begin, int64_t n, float* __restrict__ out) {
  const int64_t i = begin + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int j = 0; j < k; ++j) acc = __fadd_rn(acc, __fmul_rn(c.p[j][i], c.w[j]));
  out[i] = acc;
}

__global__ void counters_max_kernel(ClientCounters c, int k, int64_t n, int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t m = c.p[0][i];
  for (int j = 1; j < k; ++j) m = c.p[j][i] > m ? c.p[j][i] : m;
  out[i] = m;
}

// ---- multi-tensor exchange: one launch over a cohort's state entries where they live.
// The table (sm_api.h "FedAvg exchange table") maps every chunk of kChunk elements to a
// segment (one state entry) and an offset in it; a block takes whole chunks, grid-stride.
// Sources and destinations may alias (in-place aggregation): a lane loads its elements
// from every source before its first store, lanes own disjoint elements, and no pointer
// here is __restrict__.
// The kernel keeps a lane layout of its own (whole 16-byte groups tid, tid + 256 of an aligned chunk, a
// stride-256 scalar tail, stride-256 elements of a misaligned one) instead of fed_table.h's load_lane /
// for_sources / store_dsts: load_group's 16-byte and element-wise forms write the same registers, the
// wait that orders them sits in front of every 16-byte load, and the copy-bound launches here ran 1.28x
// (4 sources) and 1.29x (8 sources) as long on them (profiles/fed_cleanup_isa_and_ab.txt).
constexpr int kVecPerLane = kChunk / (256 * 4);   // float4 groups per lane per source
static_assert(kChunk % 1024 == 0, "a chunk is a whole number of 256-lane float4 rows");

// KC > 0: source count known at compile time (all KC * kVecPerLane loads of a lane are issued
// before the first multiply-add); KC == 0: runtime count.  COPY: one source, stored as loaded.
template <int KC, bool COPY>
SM_DEV float exchange_one(const ExchangeArgs& a, const TableView& t, int64_t seg, int k, int64_t i) {
  if constexpr (COPY) {
    return ((const float*)t.addr[a.src[0] * t.S + seg])[i];
  } else {
    float acc = 0.f;
    if constexpr (KC > 0) {
      float x[KC];
#pragma unroll
      for (int j = 0; j < KC; ++j) x[j] = ((const float*)t.addr[a.src[j] * t.S + seg])[i];
#pragma unroll
      for (int j = 0; j < KC; ++j) acc = __fadd_rn(acc, __fmul_rn(x[j], a.w[j]));
    } else {
      for (int j = 0; j < k; ++j)
        acc = __fadd_rn(acc, __fmul_rn(((const float*)t.addr[a.src[j] * t.S + seg])[i], a.w[j]));
    }
    return acc;
  }
}

template <int KC, bool COPY>
__global__ void __launch_bounds__(256) fedavg_exchange_kernel(ExchangeArgs a, const unsigned char* tab) {
  const TableView t = table_view(tab);
  const int k = KC > 0 ? KC : a.num_src;
  const int tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < t.C; c += gridDim.x) {
    int64_t seg, off, n;
    if (!chunk_range(t, c, seg, off, n)) continue;
    uint64_t bits = (uint64_t)off * 4;   // vector path: this chunk 16-byte aligned in every model of the launch
    for (int j = 0; j < k; ++j) bits |= t.addr[a.src[j] * t.S + seg];
    for (int d = 0; d < a.num_dst; ++d) bits |= t.addr[a.dst[d] * t.S + seg];
    if ((bits & 15u) != 0) {
      for (int64_t i = off + tid; i < off + n; i += 256) {
        const float v = exchange_one<KC, COPY>(a, t, seg, k, i);
        for (int d = 0; d < a.num_dst; ++d) ((float*)t.addr[a.dst[d] * t.S + seg])[i] = v;
      }
      continue;
    }
    const int64_t n4 = n / 4;
    f32x4 acc[kVecPerLane] = {};
    if constexpr (COPY) {
      const f32x4* p = (const f32x4*)((const float*)t.addr[a.src[0] * t.S + seg] + off);
#pragma unroll
      for (int u = 0; u < kVecPerLane; ++u)
        if (tid + 256 * u < n4) acc[u] = __builtin_nontemporal_load(p + tid + 256 * u);
    } else if constexpr (KC > 0) {
      f32x4 x[KC][kVecPerLane];
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        const f32x4* p = (const f32x4*)((const float*)t.addr[a.src[j] * t.S + seg] + off);
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u)
          x[j][u] = tid + 256 * u < n4 ? __builtin_nontemporal_load(p + tid + 256 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < kVecPerLane; ++u) {
        acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KC; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[u][e] = __fadd_rn(acc[u][e], __fmul_rn(x[j][u][e], a.w[j]));
      }
    } else {
#pragma unroll
      for (int u = 0; u < kVecPerLane; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < k; ++j) {
        const f32x4* p = (const f32x4*)((const float*)t.addr[a.src[j] * t.S + seg] + off);
        f32x4 x[kVecPerLane];
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u)
          x[u] = tid + 256 * u < n4 ? __builtin_nontemporal_load(p + tid + 256 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < kVecPerLane; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[u][e] = __fadd_rn(acc[u][e], __fmul_rn(x[u][e], a.w[j]));
      }
    }
    // the segment's scalar tail (n % 4 elements, last chunk only): loaded before any store too
    const int64_t ti = off + n4 * 4 + tid;
    const bool has_tail = ti < off + n;
    float tail = 0.f;
    if (has_tail) tail = exchange_one<KC, COPY>(a, t, seg, k, ti);
    for (int d = 0; d < a.num_dst; ++d) {
      float* q = (float*)t.addr[a.dst[d] * t.S + seg];
#pragma unroll
      for (int u = 0; u < kVecPerLane; ++u)
        if (tid + 256 * u < n4) __builtin_nontemporal_store(acc[u], (f32x4*)(q + off) + tid + 256 * u);
      if (has_tail) q[ti] = tail;
    }
  }
}

__global__ void __launch_bounds__(256) fedavg_exchange_counters_kernel(ExchangeArgs a, const unsigned char* tab) {
  const TableView t = table_view(tab);
  for (int64_t c = blockIdx.x; c < t.C; c += gridDim.x) {
    int64_t seg, off, n;
    if (!chunk_range(t, c, seg, off, n)) continue;
    for (int64_t i = off + threadIdx.x; i < off + n; i += 256) {
      int64_t m = ((const int64_t*)t.addr[a.src[0] * t.S + seg])[i];
      for (int j = 1; j < a.num_src; ++j) {
        const int64_t v = ((const int64_t*)t.addr[a.src[j] * t.S + seg])[i];
        m = v > m ? v : m;
      }
      for (int d = 0; d < a.num_dst; ++d) ((int64_t*)t.addr[a.dst[d] * t.S + seg])[i] = m;
    }
  }
}

}  // namespace

extern "C" int sm_fedavg_exchange(int num_src, const int32_t* src_models, const float* weights, int num_dst,
                                  const int32_t* dst_models, const void* table, int64_t table_bytes, int copy_only,
                                  hipStream_t st) {
  if (copy_only ? num_src != 1 : !weights) return -2;
  ExchangeArgs a;
  SmFedTableHeader h{};
  const int rc = exchange_args(num_src, src_models, weights, num_dst, dst_models, table, table_bytes, 4, st, a, h);
  const int64_t chunks = h.num_chunks;
  if (rc != 0 || chunks == 0) return rc;
  const dim3 g = exchange_grid(chunks), b(256);
  const unsigned char* tab = (const unsigned char*)table;
  if (copy_only) hipLaunchKernelGGL((fedavg_exchange_kernel<1, true>), g, b, 0, st, a, tab);
  else FED_DISPATCH_KC(num_src, hipLaunchKernelGGL((fedavg_exchange_kernel<KC, false>), g, b, 0, st, a, tab));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_fedavg_exchange_counters(int num_src, const int32_t* src_models, int num_dst,
                                           const int32_t* dst_models, const void* table, int64_t table_bytes,
                                           hipStream_t st) {
  ExchangeArgs a;
  SmFedTableHeader h{};
  const int rc = exchange_args(num_src, src_models, nullptr, num_dst, dst_models, table, table_bytes, 8, st, a, h);
  const int64_t chunks = h.num_chunks;
  if (rc != 0 || chunks == 0) return rc;
  hipLaunchKernelGGL(fedavg_exchange_counters_kernel, exchange_grid(chunks), dim3(256), 0, st, a,
                     (const unsigned char*)table);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_fedavg_weighted_sum(int num_clients, const float* const* client_bufs, const float* weights,
                                      int64_t n, float* out, hipStream_t st) {
  if (num_clients < 1 || num_clients > kMaxClients || n < 0) return -2;
  if (n == 0) return 0;
  if (!client_bufs || !weights || !out) return -2;
  ClientPtrs c{};
  bool vec = aligned16(out);
  for (int j = 0; j < num_clients; ++j) {
    if (!client_bufs[j]) return -2;
    c.p[j] = client_bufs[j];
    c.w[j] = weights[j];
    vec = vec && aligned16(client_bufs[j]);
  }
  int64_t done = 0;
  if (vec && n >= 4) {
    const int64_t n4 = n / 4;
    const dim3 g = exchange_grid((n4 + 255) / 256), b(256);   // grid-stride over the float4 groups beyond the cap
    FED_DISPATCH_KC(num_clients, hipLaunchKernelGGL(fedavg_sum4_kernel<KC>, g, b, 0, st, c, num_clients, n4, out));
    SM_CHECK_LAUNCH();
    done = n4 * 4;
  }
  if (done < n) {
    const int64_t rest = n - done;
    hipLaunchKernelGGL(fedavg_sum1_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, st, c, num_clients,
                       done, n, out);
    SM_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int sm_fedavg_counters_max(int num_clients, const int64_t* const* client_counters, int64_t n,
                                      int64_t* out, hipStream_t st) {
  if (num_clients < 1 || num_clients > kMaxClients || n < 0) return -2;
  if (n == 0) return 0;
  if (!client_counters || !out) return -2;
  ClientCounters c{};
  for (int j = 0; j < num_clients; ++j) {
    if (!client_counters[j]) return -2;
    c.p[j] = client_counters[j];
  }
  hipLaunchKernelGGL(counters_max_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c, num_clients, n, out);
  SM_CHECK_LAUNCH();
  return 0;
}

// The FedAvg exchange table (include/sm_api.h "FedAvg exchange table") as the kernels of
// csrc/fed.hip, csrc/fed_dp.hip and csrc/fed_q8.hip see it, the pieces of a chunk's exchange that they
// share (a lane's loads and stores, the alignment test, the source loop; the launch grid and the
// dispatch over the source count), and the host-side check of a launch's arguments.
#pragma once
#include "common.h"
#include "sm_api.h"

namespace fedtab {

constexpr int kMaxClients = SM_FEDAVG_MAX_CLIENTS;
constexpr int kChunk = SM_FEDAVG_CHUNK_ELEMS;

struct ExchangeArgs {
  int32_t src[kMaxClients];
  float w[kMaxClients];
  int32_t dst[kMaxClients + 1];
  int num_src, num_dst;
};

struct TableView {
  int64_t S, C;
  const uint64_t* addr;      // [P][S]
  const int64_t* seg_len;    // [S]
  const int64_t* chunk_off;  // [C]
  const int32_t* chunk_seg;  // [C]
};

// The view from the header's counts (the host has read them back: exchange_args).
SM_DEV TableView table_view(const unsigned char* tab, int64_t P, int64_t S, int64_t C) {
  TableView t;
  t.S = S;
  t.C = C;
  t.addr = (const uint64_t*)(tab + sizeof(SmFedTableHeader));
  t.seg_len = (const int64_t*)(t.addr + P * t.S);
  t.chunk_off = t.seg_len + t.S;
  t.chunk_seg = (const int32_t*)(t.chunk_off + t.C);
  return t;
}

// The same from the header in device memory.
SM_DEV TableView table_view(const unsigned char* tab) {
  const SmFedTableHeader* h = (const SmFedTableHeader*)tab;
  return table_view(tab, h->num_models, h->num_segments, h->num_chunks);
}

// Elements [off, off + n) of segment `seg`: false when the chunk entry points outside it.
SM_DEV bool chunk_range(const TableView& t, int64_t c, int64_t& seg, int64_t& off, int64_t& n) {
  seg = t.chunk_seg[c];
  off = t.chunk_off[c];
  if (seg < 0 || seg >= t.S || off < 0) return false;
  const int64_t len = t.seg_len[seg];
  if (off >= len) return false;
  n = len - off < kChunk ? len - off : kChunk;
  return true;
}

// ---- a lane's share of a chunk in csrc/fed_dp.hip and csrc/fed_q8.hip: the 4-element groups tid and
// tid + 256 of the chunk, in the 16-byte form and in the element-wise form alike.  (fedavg_exchange_kernel
// in csrc/fed.hip keeps a layout of its own: see there.)
constexpr int kGroups = kChunk / (256 * 4);   // 4-element groups per lane per model
static_assert(kChunk % 1024 == 0, "a chunk is a whole number of 256-lane float4 rows");

// Elements [e0, e0 + 4) of a chunk of n elements at p: 16 bytes when the chunk is aligned (vec)
// and the group is whole, else element by element; slots past n read as +0.
SM_DEV f32x4 load_group(const float* p, int e0, int n, bool vec) {
  if (vec && e0 + 4 <= n) return __builtin_nontemporal_load((const f32x4*)(p + e0));
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e0 + e < n) v[e] = p[e0 + e];
  return v;
}

SM_DEV void store_group(float* q, int e0, int n, bool vec, f32x4 v) {
  if (vec && e0 + 4 <= n) {
    __builtin_nontemporal_store(v, (f32x4*)(q + e0));
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e0 + e < n) q[e0 + e] = v[e];
}

SM_DEV const float* seg_ptr(const TableView& t, int model, int64_t seg, int64_t off) {
  return (const float*)t.addr[model * t.S + seg] + off;
}

// acc += x w: sm_fedavg_exchange's operations.
SM_DEV void add_plain(f32x4* acc, const f32x4* x, float w) {
#pragma unroll
  for (int u = 0; u < kGroups; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[u][e] = __fadd_rn(acc[u][e], __fmul_rn(x[u][e], w));
}

// A lane's kGroups groups of a chunk of n elements at p.
SM_DEV void load_lane(const float* p, int n, bool vec, f32x4* x) {
#pragma unroll
  for (int u = 0; u < kGroups; ++u) x[u] = load_group(p, 4 * ((int)threadIdx.x + 256 * u), n, vec);
}

SM_DEV void store_lane(float* q, int n, bool vec, const f32x4* v) {
#pragma unroll
  for (int u = 0; u < kGroups; ++u) store_group(q, 4 * ((int)threadIdx.x + 256 * u), n, vec, v[u]);
}

// Segment `seg` 16-byte aligned in the k sources, with_dst in the destinations too, and at `more`
// (the address of a model that is neither, such as theta's; 0: none).
SM_DEV bool seg_aligned(const TableView& t, const ExchangeArgs& a, int k, int64_t seg, bool with_dst,
                        uint64_t more = 0) {
  uint64_t bits = more;
  for (int j = 0; j < k; ++j) bits |= t.addr[a.src[j] * t.S + seg];
  if (with_dst)
    for (int d = 0; d < a.num_dst; ++d) bits |= t.addr[a.dst[d] * t.S + seg];
  return (bits & 15u) == 0;
}

// f(j, x) for every source j in source order, x the lane's groups of source j.  KC > 0: source count
// known at compile time, every load of the lane is issued before the first f; KC == 0: runtime count k.
// Followed by store_dsts this keeps in-place exchange sound: a lane has loaded its elements from
// every source before its first store, and lanes own disjoint elements.
template <int KC, class F>
SM_DEV void for_sources(const TableView& t, const ExchangeArgs& a, int k, int64_t seg, int64_t off, int n, bool vec,
                        F&& f) {
  if constexpr (KC > 0) {
    // every source's address first: an address read between two sources' loads would wait for the
    // loads before it
    const float* p[KC];
    f32x4 x[KC][kGroups];
#pragma unroll
    for (int j = 0; j < KC; ++j) p[j] = seg_ptr(t, a.src[j], seg, off);
#pragma unroll
    for (int j = 0; j < KC; ++j) load_lane(p[j], n, vec, x[j]);
#pragma unroll
    for (int j = 0; j < KC; ++j) f(j, x[j]);
  } else {
    for (int j = 0; j < k; ++j) {
      f32x4 x[kGroups];
      load_lane(seg_ptr(t, a.src[j], seg, off), n, vec, x);
      f(j, x);
    }
  }
}

// acc into every destination of the launch.
SM_DEV void store_dsts(const TableView& t, const ExchangeArgs& a, int64_t seg, int64_t off, int n, bool vec,
                       const f32x4* acc) {
  for (int d = 0; d < a.num_dst; ++d) store_lane((float*)t.addr[a.dst[d] * t.S + seg] + off, n, vec, acc);
}

// One block per chunk (per 256 float4 groups in the weighted sum) up to 8 resident 256-lane blocks
// per CU on 256 CUs, grid-stride beyond that.
inline dim3 exchange_grid(int64_t blocks) { return dim3((unsigned)(blocks < 2048 ? blocks : 2048)); }

// Run the statement(s) with constexpr int KC = NUM_SRC where the kernels are instantiated for that
// count, else 0 (their runtime-count form).
#define FED_DISPATCH_KC(NUM_SRC, ...)                              \
  do {                                                             \
    switch (NUM_SRC) {                                             \
      case 1: { constexpr int KC = 1; __VA_ARGS__; } break;        \
      case 2: { constexpr int KC = 2; __VA_ARGS__; } break;        \
      case 3: { constexpr int KC = 3; __VA_ARGS__; } break;        \
      case 4: { constexpr int KC = 4; __VA_ARGS__; } break;        \
      case 8: { constexpr int KC = 8; __VA_ARGS__; } break;        \
      default: { constexpr int KC = 0; __VA_ARGS__; } break;       \
    }                                                              \
  } while (0)

// Counts, model indices and the table's header (read back from the device: 64 bytes, once
// per launch) against table_bytes and the entry point's element size.  0, or -2.
inline int exchange_args(int num_src, const int32_t* src_models, const float* weights, int num_dst,
                         const int32_t* dst_models, const void* table, int64_t table_bytes, int elem_bytes,
                         hipStream_t st, ExchangeArgs& a, SmFedTableHeader& h) {
  if (num_src < 1 || num_src > kMaxClients || num_dst < 1 || num_dst > kMaxClients + 1) return -2;
  if (!src_models || !dst_models || !table || table_bytes < (int64_t)sizeof(SmFedTableHeader)) return -2;
  hipError_t e = hipMemcpyAsync(&h, table, sizeof(h), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  if (h.magic != SM_FEDAVG_TABLE_MAGIC || h.elem_bytes != elem_bytes || h.chunk_elems != kChunk) return -2;
  if (h.num_models < 1 || h.num_models > kMaxClients + 1 || h.num_segments < 0 || h.num_chunks < 0) return -2;
  if (h.num_segments > (int64_t)1 << 31 || h.num_chunks > (int64_t)1 << 40) return -2;
  int64_t bytes = (int64_t)sizeof(SmFedTableHeader) + 8 * h.num_models * h.num_segments + 8 * h.num_segments +
                  12 * h.num_chunks;
  bytes = (bytes + 15) / 16 * 16;
  if (h.total_bytes != bytes || table_bytes != bytes) return -2;
  a = ExchangeArgs{};
  for (int j = 0; j < num_src; ++j) {
    if (src_models[j] < 0 || src_models[j] >= h.num_models) return -2;
    a.src[j] = src_models[j];
    a.w[j] = weights ? weights[j] : 0.f;
  }
  for (int d = 0; d < num_dst; ++d) {
    if (dst_models[d] < 0 || dst_models[d] >= h.num_models) return -2;
    a.dst[d] = dst_models[d];
  }
  a.num_src = num_src;
  a.num_dst = num_dst;
  return 0;
}

}  // namespace fedtab

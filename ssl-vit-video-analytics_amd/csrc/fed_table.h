// The FedAvg exchange table (include/sm_api.h "FedAvg exchange table") as the kernels of
// csrc/fed.hip, csrc/fed_dp.hip and csrc/fed_q8.hip see it, and the host-side check of a launch's arguments.
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
// tid + 256 of the chunk, in the 16-byte form and in the element-wise form alike.
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

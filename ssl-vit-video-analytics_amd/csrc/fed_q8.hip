// Compressed FedAvg round exchange: every client's update is quantised to 8 bits per element with
// one fp32 scale per block of 256 elements, and the quantisation error stays with the client as a
// residual that is added to its next update (error feedback: Seide et al. 2014, "1-Bit Stochastic
// Gradient Descent"; Karimireddy et al. 2019, "Error Feedback Fixes SignSGD").  One launch over the
// FedAvg exchange table of csrc/fed.hip, no workspace.  For every element of a quantised segment
// (mode 1), for every source j in source order, each operation rounded on its own:
//   v    = fadd(fsub(x_j, theta), e_j)
//   m    = max over the block of |v|                   (a NaN in the block makes m NaN)
//   live = m >= 1e-30f and m finite
//   s    = live ? fdiv(m, 127) : 0;  inv = live ? fdiv(127, m) : 0
//   q    = live ? clamp(rint(fmul(v, inv)), -127, 127) : 0        (round-half-even)
//   d    = fmul((float)q, s)
//   e_j  = fsub(v, d)                                  (a dead block keeps all of v)
//   acc  = theta, then acc = fadd(acc, fmul(w_j, d)) in source order
// Segments with mode 0 take sm_fedavg_exchange's plain weighted sum instead.
// A block is one wave's 4-element groups of one u in the lane ownership of fed_table.h (lane tid
// owns groups tid and tid + 256 of a chunk, so wave wv's groups of u are elements [256 (wv + 4 u),
// + 256) of the chunk), and the block maximum is a wave reduction: no LDS but for the chunk's two
// statistics.  |v| is compared as its bit pattern, which orders non-negative floats as their values
// and every NaN above infinity, so the maximum is exact and a NaN wins.  No atomics; a call's bits
// do not depend on the launch geometry, and the 16-byte and element-wise forms give the same bits.
// Compiled with -ffp-contract=off (build.py FILE_FLAGS): there is no fma here.
#include "common.h"
#include "fed_table.h"
#include "sm_api.h"

using namespace fedtab;

namespace {

constexpr int kBlocks = kChunk / SM_FEDAVG_Q8_BLOCK;   // quantisation blocks per chunk
static_assert(SM_FEDAVG_Q8_BLOCK == 64 * 4, "a block is one wave's 4-element groups of one u");
static_assert(kBlocks == 4 * kGroups, "4 waves, kGroups blocks each");
constexpr uint32_t kLiveBits = __builtin_bit_cast(uint32_t, 1e-30f);
constexpr uint32_t kInfBits = 0x7F800000u;

struct Q8Args {
  float* resid;        // [num_rows][C * kChunk]
  int8_t* codes;       // [num_src][C][kChunk], or null
  float* scales;       // [num_src][C][kBlocks], or null
  double* part;        // [num_src][C][2]
  int theta;
  int64_t P, S, C;   // the table's models, segments and chunks, from the header the host read back
};

SM_DEV uint32_t wave_max_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// Source j of chunk c: quantises v = (x - g) + e, adds w d to acc, stores the new residual and the
// payload, and leaves the wave's share of the chunk statistics in red_s / red_m.
SM_DEV void q8_source(const Q8Args& q, const ExchangeArgs& a, int j, int64_t C, int64_t c, int n, const f32x4* x,
                      const f32x4* e, const f32x4* g, f32x4* acc, double (*red_s)[kMaxClients],
                      uint32_t (*red_m)[kMaxClients]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool pay = q.codes != nullptr && q.scales != nullptr;
  const float w = a.w[j];
  f32x4 v[kGroups];
  uint32_t mb[kGroups];
#pragma unroll
  for (int u = 0; u < kGroups; ++u) {
    mb[u] = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[u][i] = __fadd_rn(__fsub_rn(x[u][i], g[u][i]), e[u][i]);
      const uint32_t b = __float_as_uint(v[u][i]) & 0x7FFFFFFFu;
      mb[u] = b > mb[u] ? b : mb[u];
    }
  }
#pragma unroll
  for (int u = 0; u < kGroups; ++u) mb[u] = wave_max_u(mb[u]);
  float* r = q.resid + (int64_t)(a.src[j] - 1) * (C * kChunk) + c * kChunk;
  float ss = 0.f;
#pragma unroll
  for (int u = 0; u < kGroups; ++u) {
    const bool live = mb[u] >= kLiveBits && mb[u] < kInfBits;   // wave-uniform
    const float m = __uint_as_float(mb[u]);
    const float s = live ? __fdiv_rn(m, 127.f) : 0.f;
    const float inv = live ? __fdiv_rn(127.f, m) : 0.f;
    f32x4 en;
    uint32_t pk = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float qf = live ? fminf(fmaxf(rintf(__fmul_rn(v[u][i], inv)), -127.f), 127.f) : 0.f;
      const float d = __fmul_rn(qf, s);
      en[i] = __fsub_rn(v[u][i], d);
      acc[u][i] = __fadd_rn(acc[u][i], __fmul_rn(w, d));
      ss = __fadd_rn(ss, __fmul_rn(en[i], en[i]));
      pk |= ((uint32_t)(int)qf & 0xFFu) << (8 * i);
    }
    const int e0 = 4 * (tid + 256 * u);
    store_group(r, e0, n, true, en);   // the residual rows are 16-byte aligned (checked on the host)
    if (pay) {
      *(uint32_t*)(q.codes + ((int64_t)j * C + c) * kChunk + e0) = pk;
      if (lane == 0) q.scales[((int64_t)j * C + c) * kBlocks + wv + 4 * u] = s;
    }
  }
  const double sd = wave_sum_d((double)ss);
  if (lane == 0) {
    red_s[wv][j] = sd;
    uint32_t mm = mb[0];
#pragma unroll
    for (int u = 1; u < kGroups; ++u) mm = mb[u] > mm ? mb[u] : mm;
    red_m[wv][j] = mm;
  }
}

// KC > 0: source count known at compile time (the loads of a lane, sources and residuals, are
// issued before the first operation, for 8 sources in two halves); KC == 0: runtime count.
// Sources, theta and destinations may alias: the models are stored to once, after the last source,
// so a lane has loaded its elements from theta and every source before its first store into a
// model; lanes own disjoint elements, and no pointer is __restrict__.  The residual and payload
// buffers are the caller's own and overlap no model.
template <int KC>
__global__ void __launch_bounds__(256) q8_exchange_kernel(ExchangeArgs a, Q8Args q, const unsigned char* tab,
                                                          const uint8_t* seg_mode) {
  __shared__ double red_s[4][kMaxClients];
  __shared__ uint32_t red_m[4][kMaxClients];
  // the counts come as arguments: read from the header here they are one 8-register scalar load whose
  // spill slot leaves the runtime-count variant with a scratch reservation
  const TableView t = table_view(tab, q.P, q.S, q.C);
  const int k = KC > 0 ? KC : a.num_src;
  const int tid = threadIdx.x;
  const bool pay = q.codes != nullptr && q.scales != nullptr;
  for (int64_t c = blockIdx.x; c < t.C; c += gridDim.x) {
    int64_t seg, off, n64;
    const bool in_range = chunk_range(t, c, seg, off, n64);
    if (!in_range || seg_mode[seg] == 0) {   // block-uniform
      if (tid < k) {
        q.part[(tid * t.C + c) * 2] = 0.0;
        q.part[(tid * t.C + c) * 2 + 1] = 0.0;
      }
      if (pay) {   // nothing of this chunk is quantised: a payload of zeros
        for (int j = 0; j < k; ++j) {
#pragma unroll
          for (int u = 0; u < kGroups; ++u)
            *(uint32_t*)(q.codes + ((int64_t)j * t.C + c) * kChunk + 4 * (tid + 256 * u)) = 0u;
          if (tid < kBlocks) q.scales[((int64_t)j * t.C + c) * kBlocks + tid] = 0.f;
        }
      }
      if (!in_range) continue;
    }
    const int n = (int)n64;
    const bool vec = seg_aligned(t, a, k, seg, true, t.addr[q.theta * t.S + seg]);
    f32x4 acc[kGroups];
    if (seg_mode[seg] == 0) {
#pragma unroll
      for (int u = 0; u < kGroups; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      for_sources<0>(t, a, k, seg, off, n, vec, [&](int j, const f32x4* x) { add_plain(acc, x, a.w[j]); });
    } else {
      f32x4 g[kGroups];
      load_lane(seg_ptr(t, q.theta, seg, off), n, vec, g);
#pragma unroll
      for (int u = 0; u < kGroups; ++u) acc[u] = g[u];
      if constexpr (KC > 0) {
        constexpr int kHalf = KC > 4 ? KC / 2 : KC;   // 8 sources at once would not fit the register file
        static_assert(KC % kHalf == 0, "the sources are loaded in equal parts");
#pragma unroll 1   // a rolled loop: the halves' addresses do not all stay live in scalar registers
        for (int j0 = 0; j0 < KC; j0 += kHalf) {
          f32x4 x[kHalf][kGroups], e[kHalf][kGroups];
#pragma unroll
          for (int j = 0; j < kHalf; ++j) {
            load_lane(seg_ptr(t, a.src[j0 + j], seg, off), n, vec, x[j]);
            load_lane(q.resid + (int64_t)(a.src[j0 + j] - 1) * (t.C * kChunk) + c * kChunk, n, true, e[j]);
          }
#pragma unroll
          for (int j = 0; j < kHalf; ++j) q8_source(q, a, j0 + j, t.C, c, n, x[j], e[j], g, acc, red_s, red_m);
        }
      } else {
#pragma unroll 1
        for (int j = 0; j < k; ++j) {
          f32x4 x[kGroups], e[kGroups];
          load_lane(seg_ptr(t, a.src[j], seg, off), n, vec, x);
          load_lane(q.resid + (int64_t)(a.src[j] - 1) * (t.C * kChunk) + c * kChunk, n, true, e);
          q8_source(q, a, j, t.C, c, n, x, e, g, acc, red_s, red_m);
        }
      }
      __syncthreads();
      if (tid < k) {
        uint32_t mm = red_m[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) mm = red_m[w][tid] > mm ? red_m[w][tid] : mm;
        q.part[(tid * t.C + c) * 2] = (double)__uint_as_float(mm);
        q.part[(tid * t.C + c) * 2 + 1] = ((red_s[0][tid] + red_s[1][tid]) + red_s[2][tid]) + red_s[3][tid];
      }
      __syncthreads();   // red_s / red_m are written again in the block's next chunk
    }
    store_dsts(t, a, seg, off, n, vec, acc);
  }
}

}  // namespace

extern "C" int sm_fedavg_q8_exchange(int num_src, const int32_t* src_models, const float* weights, int global_model,
                                     int num_dst, const int32_t* dst_models, const void* table, int64_t table_bytes,
                                     const uint8_t* seg_mode, float* resid, int num_rows, int8_t* codes, float* scales,
                                     double* part, hipStream_t st) {
  if (!weights || !seg_mode || !resid || !part || global_model < 0 || num_rows < 1) return -2;
  ExchangeArgs a;
  SmFedTableHeader h{};
  const int rc = exchange_args(num_src, src_models, weights, num_dst, dst_models, table, table_bytes, 4, st, a, h);
  if (rc != 0) return rc;
  if (global_model >= h.num_models) return -2;
  for (int j = 0; j < num_src; ++j)   // a source is a client model with a residual row of its own
    if (a.src[j] == global_model || a.src[j] < 1 || a.src[j] - 1 >= num_rows) return -2;
  if (((uintptr_t)resid & 15u) || ((uintptr_t)part & 7u) || ((uintptr_t)codes & 3u) || ((uintptr_t)scales & 3u))
    return -4;
  const int64_t chunks = h.num_chunks;
  if (chunks == 0) return 0;
  const Q8Args q{resid, codes, scales, part, global_model, h.num_models, h.num_segments, h.num_chunks};
  const dim3 g = exchange_grid(chunks), b(256);
  const unsigned char* tab = (const unsigned char*)table;
  FED_DISPATCH_KC(num_src, hipLaunchKernelGGL(q8_exchange_kernel<KC>, g, b, 0, st, a, q, tab, seg_mode));
  SM_CHECK_LAUNCH();
  return 0;
}

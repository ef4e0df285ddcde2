// DP-FedAvg round exchange (McMahan et al. 2018, "Learning Differentially Private Recurrent
// Language Models"): every client's update x_c - theta is clipped to an L2 bound over the clipped
// segments, the clipped updates are averaged onto theta and Gaussian noise is added, over the
// FedAvg exchange table of csrc/fed.hip (the models' tensors where they live).  Three launches:
//   norms     part[c][chunk] = sum of (x_c - theta)^2 over one chunk of a clipped segment: a lane
//             adds its 8 squares in fp32, the 64 lanes of a wave and the 4 waves add in fp64
//   finalise  norm_c = sqrt(sum of part[c][.]) in fp64 (thread t takes chunks t, t + 256, ...
//             ascending, then the 256 partials in thread order), scale_c = min(1, clip / (norm_c +
//             1e-6)) in fp32 (sm_grad_clip's form), ws_c = w_c scale_c
//   update    acc = theta; acc += ws_c (x_c - theta) in source order, every operation rounded on
//             its own; acc = fma(noise_std, n(seed, segment, element), acc); segments with mode 0
//             take sm_fedavg_exchange's plain weighted sum instead
// No atomics; every sum has a fixed partition and order, so a call's bits do not depend on the
// launch geometry and two calls agree bit for bit.  A lane owns the same elements in the 16-byte
// form and in the element-wise form (the 4-element groups tid and tid + 256 of a chunk), so both
// give the same bits.  Compiled with -ffp-contract=off (build.py FILE_FLAGS): the only fma is the
// explicit one of the noise.
#include <stdlib.h>

#include "common.h"
#include "fed_table.h"
#include "sm_api.h"

using namespace fedtab;

namespace {

// One lane's share of sum (x - g)^2, groups then elements ascending (padding slots add +0).
SM_DEV float lane_sq(const f32x4* x, const f32x4* g) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < kGroups; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = __fsub_rn(x[u][e], g[u][e]);
      s = __fadd_rn(s, __fmul_rn(d, d));
    }
  return s;
}

// KC > 0: source count known at compile time (every load of a lane is issued before the first
// subtraction); KC == 0: runtime count.  part [num_src][C]; a chunk outside the clipped segments
// gets zeros, so finalise adds every entry.
template <int KC>
__global__ void __launch_bounds__(256) dp_norms_kernel(ExchangeArgs a, int theta, const unsigned char* tab,
                                                       const uint8_t* seg_clip, double* part) {
  __shared__ double red[4][kMaxClients];
  const TableView t = table_view(tab);
  const int k = KC > 0 ? KC : a.num_src;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t c = blockIdx.x; c < t.C; c += gridDim.x) {
    int64_t seg, off, n64;
    if (!chunk_range(t, c, seg, off, n64) || seg_clip[seg] == 0) {   // block-uniform
      if (tid < k) part[tid * t.C + c] = 0.0;
      continue;
    }
    const int n = (int)n64;
    const bool vec = seg_aligned(t, a, k, seg, false, t.addr[theta * t.S + seg]);
    f32x4 g[kGroups];
    load_lane(seg_ptr(t, theta, seg, off), n, vec, g);
    for_sources<KC>(t, a, k, seg, off, n, vec, [&](int j, const f32x4* x) {
      const double s = wave_sum_d((double)lane_sq(x, g));
      if (lane == 0) red[wv][j] = s;
    });
    __syncthreads();
    if (tid < k) part[tid * t.C + c] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();   // red is written again in the block's next chunk
  }
}

// Block c: source c's norm, scale and scaled weight.  stats [2 num_src] = norms, then scales.
__global__ void __launch_bounds__(256) dp_finalise_kernel(ExchangeArgs a, int64_t C, const double* part,
                                                          float clip_norm, float* stats, float* wsc) {
  const int j = blockIdx.x, tid = threadIdx.x;
  double s[1] = {0.0};
  for (int64_t c = tid; c < C; c += 256) s[0] += part[j * C + c];
  thread_order_sum_d<1, SUM_THREAD0>(s);
  if (tid == 0) {
    const float norm = (float)sqrt(s[0]);
    const float scale = clip_coef(clip_norm, norm);
    stats[j] = norm;
    stats[a.num_src + j] = scale;
    wsc[j] = __fmul_rn(a.w[j], scale);
  }
}

// acc += ws (x - g) over one lane's groups, each operation rounded on its own.
SM_DEV void add_clipped(f32x4* acc, const f32x4* x, const f32x4* g, float ws) {
#pragma unroll
  for (int u = 0; u < kGroups; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[u][e] = __fadd_rn(acc[u][e], __fmul_rn(ws, __fsub_rn(x[u][e], g[u][e])));
}

// Sources, theta and destinations may alias: a lane loads its elements from theta and every
// source before its first store, lanes own disjoint elements, and no pointer is __restrict__.
template <int KC>
__global__ void __launch_bounds__(256) dp_update_kernel(ExchangeArgs a, int theta, const unsigned char* tab,
                                                        const uint8_t* seg_clip, const float* wsc, float noise_std,
                                                        uint32_t s32) {
  const TableView t = table_view(tab);
  const int k = KC > 0 ? KC : a.num_src;
  const int tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < t.C; c += gridDim.x) {
    int64_t seg, off, n64;
    if (!chunk_range(t, c, seg, off, n64)) continue;
    const int n = (int)n64;
    const bool clip = seg_clip[seg] != 0;   // block-uniform
    const bool vec = seg_aligned(t, a, k, seg, true, t.addr[theta * t.S + seg]);
    f32x4 acc[kGroups], g[kGroups];
#pragma unroll
    for (int u = 0; u < kGroups; ++u) acc[u] = g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (clip) {
      load_lane(seg_ptr(t, theta, seg, off), n, vec, g);
#pragma unroll
      for (int u = 0; u < kGroups; ++u) acc[u] = g[u];
    }
    // for_sources with the clip test in its operation, or around two of them, costs dp_update_kernel<4>
    // a wave (73 and 81 VGPRs against 70: the kernel sits at the SGPR ceiling and spills into VGPR
    // lanes), so the two-shaped loop stays written out here.
    if constexpr (KC > 0) {
      f32x4 x[KC][kGroups];
#pragma unroll
      for (int j = 0; j < KC; ++j) load_lane(seg_ptr(t, a.src[j], seg, off), n, vec, x[j]);
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        if (clip) add_clipped(acc, x[j], g, wsc[j]);
        else add_plain(acc, x[j], a.w[j]);
      }
    } else {
      for (int j = 0; j < k; ++j) {
        f32x4 x[kGroups];
        load_lane(seg_ptr(t, a.src[j], seg, off), n, vec, x);
        if (clip) add_clipped(acc, x, g, wsc[j]);
        else add_plain(acc, x, a.w[j]);
      }
    }
    if (clip && noise_std > 0.f) {
      const RowKeys rk = row_keys(s32, (uint32_t)seg);
#pragma unroll
      for (int u = 0; u < kGroups; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t col = (uint32_t)(off + 4 * (tid + 256 * u) + e);   // a clipped segment has <= 2^32 elements
          acc[u][e] = fmaf(noise_std, gauss_draw(rk, col * kColMul), acc[u][e]);
        }
    }
    store_dsts(t, a, seg, off, n, vec, acc);
  }
}

constexpr int64_t kMaxSegElems = (int64_t)1 << 32;   // the noise draw's column is 32 bits

// A clipped segment longer than 2^32 elements: only a table of more than 2^32 / kChunk chunks can
// hold one, and only then are the lengths and the modes read back.  0, -2, or a HIP error.
int check_clipped_lengths(const SmFedTableHeader& h, const void* table, const uint8_t* seg_clip, hipStream_t st) {
  if (h.num_chunks <= kMaxSegElems / kChunk || h.num_segments == 0) return 0;
  const int64_t S = h.num_segments;
  int64_t* len = (int64_t*)malloc(S * sizeof(int64_t));
  uint8_t* mode = (uint8_t*)malloc(S);
  int rc = len && mode ? 0 : -2;
  if (rc == 0) {
    const unsigned char* seg_len = (const unsigned char*)table + sizeof(SmFedTableHeader) + 8 * h.num_models * S;
    hipError_t e = hipMemcpyAsync(len, seg_len, S * sizeof(int64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(mode, seg_clip, S, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    rc = (int)e;
    for (int64_t s = 0; rc == 0 && s < S; ++s)
      if (mode[s] != 0 && len[s] > kMaxSegElems) rc = -2;
  }
  free(len);
  free(mode);
  return rc;
}

}  // namespace

extern "C" int64_t sm_fedavg_dp_exchange_workspace_bytes(int num_src, int64_t num_chunks) {
  if (num_src < 1 || num_src > kMaxClients || num_chunks < 0 || num_chunks > (int64_t)1 << 40) return -1;
  return (num_src * num_chunks * (int64_t)sizeof(double) + kMaxClients * (int64_t)sizeof(float) + 15) / 16 * 16;
}

extern "C" int sm_fedavg_dp_exchange(int num_src, const int32_t* src_models, const float* weights, int global_model,
                                     int num_dst, const int32_t* dst_models, const void* table, int64_t table_bytes,
                                     const uint8_t* seg_clip, float clip_norm, float noise_std, uint64_t seed,
                                     float* stats, void* ws, int64_t ws_bytes, hipStream_t st) {
  if (!weights || !seg_clip || !stats || global_model < 0) return -2;
  if (!(clip_norm > 0.f) || !(noise_std >= 0.f)) return -2;   // a NaN fails either comparison
  ExchangeArgs a;
  SmFedTableHeader h{};
  int rc = exchange_args(num_src, src_models, weights, num_dst, dst_models, table, table_bytes, 4, st, a, h);
  if (rc != 0) return rc;
  if (global_model >= h.num_models || h.num_segments > kMaxSegElems) return -2;
  rc = check_clipped_lengths(h, table, seg_clip, st);
  if (rc != 0) return rc;
  const int64_t chunks = h.num_chunks;
  if (!ws || ((uintptr_t)ws & 15u) || ws_bytes < sm_fedavg_dp_exchange_workspace_bytes(num_src, chunks)) return -4;
  double* part = (double*)ws;
  float* wsc = (float*)(part + num_src * chunks);
  const dim3 g = exchange_grid(chunks), b(256);
  const unsigned char* tab = (const unsigned char*)table;
  const uint32_t s32 = (uint32_t)seed ^ (uint32_t)(seed >> 32);   // seed32
  if (chunks > 0) {
    FED_DISPATCH_KC(num_src, hipLaunchKernelGGL(dp_norms_kernel<KC>, g, b, 0, st, a, global_model, tab, seg_clip, part));
    SM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(dp_finalise_kernel, dim3((unsigned)num_src), b, 0, st, a, chunks, part, clip_norm, stats, wsc);
  SM_CHECK_LAUNCH();
  if (chunks == 0) return 0;
  FED_DISPATCH_KC(num_src, hipLaunchKernelGGL(dp_update_kernel<KC>, g, b, 0, st, a, global_model, tab, seg_clip, wsc, noise_std, s32));
  SM_CHECK_LAUNCH();
  return 0;
}

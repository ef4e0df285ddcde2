// Feature-privacy evaluation (src/run_privacy.py:229-348 run_feature_privacy of the reference,
// src/privacy/feature_noise.py, metrics_privacy.py, attacker.py): the video embeddings under
// Gaussian noise and random feature masking, the head's utility numbers over the whole grid,
// and the hidden layer of the attacker probe.  All fp32:
//   privacy_perturb   out[g] = (z + sigma_g n_g(r, c)) keep_g(r, c) for G configurations, z read once
//   logits_metrics    per row cross-entropy / entropy / top-1 / top-k (+ the softmax gradient),
//                     summed per segment in fp64
//   soft_ce           the same row kernel against a two-label, smoothed target (Mixup / CutMix and
//                     label smoothing in fine-tuning): loss, top-1 and the gradient
//   relu_fwd          h = max(pre, 0)
//   relu_bias_bwd     dpre = dh (h > 0) and its column sums in one pass
// No atomics, no LDS tiling, no MFMA; every reduction has a fixed partition and order, so no
// result depends on the launch geometry.  Each kernel has a 16-byte form and a scalar form with
// the same element ownership and summation order: same bits.
#include "common.h"
#include "sm_api.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------- perturbation draws
// The streams, their keys (row_keys) and the Gaussian (gauss_draw) are csrc/common.h's counter-based
// perturbation draws, shared with csrc/fed_dp.hip.
struct PerturbCfg {
  uint64_t thr[SM_PRIVACY_MAX_CONFIGS];   // keep iff (uint64)h2 >= thr; 0 keeps all, 2^32 drops all
  float sigma[SM_PRIVACY_MAX_CONFIGS];
  uint32_t s32[SM_PRIVACY_MAX_CONFIGS];
};

// One element: noise first, then the 0/1 mask without a 1 / keep rescale (feature_noise.py:4-15).
// sigma <= 0 and thr == 0 leave the value untouched (bit-exact).
SM_DEV float perturb_one(float z, const RowKeys& rk, uint32_t col, float sigma, uint64_t thr) {
  const uint32_t cm = col * kColMul;
  float v = z;
  if (sigma > 0.f) v = fmaf(sigma, gauss_draw(rk, cm), z);
  if (thr != 0) {
    const uint32_t h2 = fmix32(rk.k2 + cm);
    v *= (uint64_t)h2 >= thr ? 1.0f : 0.0f;
  }
  return v;
}

// One thread per group of 4 consecutive elements (flat index 4 t .. 4 t + 3), every configuration
// in turn.  VEC: D % 4 == 0, so a group lies in one row and moves as 16 bytes.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void perturb_kernel(const float* __restrict__ z, int64_t total, int D, int G,
                                                           PerturbCfg cfg, float* __restrict__ out) {
  const int64_t e0 = (blockIdx.x * (int64_t)kThreads + threadIdx.x) * 4;
  if (e0 >= total) return;
  if constexpr (VEC) {
    const uint32_t row = (uint32_t)(e0 / D), col = (uint32_t)(e0 % D);
    const f32x4 x = *(const f32x4*)(z + e0);
    for (int g = 0; g < G; ++g) {
      const RowKeys rk = row_keys(cfg.s32[g], row);
      f32x4 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = perturb_one(x[j], rk, col + j, cfg.sigma[g], cfg.thr[g]);
      __builtin_nontemporal_store(y, (f32x4*)(out + (int64_t)g * total + e0));
    }
  } else {
    const int n = total - e0 < 4 ? (int)(total - e0) : 4;
    float x[4];
    uint32_t row[4], col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = e0 + j;
      row[j] = (uint32_t)(e / D);
      col[j] = (uint32_t)(e % D);
      x[j] = j < n ? z[e] : 0.f;
    }
    for (int g = 0; g < G; ++g) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n)
          out[(int64_t)g * total + e0 + j] = perturb_one(x[j], row_keys(cfg.s32[g], row[j]), col[j], cfg.sigma[g],
                                                         cfg.thr[g]);
    }
  }
}

// ---------------------------------------------------------------- logits metrics
SM_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// x where in == ~0, -inf where in == 0
SM_DEV float pad_neg_inf(float x, int in) {
  return __int_as_float((__float_as_int(x) & in) | ((int)0xFF800000 & ~in));
}

// The row kernel's target.  HardTarget: the one-hot of labels[r % N] (sm_logits_metrics).
// SoftTarget (sm_soft_ce): t_c = lam s(ya)_c + (1 - lam) s(yb)_c with s(y)_c = eps / C + (1 - eps) [c == y],
// ya = labels[r], yb = labels_b[r] (null: ya), lam = lam[r] (null: 1).
struct HardTarget {
  static constexpr bool soft = false;
};
struct SoftTarget {
  static constexpr bool soft = true;
  const int64_t* labels_b;
  const float* lam;
  float eps;
};
// One row's soft target.  With eps == 0 and lam == 1 it is exactly 1 at ya and exactly 0 elsewhere.
struct SoftRow {
  int ya, yb;
  float lam, oml, off, on;                            // oml = 1 - lam, off = eps / C, on = 1 - eps
  SM_DEV float t(int c) const {
    const float ta = off + (c == ya ? on : 0.f), tb = off + (c == yb ? on : 0.f);
    return lam * ta + oml * tb;
  }
};

// One wave per row, four rows per block.  Lane l owns columns 256 j + 4 l + i (j < NG, i < 4):
// NG 16-byte groups in registers.  rowvals [rows][4] = loss, entropy, hit1, hitk.
// Target::soft: rowvals [rows][2] = loss, hit1 (no entropy, k unused), the gradient is softmax - t, and
// the loss is (lse - l_ya) - sum_c d_c (l_c - m) with d = t - onehot(ya) (sum_c d_c = 0, so this is
// lse - sum_c t_c l_c): the hard kernel's expression plus a correction formed from the max-subtracted
// logits, which is finite for large logits and exactly 0 when the target is the one-hot of ya.
template <int NG, bool VEC, typename Target>
__global__ __launch_bounds__(kThreads) void logits_rows_kernel(const float* __restrict__ logits, int64_t rows, int C,
                                                               const int64_t* __restrict__ labels, int64_t N, int k,
                                                               float* __restrict__ dlogits, float grad_scale,
                                                               float* __restrict__ rowvals, Target tgt) {
  constexpr bool SOFT = Target::soft;
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * (int64_t)(kThreads / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                              // wave-uniform
  const float* x = logits + r * C;
  float v[NG][4];
  // every load is unconditional (a slot past the row reads column 0 instead) and is then set to
  // -inf with an integer mask: no load sits under a per-lane branch and no lane mask stays live
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int c0 = 256 * j + 4 * lane;
    if constexpr (VEC) {
      const int in = (c0 - C) >> 31;                    // all ones when c0 < C
      const f32x4 a = *(const f32x4*)(x + (c0 & in));
#pragma unroll
      for (int i = 0; i < 4; ++i) v[j][i] = pad_neg_inf(a[i], in);
    } else if (256 * j + 256 <= C) {                    // wave-uniform: a whole 256-column slab
#pragma unroll
      for (int i = 0; i < 4; ++i) v[j][i] = x[c0 + i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int in = (c0 + i - C) >> 31;
        v[j][i] = pad_neg_inf(x[(c0 + i) & in], in);
      }
    }
  }
  const int64_t y64 = labels[r % N];
  const bool y_ok = y64 >= 0 && y64 < C;
  const int y = y_ok ? (int)y64 : -1;
  const float lx = x[y_ok ? y : 0];                    // the label's logit: one wave-uniform load
  bool t_ok = y_ok;                                    // every label of the target lies in [0, C)
  SoftRow sr;
  if constexpr (SOFT) {
    const int64_t yb64 = tgt.labels_b ? tgt.labels_b[r] : y64;
    t_ok = y_ok && yb64 >= 0 && yb64 < C;
    sr.ya = y;
    sr.yb = t_ok ? (int)yb64 : -1;
    sr.lam = tgt.labels_b && tgt.lam ? tgt.lam[r] : 1.0f;
    sr.oml = 1.0f - sr.lam;
    sr.off = tgt.eps / (float)C;
    sr.on = 1.0f - tgt.eps;
  }
  const float ly = t_ok ? lx : NAN;
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) m = fmaxf(m, v[j][i]);
  m = wave_max(m);
  float s = 0.f;
  float corr = 0.f;                                    // SOFT: sum_c d_c (l_c - m)
  int rank = 0;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 256 * j + 4 * lane + i;
      const float l = v[j][i];
      // rank of the label: larger logits, and equal ones at a lower index, come first
      // (a padding slot holds -inf at c >= C > y: it never counts, and its exp is 0)
      rank += (l > ly || (l == ly && c < y)) ? 1 : 0;
      const float e = expf(l - m);                       // a NaN or +inf logit makes the sum NaN
      s += e;
      v[j][i] = e;
      if constexpr (SOFT) {
        // a column whose weight does not move (d == 0) adds nothing, whatever its logit (-inf is an
        // ordinary value); padding slots (c >= C) have no target
        const float d = sr.t(c) - (c == y ? 1.0f : 0.0f);
        corr += c < C && d != 0.f ? d * (l - m) : 0.f;
      }
    }
  s = wave_sum(s);
  if constexpr (SOFT) corr = wave_sum(corr);
  rank = wave_sum_i(rank);
  const float lse = m + logf(s);
  const float inv = 1.0f / s;
  float ent = 0.f;
#pragma unroll
  for (int j = 0; j < NG; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float p = v[j][i] * inv;
      // SOFT has no entropy to keep p a value of its own: without this (empty) statement the compiler
      // contracts e * inv - t into one fma and the gradient loses the hard form's rounding of p
      if constexpr (SOFT) asm volatile("" : "+v"(p));
      if constexpr (!SOFT) ent -= p * logf(p + 1e-12f);   // metrics_privacy.py:7; padding: p = 0 adds 0
      v[j][i] = p;
    }
  if constexpr (!SOFT) ent = wave_sum(ent);
  if (dlogits) {
    float* d = dlogits + r * C;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int c0 = 256 * j + 4 * lane;
      float gq[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (SOFT) gq[i] = (v[j][i] - sr.t(c0 + i)) * grad_scale;
        else gq[i] = (v[j][i] - (c0 + i == y ? 1.0f : 0.0f)) * grad_scale;
      }
      if constexpr (VEC) {
        if (c0 < C) *(f32x4*)(d + c0) = f32x4{gq[0], gq[1], gq[2], gq[3]};
      } else if (256 * j + 256 <= C) {                  // wave-uniform: a whole 256-column slab
#pragma unroll
        for (int i = 0; i < 4; ++i) d[c0 + i] = gq[i];
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < C) d[c0 + i] = gq[i];
      }
    }
  }
  if (lane == 0) {
    const float loss = lse - ly;
    const bool finite = fabsf(lse) < INFINITY && y_ok && ly == ly;   // false for NaN
    if constexpr (SOFT) {
      float* o = rowvals + r * 2;
      o[0] = loss - corr;
      o[1] = finite && rank < 1 ? 1.f : 0.f;
    } else {
      float* o = rowvals + r * 4;
      o[0] = loss;
      o[1] = ent;
      o[2] = finite && rank < 1 ? 1.f : 0.f;
      o[3] = finite && rank < k ? 1.f : 0.f;
    }
  }
}

// The row kernel of the class-count tier of C
template <bool VEC, typename Target>
auto rows_kernel_for(int C) {
  return C <= 256    ? logits_rows_kernel<1, VEC, Target>
         : C <= 512  ? logits_rows_kernel<2, VEC, Target>
         : C <= 1024 ? logits_rows_kernel<4, VEC, Target>
         : C <= 2048 ? logits_rows_kernel<8, VEC, Target>
                     : logits_rows_kernel<16, VEC, Target>;
}

// out[s][q] = sum over the N rows of segment s of rowvals[.][q], fp64: thread t takes rows t,
// t + 256, ... ascending, then the 256 partials are added in thread order.
__global__ __launch_bounds__(kThreads) void logits_segments_kernel(const float* __restrict__ rowvals, int64_t N,
                                                                   double* __restrict__ out) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const float* base = rowvals + (int64_t)s * N * 4;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t i = tid; i < N; i += kThreads) {
    const f32x4 q = *(const f32x4*)(base + i * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] += (double)q[c];
  }
  static_assert(kThreads == 256, "thread_order_sum_d adds 256 threads' partials");
  thread_order_sum_d<4, SUM_FIRST_K>(a);               // thread q < 4: column q's sum in a[0]
  if (tid < 4) out[(int64_t)s * 4 + tid] = a[0];
}

// out[q] = sum over the N rows of rowvals[.][q] (q < 2), in logits_segments_kernel's order: the loss
// sum of a one-hot target has sm_logits_metrics' bits
__global__ __launch_bounds__(kThreads) void soft_sum_kernel(const float* __restrict__ rowvals, int64_t N,
                                                            double* __restrict__ out) {
  const int tid = threadIdx.x;
  double a[2] = {0.0, 0.0};
  for (int64_t i = tid; i < N; i += kThreads) {
    a[0] += (double)rowvals[i * 2];
    a[1] += (double)rowvals[i * 2 + 1];
  }
  thread_order_sum_d<2, SUM_FIRST_K>(a);               // thread q < 2: column q's sum in a[0]
  if (tid < 2) out[tid] = a[0];
}

// ---------------------------------------------------------------- ReLU
template <bool VEC>
__global__ __launch_bounds__(kThreads) void relu_fwd_kernel(const float* __restrict__ pre, int64_t n,
                                                            float* __restrict__ h) {
  const int64_t e0 = (blockIdx.x * (int64_t)kThreads + threadIdx.x) * 4;
  if (e0 >= n) return;
  auto relu = [](float x) { return x > 0.f ? x : (x == x ? 0.f : x); };   // NaN stays NaN
  if constexpr (VEC) {
    const f32x4 a = *(const f32x4*)(pre + e0);
    *(f32x4*)(h + e0) = f32x4{relu(a[0]), relu(a[1]), relu(a[2]), relu(a[3])};
  } else {
    for (int j = 0; j < 4 && e0 + j < n; ++j) h[e0 + j] = relu(pre[e0 + j]);
  }
}

// Block (one wave) = kReluRows rows x 256 columns, thread = 4 consecutive columns: dpre written,
// the chunk's column sums to part [nchunks][C] (fp32, rows ascending); colred adds the chunks in fp64.
constexpr int kReluRows = 32;

template <bool VEC>
__global__ __launch_bounds__(64) void relu_bias_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ h,
                                                           int64_t M, int C, float* __restrict__ dpre,
                                                           float* __restrict__ part) {
  const int c0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (c0 >= C) return;
  const int64_t r0 = (int64_t)blockIdx.y * kReluRows;
  const int64_t r1 = r0 + kReluRows < M ? r0 + kReluRows : M;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t r = r0; r < r1; ++r) {
    const int64_t o = r * C + c0;
    if constexpr (VEC) {
      const f32x4 g = *(const f32x4*)(dh + o), a = *(const f32x4*)(h + o);
      f32x4 d;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d[j] = a[j] > 0.f ? g[j] : 0.f;
        acc[j] += d[j];
      }
      *(f32x4*)(dpre + o) = d;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) {
          const float d = h[o + j] > 0.f ? dh[o + j] : 0.f;
          dpre[o + j] = d;
          acc[j] += d;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (c0 + j < C) part[(int64_t)blockIdx.y * C + c0 + j] = acc[j];
}

}  // namespace

extern "C" int sm_privacy_perturb(const float* z, int64_t N, int D, int G, const float* sigmas,
                                  const uint64_t* thresholds, const uint64_t* seeds, float* out, hipStream_t st) {
  if (N <= 0 || D <= 0 || G <= 0 || G > SM_PRIVACY_MAX_CONFIGS || N > 0x7fffffff || !z || !sigmas || !thresholds ||
      !seeds || !out)
    return -2;
  const int64_t total = N * D;
  const int64_t nblk = ((total + 3) / 4 + kThreads - 1) / kThreads;
  if (nblk > 0x7fffffff) return -2;
  PerturbCfg cfg{};
  for (int g = 0; g < G; ++g) {
    if (thresholds[g] > (1ull << 32)) return -2;
    cfg.thr[g] = thresholds[g];
    cfg.sigma[g] = sigmas[g];
    cfg.s32[g] = (uint32_t)seeds[g] ^ (uint32_t)(seeds[g] >> 32);      // seed32
  }
  DISPATCH_BOOL(D % 4 == 0 && aligned16(z) && aligned16(out), VEC,
                hipLaunchKernelGGL(perturb_kernel<VEC>, dim3((unsigned)nblk), dim3(kThreads), 0, st, z, total, D, G, cfg,
                                   out));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_logits_metrics_workspace_bytes(int64_t rows) {
  return rows > 0 ? rows * 4 * (int64_t)sizeof(float) : 0;
}

extern "C" int sm_logits_metrics(const float* logits, int64_t rows, int C, const int64_t* labels, int64_t N, int k,
                                 float* dlogits, float grad_scale, double* out, void* ws, int64_t ws_bytes,
                                 hipStream_t st) {
  if (rows <= 0 || N <= 0 || rows % N || C <= 0 || C > SM_LOGITS_MAX_CLASSES || k <= 0 || !logits || !labels || !out)
    return -2;
  const int64_t S = rows / N;
  const int64_t nblk = (rows + kThreads / 64 - 1) / (kThreads / 64);
  if (nblk > 0x7fffffff || S > 0x7fffffff) return -2;
  if (!ws || ws_bytes < sm_logits_metrics_workspace_bytes(rows) || !aligned16(ws)) return -4;
  float* rowvals = (float*)ws;
  const bool vec = C % 4 == 0 && aligned16(logits) && (!dlogits || aligned16(dlogits));
  DISPATCH_BOOL(vec, VEC,
                hipLaunchKernelGGL((rows_kernel_for<VEC, HardTarget>(C)), dim3((unsigned)nblk), dim3(kThreads), 0, st,
                                   logits, rows, C, labels, N, k, dlogits, grad_scale, rowvals, HardTarget{}));
  SM_CHECK_LAUNCH();
  hipLaunchKernelGGL(logits_segments_kernel, dim3((unsigned)S), dim3(kThreads), 0, st, rowvals, N, out);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_soft_ce_workspace_bytes(int64_t N) { return N > 0 ? N * 2 * (int64_t)sizeof(float) : 0; }

extern "C" int sm_soft_ce(const float* logits, int64_t N, int C, const int64_t* labels_a, const int64_t* labels_b,
                          const float* lam, float eps, float* dlogits, float grad_scale, double* out, void* ws,
                          int64_t ws_bytes, hipStream_t st) {
  if (N <= 0 || C <= 0 || C > SM_LOGITS_MAX_CLASSES || !(eps >= 0.f && eps < 1.f) || !logits || !labels_a || !out)
    return -2;
  const int64_t nblk = (N + kThreads / 64 - 1) / (kThreads / 64);
  if (nblk > 0x7fffffff) return -2;
  if (!ws || ws_bytes < sm_soft_ce_workspace_bytes(N) || !aligned16(ws)) return -4;
  float* rowvals = (float*)ws;
  const bool vec = C % 4 == 0 && aligned16(logits) && (!dlogits || aligned16(dlogits));
  DISPATCH_BOOL(vec, VEC,
                hipLaunchKernelGGL((rows_kernel_for<VEC, SoftTarget>(C)), dim3((unsigned)nblk), dim3(kThreads), 0, st,
                                   logits, N, C, labels_a, N, 1, dlogits, grad_scale, rowvals,
                                   SoftTarget{labels_b, lam, eps}));
  SM_CHECK_LAUNCH();
  hipLaunchKernelGGL(soft_sum_kernel, dim3(1), dim3(kThreads), 0, st, rowvals, N, out);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_relu_fwd(const float* pre, int64_t n, float* h, hipStream_t st) {
  if (n <= 0) return 0;
  if (!pre || !h) return -2;
  const int64_t nblk = ((n + 3) / 4 + kThreads - 1) / kThreads;
  if (nblk > 0x7fffffff) return -2;
  DISPATCH_BOOL(aligned16(pre) && aligned16(h) && n % 4 == 0, VEC,
                hipLaunchKernelGGL(relu_fwd_kernel<VEC>, dim3((unsigned)nblk), dim3(kThreads), 0, st, pre, n, h));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_relu_bias_bwd_workspace_bytes(int64_t M, int C) {
  if (M <= 0 || C <= 0) return 0;
  return ((M + kReluRows - 1) / kReluRows) * C * (int64_t)sizeof(float);
}

extern "C" int sm_relu_bias_bwd(const float* dh, const float* h, int64_t M, int C, float* dpre, float* db, void* ws,
                                int64_t ws_bytes, hipStream_t st) {
  if (M <= 0 || C <= 0 || !dh || !h || !dpre || !db) return -2;
  const int64_t nchunks = (M + kReluRows - 1) / kReluRows;
  if (nchunks > 65535) return -2;
  if (!ws || ws_bytes < sm_relu_bias_bwd_workspace_bytes(M, C)) return -4;
  float* part = (float*)ws;
  const dim3 grid((unsigned)((C + 255) / 256), (unsigned)nchunks);
  DISPATCH_BOOL(C % 4 == 0 && aligned16(dh) && aligned16(h) && aligned16(dpre), VEC,
                hipLaunchKernelGGL(relu_bias_bwd_kernel<VEC>, grid, dim3(64), 0, st, dh, h, M, C, dpre, part));
  SM_CHECK_LAUNCH();
  colred(part, (int)nchunks, C, nullptr, db, 0, st);
  SM_CHECK_LAUNCH();
  return 0;
}

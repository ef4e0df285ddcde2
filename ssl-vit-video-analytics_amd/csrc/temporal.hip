// Temporal SSL pretraining (the reference's src/train_ssl.py): the masked-frame objective, the
// teacher's EMA update, global-norm gradient clipping and the ReLU + dropout of the temporal
// layers' feed-forward.
//   mfm_loss_fwd/bwd   cosine_loss + variance_loss (train_ssl.py:26-34, :215-220) over the masked
//                      rows of pred / teacher, read in place through the index list: the gathered
//                      and normalised rows never exist in HBM
//   ema_update         update_ema (:36-39) over the two flat parameter buffers, one launch
//   grad_clip          torch.nn.utils.clip_grad_norm_ (:258-259) over the touched gradient ranges,
//                      the norm and the coefficient staying on the device
//   relu_dropout       nn.TransformerEncoderLayer's activation + dropout, mask from the counter hash
// No atomics, no MFMA; every reduction has a fixed partition and order (fp64 across rows, blocks
// and partials), so no result depends on the launch geometry and runs are bitwise reproducible.
// The loss kernels have a 16-byte form and a scalar form with the same element ownership and
// summation order: same bits from a misaligned view.  The file is compiled with -ffp-contract=off
// (build.py FILE_FLAGS): the only fused operations are the explicit fmaf calls, in both forms.
#include "common.h"
#include "sm_api.h"

namespace {

// ------------------------------------------------------------------ masked-frame loss
// A row of D elements is owned by one wave: lane l holds the groups g = l, l + 64, ... of V
// consecutive columns (V = 16 bytes of the pred dtype), accumulates over its elements in
// ascending order with explicit fmas, then the wave butterfly adds the 64 lane sums.
template <typename T> struct Own { static constexpr int V = 16 / sizeof(T); };

template <int V, bool VEC, typename TV>
SM_DEV void load_group(const TV* p, int c0, int D, float* v) {
  if constexpr (VEC) {
    if constexpr (V == 8) load8(p + c0, v);
    else load4(p + c0, v);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = c0 + j < D ? to_f<TV>(p[c0 + j]) : 0.f;
  }
}
template <int V, bool VEC, typename TV>
SM_DEV void store_group(TV* p, int c0, int D, const float* v) {
  if constexpr (VEC) {
    if constexpr (V == 8) store8(p + c0, v);
    else store4(p + c0, v);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (c0 + j < D) p[c0 + j] = from_f<TV>(v[j]);
  }
}

constexpr float kNormEps = 1e-12f;   // F.normalize's clamp

// rowstat [N][3] = 1 / max(|pred_i|, eps), 1 / max(|teacher_i|, eps), s_i . u_i; one wave per masked row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mfm_row_kernel(const T* __restrict__ pred, const float* __restrict__ teacher,
                                                      const int32_t* __restrict__ idx, int R, int N, int D,
                                                      float* __restrict__ rowstat) {
  constexpr int V = Own<T>::V;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;                                    // wave-uniform
  const int r = idx[i];
  if ((unsigned)r >= (unsigned)R) {                      // an index outside the matrix contributes nothing
    if (lane == 0) rowstat[i * 3] = rowstat[i * 3 + 1] = rowstat[i * 3 + 2] = 0.f;
    return;
  }
  const T* p = pred + (int64_t)r * D;
  const float* t = teacher + (int64_t)r * D;
  float pp = 0.f, tt = 0.f, pt = 0.f;
  for (int c0 = lane * V; c0 < D; c0 += 64 * V) {
    float a[V], b[V];
    load_group<V, VEC>(p, c0, D, a);
    load_group<V, VEC>(t, c0, D, b);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      pp = fmaf(a[j], a[j], pp);
      tt = fmaf(b[j], b[j], tt);
      pt = fmaf(a[j], b[j], pt);
    }
  }
  pp = wave_sum(pp);
  tt = wave_sum(tt);
  pt = wave_sum(pt);
  const float ip = 1.f / fmaxf(sqrtf(pp), kNormEps), it = 1.f / fmaxf(sqrtf(tt), kNormEps);
  if (lane == 0) {
    rowstat[i * 3] = ip;
    rowstat[i * 3 + 1] = it;
    rowstat[i * 3 + 2] = (pt * ip) * it;
  }
}

// Column sums of s and s^2 over one partition of kRowPart masked rows (rows ascending, fp64):
// part [nparts][2][D].  Thread = V consecutive columns; a column's sum does not depend on the grouping.
constexpr int kRowPart = 32;

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void mfm_col_kernel(const T* __restrict__ pred, const int32_t* __restrict__ idx,
                                                      int R, int N, int D, const float* __restrict__ rowstat,
                                                      double* __restrict__ part) {
  constexpr int V = Own<T>::V;
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * V;
  if (c0 >= D) return;
  const int i0 = blockIdx.y * kRowPart;
  const int i1 = i0 + kRowPart < N ? i0 + kRowPart : N;
  double s[V], q[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = q[j] = 0.0;
#pragma unroll 4
  for (int i = i0; i < i1; ++i) {
    const int r = idx[i];
    if ((unsigned)r >= (unsigned)R) continue;
    const float ip = rowstat[i * 3];
    float a[V];
    load_group<V, VEC>(pred + (int64_t)r * D, c0, D, a);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float sv = a[j] * ip;
      s[j] += (double)sv;
      q[j] += (double)sv * (double)sv;
    }
  }
  double* ps = part + (int64_t)blockIdx.y * 2 * D;
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (c0 + j < D) {
      ps[c0 + j] = s[j];
      ps[D + c0 + j] = q[j];
    }
}

// One block: the partitions in order per column, the hinge over the columns and the cosines over the
// rows as 256 strided fp64 sums that thread 0 adds in thread order.
// colstat [D][2] = mean_c, d var_loss / d s_ic / (s_ic - mean_c) = -[sigma_c < target] / (D N sigma_c)
__global__ __launch_bounds__(256) void mfm_final_kernel(const double* __restrict__ part, int nparts, int N, int D,
                                                        const float* __restrict__ rowstat, float w_mfm, float w_var,
                                                        float target_std, float eps, float* __restrict__ colstat,
                                                        float* __restrict__ out) {
  const int tid = threadIdx.x;
  double hs = 0.0, cs = 0.0;
  for (int c = tid; c < D; c += 256) {
    double S = 0.0, Q = 0.0;
    for (int pb = 0; pb < nparts; ++pb) {
      S += part[(int64_t)pb * 2 * D + c];
      Q += part[(int64_t)pb * 2 * D + D + c];
    }
    const double mean = S / N;
    double var = Q / N - mean * mean;
    if (var < 0.0) var = 0.0;
    const double sigma = sqrt(var + (double)eps);
    const double h = (double)target_std - sigma;
    if (h > 0.0) hs += h;
    colstat[c * 2] = (float)mean;
    colstat[c * 2 + 1] = h > 0.0 ? (float)(-1.0 / ((double)D * (double)N * sigma)) : 0.f;
  }
  for (int i = tid; i < N; i += 256) cs += (double)rowstat[i * 3 + 2];
  double v[2] = {hs, cs};
  thread_order_sum_d<2, SUM_THREAD0>(v);
  if (tid == 0) {
    const double mfm = 2.0 - 2.0 * v[1] / N, var = v[0] / D;
    out[0] = (float)mfm;
    out[1] = (float)var;
    out[2] = (float)((double)w_mfm * mfm + (double)w_var * var);
  }
}

// One wave per row of dpred.  A row outside idx (binary search: idx ascends) is zeroed; a masked row
// gets ds_c = g (w_mfm (-2 / N) u_c + w_var k_c (s_c - mean_c)) taken through the normalisation,
// dp = (ds - s (s . ds)) / |p|  (ds / eps where the norm was clamped, as F.normalize's backward).
template <typename T, typename TO, bool VEC>
__global__ __launch_bounds__(256) void mfm_bwd_kernel(const T* __restrict__ pred, const float* __restrict__ teacher,
                                                      const int32_t* __restrict__ idx, int R, int N, int D,
                                                      const float* __restrict__ rowstat,
                                                      const float* __restrict__ colstat,
                                                      const float* __restrict__ gout, float w_mfm, float w_var,
                                                      TO* __restrict__ dpred) {
  constexpr int V = Own<T>::V;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                    // wave-uniform
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  TO* dp = dpred + (int64_t)r * D;
  if (lo >= N || idx[lo] != r) {
    float z[V];
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = 0.f;
    for (int c0 = lane * V; c0 < D; c0 += 64 * V) store_group<V, VEC>(dp, c0, D, z);
    return;
  }
  const float ip = rowstat[lo * 3], it = rowstat[lo * 3 + 1];
  const float g = gout[0];
  const float ka = (g * w_mfm) * (-2.f / (float)N) * it, kb = g * w_var;
  const T* p = pred + (int64_t)r * D;
  const float* t = teacher + (int64_t)r * D;
  auto ds_of = [&](int c0, const float* a, const float* b, float* s, float* ds) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool in = c0 + j < D;
      const float mean = in ? colstat[(c0 + j) * 2] : 0.f, kc = in ? colstat[(c0 + j) * 2 + 1] : 0.f;
      s[j] = a[j] * ip;
      ds[j] = fmaf(ka, b[j], (kb * kc) * (s[j] - mean));
    }
  };
  float dot = 0.f;
  for (int c0 = lane * V; c0 < D; c0 += 64 * V) {
    float a[V], b[V], s[V], ds[V];
    load_group<V, VEC>(p, c0, D, a);
    load_group<V, VEC>(t, c0, D, b);
    ds_of(c0, a, b, s, ds);
#pragma unroll
    for (int j = 0; j < V; ++j) dot = fmaf(s[j], ds[j], dot);
  }
  dot = ip >= 1.f / kNormEps ? 0.f : wave_sum(dot);
  for (int c0 = lane * V; c0 < D; c0 += 64 * V) {
    float a[V], b[V], s[V], ds[V], o[V];
    load_group<V, VEC>(p, c0, D, a);
    load_group<V, VEC>(t, c0, D, b);
    ds_of(c0, a, b, s, ds);
#pragma unroll
    for (int j = 0; j < V; ++j) o[j] = ip * fmaf(-s[j], dot, ds[j]);
    store_group<V, VEC>(dp, c0, D, o);
  }
}

// ------------------------------------------------------------------ EMA
// dst = m dst + a src: the product rounded, then one fma (pe.mul_(m).add_(p, alpha=1 - m))
SM_DEV float ema1(float d, float s, float m, float a) {
  const float t = d * m;
  return fmaf(a, s, t);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n,
                                                  float m, float a) {
  const int64_t stride = (int64_t)gridDim.x * 256, t0 = blockIdx.x * (int64_t)256 + threadIdx.x;
  if constexpr (VEC) {
    const int64_t n4 = n / 4;
    for (int64_t i = t0; i < n4; i += stride) {
      const f32x4 d = *(const f32x4*)(dst + i * 4), s = *(const f32x4*)(src + i * 4);
      *(f32x4*)(dst + i * 4) = f32x4{ema1(d[0], s[0], m, a), ema1(d[1], s[1], m, a), ema1(d[2], s[2], m, a),
                                     ema1(d[3], s[3], m, a)};
    }
    const int64_t e = n4 * 4 + t0;                       // the tail of n % 4 elements
    if (e < n) dst[e] = ema1(dst[e], src[e], m, a);
  } else {
    for (int64_t i = t0; i < n; i += stride) dst[i] = ema1(dst[i], src[i], m, a);
  }
}

// ------------------------------------------------------------------ gradient clipping
// First level: block = one chunk of kClipChunk elements of one range (chunks counted from the
// range's start), thread t the elements (k 256 + t) 4 + j ascending, squares added in fp64; the wave
// butterfly, then the four waves in order.  Second level: one block over the partials.
constexpr int kClipChunk = 8192;
constexpr int kClipRanges = 16;

struct ClipRanges {
  int64_t start[kClipRanges], len[kClipRanges];
  int blk0[kClipRanges + 1];
  int n;
};

SM_DEV int clip_range_of(const ClipRanges& rg, int b) {
  int k = 0;
  while (k + 1 < rg.n && b >= rg.blk0[k + 1]) ++k;
  return k;
}

__global__ __launch_bounds__(256) void clip_sumsq_kernel(const float* __restrict__ grad, ClipRanges rg,
                                                         double* __restrict__ part) {
  const int k = clip_range_of(rg, blockIdx.x);
  const float* g = grad + rg.start[k];
  const int64_t e0 = (int64_t)(blockIdx.x - rg.blk0[k]) * kClipChunk;
  const int64_t e1 = e0 + kClipChunk < rg.len[k] ? e0 + kClipChunk : rg.len[k];
  const bool vec = aligned16(g);                     // block-uniform (e0 is a multiple of 4)
  double s[1] = {0.0};
  for (int64_t e = e0 + threadIdx.x * 4; e < e1; e += 1024) {
    float v[4];
    if (vec && e + 4 <= e1) load4(g + e, v);
    else
      for (int j = 0; j < 4; ++j) v[j] = e + j < e1 ? g[e + j] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[0] += (double)v[j] * (double)v[j];
  }
  block_sum4_d<1>(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

// norm = sqrt(sum), coef = clip_coef(max_norm, norm)
__global__ __launch_bounds__(256) void clip_final_kernel(const double* __restrict__ part, int nb, float max_norm,
                                                         float* __restrict__ norm_out, float* __restrict__ coef) {
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < nb; i += 256) s[0] += part[i];
  thread_order_sum_d<1, SUM_THREAD0>(s);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s[0]);
    norm_out[0] = norm;
    coef[0] = clip_coef(max_norm, norm);
  }
}

__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ grad, ClipRanges rg,
                                                         const float* __restrict__ coef) {
  const float c = coef[0];
  if (c == 1.f) return;                                  // g * 1 is g: nothing to write
  const int k = clip_range_of(rg, blockIdx.x);
  float* g = grad + rg.start[k];
  const int64_t e0 = (int64_t)(blockIdx.x - rg.blk0[k]) * kClipChunk;
  const int64_t e1 = e0 + kClipChunk < rg.len[k] ? e0 + kClipChunk : rg.len[k];
  const bool vec = aligned16(g);
  for (int64_t e = e0 + threadIdx.x * 4; e < e1; e += 1024) {
    if (vec && e + 4 <= e1) {
      const f32x4 v = *(const f32x4*)(g + e);
      *(f32x4*)(g + e) = f32x4{v[0] * c, v[1] * c, v[2] * c, v[3] * c};
    } else {
      for (int j = 0; j < 4 && e + j < e1; ++j) g[e + j] *= c;
    }
  }
}

int64_t clip_blocks(const int64_t* starts, const int64_t* ends, int nranges) {
  int64_t nb = 0;
  for (int i = 0; i < nranges; ++i) {
    if (starts[i] < 0 || ends[i] < starts[i]) return -1;
    nb += (ends[i] - starts[i] + kClipChunk - 1) / kClipChunk;
  }
  return nb;
}

// ------------------------------------------------------------------ ReLU + dropout
// 8 consecutive elements of one row (ncols % 8 == 0): keep multipliers from the counter hash with
// its 16-bit threshold (common.h: keep rate 0.899994 at p = 0.1, as nn.Dropout(0.1) to 6e-6)
SM_DEV void keep_mult8(int64_t e, int ncols, float drop_p, uint64_t seed, float* m) {
  const float ks = drop_scale16(drop_p);
  const int64_t row = e / ncols;
  const uint32_t c0 = (uint32_t)(e - row * ncols);
  const uint32_t rb = drop_rowbase(seed32(seed), (uint64_t)row), thr = drop_thr16(drop_p);
#pragma unroll
  for (int j2 = 0; j2 < 8; j2 += 2) {
    const uint32_t h = drop_hash16(rb, c0 + j2);         // c0 % 8 == 0
#pragma unroll
    for (int j = 0; j < 2; ++j) m[j2 + j] = drop_keep_bits16(h, (uint32_t)j, thr) ? ks : 0.f;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void relu_dropout_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                               int64_t total8, int ncols, float drop_p,
                                                               uint64_t seed) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total8; i += (int64_t)gridDim.x * 256) {
    float v[8], m[8];
    load8(x + i * 8, v);
    if (drop_p > 0.f) keep_mult8(i * 8, ncols, drop_p, seed, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float r = v[j] > 0.f ? v[j] : (v[j] == v[j] ? 0.f : v[j]);   // NaN stays NaN
      v[j] = drop_p > 0.f ? r * m[j] : r;
    }
    store8(y + i * 8, v);
  }
}

// dx = dy keep scale where ref > 0; ref is the forward's input or its output (the output is
// positive exactly where the input was positive and kept)
template <typename T>
__global__ __launch_bounds__(256) void relu_dropout_bwd_kernel(const T* __restrict__ ref, const T* __restrict__ dy,
                                                               T* __restrict__ dx, int64_t total8, int ncols,
                                                               float drop_p, uint64_t seed) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total8; i += (int64_t)gridDim.x * 256) {
    float v[8], d[8], m[8];
    load8(ref + i * 8, v);
    load8(dy + i * 8, d);
    if (drop_p > 0.f) keep_mult8(i * 8, ncols, drop_p, seed, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = v[j] > 0.f ? (drop_p > 0.f ? d[j] * m[j] : d[j]) : 0.f;
    store8(dx + i * 8, d);
  }
}

template <typename T>
int mfm_fwd(const T* pred, const float* teacher, const int32_t* idx, int R, int N, int D, float w_mfm, float w_var,
            float target_std, float eps, float* out, float* stats, double* part, hipStream_t st) {
  constexpr int V = Own<T>::V;
  const bool vec = D % V == 0 && aligned16(pred) && aligned16(teacher);
  float* rowstat = stats;
  float* colstat = stats + (int64_t)N * 3;
  const int nparts = (N + kRowPart - 1) / kRowPart;
  const dim3 rgrid((unsigned)((N + 3) / 4)), cgrid((unsigned)((D + 256 * V - 1) / (256 * V)), (unsigned)nparts);
  DISPATCH_BOOL(vec, VEC, {
    hipLaunchKernelGGL((mfm_row_kernel<T, VEC>), rgrid, dim3(256), 0, st, pred, teacher, idx, R, N, D, rowstat);
    hipLaunchKernelGGL((mfm_col_kernel<T, VEC>), cgrid, dim3(256), 0, st, pred, idx, R, N, D, rowstat, part);
  });
  hipLaunchKernelGGL(mfm_final_kernel, dim3(1), dim3(256), 0, st, part, nparts, N, D, rowstat, w_mfm, w_var,
                     target_std, eps, colstat, out);
  return 0;
}

template <typename T, typename TO>
void mfm_bwd(const T* pred, const float* teacher, const int32_t* idx, int R, int N, int D, const float* stats,
             const float* gout, float w_mfm, float w_var, TO* dpred, hipStream_t st) {
  constexpr int V = Own<T>::V;
  const bool vec = D % V == 0 && aligned16(pred) && aligned16(teacher) && aligned16(dpred);
  const dim3 grid((unsigned)((R + 3) / 4));
  DISPATCH_BOOL(vec, VEC,
                hipLaunchKernelGGL((mfm_bwd_kernel<T, TO, VEC>), grid, dim3(256), 0, st, pred, teacher, idx, R, N, D,
                                   stats, stats + (int64_t)N * 3, gout, w_mfm, w_var, dpred));
}

bool mfm_shape_ok(int pred_dtype, int R, int N, int D) {
  return (pred_dtype == SM_F32 || pred_dtype == SM_BF16) && R > 0 && N > 0 && D > 0 && N <= R &&
         (int64_t)N * 3 <= 0x7fffffff && (int64_t)D * 2 <= 0x7fffffff && (N + kRowPart - 1) / kRowPart <= 65535;
}

}  // namespace

extern "C" int64_t sm_mfm_loss_workspace_bytes(int N, int D) {
  if (N <= 0 || D <= 0) return 0;
  return (int64_t)((N + kRowPart - 1) / kRowPart) * 2 * D * (int64_t)sizeof(double);
}

extern "C" int sm_mfm_loss_fwd(int pred_dtype, const void* pred, const float* teacher, const int32_t* idx, int R,
                               int N, int D, float w_mfm, float w_var, float target_std, float eps, float* out,
                               float* stats, void* ws, int64_t ws_bytes, hipStream_t st) {
  if (!mfm_shape_ok(pred_dtype, R, N, D) || !pred || !teacher || !idx || !out || !stats) return -2;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < sm_mfm_loss_workspace_bytes(N, D)) return -4;
  DISPATCH1(pred_dtype, mfm_fwd<T>((const T*)pred, teacher, idx, R, N, D, w_mfm, w_var, target_std, eps, out, stats,
                                   (double*)ws, st));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_mfm_loss_bwd(int pred_dtype, int dpred_dtype, const void* pred, const float* teacher,
                               const int32_t* idx, int R, int N, int D, const float* stats, const float* grad_out,
                               float w_mfm, float w_var, void* dpred, hipStream_t st) {
  if (!mfm_shape_ok(pred_dtype, R, N, D) || (dpred_dtype != SM_F32 && dpred_dtype != SM_BF16) || !pred || !teacher ||
      !idx || !stats || !grad_out || !dpred)
    return -2;
  DISPATCH2(pred_dtype, dpred_dtype, mfm_bwd<T1, T2>((const T1*)pred, teacher, idx, R, N, D, stats, grad_out, w_mfm,
                                                     w_var, (T2*)dpred, st));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_ema_update(float* dst, const float* src, int64_t n, float mf, float af, hipStream_t st) {
  if (n < 0) return -2;
  if (n == 0) return 0;
  if (!dst || !src) return -2;
  DISPATCH_BOOL(aligned16(dst) && aligned16(src), VEC,
                hipLaunchKernelGGL(ema_kernel<VEC>, dim3(ew_grid(VEC ? (n + 3) / 4 : n)), dim3(256), 0, st, dst, src,
                                   n, mf, af));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_grad_clip_workspace_bytes(const int64_t* starts, const int64_t* ends, int nranges) {
  if (nranges < 0 || (nranges > 0 && (!starts || !ends))) return -1;
  const int64_t nb = clip_blocks(starts, ends, nranges);
  return nb < 0 ? -1 : (nb + 1) * (int64_t)sizeof(double);
}

extern "C" int sm_grad_clip(float* grad, const int64_t* starts, const int64_t* ends, int nranges, float max_norm,
                            float* norm_out, void* ws, int64_t ws_bytes, hipStream_t st) {
  if (nranges < 0 || !norm_out || (nranges > 0 && (!grad || !starts || !ends))) return -2;
  const int64_t nb = clip_blocks(starts, ends, nranges);
  if (nb < 0 || nb > 0x7fffffff) return -2;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < (nb + 1) * (int64_t)sizeof(double)) return -4;
  double* part = (double*)ws;
  float* coef = (float*)(part + nb);
  // the non-empty ranges in groups of kClipRanges per launch, each range in exactly one group (one
  // index walks all of them); a group's partials follow the previous group's
  for (int pass = 0; pass < 2; ++pass) {
    int64_t done = 0;
    for (int i = 0; i < nranges;) {
      ClipRanges rg;
      rg.n = 0;
      rg.blk0[0] = 0;
      for (; i < nranges && rg.n < kClipRanges; ++i) {
        const int64_t len = ends[i] - starts[i];
        if (len == 0) continue;
        rg.start[rg.n] = starts[i];
        rg.len[rg.n] = len;
        rg.blk0[rg.n + 1] = rg.blk0[rg.n] + (int)((len + kClipChunk - 1) / kClipChunk);
        ++rg.n;
      }
      if (rg.n == 0) continue;
      const unsigned grid = (unsigned)rg.blk0[rg.n];
      if (done + grid > nb) return -2;                     // (cannot happen: nb counts the same chunks)
      if (pass == 0)
        hipLaunchKernelGGL(clip_sumsq_kernel, dim3(grid), dim3(256), 0, st, grad, rg, part + done);
      else
        hipLaunchKernelGGL(clip_scale_kernel, dim3(grid), dim3(256), 0, st, grad, rg, coef);
      done += grid;
    }
    if (pass == 0)
      hipLaunchKernelGGL(clip_final_kernel, dim3(1), dim3(256), 0, st, part, (int)nb, max_norm, norm_out, coef);
  }
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_relu_dropout_fwd(int dtype, int64_t n, int ncols, const void* x, void* y, float drop_p,
                                   uint64_t seed, hipStream_t st) {
  if ((dtype != SM_F32 && dtype != SM_BF16) || n < 0 || ncols <= 0 || ncols % 8 || n % ncols || !(drop_p >= 0.f) ||
      drop_p > 1.f)
    return -2;
  if (n == 0) return 0;
  if (!x || !y || !aligned16(x) || !aligned16(y)) return -2;
  DISPATCH1(dtype, hipLaunchKernelGGL(relu_dropout_fwd_kernel<T>, dim3(ew_grid(n / 8)), dim3(256), 0, st,
                                      (const T*)x, (T*)y, n / 8, ncols, drop_p, seed));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_relu_dropout_bwd(int dtype, int64_t n, int ncols, const void* ref, const void* dy, void* dx,
                                   float drop_p, uint64_t seed, hipStream_t st) {
  if ((dtype != SM_F32 && dtype != SM_BF16) || n < 0 || ncols <= 0 || ncols % 8 || n % ncols || !(drop_p >= 0.f) ||
      drop_p > 1.f)
    return -2;
  if (n == 0) return 0;
  if (!ref || !dy || !dx || !aligned16(ref) || !aligned16(dy) || !aligned16(dx)) return -2;
  DISPATCH1(dtype, hipLaunchKernelGGL(relu_dropout_bwd_kernel<T>, dim3(ew_grid(n / 8)), dim3(256), 0, st,
                                      (const T*)ref, (const T*)dy, (T*)dx, n / 8, ncols, drop_p, seed));
  SM_CHECK_LAUNCH();
  return 0;
}

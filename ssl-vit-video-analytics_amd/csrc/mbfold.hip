// BN0's backward dx map folded into the MBConv expand conv's gradient GEMMs (tiny_vit.py:43-48).
//
// With a1 = x W^T (the expand conv), xhat = (a1 - mu) rho and the first depthwise-backward
// pass's dz and coef = (k0, k1) = (mean dz, mean dz xhat), the BatchNorm's data gradient is
//   da1 = gamma rho (dz - k0 - xhat k1) = omega dz - delta a1 + c          per channel, with
//   omega = gamma rho,  delta = omega rho k1,  c = omega (rho k1 mu - k0).
// Its two consumers are GEMMs whose other side is Cin = mid / 4 wide, so the map goes into
// their weights and da1 is never written (sm_dwconv_bn_bwd's streaming dx pass: two reads and
// one write of the block's largest tensor):
//   dX  = da1 W     = dz W' - x T + r0,   W' = diag(omega) W,  T = W^T diag(delta) W,  r0 = c^T W
//   dW += da1^T x   = diag(omega) P - diag(delta) (W G) + c s^T,   P = dz^T x, G = x^T x, s = sum_m x
// sm_mbconv_fold_prep writes the stacked data-gradient weight [W'; -T] (sm_linear_dx2's B
// operand), r0 (its bias) and the three vectors; sm_mbconv_fold_dw combines P, G and s into the
// weight gradient (fp64: c s^T and diag(delta) W G cancel to the BatchNorm's zero-mean da1).
// Block input stored before its own BatchNorm (x = BN(xs) = xs sc + sh formed on load elsewhere,
// the stem's folded BN2): the data-gradient GEMM and G / s read the stored xs, and the affine
// goes into the small factors: x T = xs (diag(sc) T) + sh T, G = diag(sc) Gs diag(sc) +
// (sc ss) sh^T + sh (sc ss)^T + M sh sh^T, s = sc ss + M sh.
#include "common.h"

namespace {

constexpr int MBF_MAXMID = 2048, MBF_MAXCIN = 1024;

// blocks [0, mid): W' row + the vectors; [mid, mid + Cin): -T row; mid + Cin: r0
__global__ __launch_bounds__(256) void mbconv_fold_prep_kernel(int mid, int Cin, const float* coef, const float* mean,
                                                               const float* rstd, const float* gamma, const __bf16* W,
                                                               ChanAffine xbn, __bf16* wst, float* r0, float* vec) {
  __shared__ float tab[MBF_MAXMID];
  const int b = blockIdx.x, t = threadIdx.x;
  if (b < mid) {
    const float rho = rstd[b], om = gamma[b] * rho, k1 = coef[mid + b];
    for (int j = t; j < Cin; j += 256) wst[(int64_t)b * Cin + j] = (__bf16)(om * (float)W[(int64_t)b * Cin + j]);
    if (t == 0) {
      vec[b] = om;
      vec[mid + b] = om * rho * k1;
      vec[2 * mid + b] = om * (rho * k1 * mean[b] - coef[b]);
    }
    return;
  }
  for (int c = t; c < mid; c += 256) {   // delta
    const float rho = rstd[c];
    tab[c] = gamma[c] * rho * rho * coef[mid + c];
  }
  __syncthreads();
  if (b < mid + Cin) {
    const int i = b - mid;
    const float sc = xbn.mean ? xbn.rstd[i] * xbn.w[i] : 1.f;
    for (int j = t; j < Cin; j += 256) {
      float acc = 0.f;
      for (int c = 0; c < mid; ++c) acc = fmaf(tab[c] * (float)W[(int64_t)c * Cin + i], (float)W[(int64_t)c * Cin + j], acc);
      wst[(int64_t)b * Cin + j] = (__bf16)(-sc * acc);
    }
    return;
  }
  // r0[j] = sum_c W[c][j] (c_c - delta_c u_c),  u_c = sum_i sh_i W[c][i] (the input BatchNorm's shift)
  for (int c = t; c < mid; c += 256) {
    double u = 0.0;
    if (xbn.mean)
      for (int i = 0; i < Cin; ++i) {
        const float sci = xbn.rstd[i] * xbn.w[i];
        u += (double)bn_shift(xbn.b[i], xbn.mean[i], sci) * (double)(float)W[(int64_t)c * Cin + i];
      }
    const float rho = rstd[c], om = gamma[c] * rho;
    const double cc = (double)om * ((double)rho * coef[mid + c] * mean[c] - (double)coef[c]);
    tab[c] = (float)(cc - (double)tab[c] * u);   // this thread's own entry
  }
  __syncthreads();
  for (int j = t; j < Cin; j += 256) {
    double acc = 0.0;
    for (int c = 0; c < mid; ++c) acc += (double)tab[c] * (double)(float)W[(int64_t)c * Cin + j];
    r0[j] = (float)acc;
  }
}

// dW[c][j] += omega_c P[c][j] + c_c s[j] - delta_c sum_i W[c][i] G[i][j]   (one block per row c)
__global__ __launch_bounds__(256) void mbconv_fold_dw_kernel(int mid, int Cin, double M, const float* vec,
                                                             const __bf16* W, const float* P, const float* G,
                                                             const float* s, ChanAffine xbn, float* dW) {
  __shared__ float wa[MBF_MAXCIN];   // W[c][i] sc_i
  const int c = blockIdx.x, t = threadIdx.x;
  double a[2] = {0.0, 0.0};   // sum_i W[c][i] sc_i ss_i,  sum_i W[c][i] sh_i
  for (int i = t; i < Cin; i += 256) {
    const float w = (float)W[(int64_t)c * Cin + i];
    const float sc = xbn.mean ? xbn.rstd[i] * xbn.w[i] : 1.f;
    wa[i] = w * sc;
    a[0] += (double)wa[i] * (double)s[i];
    if (xbn.mean) a[1] += (double)w * (double)bn_shift(xbn.b[i], xbn.mean[i], sc);
  }
  thread_order_sum_d<2, SUM_EVERY_THREAD>(a);   // (its barrier also publishes wa)
  const double a1 = a[0], a2 = a[1];
  const double om = vec[c], dl = vec[mid + c], cc = vec[2 * mid + c];
  for (int j = t; j < Cin; j += 256) {
    double wg = 0.0;
    for (int i = 0; i < Cin; ++i) wg += (double)wa[i] * (double)G[(int64_t)i * Cin + j];
    double sj = s[j];
    if (xbn.mean) {
      const float sc = xbn.rstd[j] * xbn.w[j];
      const double sh = bn_shift(xbn.b[j], xbn.mean[j], sc);
      sj = (double)sc * sj + M * sh;
      wg = (double)sc * wg + a1 * sh + a2 * sj;
    }
    const int64_t e = (int64_t)c * Cin + j;
    dW[e] += (float)(om * (double)P[e] + cc * sj - dl * wg);
  }
}

bool xbn_ok(const float* m, const float* r, const float* w, const float* b) {
  return (m == nullptr) == (r == nullptr) && (m == nullptr) == (w == nullptr) && (m == nullptr) == (b == nullptr);
}

}  // namespace

extern "C" int sm_mbconv_fold_prep(int mid, int Cin, const float* coef, const float* bn_mean, const float* bn_rstd,
                                   const float* bn_w, const void* w, const float* x_mean, const float* x_rstd,
                                   const float* x_w, const float* x_b, void* wst, float* r0, float* vec,
                                   hipStream_t st) {
  if (mid <= 0 || Cin <= 0 || mid > MBF_MAXMID || Cin > MBF_MAXCIN || !coef || !bn_mean || !bn_rstd || !bn_w || !w ||
      !wst || !r0 || !vec || !xbn_ok(x_mean, x_rstd, x_w, x_b))
    return -2;
  ChanAffine xbn{x_mean, x_rstd, x_w, x_b, 0};
  hipLaunchKernelGGL(mbconv_fold_prep_kernel, dim3(mid + Cin + 1), dim3(256), 0, st, mid, Cin, coef, bn_mean, bn_rstd,
                     bn_w, (const __bf16*)w, xbn, (__bf16*)wst, r0, vec);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_mbconv_fold_dw(int mid, int Cin, int64_t M, const float* vec, const void* w, const float* P,
                                 const float* G, const float* s, const float* x_mean, const float* x_rstd,
                                 const float* x_w, const float* x_b, float* dW, hipStream_t st) {
  if (mid <= 0 || Cin <= 0 || mid > MBF_MAXMID || Cin > MBF_MAXCIN || M <= 0 || !vec || !w || !P || !G || !s || !dW ||
      !xbn_ok(x_mean, x_rstd, x_w, x_b))
    return -2;
  ChanAffine xbn{x_mean, x_rstd, x_w, x_b, 0};
  hipLaunchKernelGGL(mbconv_fold_dw_kernel, dim3(mid), dim3(256), 0, st, mid, Cin, (double)M, vec, (const __bf16*)w, P,
                     G, s, xbn, dW);
  SM_CHECK_LAUNCH();
  return 0;
}

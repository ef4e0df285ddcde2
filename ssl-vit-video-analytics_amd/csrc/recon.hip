// MAE reconstruction evaluation (the reference's src/visualize_mae.py:162-208 and the token-error
// map of src/mae/visualize.py:47-58): from the decoder's prediction, the clip and the mask, one
// launch writes the [ original | masked original | reconstruction ] strips as bytes ready for
// PNG, the display-space reconstruction and the per-token errors; a second, one block per clip,
// reduces the errors to the clip's metrics.  The target and the reconstruction never exist as
// token tensors: pred, clip and mask are read once.
//
// One wave per four consecutive tokens, lane = pixel column: lane bits 0..2 are the patch column
// q, bits 3..4 the token of the four, bit 5 the row half h; the lane walks the patch rows
// p = 2 k + h, k = 0..3, and owns the three features f = (p * 8 + q) * 3 + c of each, which are
// the three bytes of one HWC pixel.  Where the four tokens share an image row (always, when
// W % 32 == 0) one access of the wave covers two image rows of 32 pixels: 128 contiguous bytes of
// a clip or recon plane, 96 of a panel, instead of the eight 32-byte pieces of a wave per token.
// Tokens are taken as they come, so a group that wraps to the next patch row, or a tail of fewer
// than four (its lanes repeat the last token and store nothing), is only less contiguous.
//   panels  a token row's 24 bytes are six dwords: every lane packs its pixel into 24 bits, takes
//           the next lane's through one cross-lane move, and lanes 0..2 of each four store a dword
//           (d_j = w_j >> 8 j | w_{j+1} << (24 - 8 j)); a panels base that is not 4-byte aligned
//           takes nine byte stores per pixel.  Same bytes either way.
// A token's reductions (mean / variance, the two errors) are per-lane sums over k and c, then a
// butterfly over its 16 lanes: a fixed order, so the outputs are bitwise reproducible.
#include "common.h"
#include "sm_api.h"

namespace {

struct ReconArgs {
  const void* pred;          // [B][T*L][192]
  const float* clip;         // [B][3][T][H][W] via strides
  int64_t sB, sC, sT, sH, sW;
  const uint8_t* mask;       // [B][T][L]
  int T, H, W, L, wp;
  int norm_pix, paste_visible, bgr_swap;
  float mean[3], std[3];     // of clip channel c (the source channel's constants)
  uint8_t* panels;           // [B][T][H][3*W][3]
  float* recon;              // [B][3][T][H][W], nullable
  float* token_err;          // [B*T*L][2]
};

SM_DEV float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
SM_DEV uint32_t level(float v) { return (uint32_t)(clamp01(v) * 255.f); }   // floor: the operand is >= 0

// sum over the 16 lanes of one token: lane bits 0..2 (q) and 5 (row half)
SM_DEV float token_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <typename TP, bool PACK>
__global__ __launch_bounds__(256) void reconstruct_kernel(ReconArgs a, int64_t ntok) {
  const int lane = threadIdx.x & 63;
  const int64_t tok0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (tok0 >= ntok) return;                              // wave-uniform
  const int q = lane & 7, h = lane >> 5;
  const bool live = tok0 + ((lane >> 3) & 3) < ntok;     // a tail lane repeats the last token and stores nothing
  const int64_t tok = live ? tok0 + ((lane >> 3) & 3) : ntok - 1;
  const int TL = a.T * a.L;
  const int b = (int)(tok / TL);
  const int rem = (int)(tok % TL);
  const int t = rem / a.L, l = rem % a.L;
  const int hi = l / a.wp, wi = l % a.wp;
  const int col = wi * 8 + q;
  const float* src = a.clip + b * a.sB + t * a.sT + (int64_t)(hi * 8 + h) * a.sH + (int64_t)col * a.sW;
  const TP* pred = (const TP*)a.pred + tok * 192 + (h * 8 + q) * 3;
  float x[4][3], pr[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                          // patch row p = 2 k + h
#pragma unroll
    for (int c = 0; c < 3; ++c) x[k][c] = src[(int64_t)(2 * k) * a.sH + c * a.sC];
#pragma unroll
    for (int c = 0; c < 3; ++c) pr[k][c] = to_f<TP>(pred[(2 * k * 8) * 3 + c]);
  }
  const bool masked = a.mask[tok] != 0;

  // target (token_terms of mae.hip) and the reconstruction in clip space
  float mu = 0.f, sd = 1.f, inv = 1.f;
  if (a.norm_pix) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += x[k][0] + x[k][1] + x[k][2];
    mu = token_sum(s) / 192.f;
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) { const float d = x[k][c] - mu; ss += d * d; }
    const float var = token_sum(ss) / 191.f;
    sd = sqrtf(var + 1e-6f);
    inv = 1.f / sd;
  }

  float en = 0.f, ep = 0.f;
  const int64_t frame = (int64_t)b * a.T + t;
  const int64_t hw = (int64_t)a.H * a.W, W3 = 3 * (int64_t)a.W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = hi * 8 + 2 * k + h;
    float vo[3], vr[3];                                  // display values: original, output
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xc = x[k][c], pc = pr[k][c];
      const float tgt = a.norm_pix ? (xc - mu) * inv : xc;
      const float r = a.norm_pix ? pc * sd + mu : pc;
      const float dn = pc - tgt;
      en += dn * dn;
      vo[c] = xc * a.std[c] + a.mean[c];
      const float v = r * a.std[c] + a.mean[c];
      // v - vo = (r - x) std = (pred - tgt) sd std: where neither value clamps, the difference is formed
      // from dn, not from two display values that may agree in most of their digits
      const bool inside = v >= 0.f && v <= 1.f && vo[c] >= 0.f && vo[c] <= 1.f;
      const float dp = inside ? dn * sd * a.std[c] : clamp01(v) - clamp01(vo[c]);
      ep += dp * dp;
      vr[c] = a.paste_visible && !masked ? vo[c] : v;    // a visible token shows the clip itself
    }
    if (a.recon && live) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = a.bgr_swap ? 2 - c : c;
        a.recon[(((int64_t)b * 3 + s) * a.T + t) * hw + (int64_t)row * a.W + col] = vr[c];
      }
    }
    // the pixel as 24 bits, byte s = RGB position s, for the three panels
    uint32_t wo = 0, wr = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int sh = 8 * (a.bgr_swap ? 2 - c : c);
      wo |= level(vo[c]) << sh;
      wr |= level(vr[c]) << sh;
    }
    const uint32_t wm = masked ? 0u : wo;
    uint8_t* dst = a.panels + (frame * a.H + row) * (3 * W3);   // the strip's row: 3 panels of 3 W bytes
    if constexpr (PACK) {
      // (next lane's pixel; lane 3 of each four stores nothing, so no value crosses a token's row)
      const uint32_t no = __shfl_down(wo, 1, 64), nm = __shfl_down(wm, 1, 64), nr = __shfl_down(wr, 1, 64);
      const int j = lane & 3;
      if (j < 3 && live) {
        const int dn = 8 * j, up = 24 - 8 * j;
        uint32_t* d = (uint32_t*)(dst + wi * 24 + (q >> 2) * 12 + j * 4);
        d[0] = (wo >> dn) | (no << up);
        *(uint32_t*)((uint8_t*)d + W3) = (wm >> dn) | (nm << up);
        *(uint32_t*)((uint8_t*)d + 2 * W3) = (wr >> dn) | (nr << up);
      }
    } else if (live) {
      uint8_t* d = dst + col * 3;
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        d[s] = (uint8_t)(wo >> (8 * s));
        d[W3 + s] = (uint8_t)(wm >> (8 * s));
        d[2 * W3 + s] = (uint8_t)(wr >> (8 * s));
      }
    }
  }
  en = token_sum(en) / 192.f;
  ep = token_sum(ep) / 192.f;
  if (q == 0 && h == 0 && live) {
    a.token_err[tok * 2] = en;
    a.token_err[tok * 2 + 1] = ep;
  }
}

// One block per clip: thread t takes tokens t, t + 256, ... ascending in fp64, then thread 0 adds
// the 256 partials in thread order.
__global__ __launch_bounds__(256) void clip_metrics_kernel(const float* __restrict__ token_err,
                                                           const uint8_t* __restrict__ mask, int64_t TL,
                                                           float* __restrict__ out) {
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * TL;
  double v[3] = {0.0, 0.0, 0.0};                         // sums of the two errors, masked tokens
  for (int64_t i = tid; i < TL; i += 256) {
    if (mask[t0 + i]) {
      v[0] += (double)token_err[(t0 + i) * 2];
      v[1] += (double)token_err[(t0 + i) * 2 + 1];
      v[2] += 1.0;
    }
  }
  thread_order_sum_d<3, SUM_THREAD0>(v);
  if (tid == 0) {
    const double sn = v[0], sp = v[1], n = v[2];
    const double en = n > 0.0 ? sn / n : 0.0, mse = n > 0.0 ? sp / n : 0.0;
    float* o = out + (int64_t)blockIdx.x * 4;
    o[0] = (float)en;
    o[1] = (float)mse;
    o[2] = mse > 0.0 ? (float)(10.0 * log10(1.0 / mse)) : INFINITY;
    o[3] = (float)n;
  }
}

}  // namespace

extern "C" int sm_mae_reconstruct(int pred_dtype, const void* pred, const float* clip, int64_t sB, int64_t sC,
                                  int64_t sT, int64_t sH, int64_t sW, const uint8_t* mask, int B, int T, int H, int W,
                                  const float* mean3, const float* std3, int norm_pix, int paste_visible,
                                  int bgr_swap, uint8_t* panels, float* recon, float* token_err, hipStream_t st) {
  if (B < 0 || T < 0 || H < 0 || W < 0 || H % 8 || W % 8 || (pred_dtype != SM_F32 && pred_dtype != SM_BF16))
    return -2;
  const int64_t L = (int64_t)(H / 8) * (W / 8), ntok = (int64_t)B * T * L;
  if (ntok == 0) return 0;
  if (!pred || !clip || !mask || !mean3 || !std3 || !panels || !token_err) return -2;
  const int64_t nblk = (ntok + 15) / 16;
  if ((int64_t)T * L > 0x7fffffff || nblk > 0x7fffffff) return -2;
  ReconArgs a;
  a.pred = pred; a.clip = clip; a.sB = sB; a.sC = sC; a.sT = sT; a.sH = sH; a.sW = sW; a.mask = mask;
  a.T = T; a.H = H; a.W = W; a.L = (int)L; a.wp = W / 8;
  a.norm_pix = norm_pix; a.paste_visible = paste_visible; a.bgr_swap = bgr_swap;
  for (int c = 0; c < 3; ++c) {                      // (mean3 / std3 are host arrays, by RGB position)
    const int s = bgr_swap ? 2 - c : c;
    a.mean[c] = mean3[s];
    a.std[c] = std3[s];
  }
  a.panels = panels; a.recon = recon; a.token_err = token_err;
  DISPATCH_BOOL(((uintptr_t)panels & 3) == 0, PACK,
                DISPATCH1(pred_dtype, hipLaunchKernelGGL((reconstruct_kernel<T, PACK>), dim3((unsigned)nblk), dim3(256),
                                                         0, st, a, ntok)));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_recon_clip_metrics(const float* token_err, const uint8_t* mask, int B, int T, int L, float* out,
                                     hipStream_t st) {
  if (B < 0 || T < 0 || L < 0) return -2;
  if (B == 0) return 0;
  if (!token_err || !mask || !out) return -2;
  hipLaunchKernelGGL(clip_metrics_kernel, dim3((unsigned)B), dim3(256), 0, st, token_err, mask, (int64_t)T * L, out);
  SM_CHECK_LAUNCH();
  return 0;
}

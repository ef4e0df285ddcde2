// Mixing regularisation for fine-tuning: Mixup and CutMix of a batch of clips with its own flip,
// one pass over the batch (the eager form x * lam + x.flip(0) * (1 - lam) plus a box paste makes
// four or five).  The reference has no augmentation; the pairing is the usual batch-flip rule.
//
// x, out : fp32 [B][planes][H][W] contiguous (planes = 3 * T; only the product matters)
// pair p < P = B / 2 is the clips p and B - 1 - p; lam_px fp32 [P]; box int32 [P][4] = (y0, x0, h, w)
//
// Per element, a the clip's own pixel and q its partner's pixel at the same position:
//   inside the pair's box (rows [y0, y0 + h) x columns [x0, x0 + w) of EVERY plane, so of every
//   frame: clip-consistent)            out = q
//   outside, lam_px == 1               out = a            (a select: a NaN or inf in q stays out)
//   outside, otherwise                 out = fl(fl(lam a) + fl(fl(1 - lam) q))
// Both clips of a pair share lam_px and the box; the middle clip of an odd batch is copied.  Every
// operation is rounded on its own (this file is built with -ffp-contract=off), so tests/mix_mirror.py
// restates it bit for bit.
//
// One thread owns the same element (or 4 consecutive ones) of BOTH clips of a pair: it loads the
// two values, then stores the two results.  Every source element is read once and every output
// element written once, by the one thread that read it, which is what makes out == x legal.
// 16-byte accesses when W % 4 == 0 and both pointers are 16-byte aligned (a vector then lies in
// one row; a box edge may cut it, hence the per-lane select), scalar ones otherwise: same bits.
// The box is only ever a predicate on (row, column), never an address: a table entry that leaves
// the frame cannot make the kernel touch memory outside x and out.
#include "common.h"
#include "sm_api.h"

namespace {

constexpr int kThreads = 256;

struct PairRule {
  float lam, oml;           // lam_px and fl(1 - lam_px)
  int y0, y1, x0, x1;       // the box's rows [y0, y1) and columns [x0, x1); empty: y1 <= y0
};

SM_DEV float mix_one(float a, float q, bool inside, const PairRule& r) {
  if (inside) return q;
  if (r.lam == 1.0f) return a;
  return r.lam * a + r.oml * q;
}

// grid.y = pair (y == P: the middle clip of an odd batch); grid.x strides over the clip's n
// elements (VEC: its n / 4 vectors).  n = planes * H * W < 2^31, HW = H * W.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void clip_mix_kernel(const float* x, int64_t B, int n, int HW, int W,
                                                            const float* __restrict__ lam_px,
                                                            const int32_t* __restrict__ box, float* out) {
  const int64_t P = B >> 1, pr = blockIdx.y;
  const int items = VEC ? n >> 2 : n;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t first = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (pr == P) {                                          // block-uniform: the unpaired clip
    const float* src = x + pr * n;
    float* dst = out + pr * n;
    if (src == dst) return;
    for (int64_t i = first; i < items; i += stride) {
      if constexpr (VEC) __builtin_nontemporal_store(*(const f32x4*)(src + 4 * i), (f32x4*)(dst + 4 * i));
      else dst[i] = src[i];
    }
    return;
  }
  PairRule r;
  r.lam = lam_px[pr];
  r.oml = 1.0f - r.lam;
  const int32_t* bx = box + pr * 4;
  r.y0 = bx[0];
  r.x0 = bx[1];
  r.y1 = r.y0 + bx[2];
  r.x1 = r.x0 + bx[3];
  const bool has_box = bx[2] > 0 && bx[3] > 0;            // block-uniform
  const float *xa = x + pr * n, *xb = x + (B - 1 - pr) * n;
  float *oa = out + pr * n, *ob = out + (B - 1 - pr) * n;
  for (int64_t i = first; i < items; i += stride) {
    if constexpr (VEC) {
      const f32x4 a = *(const f32x4*)(xa + 4 * i), q = *(const f32x4*)(xb + 4 * i);
      int col = 0;
      bool row_in = false;
      if (has_box) {
        const unsigned pos = (unsigned)(4 * i) % (unsigned)HW;
        const int y = (int)(pos / (unsigned)W);
        col = (int)pos - y * W;
        row_in = y >= r.y0 && y < r.y1;
      }
      f32x4 ra, rb;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool inside = row_in && col + j >= r.x0 && col + j < r.x1;
        ra[j] = mix_one(a[j], q[j], inside, r);
        rb[j] = mix_one(q[j], a[j], inside, r);
      }
      __builtin_nontemporal_store(ra, (f32x4*)(oa + 4 * i));
      __builtin_nontemporal_store(rb, (f32x4*)(ob + 4 * i));
    } else {
      const float a = xa[i], q = xb[i];
      bool inside = false;
      if (has_box) {
        const unsigned pos = (unsigned)i % (unsigned)HW;
        const int y = (int)(pos / (unsigned)W), col = (int)pos - y * W;
        inside = y >= r.y0 && y < r.y1 && col >= r.x0 && col < r.x1;
      }
      oa[i] = mix_one(a, q, inside, r);
      ob[i] = mix_one(q, a, inside, r);
    }
  }
}

}  // namespace

extern "C" int sm_clip_mix(const float* x, int64_t B, int64_t planes, int H, int W, const float* lam_px,
                           const int32_t* box, float* out, hipStream_t st) {
  if (B == 0) return 0;
  if (B < 0 || planes <= 0 || H <= 0 || W <= 0 || !x || !out) return -2;
  const int64_t P = B / 2, rows = P + (B & 1);
  if (P > 0 && (!lam_px || !box)) return -2;
  const int64_t HW = (int64_t)H * W;
  if (planes > 0x7fffffffLL / HW || rows > 65535) return -2;      // n < 2^31; grid.y
  const int n = (int)(planes * HW);
  DISPATCH_BOOL(W % 4 == 0 && aligned16(x) && aligned16(out), VEC, {
    const dim3 grid((unsigned)ew_grid(VEC ? n / 4 : n), (unsigned)rows);
    hipLaunchKernelGGL(clip_mix_kernel<VEC>, grid, dim3(kThreads), 0, st, x, B, n, (int)HW, W, lam_px, box, out);
  });
  SM_CHECK_LAUNCH();
  return 0;
}

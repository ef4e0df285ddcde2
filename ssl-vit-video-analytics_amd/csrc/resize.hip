// Clip resize + normalisation on the GPU: the reference's MAE frame path
// (src/datasets/mae_dataset.py:84-90 u8 / 255 -> F.interpolate(bilinear,
// align_corners=False) -> clip-level torch.flip -> (x - mean) / std, stacked to
// [C,T,H,W]) applied to a whole batch of decoded frames in ONE launch after one
// host-to-device copy of the uint8 pixels.  Each clip keeps its own source size.
//
// in  : packed uint8, clip b = [T][Hs_b][Ws_b][3] (RGB, HWC) at byte desc[b][0]
//       desc   int64 [B][4] = {byte offset, Hs, Ws, flags}; flags bit 0 = horizontal
//       flip, bit 1 = invalid clip (zeros)
// out : fp32 [B][3][T][Ho][Wo]
//
// Arithmetic (fixed, so tests/resize_mirror.py reproduces it bit for bit; this file is
// built with -ffp-contract=off and the one fused operation is an explicit fma).  Per
// axis with n_in source and n_out output samples, output index d:
//   n_in == n_out : i0 = i1 = d, l1 = 0
//   otherwise     : scale = fp32(n_in) / fp32(n_out)
//                   src = max(fma(scale, d + 0.5, -0.5), 0)
//                   i0 = min((int)src, n_in - 1), l1 = clamp(src - i0, 0, 1)
//                   i1 = i0 + (i0 < n_in - 1)
//   l0 = 1 - l1
// p = fp32(u) / 255; top = l0x p00 + l1x p01; bot = l0x p10 + l1x p11;
// r = l0y top + l1y bot (every product and sum rounded on its own); a flipped clip
// writes r of column x to column Wo-1-x; out[c] = (r - mean[s]) / std[s] with
// s = bgr_swap ? 2 - c : c reading source channel s.  A clip already at (Ho, Wo)
// therefore equals sm_frames_normalize bit for bit (1 * p + 0 * q = p).
//
// A clip is written as zeros when its flag says so, when Hs or Ws is outside
// [1, 8192], or when its byte range leaves [0, packed_bytes): nothing outside
// `packed` is ever read.
//
// sm_frames_crop_resize_normalize is the same kernel body with a source window per clip
// (desc int64 [B][8] = {byte offset, Hs, Ws, flags, y0, x0, Hc, Wc}): the result is, bit for
// bit, the above applied to a buffer that holds only rows [y0, y0 + Hc) x columns
// [x0, x0 + Wc) of every frame.  Each axis runs over the window (n_in = Hc resp. Wc, so the
// edge clamp is the window's edge and no pixel outside it contributes) and y0 / x0 enter
// only the byte address of the window's first pixel; the flip is within the window.  A window
// that leaves its frame, or has Hc < 1 or Wc < 1, also gives a zero clip.  The full frame is
// the window (0, 0, Hs, Ws), which is what the 4-column instantiation fixes at compile time.
//
// Output-stationary and HBM-bound (12 B written, at most 12 B read per output pixel).
// A block owns kRows output rows x kCols output columns of one frame.  It tabulates
// u / 255 (256 values) and the per-column (x0, l1x) once in LDS, stages the source
// rows the band touches into LDS with aligned dword loads, four in flight per lane (clip
// offsets and Ws * 3 are arbitrary: the byte range is aligned down, the dwords that straddle
// the ends of `packed` are assembled from in-range bytes; a tile as wide as the frame needs
// one contiguous range (so does a full-width window), a narrower one a segment per row) and
// gathers from LDS.  A tile whose source footprint exceeds kStage (very wide rows, extreme
// downscales) gathers from global memory instead; same arithmetic, same bits.  One lane
// produces 4 consecutive columns: a 16-B non-temporal store per channel plane when
// Wo % 4 == 0 and `out` is 16-B aligned, scalar stores of the same elements otherwise.
#include "common.h"
#include "sm_api.h"

namespace {

constexpr int kRows = 8;             // output rows per block
constexpr int kCols = 1024;          // output columns per block
constexpr int kStage = 24 * 1024;    // staged source bytes per block
constexpr int kLoads = 4;            // staging loads in flight per lane
constexpr int kMaxSrc = 8192;        // largest source height / width
constexpr int kMaxDst = 4096;        // largest output height / width

struct Norm {
  float mean[3];
  float std[3];
};

struct Axis {
  int i0, i1;
  float l1;
};

SM_DEV Axis axis_at(int n_in, int n_out, int d) {
  Axis a;
  if (n_in == n_out) {
    a.i0 = a.i1 = d;
    a.l1 = 0.0f;
    return a;
  }
  const float scale = (float)n_in / (float)n_out;
  float src = __builtin_fmaf(scale, (float)d + 0.5f, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  a.i0 = min((int)src, n_in - 1);
  a.l1 = fminf(fmaxf(src - (float)a.i0, 0.0f), 1.0f);
  a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
  return a;
}

SM_DEV float lerp2(float l0x, float l1x, float l0y, float l1y, float p00, float p01, float p10, float p11) {
  const float top = l0x * p00 + l1x * p01;
  const float bot = l0x * p10 + l1x * p11;
  return l0y * top + l1y * bot;
}

// The rows [r0, r1) x columns [c0, c1) of one output frame.  Hs x Ws is the source window and
// every source index is relative to it; row_ptr(y) yields the byte pointer of pixel xlo in
// row y of the window: LDS (staged) or global memory.
template <typename RowPtr>
SM_DEV void produce(RowPtr row_ptr, const float* lut, const int* col_x0, const float* col_l1, int Hs, int Ws, int Ho,
                    int Wo, int r0, int r1, int c0, int c1, int xlo, const float* mean, const float* sd, int bgr,
                    bool vec, float* __restrict__ out_frame, int64_t plane) {
  const int ng = (c1 - c0 + 3) >> 2, items = (r1 - r0) * ng;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int r = it / ng, g = it - r * ng;
    const int y = r0 + r, ox = c0 + g * 4;
    const Axis ay = axis_at(Hs, Ho, y);
    const float l1y = ay.l1, l0y = 1.0f - l1y;
    const uint8_t *A = row_ptr(ay.i0), *Bp = row_ptr(ay.i1);
    float v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int oc = ox + e < c1 ? ox + e : c1 - 1;      // (a clamped column is computed, never stored)
      const int x0 = col_x0[oc - c0];
      const float l1x = col_l1[oc - c0], l0x = 1.0f - l1x;
      const int k0 = (x0 - xlo) * 3, k1 = k0 + (x0 < Ws - 1 ? 3 : 0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = bgr ? 2 - c : c;
        const float rr = lerp2(l0x, l1x, l0y, l1y, lut[A[k0 + s]], lut[A[k1 + s]], lut[Bp[k0 + s]],
                               lut[Bp[k1 + s]]);
        v[c][e] = (rr - mean[c]) / sd[c];
      }
    }
    float* dst = out_frame + (int64_t)y * Wo + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {                                          // Wo % 4 == 0: ox + 3 < c1 always
        __builtin_nontemporal_store(f32x4{v[c][0], v[c][1], v[c][2], v[c][3]}, (f32x4*)(dst + c * plane));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (ox + e < c1) dst[c * plane + e] = v[c][e];
      }
    }
  }
}

// kWin: desc rows carry a source window (8 columns); otherwise the window is the frame.
template <bool kWin>
__global__ void __launch_bounds__(256) resize_norm_kernel(const uint8_t* __restrict__ packed,
                                                         const int64_t* __restrict__ desc, int64_t packed_bytes,
                                                         int T, int Ho, int Wo, int bands, int ctiles, Norm nm,
                                                         int bgr, int vec, float* __restrict__ out) {
  __shared__ float lut[256];                 // u / 255
  __shared__ int col_x0[kCols];              // source column x0 of each output column of the tile
  __shared__ float col_l1[kCols];
  __shared__ uint32_t stage[kStage / 4];

  const int ct = blockIdx.x % ctiles;
  const int rest = blockIdx.x / ctiles;
  const int band = rest % bands;
  const int frame = rest / bands;            // b * T + t
  const int b = frame / T, t = frame - b * T;
  const int r0 = band * kRows, r1 = min(r0 + kRows, Ho);
  const int c0 = ct * kCols, c1 = min(c0 + kCols, Wo);
  const int64_t plane = (int64_t)T * Ho * Wo;           // one output channel of one clip
  float* out_frame = out + (int64_t)b * 3 * plane + (int64_t)t * Ho * Wo;

  constexpr int kDesc = kWin ? 8 : 4;
  const int64_t* d = desc + (int64_t)b * kDesc;
  const int64_t off = d[0], hs64 = d[1], ws64 = d[2], flags = d[3];
  bool ok = (flags & 2) == 0 && hs64 >= 1 && hs64 <= kMaxSrc && ws64 >= 1 && ws64 <= kMaxSrc && off >= 0 &&
            off <= packed_bytes;
  if (ok) ok = (int64_t)T * hs64 * ws64 * 3 <= packed_bytes - off;
  int wy = 0, wx = 0;                                   // the window's origin in the frame
  int64_t hc64 = hs64, wc64 = ws64;
  if (kWin && ok) {                                     // (hs64, ws64 <= kMaxSrc: the sums cannot overflow)
    const int64_t y064 = d[4], x064 = d[5];
    hc64 = d[6];
    wc64 = d[7];
    ok = y064 >= 0 && x064 >= 0 && hc64 >= 1 && wc64 >= 1 && hc64 <= hs64 && wc64 <= ws64 &&
         y064 <= hs64 - hc64 && x064 <= ws64 - wc64;
    wy = (int)y064;
    wx = (int)x064;
  }
  if (!ok) {                                            // block-uniform: zero clip
    const int ng = (c1 - c0 + 3) >> 2, items = (r1 - r0) * ng;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      const int r = it / ng, g = it - r * ng;
      float* dst = out_frame + (int64_t)(r0 + r) * Wo + c0 + g * 4;
      for (int c = 0; c < 3; ++c) {
        if (vec) {
          __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, (f32x4*)(dst + c * plane));
        } else {
          for (int e = 0; e < 4; ++e)
            if (c0 + g * 4 + e < c1) dst[c * plane + e] = 0.0f;
        }
      }
    }
    return;
  }
  const int Ws = (int)ws64;                             // the frame's row pitch in pixels
  const int Hc = (int)hc64, Wc = (int)wc64;             // the window (the frame when !kWin)
  const bool flip = (flags & 1) != 0;

  for (int i = threadIdx.x; i < 256; i += blockDim.x) lut[i] = (float)i / 255.0f;
  for (int i = threadIdx.x; i < c1 - c0; i += blockDim.x) {
    const int ox = c0 + i;
    const Axis ax = axis_at(Wc, Wo, flip ? Wo - 1 - ox : ox);
    col_x0[i] = ax.i0;
    col_l1[i] = ax.l1;
  }
  // source footprint of the tile, relative to the window (i0 and i1 never decrease with the
  // output index)
  const int xa = flip ? Wo - c1 : c0, xb = flip ? Wo - 1 - c0 : c1 - 1;
  const int xlo = axis_at(Wc, Wo, xa).i0, xhi = axis_at(Wc, Wo, xb).i1;
  const int ylo = axis_at(Hc, Ho, r0).i0, yhi = axis_at(Hc, Ho, r1 - 1).i1;
  const int nrows = yhi - ylo + 1, seg = (xhi - xlo + 1) * 3;
  // A tile that spans the frame's width (so Wc == Ws) needs one contiguous byte range (nrows
  // whole rows): one segment, rows Ws * 3 bytes apart in LDS.  A narrower tile or window stages
  // one segment per row, each aligned down on its own, `pitch` bytes apart (a segment plus its
  // shift, whole dwords).
  const bool whole = seg == Ws * 3;
  const int nseg = whole ? 1 : nrows, seg_bytes = whole ? nrows * seg : seg;
  const int pitch = whole ? seg : (seg + 6) & ~3;
  const bool staged = whole ? seg_bytes + 6 <= kStage : (int64_t)nrows * pitch <= kStage;

  float mean[3], sd[3];                                 // per output channel
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    mean[c] = bgr ? nm.mean[2 - c] : nm.mean[c];
    sd[c] = bgr ? nm.std[2 - c] : nm.std[c];
  }
  // byte index in `packed` of pixel xlo of the window's row 0 in this frame; the window's row y
  // is y * row_bytes further
  const int64_t frame_byte = off + ((int64_t)t * hs64 * Ws + (int64_t)wy * Ws + wx + xlo) * 3;
  const int64_t row_bytes = (int64_t)Ws * 3;

  if (staged) {
    const uint8_t* end = packed + packed_bytes;
    const uint8_t* g0 = packed + frame_byte + ylo * row_bytes;        // pixel xlo of the first staged row
    // Stage dword i is dword i % pdw of segment i / pdw, counted from that segment's aligned-down
    // start.  whole has one segment.  Otherwise every row segment is in the same pass, pdw =
    // pitch / 4 dwords each (a row's shift and segment fit: shift + seg + 3 <= pitch), so that
    // short segments (a narrow window) fill the lanes together instead of paying one pass, and
    // one memory latency, per row.  In all ndw * 4 <= kStage.
    const int shift0 = (int)((uintptr_t)g0 & 3u);
    const int pdw = whole ? (shift0 + seg_bytes + 3) >> 2 : pitch >> 2;
    const int ndw = nseg * pdw;
    // kLoads independent loads per lane in flight, then their LDS stores
    for (int i0 = threadIdx.x; i0 < ndw; i0 += kLoads * (int)blockDim.x) {
      uint32_t w[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        // The address is formed in front of the guarded load, the division only behind the
        // block-uniform !whole branch: this keeps the kLoads loads in flight.  For i >= ndw the
        // pointer lies behind the staged rows and is never dereferenced.
        const uint8_t* p;
        if (whole) {
          p = g0 - shift0 + 4 * (int64_t)i;
        } else {
          const int r = i / pdw;
          const uint8_t* g = g0 + r * row_bytes;
          p = g - ((uintptr_t)g & 3u) + 4 * (i - r * pdw);
        }
        w[u] = 0;
        if (i < ndw) {
          if (p >= packed && p + 4 <= end) {
            w[u] = *(const uint32_t*)p;
          } else {                                      // a dword across an end of `packed`
            for (int k = 0; k < 4; ++k)
              if (p + k >= packed && p + k < end) w[u] |= (uint32_t)p[k] << (8 * k);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kLoads; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        if (i < ndw) stage[i] = w[u];
      }
    }
    __syncthreads();
    const uint8_t* sbytes = (const uint8_t*)stage;
    auto row_ptr = [&](int y) -> const uint8_t* {
      // whole: every row sits at its own distance from the one aligned start
      const int64_t first = frame_byte + (whole ? ylo : y) * row_bytes;
      const int shift = (int)(((uintptr_t)packed + (uint64_t)first) & 3u);
      return sbytes + (y - ylo) * pitch + shift;
    };
    produce(row_ptr, lut, col_x0, col_l1, Hc, Wc, Ho, Wo, r0, r1, c0, c1, xlo, mean, sd, bgr,
                            vec != 0, out_frame, plane);
  } else {
    __syncthreads();
    auto row_ptr = [&](int y) -> const uint8_t* { return packed + frame_byte + y * row_bytes; };
    produce(row_ptr, lut, col_x0, col_l1, Hc, Wc, Ho, Wo, r0, r1, c0, c1, xlo, mean, sd, bgr,
                            vec != 0, out_frame, plane);
  }
}

template <bool kWin>
int launch_resize(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int B, int T, int Ho, int Wo,
                  const float* mean3, const float* std3, int bgr_swap, float* out, hipStream_t st) {
  if (B < 0 || T < 0 || Ho < 0 || Wo < 0 || Ho > kMaxDst || Wo > kMaxDst || packed_bytes < 0) return -2;
  if ((int64_t)B * T * Ho * Wo == 0) return 0;
  if (!desc || !mean3 || !std3 || !out || (!packed && packed_bytes > 0)) return -2;   // (mean3 / std3: host arrays)
  const int bands = (Ho + kRows - 1) / kRows, ctiles = (Wo + kCols - 1) / kCols;
  const int64_t blocks = (int64_t)B * T * bands * ctiles;
  if (blocks > 0x7fffffffLL) return -2;
  Norm nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = mean3[c];
    nm.std[c] = std3[c];
  }
  const int vec = Wo % 4 == 0 && ((uintptr_t)out & 15u) == 0;
  hipLaunchKernelGGL(resize_norm_kernel<kWin>, dim3((unsigned)blocks), dim3(256), 0, st, packed, desc, packed_bytes,
                     T, Ho, Wo, bands, ctiles, nm, bgr_swap, vec, out);
  SM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int sm_frames_resize_normalize(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int B,
                                          int T, int Ho, int Wo, const float* mean3, const float* std3,
                                          int bgr_swap, float* out, hipStream_t st) {
  return launch_resize<false>(packed, desc, packed_bytes, B, T, Ho, Wo, mean3, std3, bgr_swap, out, st);
}

extern "C" int sm_frames_crop_resize_normalize(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes,
                                               int B, int T, int Ho, int Wo, const float* mean3, const float* std3,
                                               int bgr_swap, float* out, hipStream_t st) {
  return launch_resize<true>(packed, desc, packed_bytes, B, T, Ho, Wo, mean3, std3, bgr_swap, out, st);
}

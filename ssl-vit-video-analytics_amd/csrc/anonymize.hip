// Visual privacy on the GPU: Gaussian blur of the boxes of a batch of decoded frames, and the
// integer statistics of what the blur changed inside them (the anonymisation half of the
// reference's src/run_privacy.py:118-226 run_visual_privacy, whose cv2.GaussianBlur runs per
// detected face on the host; the detector is not part of this build, the boxes are an input).
//
// packed : uint8, frame n = [H_n][W_n][3] (RGB, HWC) at byte desc[n][0]; `out` has the same layout
// desc   : int64 [N][3] = {byte offset, H, W}                      (device)
// boxes  : int32 [num_boxes][4] = {x, y, w, h}; frame n owns [box_start[n], box_start[n + 1])
//
// Arithmetic of the blur (fixed, so tests/blur_mirror.py reproduces it bit for bit; this file is
// built with -ffp-contract=off and holds no fma).  With r = (ksize - 1) / 2 and refl(i, n) the
// reflect-101 index (n == 1: 0; otherwise p = 2 (n - 1), i = i mod p >= 0, i >= n -> p - i):
//   h(y, x) = acc after acc = acc + w[i] * fp32(u[y][refl(x + i - r, W)]), i = 0 .. ksize - 1, acc = 0
//   v(y, x) = the same over w[i] * h(refl(y + i - r, H), x)
//   byte    = (uint8) min(255, max(0, rintf(v)))
// for every pixel of the union U of the frame's clipped boxes and every channel; a pixel outside
// U keeps its bytes.  h and v always read the ORIGINAL frame, so a pixel has one summation order
// whatever the tiling and however the boxes are ordered or overlap.
//
// A frame is skipped (nothing written, statistics zero) when H or W is outside [1, 8192], above
// max_h / max_w, or its byte range leaves [0, packed_bytes); box ranges are clamped into
// [0, num_boxes]; a box is clipped to its frame in 64-bit sums.  Nothing outside `packed`,
// `boxes` or `box_start` is read.
//
// A block owns a tile of kTH x kTW pixels of one frame; the grid is N x the tiles of
// (max_h, max_w), and a block whose tile lies outside its frame leaves at once.  Every thread
// walks the frame's boxes (uniform loads), so "does this tile meet a box" costs no barrier.
//   * no box: the tile's row segments are copied with 16-byte, 4-byte or 1-byte accesses, the widest
//     at which `packed` and `out` are congruent; the ends of a segment go byte by byte.
//   * a box:  tile + halo of the source, reflected at the frame's edge, is staged once in LDS as
//     three channel planes (a lane then reads consecutive bytes: four lanes share a dword, no bank
//     conflict from the 3-byte pixel stride).  Per channel the horizontal pass writes fp32 rows to
//     LDS (row pitch kTW + 1 dwords, so the rows of a narrow box region fall on different banks),
//     the vertical pass reads them and puts the rounded byte back into the plane's centre where the
//     tile's mask says U; the planes' centres are then written out interleaved with dword stores.
//     Both passes run only over the bounding rectangle of the boxes within the tile.
//     LDS is dynamic, sized by the radius: 3 x (32 + 2 r) x 128 B planes + (32 + 2 r) x 65 x 4 B rows +
//     2 KiB mask; 61.4 KiB at ksize = 63, two workgroups per CU of the 160 KiB, 31.2 KiB at ksize = 15.
// sm_box_region_stats uses the same tiles and mask and adds its exact integer sums with one 64-bit
// atomic per value and tile, after the call's own memset of `stats`.
#include "common.h"
#include "sm_api.h"

namespace {

constexpr int kTH = SM_BOX_TILE_H;   // tile rows
constexpr int kTW = SM_BOX_TILE_W;   // tile columns
constexpr int kMaxK = 63;            // largest kernel size
constexpr int kMaxR = (kMaxK - 1) / 2;
constexpr int kSP = 128;             // plane row pitch in bytes (kTW + 2 kMaxR = 126 staged columns)
constexpr int kHP = kTW + 1;         // pitch of the horizontal pass's rows in dwords
constexpr int kMaxSide = 8192;       // largest frame height / width

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Taps {
  float w[kMaxK];
};

struct Frame {
  int64_t off;       // first byte of the frame
  int H, W;
  int64_t b0, b1;    // its boxes
};

struct Rect {
  int x0, y0, x1, y1;
};

// Block -> (frame, tile); false when the frame is skipped or the tile lies outside it.
SM_DEV bool tile_at(const int64_t* __restrict__ desc, const int32_t* __restrict__ box_start, int64_t packed_bytes,
                    int64_t num_boxes, int max_h, int max_w, int tiles_y, int tiles_x, Frame& f, Rect& tile) {
  const int tx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y;
  const int n = rest / tiles_y;
  const int64_t off = desc[3 * (int64_t)n], h = desc[3 * (int64_t)n + 1], w = desc[3 * (int64_t)n + 2];
  if (h < 1 || h > kMaxSide || w < 1 || w > kMaxSide || h > max_h || w > max_w || off < 0 || off > packed_bytes)
    return false;
  if (h * w * 3 > packed_bytes - off) return false;
  f.off = off;
  f.H = (int)h;
  f.W = (int)w;
  tile.x0 = tx * kTW;
  tile.y0 = ty * kTH;
  if (tile.x0 >= f.W || tile.y0 >= f.H) return false;
  tile.x1 = min(tile.x0 + kTW, f.W);
  tile.y1 = min(tile.y0 + kTH, f.H);
  int64_t b0 = box_start[n], b1 = box_start[n + 1];
  f.b0 = b0 < 0 ? 0 : (b0 > num_boxes ? num_boxes : b0);
  f.b1 = b1 < 0 ? 0 : (b1 > num_boxes ? num_boxes : b1);
  return true;
}

// The part of box b of the frame that lies in `tile`; false when nothing does.
SM_DEV bool box_in_tile(const int32_t* __restrict__ boxes, int64_t b, const Frame& f, const Rect& tile, Rect& r) {
  const int x = boxes[4 * b], y = boxes[4 * b + 1], w = boxes[4 * b + 2], h = boxes[4 * b + 3];
  if (w <= 0 || h <= 0) return false;
  const int64_t x1 = (int64_t)x + w, y1 = (int64_t)y + h;
  r.x0 = max(max(x, 0), tile.x0);
  r.y0 = max(max(y, 0), tile.y0);
  r.x1 = (int)(x1 < tile.x1 ? x1 : tile.x1);
  r.y1 = (int)(y1 < tile.y1 ? y1 : tile.y1);
  return r.x1 > r.x0 && r.y1 > r.y0;
}

// mask [kTH][kTW] = 1 where the tile's pixel lies in U; `bound` = the boxes' bounding rectangle
// within the tile.  The result is the same in every thread; false (and no barrier) when the tile
// meets no box.  Every thread walks all of the frame's boxes, twice in a tile that meets one and
// once in a copy tile: the cost per tile is linear in the frame's box count, meant for a few boxes
// per frame (faces), not for dense box files.
SM_DEV bool mark_boxes(const int32_t* __restrict__ boxes, const Frame& f, const Rect& tile, uint8_t* mask,
                       Rect& bound) {
  bound = Rect{tile.x1, tile.y1, tile.x0, tile.y0};
  bool any = false;
  for (int64_t b = f.b0; b < f.b1; ++b) {
    Rect r;
    if (!box_in_tile(boxes, b, f, tile, r)) continue;
    any = true;
    bound.x0 = min(bound.x0, r.x0);
    bound.y0 = min(bound.y0, r.y0);
    bound.x1 = max(bound.x1, r.x1);
    bound.y1 = max(bound.y1, r.y1);
  }
  if (!any) return false;
  for (int i = threadIdx.x; i < kTH * kTW / 4; i += blockDim.x) ((uint32_t*)mask)[i] = 0;
  __syncthreads();
  for (int64_t b = f.b0; b < f.b1; ++b) {
    Rect r;
    if (!box_in_tile(boxes, b, f, tile, r)) continue;
    const int rw = r.x1 - r.x0, items = (r.y1 - r.y0) * rw;
    for (int i = threadIdx.x; i < items; i += blockDim.x) {
      const int yy = i / rw, xx = i - yy * rw;
      mask[(r.y0 - tile.y0 + yy) * kTW + r.x0 - tile.x0 + xx] = 1;   // (boxes overlap: the same value)
    }
  }
  __syncthreads();
  return true;
}

SM_DEV int refl(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

// `rows` row segments of `seg` bytes, row_bytes apart, the first at byte `first` of both buffers.
// V = 16, 4 or 1: src and dst are congruent modulo V; a segment is cut into V-byte chunks aligned
// in dst, whole chunks move as one access, the chunks across a segment's ends byte by byte.
template <int V>
SM_DEV void copy_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t first, int64_t row_bytes,
                      int rows, int seg) {
  constexpr int cpr = kTW * 3 / V + 1;                  // chunks per row at most
  for (int it = threadIdx.x; it < rows * cpr; it += blockDim.x) {
    const int r = it / cpr, j = it - r * cpr;
    const int64_t s = first + r * row_bytes, e = s + seg;
    const int64_t c0 = s - (int64_t)((uintptr_t)(dst + s) & (uintptr_t)(V - 1)) + (int64_t)j * V;
    if (c0 >= e) continue;
    if (c0 >= s && c0 + V <= e) {
      if constexpr (V == 16) *(u32x4*)(dst + c0) = *(const u32x4*)(src + c0);
      else if constexpr (V == 4) *(uint32_t*)(dst + c0) = *(const uint32_t*)(src + c0);
      else dst[c0] = src[c0];
    } else {
      for (int k = 0; k < V; ++k)
        if (c0 + k >= s && c0 + k < e) dst[c0 + k] = src[c0 + k];
    }
  }
}

__global__ void __launch_bounds__(256) box_blur_kernel(const uint8_t* __restrict__ packed,
                                                      const int64_t* __restrict__ desc, int64_t packed_bytes,
                                                      int tiles_y, int tiles_x, int max_h, int max_w,
                                                      const int32_t* __restrict__ boxes,
                                                      const int32_t* __restrict__ box_start, int64_t num_boxes,
                                                      Taps taps, int ksize, int vec, uint8_t* __restrict__ out) {
  // dynamic LDS, blur_lds_bytes(ksize): sized by the radius, so a small kernel leaves room for more
  // workgroups per CU (the copy tiles live in the same launch).  A launch with num_boxes == 0 gets
  // none: every tile is then a copy and nothing below touches LDS.
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int r = (ksize - 1) >> 1;
  const int srows = kTH + 2 * r;                              // staged rows
  float* hrow = (float*)lds;                                  // [srows][kHP]: the horizontal pass of one channel
  float* wl = hrow + srows * kHP;                             // [kMaxK + 1]
  uint8_t* mask = (uint8_t*)(wl + kMaxK + 1);                 // [kTH][kTW]
  uint8_t* planes = mask + kTH * kTW;                         // [3][srows][kSP]: tile + halo, one plane per channel
  const int psz = srows * kSP;

  Frame f;
  Rect tile, bound;
  if (!tile_at(desc, box_start, packed_bytes, num_boxes, max_h, max_w, tiles_y, tiles_x, f, tile)) return;
  const int tw = tile.x1 - tile.x0, th = tile.y1 - tile.y0;
  const int64_t row_bytes = (int64_t)f.W * 3;
  const int64_t first = f.off + ((int64_t)tile.y0 * f.W + tile.x0) * 3;   // the tile's first byte

  if (!mark_boxes(boxes, f, tile, mask, bound)) {       // block-uniform: straight copy
    if (vec == 16) copy_rows<16>(packed, out, first, row_bytes, th, tw * 3);
    else if (vec == 4) copy_rows<4>(packed, out, first, row_bytes, th, tw * 3);
    else copy_rows<1>(packed, out, first, row_bytes, th, tw * 3);
    return;
  }

  if (threadIdx.x < kMaxK) wl[threadIdx.x] = taps.w[threadIdx.x];
  // stage row sy / column sx = source pixel (refl(tile.y0 - r + sy), refl(tile.x0 - r + sx))
  const int sw = tw + 2 * r, sh = th + 2 * r;
  const uint8_t* src = packed + f.off;
  for (int i = threadIdx.x; i < sh * sw; i += blockDim.x) {
    const int sy = i / sw, sx = i - sy * sw;
    const int yy = refl(tile.y0 - r + sy, f.H), xx = refl(tile.x0 - r + sx, f.W);
    const uint8_t* p = src + ((int64_t)yy * f.W + xx) * 3;
    planes[sy * kSP + sx] = p[0];
    planes[psz + sy * kSP + sx] = p[1];
    planes[2 * psz + sy * kSP + sx] = p[2];
  }
  __syncthreads();

  // the boxes' bounding rectangle, relative to the tile
  const int bx0 = bound.x0 - tile.x0, by0 = bound.y0 - tile.y0;
  const int bw = bound.x1 - bound.x0, bh = bound.y1 - bound.y0;
  for (int c = 0; c < 3; ++c) {
    uint8_t* plane = planes + c * psz;
    // horizontal: stage rows by0 .. by0 + bh + 2 r, tile columns bx0 .. bx0 + bw
    for (int i = threadIdx.x; i < (bh + 2 * r) * bw; i += blockDim.x) {
      const int rr = i / bw, row = by0 + rr, col = bx0 + i - rr * bw;
      const uint8_t* s = &plane[row * kSP + col];    // tap t reads stage column col + t
      float acc = 0.0f;
      for (int t = 0; t < ksize; ++t) acc = acc + wl[t] * (float)s[t];
      hrow[row * kHP + col] = acc;
    }
    __syncthreads();
    // vertical, where the mask says U: the byte replaces the source byte in the plane's centre
    for (int i = threadIdx.x; i < bh * bw; i += blockDim.x) {
      const int rr = i / bw, ly = by0 + rr, lx = bx0 + i - rr * bw;
      if (!mask[ly * kTW + lx]) continue;
      const float* hp = &hrow[ly * kHP + lx];           // tap t reads stage row ly + t
      float acc = 0.0f;
      for (int t = 0; t < ksize; ++t) acc = acc + wl[t] * hp[t * kHP];
      const float q = fminf(255.0f, fmaxf(0.0f, rintf(acc)));
      plane[(ly + r) * kSP + lx + r] = (uint8_t)q;
    }
    __syncthreads();
  }

  // write the planes' centres out interleaved: dwords aligned in `out`, bytes across a row's ends
  constexpr int cpr = kTW * 3 / 4 + 1;
  const int seg = tw * 3;
  for (int it = threadIdx.x; it < th * cpr; it += blockDim.x) {
    const int ly = it / cpr, j = it - ly * cpr;
    const int64_t s = first + ly * row_bytes, e = s + seg;
    const int64_t c0 = s - (int64_t)((uintptr_t)(out + s) & 3u) + 4 * (int64_t)j;
    if (c0 >= e) continue;
    uint32_t word = 0;
    uint8_t b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int pos = (int)(c0 - s) + k;                      // byte of the row segment
      pos = pos < 0 ? 0 : (pos >= seg ? seg - 1 : pos); // (a clamped byte is formed, never stored)
      const int px = pos / 3, ch = pos - px * 3;
      b[k] = planes[ch * psz + (ly + r) * kSP + px + r];
      word |= (uint32_t)b[k] << (8 * k);
    }
    if (c0 >= s && c0 + 4 <= e) {
      *(uint32_t*)(out + c0) = word;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k >= s && c0 + k < e) out[c0 + k] = b[k];
    }
  }
}

SM_DEV int64_t wave_sum_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
  return v;
}

__global__ void __launch_bounds__(256) box_stats_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                       const int64_t* __restrict__ desc, int64_t packed_bytes,
                                                       int tiles_y, int tiles_x, int max_h, int max_w,
                                                       const int32_t* __restrict__ boxes,
                                                       const int32_t* __restrict__ box_start, int64_t num_boxes,
                                                       unsigned long long* __restrict__ stats) {
  __shared__ __attribute__((aligned(4))) uint8_t mask[kTH * kTW];
  __shared__ int64_t red[4][4];
  Frame f;
  Rect tile, bound;
  if (!tile_at(desc, box_start, packed_bytes, num_boxes, max_h, max_w, tiles_y, tiles_x, f, tile)) return;
  if (!mark_boxes(boxes, f, tile, mask, bound)) return;
  const int bw = bound.x1 - bound.x0, bh = bound.y1 - bound.y0;
  const int64_t row_bytes = (int64_t)f.W * 3;
  int64_t v[4] = {0, 0, 0, 0};                          // P, SSE, Ea, Eb
  for (int i = threadIdx.x; i < bh * bw; i += blockDim.x) {
    const int rr = i / bw, y = bound.y0 + rr, x = bound.x0 + i - rr * bw;
    if (!mask[(y - tile.y0) * kTW + x - tile.x0]) continue;
    const int64_t at = f.off + ((int64_t)y * f.W + x) * 3;
    const bool right = x + 1 < f.W, down = y + 1 < f.H;
    v[0] += 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int av = a[at + c], bv = b[at + c];
      v[1] += (av - bv) * (av - bv);
      if (right) {
        const int da = (int)a[at + 3 + c] - av, db = (int)b[at + 3 + c] - bv;
        v[2] += da * da;
        v[3] += db * db;
      }
      if (down) {
        const int da = (int)a[at + row_bytes + c] - av, db = (int)b[at + row_bytes + c] - bv;
        v[2] += da * da;
        v[3] += db * db;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_sum_i64(v[k]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = v[k];
  __syncthreads();
  if (threadIdx.x < 4) {                                // exact integers: the order of the adds is free
    const int64_t t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    const int n = blockIdx.x / (tiles_x * tiles_y);
    if (t != 0) atomicAdd(&stats[4 * (int64_t)n + threadIdx.x], (unsigned long long)t);
  }
}

// Dynamic LDS of box_blur_kernel: fp32 rows, weights, mask, three planes (61.4 KiB at ksize = 63).
int blur_lds_bytes(int ksize) {
  const int srows = kTH + (ksize - 1);
  return srows * kHP * 4 + (kMaxK + 1) * 4 + kTH * kTW + 3 * srows * kSP;
}

// The checks both entry points share; 1 = launch, 0 = nothing to do, -2 = bad argument.
int check_batch(int64_t packed_bytes, int N, int max_h, int max_w, int64_t num_boxes, int& tiles_y, int& tiles_x) {
  if (N < 0 || packed_bytes < 0 || num_boxes < 0 || max_h < 1 || max_h > kMaxSide || max_w < 1 || max_w > kMaxSide)
    return -2;
  tiles_y = (max_h + kTH - 1) / kTH;
  tiles_x = (max_w + kTW - 1) / kTW;
  if ((int64_t)N * tiles_y * tiles_x > 0x7fffffffLL) return -2;
  return N == 0 ? 0 : 1;
}

}  // namespace

extern "C" int sm_frames_box_blur(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int N, int max_h,
                                  int max_w, const int32_t* boxes, const int32_t* box_start, int64_t num_boxes,
                                  const float* weights, int ksize, uint8_t* out, hipStream_t st) {
  int tiles_y = 0, tiles_x = 0;
  const int go = check_batch(packed_bytes, N, max_h, max_w, num_boxes, tiles_y, tiles_x);
  if (go < 0 || ksize < 3 || ksize > kMaxK || (ksize & 1) == 0) return -2;
  if (go == 0) return 0;
  if (!packed || !desc || !box_start || !weights || !out || (!boxes && num_boxes > 0) || out == packed) return -2;
  // the blur reads halos of the original while other blocks write: the two buffers must be disjoint
  const uintptr_t pa = (uintptr_t)packed, oa = (uintptr_t)out;
  if (pa < oa + (uint64_t)packed_bytes && oa < pa + (uint64_t)packed_bytes) return -2;
  Taps taps;
  for (int i = 0; i < kMaxK; ++i) taps.w[i] = i < ksize ? weights[i] : 0.0f;
  const uintptr_t x = (uintptr_t)packed ^ (uintptr_t)out;
  const int vec = (x & 15u) == 0 ? 16 : ((x & 3u) == 0 ? 4 : 1);
  hipLaunchKernelGGL(box_blur_kernel, dim3((unsigned)((int64_t)N * tiles_y * tiles_x)), dim3(256),
                     num_boxes > 0 ? blur_lds_bytes(ksize) : 0, st, packed, desc, packed_bytes, tiles_y, tiles_x, max_h, max_w, boxes,
                     box_start, num_boxes, taps, ksize, vec, out);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_box_region_stats(const uint8_t* a, const uint8_t* b, const int64_t* desc, int64_t packed_bytes, int N,
                                   int max_h, int max_w, const int32_t* boxes, const int32_t* box_start,
                                   int64_t num_boxes, int64_t* stats, hipStream_t st) {
  int tiles_y = 0, tiles_x = 0;
  const int go = check_batch(packed_bytes, N, max_h, max_w, num_boxes, tiles_y, tiles_x);
  if (go < 0) return -2;
  if (go == 0) return 0;
  if (!a || !b || !desc || !box_start || !stats || (!boxes && num_boxes > 0)) return -2;
  hipError_t e = hipMemsetAsync(stats, 0, (size_t)N * 4 * sizeof(int64_t), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(box_stats_kernel, dim3((unsigned)((int64_t)N * tiles_y * tiles_x)), dim3(256), 0, st, a, b, desc,
                     packed_bytes, tiles_y, tiles_x, max_h, max_w, boxes, box_start, num_boxes,
                     (unsigned long long*)stats);
  SM_CHECK_LAUNCH();
  return 0;
}

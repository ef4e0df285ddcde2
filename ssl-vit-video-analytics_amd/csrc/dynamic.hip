// Streaming dynamic inference (src/models/dynamic_infer.py of the reference): motion-score
// frame gating and confidence early-exit over the fine-tuned VideoClassifier.
//
// The encoder does the heavy work; these are the small streaming / reduction kernels
// around it, all fp32 (the embeddings and the head are fp32, finetune.HeadLinearFn):
//   motion_scores   mean |x[t] - x[t-1]| per frame, the clip read once through its strides
//   topk_frames     the k highest-scoring frames per sample, ascending frame order
//   gather_frames   frames (b_i, t_i) of a strided clip -> one dense [n][C][H][W] batch
//   exit_step       running-mean embedding + head + max-softmax + exit decision per sample
//   active_compact  undecided samples, ascending, and their count (the loop's one readback)
// No atomics, no LDS tiling, no MFMA; every reduction has a fixed partition and order.
#include "common.h"
#include "sm_api.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;                            // 16-byte groups per thread per frame
constexpr int kBandElems = kThreads * kVec * 4;    // 4096 pixels of one (b, c) plane per block

struct ClipView {
  const float* p;
  int64_t sB, sC, sT, sH, sW;
  int B, C, T, H, W;
};

// Plane bands: nbands = ceil(HW / 4096) equal bands whose length is a multiple of 4, so a
// 16-byte group never straddles two bands (nor two rows when W % 4 == 0).
SM_DEV int band_len(int HW, int nbands) { return (((HW + nbands - 1) / nbands) + 3) & ~3; }
static inline int num_bands(int64_t HW) { return (int)((HW + kBandElems - 1) / kBandElems); }

// Offsets (within one frame plane) of the pixels a thread owns: group g = tid + k * 256 of
// its band holds pixels 4g .. 4g + 3.  The vector form keeps one offset per group; the scalar
// form one per pixel (a group may cross a row there).  Ownership and summation order are the
// same in both forms, so the two paths give the same bits.
template <bool VEC>
struct Owned {
  int64_t off[VEC ? kVec : kVec * 4];
  int p0[kVec];
  SM_DEV void init(const ClipView& v, int start, int end) {
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
      const int p = start + 4 * ((int)threadIdx.x + k * kThreads);
      p0[k] = p < end ? p : -1;
      if constexpr (VEC) {
        off[k] = p < end ? (int64_t)(p / v.W) * v.sH + (int64_t)(p % v.W) : 0;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = p + j;
          off[k * 4 + j] = q < end ? (int64_t)(q / v.W) * v.sH + (int64_t)(q % v.W) * v.sW : 0;
        }
      }
    }
  }
  // valid pixels of group k given the band / plane end (whole groups in the vector form)
  SM_DEV int count(int k, int end) const { return p0[k] < 0 ? 0 : (end - p0[k] < 4 ? end - p0[k] : 4); }
  SM_DEV void load(const float* base, int k, int end, float* x) const {
    if constexpr (VEC) {
      if (p0[k] >= 0) {
        const f32x4 a = __builtin_nontemporal_load((const f32x4*)(base + off[k]));
        x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
      } else {
        x[0] = x[1] = x[2] = x[3] = 0.f;
      }
    } else {
      const int n = count(k, end);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = j < n ? base[off[k * 4 + j]] : 0.f;
    }
  }
};

// ---------------------------------------------------------------- motion scores
// One block per (b, c, band).  part [B][C][nbands][4 waves][T]: entry t >= 1 of every row is
// written, entry 0 never read.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void motion_partials_kernel(ClipView v, int nbands, float* __restrict__ part) {
  const int band = blockIdx.x % nbands;
  const int plane = blockIdx.x / nbands;          // b * C + c
  const int b = plane / v.C, c = plane % v.C;
  const int HW = v.H * v.W;
  const int len = band_len(HW, nbands);
  const int start = band * len;
  const int end = start + len < HW ? start + len : HW;
  Owned<VEC> own;
  own.init(v, start, end);
  const float* base = v.p + (int64_t)b * v.sB + (int64_t)c * v.sC;
  float prev[kVec][4];
#pragma unroll
  for (int k = 0; k < kVec; ++k) own.load(base, k, end, prev[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* row = part + ((int64_t)blockIdx.x * 4 + wave) * v.T;
  for (int t = 1; t < v.T; ++t) {
    const float* fr = base + (int64_t)t * v.sT;
    float cur[kVec][4];
#pragma unroll
    for (int k = 0; k < kVec; ++k) own.load(fr, k, end, cur[k]);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kVec; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc += fabsf(cur[k][j] - prev[k][j]);     // padding lanes hold 0 in both frames
        prev[k][j] = cur[k][j];
      }
    acc = wave_sum(acc);
    if (lane == 0) row[t] = acc;
  }
}

// scores[b][t] = (sum over the C * nbands * 4 partials of sample b, ascending, fp64) / (C H W)
__global__ __launch_bounds__(kThreads) void motion_finish_kernel(const float* __restrict__ part, int B, int T,
                                                                 int rows_per_b, double inv_n,
                                                                 float* __restrict__ scores) {
  const int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  if (i >= (int64_t)B * T) return;
  const int b = (int)(i / T), t = (int)(i % T);
  double s = 0.0;
  if (t > 0) {
    const float* p = part + (int64_t)b * rows_per_b * T + t;
    for (int r = 0; r < rows_per_b; ++r) s += (double)p[(int64_t)r * T];
  }
  scores[i] = (float)(s * inv_n);
}

// ---------------------------------------------------------------- top-k frames
// u ranks before t: higher score first, equal scores by lower frame index, NaN last.
SM_DEV bool ranks_before(float su, int u, float st, int t) {
  const bool nu = su != su, nt = st != st;
  if (nt) return !nu || u < t;
  if (nu) return false;
  return su > st || (su == st && u < t);
}

__global__ __launch_bounds__(64) void topk_frames_kernel(const float* __restrict__ scores, int T, int k_eff,
                                                         int32_t* __restrict__ idx) {
  __shared__ float s[256];
  const int b = blockIdx.x, lane = threadIdx.x;
  for (int t = lane; t < T; t += 64) s[t] = scores[(int64_t)b * T + t];
  __syncthreads();
  int base = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {           // ascending chunks -> ascending output
    const int t = t0 + lane;
    bool sel = false;
    if (t < T) {
      const float st = s[t];
      int rank = 0;
      for (int u = 0; u < T; ++u) rank += ranks_before(s[u], u, st, t) ? 1 : 0;
      sel = rank < k_eff;
    }
    const unsigned long long m = __ballot(sel);
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (sel) idx[(int64_t)b * k_eff + pos] = t;
    base += __popcll(m);
  }
}

// ---------------------------------------------------------------- frame gather
// One block per (i, c, band): out[i][c] band <- clip[b_i][c][t_i] band.  An index outside the
// clip writes zeros instead of reading out of bounds.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void gather_frames_kernel(ClipView v, int nbands,
                                                                 const int32_t* __restrict__ b_idx, int rows_per_b,
                                                                 const int32_t* __restrict__ t_idx, int t_fixed,
                                                                 float* __restrict__ out) {
  const int band = blockIdx.x % nbands;
  const int plane = blockIdx.x / nbands;          // i * C + c
  const int i = plane / v.C, c = plane % v.C;
  const int HW = v.H * v.W;
  const int len = band_len(HW, nbands);
  const int start = band * len;
  const int end = start + len < HW ? start + len : HW;
  const int b = b_idx ? b_idx[i] : i / rows_per_b;
  const int t = t_idx ? t_idx[i] : t_fixed;
  const bool ok = (unsigned)b < (unsigned)v.B && (unsigned)t < (unsigned)v.T;
  Owned<VEC> own;
  own.init(v, start, end);
  const float* src = v.p + (ok ? (int64_t)b * v.sB + (int64_t)c * v.sC + (int64_t)t * v.sT : 0);
  float* dst = out + (int64_t)plane * HW;
#pragma unroll
  for (int k = 0; k < kVec; ++k) {
    const int n = own.count(k, end);
    if (n == 0) continue;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (ok) own.load(src, k, end, x);
    if constexpr (VEC) {
      *(f32x4*)(dst + own.p0[k]) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) dst[own.p0[k] + j] = x[j];
    }
  }
}

// ---------------------------------------------------------------- exit step
// One block (4 waves) per active row.  LDS: mean[D], logit[K].
__global__ __launch_bounds__(kThreads) void exit_step_kernel(const float* __restrict__ emb,
                                                             const int32_t* __restrict__ active, int B, int D, int K,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             float threshold, int min_frames, int final_pass,
                                                             float* __restrict__ sum, int32_t* __restrict__ cnt,
                                                             uint8_t* __restrict__ decided,
                                                             float* __restrict__ final_logits,
                                                             int32_t* __restrict__ used, float* __restrict__ conf) {
  extern __shared__ float lds[];
  float* mean = lds;
  float* logit = lds + D;
  const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = active[i];
  if ((unsigned)s >= (unsigned)B) return;         // block-uniform
  const int c = cnt[s] + (emb ? 1 : 0);
  const float denom = (float)(c > 1 ? c : 1);
  for (int d = tid; d < D; d += kThreads) {
    float v = sum[(int64_t)s * D + d];
    if (emb) {
      v += emb[(int64_t)i * D + d];
      sum[(int64_t)s * D + d] = v;
    }
    mean[d] = v / denom;
  }
  __syncthreads();                                // every thread has read cnt[s]
  if (tid == 0 && emb) cnt[s] = c;
  // waves split the classes, lanes split D; four classes of a wave in flight (independent
  // loads), each class's own sum in the same order whatever its slot
  for (int k0 = wave; k0 < K; k0 += 16) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* wk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wk[j] = w + (int64_t)(k0 + 4 * j < K ? k0 + 4 * j : k0) * D;
    for (int d = lane; d < D; d += 64) {
      const float m = mean[d];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk[j][d], m, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = wave_sum(acc[j]);
      if (lane == 0 && k0 + 4 * j < K) logit[k0 + 4 * j] = a + bias[k0 + 4 * j];
    }
  }
  __syncthreads();
  // max softmax = exp(0) / sum_k exp(l_k - max l): wave-uniform in every wave
  float m = -INFINITY;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, logit[k]);
  m = wave_max(m);
  float e = 0.f;
  for (int k = lane; k < K; k += 64) e += expf(logit[k] - m);
  e = wave_sum(e);
  const float cf = 1.0f / e;
  const bool decide = final_pass || (cf >= threshold && c >= min_frames);
  if (!decide) return;
  for (int k = tid; k < K; k += kThreads) final_logits[(int64_t)s * K + k] = logit[k];
  if (tid == 0) {
    used[s] = c;
    conf[s] = cf;
    decided[s] = 1;
  }
}

// ---------------------------------------------------------------- active-list compaction
// One wave: ascending chunks of 64 samples, ballot prefix.
__global__ __launch_bounds__(64) void active_compact_kernel(const uint8_t* __restrict__ decided, int B,
                                                            int32_t* __restrict__ active,
                                                            int32_t* __restrict__ count) {
  const int lane = threadIdx.x;
  int base = 0;
  for (int s0 = 0; s0 < B; s0 += 64) {
    const int s = s0 + lane;
    const bool live = s < B && decided[s] == 0;
    const unsigned long long m = __ballot(live);
    if (live) active[base + __popcll(m & ((1ull << lane) - 1ull))] = s;
    base += __popcll(m);
  }
  if (lane == 0) *count = base;
}

bool clip_ok(int B, int C, int T, int H, int W) {
  return B > 0 && C > 0 && T > 0 && H > 0 && W > 0 && (int64_t)H * W <= 0x7fffffff - 4 * kBandElems;
}

// 16-byte loads: unit pixel stride, W % 4 == 0 and every plane / row start 16-byte aligned
bool clip_vec(const float* clip, int W, int64_t sB, int64_t sC, int64_t sT, int64_t sH, int64_t sW) {
  return sW == 1 && W % 4 == 0 && aligned16(clip) && ((sB | sC | sT | sH) & 3) == 0;
}

}  // namespace

extern "C" int64_t sm_motion_scores_workspace_bytes(int B, int C, int T, int H, int W) {
  if (!clip_ok(B, C, T, H, W)) return 0;
  return (int64_t)B * C * num_bands((int64_t)H * W) * 4 * T * (int64_t)sizeof(float);
}

extern "C" int sm_motion_scores(const float* clip, int B, int C, int T, int H, int W, int64_t sB, int64_t sC,
                                int64_t sT, int64_t sH, int64_t sW, float* scores, void* ws, int64_t ws_bytes,
                                hipStream_t st) {
  if (!clip_ok(B, C, T, H, W) || !clip || !scores) return -2;
  const int nbands = num_bands((int64_t)H * W);
  const int64_t nblk = (int64_t)B * C * nbands;
  if (nblk > 0x7fffffff || (int64_t)B * T > 0x7fffffff) return -2;
  if (!ws || ws_bytes < sm_motion_scores_workspace_bytes(B, C, T, H, W)) return -4;
  const ClipView v{clip, sB, sC, sT, sH, sW, B, C, T, H, W};
  float* part = (float*)ws;
  if (T > 1) {
    DISPATCH_BOOL(clip_vec(clip, W, sB, sC, sT, sH, sW), VEC,
                  hipLaunchKernelGGL(motion_partials_kernel<VEC>, dim3((unsigned)nblk), dim3(kThreads), 0, st, v, nbands,
                                     part));
    SM_CHECK_LAUNCH();
  }
  const int64_t n = (int64_t)B * T;
  hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part,
                     B, T, C * nbands * 4, 1.0 / ((double)C * H * W), scores);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_topk_frames(const float* scores, int B, int T, int k, int32_t* idx, hipStream_t st) {
  if (B <= 0 || T <= 0 || T > 256 || k <= 0 || !scores || !idx) return -2;
  hipLaunchKernelGGL(topk_frames_kernel, dim3((unsigned)B), dim3(64), 0, st, scores, T, k < T ? k : T, idx);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_gather_frames(const float* clip, int B, int C, int T, int H, int W, int64_t sB, int64_t sC,
                                int64_t sT, int64_t sH, int64_t sW, const int32_t* b_idx, int rows_per_b,
                                const int32_t* t_idx, int t_fixed, int n, float* out, hipStream_t st) {
  if (!clip_ok(B, C, T, H, W) || n <= 0 || !clip || !out || (!b_idx && rows_per_b <= 0)) return -2;
  const int nbands = num_bands((int64_t)H * W);
  const int64_t nblk = (int64_t)n * C * nbands;
  if (nblk > 0x7fffffff) return -2;
  const ClipView v{clip, sB, sC, sT, sH, sW, B, C, T, H, W};
  DISPATCH_BOOL(clip_vec(clip, W, sB, sC, sT, sH, sW) && aligned16(out), VEC,
                hipLaunchKernelGGL(gather_frames_kernel<VEC>, dim3((unsigned)nblk), dim3(kThreads), 0, st, v, nbands,
                                   b_idx, rows_per_b, t_idx, t_fixed, out));
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_exit_step(const float* emb, const int32_t* active, int n, int B, int D, int K, const float* w,
                            const float* bias, float threshold, int min_frames, int final_pass, float* sum,
                            int32_t* cnt, uint8_t* decided, float* final_logits, int32_t* used, float* conf,
                            hipStream_t st) {
  if (n <= 0 || n > B || D <= 0 || K <= 0 || !active || !w || !bias || !sum || !cnt || !decided || !final_logits ||
      !used || !conf)
    return -2;
  const int64_t lds_bytes = ((int64_t)D + K) * (int64_t)sizeof(float);
  if (lds_bytes > 64 * 1024) return -2;
  hipLaunchKernelGGL(exit_step_kernel, dim3((unsigned)n), dim3(kThreads), (size_t)lds_bytes, st, emb, active, B, D, K,
                     w, bias, threshold, min_frames, final_pass, sum, cnt, decided, final_logits, used, conf);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int sm_active_compact(const uint8_t* decided, int B, int32_t* active, int32_t* count, hipStream_t st) {
  if (B <= 0 || !decided || !active || !count) return -2;
  hipLaunchKernelGGL(active_compact_kernel, dim3(1), dim3(64), 0, st, decided, B, active, count);
  SM_CHECK_LAUNCH();
  return 0;
}

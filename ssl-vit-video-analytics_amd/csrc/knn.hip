// Weighted k-nearest-neighbour evaluation of frozen features (Wu et al. 2018, the training-free
// probe DINO and others report): the similarity search and the vote.  All fp32:
//   row_rnorm   rn[i] = 1 / sqrt(sum_d x[i][d]^2), 0 for a zero row
//   knn_topk    the k most similar bank rows of every query under a total order, from fp32-input
//               MFMA similarities that are never written to memory as an Nq x Nb matrix
//   knn_vote    scores[s][i][c] = sum over the first ks[s] neighbours of class c of exp(sim / T)
// No atomics.  Every sum has one fixed order and the neighbour order is total, so no result
// depends on the tiling, on the bank partition (`splits`) or on the 16-byte / scalar load form.
#include "common.h"
#include "sm_api.h"

namespace {

// ---------------------------------------------------------------- the total order
// (sim, idx) entries: larger sim first, equal sims (-0 == +0) by lower index, NaN after every
// number (NaNs among themselves by index), an empty slot (idx < 0) after everything.
// Branch-free (bitwise operators on purpose): it runs once per insertion step in every lane.
SM_DEV bool before(float as, int ai, float bs, int bi) {
  const bool an = as != as, bn = bs != bs, lower = ai < bi;
  const bool num = (as > bs) | ((as == bs) & lower);        // false when either is NaN
  const bool nan = bn & (!an | lower);                      // a number before a NaN, two NaNs by index
  return (ai >= 0) & ((bi < 0) | num | nan);
}

SM_DEV float lane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
SM_DEV int lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

// A wave holds one query's sorted list, entry e on lane e (64 entries; the first k are the result).
// insert: the wave-uniform candidate (cs, ci) takes its place, the entries after it move down one lane.
SM_DEV void list_insert(float& ms, int& mi, float cs, int ci, int lane) {
  // lane l - 1's entry by DPP wave_shr:1 (one VALU move, no LDS round trip); lane 0 keeps its own
  const int pi = __builtin_amdgcn_update_dpp(mi, mi, 0x138, 0xf, 0xf, false);
  const int msb = __float_as_int(ms);
  const float ps = __int_as_float(__builtin_amdgcn_update_dpp(msb, msb, 0x138, 0xf, 0xf, false));
  const bool bme = before(cs, ci, ms, mi);
  const bool bprev = (lane > 0) & before(cs, ci, ps, pi);
  ms = bme ? (bprev ? ps : cs) : ms;
  mi = bme ? (bprev ? pi : ci) : mi;
}

// offer: one candidate per lane (c, cj; `valid` false: none).  Only the candidates that come
// before the k-th entry are inserted, lowest lane first; the threshold is re-read after each.
SM_DEV void list_offer(float& ms, int& mi, float c, int cj, bool valid, int k, int lane) {
  float ts = lane_f(ms, k - 1);
  int ti = lane_i(mi, k - 1);
  uint64_t m = __ballot(valid & before(c, cj, ts, ti));
  while (m) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    list_insert(ms, mi, lane_f(c, src), lane_i(cj, src), lane);
    ts = lane_f(ms, k - 1);
    ti = lane_i(mi, k - 1);
    m &= m - 1;
    m &= __ballot(valid & before(c, cj, ts, ti));
  }
}

// ---------------------------------------------------------------- row_rnorm
// One wave per row, four rows per block.  Lane l adds x[d]^2 for d = l, l + 64, ... ascending with
// one fmaf each; the 64 partials are added by the xor butterfly (offsets 32, 16, ..., 1).
__global__ __launch_bounds__(256) void row_rnorm_kernel(const float* __restrict__ x, int64_t N, int D,
                                                        float* __restrict__ rn) {
  const int lane = threadIdx.x & 63;
  const int64_t r = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  if (r >= N) return;                                  // wave-uniform
  const float* p = x + r * D;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) ss = fmaf(p[d], p[d], ss);
  ss = wave_sum(ss);
  if (lane == 0) rn[r] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
}

// ---------------------------------------------------------------- knn_topk
// Block = 4 waves = a tile of kTQ queries against one bank partition, walked in tiles of kTB rows.
// Wave (wm, wn) of the 2 x 2 grid holds a 32 x 64 piece of the tile's dot products in two
// v_mfma_f32_32x32x2_f32 accumulators; each accumulator element is one fmaf chain over d ascending
// (D padded with zeros to a multiple of kBK: a zero product leaves the sum as it is), so a pair's
// dot product does not depend on where the pair lies in a tile.  The operands go through LDS in
// chunks of kBK columns, the next chunk's global loads in flight under the current chunk's MFMAs.
// The finished tile goes to LDS, and wave w selects for queries 16 w .. 16 w + 15, their sorted
// lists in registers (one entry per lane).
constexpr int kTQ = 64, kTB = 128, kBK = 32, kLDK = kBK + 1, kLDS = kTB + 4, kQW = kTQ / 4;

struct KnnArgs {
  const float *q, *b, *rq, *rb;
  int Nq, Nb, D, k, per;            // per: bank rows per partition
  int64_t self_offset;
  float* osim;                      // [gridDim.y][Nq][k]
  int32_t* oidx;
};

// NV 16-byte groups per thread of a [rows][kBK] chunk: group f = tid + 256 i is row f / 8,
// columns 4 (f % 8) .. + 3.  VEC (D % 4 == 0, 16-byte aligned bases) loads a group at once, the
// scalar form element by element: the same values either way.
template <bool VEC, int NV>
SM_DEV void chunk_load(const float* __restrict__ base, int D, int row0, int row_end, int k0, f32x4* v) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int f = threadIdx.x + 256 * i;
    const int gr = row0 + (f >> 3), gk = k0 + (f & 7) * 4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (gr < row_end) {
      const float* p = base + (int64_t)gr * D + gk;
      if constexpr (VEC) {
        if (gk < D) a = *(const f32x4*)p;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (gk + j < D) a[j] = p[j];
      }
    }
    v[i] = a;
  }
}

template <int NV>
SM_DEV void chunk_store(float* lds, const f32x4* v) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int f = threadIdx.x + 256 * i;
    float* d = lds + (f >> 3) * kLDK + (f & 7) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = v[i][j];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void knn_topk_kernel(KnnArgs a) {
  __shared__ float lq[kTQ * kLDK], lb[kTB * kLDK], ls[kTQ * kLDS], lrq[kTQ];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, h = l >> 5, l31 = l & 31;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 64;
  const int q0 = blockIdx.x * kTQ;
  const int q_end = a.Nq;
  const int64_t jb64 = (int64_t)blockIdx.y * a.per;
  const int jb = (int)(jb64 < a.Nb ? jb64 : a.Nb);
  const int je = (int)(jb64 + a.per < a.Nb ? jb64 + a.per : a.Nb);
  if (tid < kTQ) lrq[tid] = q0 + tid < q_end ? (a.rq ? a.rq[q0 + tid] : 1.0f) : 0.f;

  float lsim[kQW];
  int lidx[kQW];
#pragma unroll
  for (int i = 0; i < kQW; ++i) {
    lsim[i] = -INFINITY;
    lidx[i] = -1;
  }
  const int nchunks = (a.D + kBK - 1) / kBK;

  for (int j0 = jb; j0 < je; j0 += kTB) {
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    f32x4 vq[2], vb[4];
    chunk_load<VEC, 2>(a.q, a.D, q0, q_end, 0, vq);
    chunk_load<VEC, 4>(a.b, a.D, j0, je, 0, vb);
    for (int c = 0; c < nchunks; ++c) {
      chunk_store<2>(lq, vq);
      chunk_store<4>(lb, vb);
      __syncthreads();
      if (c + 1 < nchunks) {
        chunk_load<VEC, 2>(a.q, a.D, q0, q_end, (c + 1) * kBK, vq);
        chunk_load<VEC, 4>(a.b, a.D, j0, je, (c + 1) * kBK, vb);
      }
#pragma unroll
      for (int s = 0; s < kBK / 2; ++s) {
        const float qa = lq[(wm + l31) * kLDK + 2 * s + h];
        const float b0 = lb[(wn + l31) * kLDK + 2 * s + h];
        const float b1 = lb[(wn + 32 + l31) * kLDK + 2 * s + h];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa, b1, acc1, 0, 0, 0);
      }
      __syncthreads();
    }
    // the previous tile's selection ended before the K loop's barriers: ls is free
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm + (r & 3) + 8 * (r >> 2) + 4 * h;
      ls[row * kLDS + wn + l31] = acc0[r];
      ls[row * kLDS + wn + 32 + l31] = acc1[r];
    }
    __syncthreads();
    float rbv[2];
    int cj[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      cj[r] = j0 + l + 64 * r;
      rbv[r] = (a.rb && cj[r] < je) ? a.rb[cj[r]] : 1.0f;
    }
#pragma unroll
    for (int qi = 0; qi < kQW; ++qi) {
      const int qrow = w * kQW + qi, qg = q0 + qrow;
      if (qg < q_end) {                                  // wave-uniform
        const float rqv = lrq[qrow];
        const int64_t ex64 = a.self_offset >= 0 ? qg + a.self_offset : -1;
        const int excl = ex64 < a.Nb ? (int)ex64 : -1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const float sim = (ls[qrow * kLDS + l + 64 * r] * rqv) * rbv[r];
          list_offer(lsim[qi], lidx[qi], sim, cj[r], cj[r] < je && cj[r] != excl, a.k, l);
        }
      }
    }
  }
  if (l < a.k) {
#pragma unroll
    for (int qi = 0; qi < kQW; ++qi) {
      const int qg = q0 + w * kQW + qi;
      if (qg < q_end) {
        const int64_t o = ((int64_t)blockIdx.y * a.Nq + qg) * a.k + l;
        a.osim[o] = lsim[qi];
        a.oidx[o] = lidx[qi];
      }
    }
  }
}

// Phase two of a split search: one wave per query offers the partitions' lists, partition 0
// first, to an empty list.  The order is total, so the result is the unsplit search's.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ psim, const int32_t* __restrict__ pidx,
                                                        int Nq, int k, int splits, float* __restrict__ osim,
                                                        int32_t* __restrict__ oidx) {
  const int l = threadIdx.x & 63;
  const int64_t q = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6);
  if (q >= Nq) return;                                 // wave-uniform
  float ms = -INFINITY;
  int mi = -1;
  for (int p = 0; p < splits; ++p) {
    const int64_t o = ((int64_t)p * Nq + q) * k + l;
    const float c = l < k ? psim[o] : 0.f;
    const int cj = l < k ? pidx[o] : -1;
    list_offer(ms, mi, c, cj, cj >= 0, k, l);
  }
  if (l < k) {
    osim[q * k + l] = ms;
    oidx[q * k + l] = mi;
  }
}

constexpr int kMaxSplits = 1024;

// splits = 0: as many partitions as keep the grid within one round of two blocks per CU on a
// 256-CU part (a 513th block would run alone after the others), none shorter than 1024 rows
int resolve_splits(int64_t Nq, int64_t Nb, int splits) {
  if (splits != 0) return splits;
  const int64_t qt = (Nq + kTQ - 1) / kTQ;
  int64_t s = 512 / qt;
  const int64_t cap = Nb / 1024;
  if (s > cap) s = cap;
  if (s > 64) s = 64;
  return s < 1 ? 1 : (int)s;
}

bool knn_shape_ok(int64_t Nq, int64_t Nb, int k, int splits) {
  return Nq >= 1 && Nb >= 1 && Nq <= 0x7fffff00 && Nb <= 0x7fffff00 && k >= 1 && k <= 64 && splits >= 0 &&
         splits <= kMaxSplits;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// ---------------------------------------------------------------- knn_vote
struct VoteKs {
  int n;
  int ks[SM_KNN_MAX_KS];
};

// One wave per query.  Lane r holds neighbour r's class and weight; lane 0 adds them to the
// class table in LDS in rank order, and the table is copied out each time a ks[s] is reached.
__global__ __launch_bounds__(64) void knn_vote_kernel(const int32_t* __restrict__ idx, const float* __restrict__ sim,
                                                      int64_t Nq, int k, const int64_t* __restrict__ labels, int64_t Nb,
                                                      int C, float inv_t, VoteKs ks, float* __restrict__ scores) {
  extern __shared__ float acc[];                       // C floats
  const int l = threadIdx.x;
  const int64_t q = blockIdx.x;
  for (int c = l; c < C; c += 64) acc[c] = 0.f;
  int lab = -1;
  float wt = 0.f;
  if (l < k) {
    const int j = idx[q * k + l];
    const float s = sim[q * k + l];
    if (j >= 0 && j < Nb && s == s) {
      const int64_t y = labels[j];
      if (y >= 0 && y < C) {
        lab = (int)y;
        wt = expf(s * inv_t);
      }
    }
  }
  __syncthreads();
  int r = 0;
  for (int s = 0; s < ks.n; ++s) {
    for (; r < ks.ks[s]; ++r) {
      const int c = lane_i(lab, r);
      const float wv = lane_f(wt, r);
      if (l == 0 && c >= 0) acc[c] += wv;
    }
    __syncthreads();
    float* out = scores + ((int64_t)s * Nq + q) * C;
    for (int c = l; c < C; c += 64) out[c] = acc[c];
    __syncthreads();
  }
}

}  // namespace

extern "C" int sm_row_rnorm(const float* x, int64_t N, int D, float* rn, hipStream_t st) {
  if (N <= 0 || D <= 0 || !x || !rn || !aligned4(x) || !aligned4(rn)) return -2;
  const int64_t nblk = (N + 3) / 4;
  if (nblk > 0x7fffffff) return -2;
  hipLaunchKernelGGL(row_rnorm_kernel, dim3((unsigned)nblk), dim3(256), 0, st, x, N, D, rn);
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_knn_topk_workspace_bytes(int64_t Nq, int64_t Nb, int k, int splits) {
  if (!knn_shape_ok(Nq, Nb, k, splits)) return 0;
  const int s = resolve_splits(Nq, Nb, splits);
  return s > 1 ? (int64_t)s * Nq * k * 8 : 0;
}

extern "C" int sm_knn_topk(const float* q, int64_t Nq, const float* b, int64_t Nb, int D, const float* rq,
                           const float* rb, int k, int64_t self_offset, int splits, int32_t* idx, float* sim, void* ws,
                           int64_t ws_bytes, hipStream_t st) {
  if (!knn_shape_ok(Nq, Nb, k, splits) || D < 1 || !q || !b || !idx || !sim || (rq == nullptr) != (rb == nullptr))
    return -2;
  if (!aligned4(q) || !aligned4(b) || !aligned4(idx) || !aligned4(sim) || (rq && (!aligned4(rq) || !aligned4(rb))))
    return -2;
  const int s = resolve_splits(Nq, Nb, splits);
  KnnArgs a{};   // more partitions than rows leaves the surplus ones empty, which the merge handles
  a.q = q;
  a.b = b;
  a.rq = rq;
  a.rb = rb;
  a.Nq = (int)Nq;
  a.Nb = (int)Nb;
  a.D = D;
  a.k = k;
  a.per = (int)((Nb + s - 1) / s);
  a.self_offset = self_offset;
  if (s > 1) {
    const int64_t need = sm_knn_topk_workspace_bytes(Nq, Nb, k, splits);
    if (!ws || ws_bytes < need || !aligned16(ws)) return -4;
    a.osim = (float*)ws;
    a.oidx = (int32_t*)((char*)ws + (int64_t)s * Nq * k * 4);
  } else {
    a.osim = sim;
    a.oidx = idx;
  }
  const dim3 grid((unsigned)((Nq + kTQ - 1) / kTQ), (unsigned)s);
  DISPATCH_BOOL(D % 4 == 0 && aligned16(q) && aligned16(b), VEC,
                hipLaunchKernelGGL(knn_topk_kernel<VEC>, grid, dim3(256), 0, st, a));
  SM_CHECK_LAUNCH();
  if (s > 1) {
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, st, a.osim, a.oidx, (int)Nq, k, s,
                       sim, idx);
    SM_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int sm_knn_vote(const int32_t* idx, const float* sim, int64_t Nq, int k, const int64_t* labels, int64_t Nb,
                           int C, float inv_temperature, const int32_t* ks, int nk, float* scores, hipStream_t st) {
  if (Nq < 1 || Nq > 0x7fffffff || Nb < 1 || k < 1 || k > 64 || C < 1 || C > SM_LOGITS_MAX_CLASSES || nk < 1 ||
      nk > SM_KNN_MAX_KS || !idx || !sim || !labels || !ks || !scores)
    return -2;
  VoteKs v{};
  v.n = nk;
  for (int s = 0; s < nk; ++s) {
    if (ks[s] < 1 || ks[s] > k || (s > 0 && ks[s] <= ks[s - 1])) return -2;
    v.ks[s] = ks[s];
  }
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)Nq), dim3(64), (size_t)C * sizeof(float), st, idx, sim, Nq, k,
                     labels, Nb, C, inv_temperature, v, scores);
  SM_CHECK_LAUNCH();
  return 0;
}

// Fused multi-head attention (flash-style, no score matrix in HBM), forward and
// backward, for the TinyViT encoder (head_dim 32, L = 3136 / 784, reference
// tiny_vit.py:86-106 -> F.scaled_dot_product_attention) and the MAE decoder
// (head_dim 64, L = T*784, torch MultiheadAttention inside
// nn.TransformerEncoderLayer, mae_vit_adapter.py:40-48).
//
// Operands are read straight out of the packed projection output
//   qkv[n][l][3][h][d]      (row stride 3*H*D)        — Linear(C, 3C) output
// and the output is written as O[n][l][h][d] (= [N*L, C]), i.e. exactly the
// `transpose(1,2).reshape(B,L,C)` layout the following projection consumes, so
// no permute copies exist anywhere.  LSE[n][h][l] (natural log, fp32) is kept
// for the backward.  Backward writes dqkv in the same packed layout.
//
// bf16 kernels: 4 waves x 32 query rows, 64-key tiles in LDS.  The score tile is
// computed transposed (S^T = K Q^T on v_mfma_f32_32x32x16_bf16) so each lane owns
// one query column: the online-softmax max/sum are in-register plus one
// cross-half exchange, the per-row rescale is a per-lane multiply, and P^T feeds
// the P.V MFMA directly from the accumulator registers.  V (and in the backward
// Q / dO / K) are read transposed from LDS with ds_read_b64_tr_b16.
//
// f32 kernels (parity mode): one thread per query (fwd, dQ) or key (dK/dV) with
// LDS-staged tiles; exact fp32.
//
// The pieces the kernels share are defined once, ahead of the kernels: HeadView (operand
// pointers of one (sample, head)), TilePipe / QdoPipe (the two-operand LDS tile pipelines),
// ragged_tiles (the tile loop with its own last-tile instantiation), the dropout-mask
// convention (drop_hash_in and friends, dkdv_*), dq_prologue and the store_acc* epilogues.
#include <type_traits>

#include "common.h"
#include "sm_api.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr float NEG_BIG = -1e30f;

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

struct AttnArgs {
  const void* qkv;   // [N][L][3][H][D]
  void* out;         // fwd: O [N][L][H][D]; bwd: dqkv [N][L][3][H][D]
  const void* o;     // bwd: O
  const void* dout;  // bwd: dO [N][L][H][D]
  float* lse;        // [N][H][L]
  float* delta;      // [N][H][L]  rowsum(dO * O)
  __bf16* qc;        // bwd (bf16): bf16(Q * scale * log2 e) [N][L][H][D], written by the dQ kernel
  int N, L, H;
  float scale;
  float drop_p;      // dropout on attention probabilities (0 = off)
  uint64_t seed;
};

// One (sample, head)'s operands: its q / k / v rows inside packed qkv (row stride ldq), its
// column offset in an [N][L][H][D] tensor (O, dO, qc; row stride C -- and dqkv, row stride
// ldq, through out()) and its row in an [N][H][L] tensor (lse, delta).
template <typename T, int D>
struct HeadView {
  int C, ldq, col;
  const T *q, *k, *v;
  int64_t row0, orow, lrow;
  SM_DEV HeadView(const AttnArgs& a, int n, int hd) {
    C = a.H * D;
    ldq = 3 * C;
    col = hd * D;
    row0 = (int64_t)n * a.L;
    const T* qkv = (const T*)a.qkv + (int64_t)n * a.L * ldq;
    q = qkv + hd * D;
    k = qkv + C + hd * D;
    v = qkv + 2 * C + hd * D;
    orow = (int64_t)n * a.L * C + hd * D;
    lrow = ((int64_t)n * a.H + hd) * a.L;
  }
  // this head's columns of row `row` of a.out, whose rows are ld (C or ldq) elements
  SM_DEV T* out(const AttnArgs& a, int row, int ld) const { return (T*)a.out + (row0 + row) * ld + col; }
};

// ---------- LDS images for a [rows][D] bf16 tile (row = key or query) -------------
// Row reads (ds_read_b128 of 8 consecutive d) and transposed reads
// (ds_read_b64_tr_b16 of 4 consecutive rows) both address through tile_off.
//
// S16: the 16x16x32 kernels' image of the same tile: row reads take rows c = l & 15 at chunk
// 4 ks + (l >> 4), transposed reads rows 4 (l >> 4) + (c >> 2) at columns 16 dt + 4 (c & 3),
// which the 32x32x16 swizzle serves 2-way on both kinds (SQ_LDS_BANK_CONFLICT ~ 1.3x
// the LDS-active cycles of the first 16x16 build, profiles/r06i_attn_sq.txt).  XORing the
// chunk with 2 ((row >> 1) & 3) (D = 64: two rows per 256-B bank row) or 2 ((row >> 2) & 1)
// (D = 32: four) makes every ds_read_b128 lane group and every ds_read_b64_tr_b16 half-wave
// cover the 64 banks once (checked against the guide's lane groups by enumeration).
template <int D, bool S16 = false>
SM_DEV int tile_off(int row, int d) {
  int chunk = d >> 3;
  if (S16) chunk ^= D == 64 ? 2 * ((row >> 1) & 3) : ((row >> 2) & 1) << 1;
  else chunk ^= D == 64 ? (((row >> 1) & 1) << 2) ^ ((row >> 2) & 3) : (row >> 2) & 3;
  return row * (D * 2) + (chunk << 4) + ((d & 7) << 1);
}

// combine a value with the lane 32 apart (the other half-wave) by v_permlane32_swap
// (no LDS round trip): the two results hold {own, other} in either order
SM_DEV float halves_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
SM_DEV float halves_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// sum over the lanes c, c + 16, c + 32, c + 48
SM_DEV float quarters_sum(float v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// 1-D grid over (query/key block, head, sample) with the bijective XCD remap: all
// blocks of one (sample, head) run on the same XCD, so the K/V (or Q/dO) panel they
// all stream is fetched into that XCD's L2 once instead of once per XCD.
struct AttnTile {
  int qb, hd, n;
  SM_DEV AttnTile(int nqb, int H) {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
    qb = v % nqb;
    hd = (v / nqb) % H;
    n = v / (nqb * H);
  }
};

SM_DEV uint32_t pack_bf16x2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(uint32_t, v);
}
// accumulator (32x32) -> bf16 B-operand fragment for k-step s (four v_cvt_pk_bf16_f32;
// the per-element form let the compiler mix in v_alignbit / v_perm repacks)
SM_DEV bf16x8 acc_to_frag(const f32x16& a, int s) {
  const int o = 8 * s;
  return __builtin_bit_cast(bf16x8, make_uint4(pack_bf16x2(a[o], a[o + 1]), pack_bf16x2(a[o + 2], a[o + 3]),
                                               pack_bf16x2(a[o + 4], a[o + 5]), pack_bf16x2(a[o + 6], a[o + 7])));
}
SM_DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// zero an accumulator vector, or an array of them (accumulators that start at zero are `= {}`)
template <typename V>
SM_DEV void zero_acc(V& v) {
#pragma unroll
  for (int i = 0; i < (int)(sizeof(V) / sizeof(float)); ++i) v[i] = 0.f;
}
template <typename V, int N>
SM_DEV void zero_acc(V (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) zero_acc(a[i]);
}

// ---------- attention-probability dropout mask ------------------------------------
// keep(row, col), row = (n*H + hd)*L + q, col = key:
//   h    = mix24(seed32 + row * AG + (col >> 2) * AC)     one hash per 4 keys
//   keep = (byte (col & 3) of h) & 0x7F >= round(128 p)   (p = 0.1: 13/128 dropped)
// and a kept probability is scaled by 128 / (128 - round(128 p)).
// common.h's fmix32 input, but mixed with 24-bit multiplies (v_mul_u32_u24, full
// rate) instead of fmix32's 32-bit ones (v_mul_lo_u32, quarter rate): these kernels
// are bound by VALU issue, and the hash was the largest item in it.  Every term
// that varies along a kernel's tile loop is wave-uniform (scalar ALU), so a hash
// costs one vector add plus the 6-op mix.  (Keep rate, row/column balance and
// neighbour correlations measured equal to fmix32's on 4096 x 4096 masks.)
constexpr uint32_t AG = 0x9E3779B1u;   // row multiplier
constexpr uint32_t AC = 0x7FEB352Du;   // column-group multiplier
SM_DEV uint32_t mix24(uint32_t x) {
  x ^= x >> 16;
  x = (x & 0xFFFFFFu) * 0xEBCA6Bu;
  x ^= x >> 13;
  x = (x & 0xFFFFFFu) * 0xB2AE35u;
  x ^= x >> 16;
  return x;
}
// The hash input of query `row` (0 .. L-1 of head (n, hd)) and key group `group` = col >> 2.
// Every kernel forms its lane-varying part once with drop_hash_in (the forward and dQ: the
// lane's query and its key group inside a tile; dK/dV: the lane's row inside a tile and its
// key's group) and adds the wave-uniform rest per tile: drop_groups(key groups) along the
// forward's and dQ's key loop, drop_rows(query rows) along dK/dV's query loop.
SM_DEV uint32_t drop_hash_in(const AttnArgs& a, int n, int hd, int row, int group) {
  return seed32(a.seed) + (uint32_t)((uint64_t)(n * a.H + hd) * a.L + row) * AG + (uint32_t)group * AC;
}
SM_DEV uint32_t drop_rows(int rows) { return (uint32_t)rows * AG; }
SM_DEV uint32_t drop_groups(int groups) { return (uint32_t)groups * AC; }
SM_DEV uint32_t attn_thr(float p) { return (uint32_t)(p * 128.f + 0.5f); }
// keep-value scale 128 / (128 - thr): the inverse of the quantised keep rate (E[mask * scale] = 1)
SM_DEV float attn_drop_scale(float p) {
  const uint32_t t = attn_thr(p);
  return t >= 128u ? 0.f : 128.f / (float)(128u - t);
}
SM_DEV bool attn_keep_byte(uint32_t h, int j, uint32_t thr) { return ((h >> (8 * j)) & 0x7Fu) >= thr; }

// Packed form for bf16 P pairs: bit 7 of byte j of keep_flags() is keep(j) (7-bit
// SWAR compare: (b & 0x7F) + 128 - thr never carries out of its byte), and v_perm's
// sign-replicating selectors (8/9: bit 15/31 of the second source, 10/11: of the
// first) expand two flags into a 16-bit-per-element mask in one instruction.
SM_DEV uint32_t keep_flags(uint32_t h, uint32_t thr) { return (h & 0x7F7F7F7Fu) + (128u - thr) * 0x01010101u; }
SM_DEV uint32_t keep_mask01(uint32_t y) { return __builtin_amdgcn_perm(y << 8, y, 0x08080A0Au); }   // bytes 0, 1
SM_DEV uint32_t keep_mask23(uint32_t y) { return __builtin_amdgcn_perm(y << 8, y, 0x09090B0Bu); }   // bytes 2, 3
// Per-element form for fp32 operands: keep_bytes() turns the four flags into bytes
// 0xFF / 0x00 (one v_perm), and keep_sel() ANDs v with its byte sign-extended to 32
// bits, which the compiler's SDWA peephole folds into one v_and_b32_sdwa (operand
// select BYTE_j with sext) -- one instruction per element, where its lowering of
// `keep ? v : 0` is byte extract + compare + select.  (Written in plain C so the
// compiler still inserts the MFMA / transcendental read-after-write wait states an
// inline-asm operand would not get.)
SM_DEV uint32_t keep_bytes(uint32_t y) { return __builtin_amdgcn_perm(y << 8, y, 0x090B080Au); }
SM_DEV float keep_sel(float v, uint32_t kb, int j) {
  const uint32_t m = (uint32_t)(int32_t)(int8_t)(kb >> (8 * j));
  return __uint_as_float(__float_as_uint(v) & m);
}

// dropout keep multiplier for P[n,hd,q,k] (f32 kernels)
SM_DEV float drop_keep_scale(const AttnArgs& a, int n, int hd, int q, int k) {
  const uint32_t h = mix24(drop_hash_in(a, n, hd, q, k >> 2));
  return attn_keep_byte(h, k & 3, attn_thr(a.drop_p)) ? attn_drop_scale(a.drop_p) : 0.0f;
}

// 4x4 byte transpose inside a DPP quad: lane i's byte j <- lane j's byte i.  Stage 1
// swaps 16-bit halves with lane i^2, stage 2 bytes with lane i^1 (v_perm selectors
// per lane: quad_sel1 / quad_sel2).
SM_DEV uint32_t quad_transpose_bytes(uint32_t v, uint32_t sel1, uint32_t sel2) {
  const uint32_t p = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);   // lane ^ 2
  v = __builtin_amdgcn_perm(p, v, sel1);
  const uint32_t q = (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);   // lane ^ 1
  return __builtin_amdgcn_perm(q, v, sel2);
}

// The dK/dV kernels' dropout plumbing.  Their lanes hold keys, so a lane hashes the row
// 4 (lane group) + kq, kq = l & 3, of each 4-row group and the quad byte transpose (selectors
// quad_sel1 / quad_sel2 of kq) hands every lane its own key's four rows: dkdv_keep4 returns
// their keep bytes for keep_sel.  The row constants are folded: log2 of the keep scale ks =
// 128/(128-thr) into the LSE (the exp yields P ks, whose kept elements are P' directly: dV needs
// no final scale), and Delta is stored as Delta / ks (dS = P' dP - (P ks) (Delta / ks) = P' dP -
// P Delta).  Without dropout the dP accumulator starts at -Delta instead (dS = P * acc).
template <bool DROP>
SM_DEV float dkdv_lkeep(float ks) { return DROP ? -log2f(ks) : 0.f; }                   // added to LSE2
template <bool DROP>
SM_DEV float dkdv_dkeep(float ks) { return DROP ? (ks > 0.f ? 1.f / ks : 0.f) : -1.f; }   // Delta's factor
SM_DEV uint32_t quad_sel1(int kq) { return (kq & 2) ? 0x03020706u : 0x05040100u; }
SM_DEV uint32_t quad_sel2(int kq) { return (kq & 1) ? 0x03070105u : 0x06020400u; }
SM_DEV uint32_t dkdv_keep4(uint32_t hash_in, uint32_t sel1, uint32_t sel2, uint32_t thr) {
  return keep_bytes(keep_flags(quad_transpose_bytes(mix24(hash_in), sel1, sel2), thr));
}

// Row-per-lane epilogue of a 32x32 accumulator tile (lane l: row l & 31; half-wave h = l >> 5
// holds columns 8g + 4h .. + 3 of 8-column group g): each pair of groups (g, g + 1) leaves as
// ONE 16-B store per lane instead of two 8-B stores (MI355X guide T21: the tail is bound by
// store issue, not bytes).  Two v_permlane32_swap per pair hand the lower half-wave the upper
// half's columns of group g and the upper half the lower half's of group g + 1: the lower
// lanes then hold columns 8g .. 8g + 7, the upper lanes 8g + 8 .. 8g + 15.  Every lane must
// execute it (EXEC full: the swap reads the partner lane); the caller predicates the store.
// va / vb: this lane's 4 values of groups g / g + 1; returns the 16 B for column 8 (g + h).
SM_DEV uint4 wide_pair(const float (&va)[4], const float (&vb)[4]) {
  const uint32_t a0 = pack_bf16x2(va[0], va[1]), a1 = pack_bf16x2(va[2], va[3]);
  const uint32_t b0 = pack_bf16x2(vb[0], vb[1]), b1 = pack_bf16x2(vb[2], vb[3]);
  const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
  const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
  return make_uint4(r0[0], r1[0], r0[1], r1[1]);
}
// acc (NT 32-column tiles of the lane's row) x scale -> the row's bf16 at `row`, stored if ok
template <int NT>
SM_DEV void store_acc32(__bf16* row, const f32x16 (&acc)[NT], float scale, bool ok, int h) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; g += 2) {
      float va[4], vb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        va[i] = acc[t][4 * g + i] * scale;
        vb[i] = acc[t][4 * g + 4 + i] * scale;
      }
      const uint4 w16 = wide_pair(va, vb);
      if (ok) *(uint4*)(row + 32 * t + 8 * g + 8 * h) = w16;
    }
}
// the 16x16 kernels' epilogue: lane (c, g) holds [row c][16 dt + 4g + i] of DT tiles: 8-B runs
// (`row` points at column 4g of the lane's row)
template <int DT>
SM_DEV void store_acc16(__bf16* row, const f32x4 (&acc)[DT], float scale) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    *(uint2*)(row + 16 * dt) = make_uint2(pack_bf16x2(acc[dt][0] * scale, acc[dt][1] * scale),
                                          pack_bf16x2(acc[dt][2] * scale, acc[dt][3] * scale));
}

// Per-thread plan for staging a [ROWS][D] bf16 tile (rows of a [L][ld] matrix) into
// the LDS image: byte offsets and LDS offsets are computed once; each tile is then
// CH 16-byte raw buffer loads issued early into registers (prefetch) and CH 16-byte
// LDS stores after the barrier.  The tile's descriptor (scalar) carries the base
// and num_records = valid rows x row bytes, so rows past L read as zero with no
// per-lane address arithmetic, compare or branch in the tile loop.
template <int D, int ROWS, int NT = 256, bool S16 = false>
struct Stager {
  static constexpr int CH = ROWS * D / 8 / NT;
  static_assert(CH >= 1 && CH * NT * 8 == ROWS * D, "tile must split evenly over the block's threads");
  uint32_t voff[CH];
  int loff[CH], ld;
  SM_DEV void init(int ld_) {
    ld = ld_;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = threadIdx.x + NT * i;
      const int row = c / (D / 8), d = (c % (D / 8)) * 8;
      voff[i] = (uint32_t)(row * ld + d) * 2u;
      loff[i] = tile_off<D, S16>(row, d);
    }
  }
  SM_DEV void load(const __bf16* base, int rows_left, uint4 (&r)[CH]) const {
    const int rows = rows_left < ROWS ? rows_left : ROWS;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, rows * ld * 2, 0x00020000);
#pragma unroll
    for (int i = 0; i < CH; ++i) r[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[i], 0, 0));
  }
  SM_DEV void store(char* lds, const uint4 (&r)[CH]) const {
#pragma unroll
    for (int i = 0; i < CH; ++i) *(uint4*)(lds + loff[i]) = r[i];
  }
};

// The tile pipeline of two operands a, b (K and V, or Q and dO: rows of [L][ld] matrices) in
// 64-row tiles: prime() prefetches tile 0 into registers; enter(r0, la, lb) is barrier, store
// the prefetched registers to LDS, barrier, prefetch the tile after r0 under r0's math.
template <int D, int NT, bool S16>
struct TilePipe {
  static constexpr int RT = 64;
  using St = Stager<D, RT, NT, S16>;
  St stg;
  uint4 ra[St::CH], rb[St::CH];
  const __bf16 *a, *b;
  int ld, L;
  SM_DEV void init(const __bf16* a_, const __bf16* b_, int ld_, int L_) {
    a = a_; b = b_; ld = ld_; L = L_;
    stg.init(ld);
  }
  SM_DEV void prime() {
    stg.load(a, L, ra);
    stg.load(b, L, rb);
  }
  SM_DEV void commit(char* la, char* lb) {
    __syncthreads();
    stg.store(la, ra);
    stg.store(lb, rb);
  }
  SM_DEV bool fetch_next(int r0) {
    __syncthreads();
    if (r0 + RT >= L) return false;
    stg.load(a + (int64_t)(r0 + RT) * ld, L - r0 - RT, ra);
    stg.load(b + (int64_t)(r0 + RT) * ld, L - r0 - RT, rb);
    return true;
  }
  SM_DEV void enter(int r0, char* la, char* lb) {
    commit(la, lb);
    fetch_next(r0);
  }
};

// The dK/dV kernels' Q / dO pipeline: TilePipe plus the tile's row constants (LSE, Delta),
// prefetched with its Q / dO rows (wave 0, one row per lane, index clamped: no branch; loading
// them between the two barriers held every wave of the block for a global-load round trip per
// tile) and stored negated with the keep scale folded in (dkdv_lkeep / dkdv_dkeep): llse = -(LSE2 + lkeep),
// -1e30 for rows past L (P = 0); ldel = Delta dkeep.
template <int D, int NT, bool S16>
struct QdoPipe : TilePipe<D, NT, S16> {
  using TP = TilePipe<D, NT, S16>;
  float rlse = 0.f, rdel = 0.f;
  const float *lse, *del;
  SM_DEV void rowc_load(int q0) {
    if (threadIdx.x < TP::RT) {
      const int qq = min(q0 + (int)threadIdx.x, this->L - 1);
      rlse = lse[qq];
      rdel = del[qq];
    }
  }
  SM_DEV void prime(const float* lse_, const float* del_) {
    lse = lse_; del = del_;
    TP::prime();
    rowc_load(0);
  }
  SM_DEV void enter(int q0, char* lq, char* ldo, float* llse, float* ldel, float lkeep, float dkeep) {
    this->commit(lq, ldo);
    if (threadIdx.x < TP::RT) {
      const bool ok = q0 + (int)threadIdx.x < this->L;
      llse[threadIdx.x] = ok ? -fmaf(rlse, LOG2E, lkeep) : -1e30f;
      ldel[threadIdx.x] = ok ? rdel * dkeep : 0.f;
    }
    if (this->fetch_next(q0)) rowc_load(q0 + TP::RT);
  }
};

// The tile loop: the ragged last tile is its own instantiation of the body (the compiler turned
// a uniform `if (ragged)` key-range masking into per-element selects executed on EVERY tile,
// ~80 VALU per tile of the d=32 kernels)
template <int RT, typename F>
SM_DEV void ragged_tiles(int L, F&& tile) {
  int r0 = 0;
  for (; r0 + RT <= L; r0 += RT) tile(r0, std::false_type{});
  if (r0 < L) tile(r0, std::true_type{});
}

// LDS byte offsets of this lane's fragments (u = 0, s = 0; +32 rows per u and +16
// rows per s keep the swizzle bits, so those are immediate offsets).
// A/B fragment of 8 consecutive d for row l & (R - 1) of an R-row MFMA operand (R = 32: k-step
// s covers 16 d; R = 16, on the S16 image: 32 d)
template <int D, int R = 32>
SM_DEV int row_frag_off(int s) {
  const int l = threadIdx.x & 63;
  return tile_off<D, R == 16>(l & (R - 1), 512 / R * s + 8 * (l / R));
}
template <int D>
SM_DEV void tr_frag_off(int t, int& lo, int& hi) {
  const int l = threadIdx.x & 63;
  const int h = l >> 5, g1 = (l >> 4) & 1, i = l & 15, q = i >> 2, p = i & 3;
  const int col = 32 * t + 16 * g1 + 4 * p;
  lo = tile_off<D>(4 * h + q, col);
  hi = tile_off<D>(4 * h + q + 8, col);
}
SM_DEV bf16x8 lds_b128(const char* lds, int off) { return *(const bf16x8*)(lds + off); }
SM_DEV bf16x8 lds_tr(const char* lds, int lo, int hi) {
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + lo));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + hi));
  s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// =============================================================== bf16 forward
// Softmax without a running maximum.  Q is pre-scaled by scale*log2(e) once in registers,
// so the MFMA leaves the exp2 argument itself and the fast pass computes P = exp2(S) with
// no maximum, no subtraction and no rescale of O (softmax is shift-invariant and fp32 /
// bf16 keep their relative precision at any scale: only the exponent range matters).  Per
// score that leaves the exp, the row-sum add and half a bf16 pack (the online-softmax form
// also spent a max, an fma and the rescale bookkeeping: ~45 % of the d = 32 loop's VALU).
// A row whose sum leaves [2^-100, 2^100] or whose O is not finite (scores beyond the
// exponent range: |S| > ~100 in log2 units) makes the block rerun the whole key loop with
// the online (max-tracking) softmax, so results never depend on the fast pass's range.
template <int D, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_fwd_bf16(AttnArgs a) {
  constexpr int KT = 64;
  constexpr int RB = 32 * D * 2;   // bytes of 32 tile rows
  __shared__ __attribute__((aligned(16))) char lk[KT * D * 2];
  __shared__ __attribute__((aligned(16))) char lv[KT * D * 2];
  __shared__ int lbad;
  const AttnTile tl((a.L + 127) / 128, a.H);
  const int n = tl.n, hd = tl.hd;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
  const HeadView<__bf16, D> hv(a, n, hd);
  const int q = tl.qb * 128 + w * 32 + (l & 31);
  // a wave whose 32 query rows all lie past L (the last block of a (sample, head) when L
  // is not a multiple of 128: 3.5 of 4 waves at L = 784) only helps stage the tiles
  const bool wact = tl.qb * 128 + w * 32 < a.L;
  if (threadIdx.x == 0) lbad = 0;   // ordered before any write by the first tile's barriers

  const float c = a.scale * LOG2E;
  bf16x8 qf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (q < a.L) qf[s] = *(const bf16x8*)(hv.q + (int64_t)q * hv.ldq + 16 * s + 8 * h);
    else for (int j = 0; j < 8; ++j) qf[s][j] = (__bf16)0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[s][j] = (__bf16)((float)qf[s][j] * c);
  }
  TilePipe<D, 256, false> kv;
  kv.init(hv.k, hv.v, hv.ldq, a.L);
  int koff[D / 16], vlo[D / 32], vhi[D / 32];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) koff[s] = row_frag_off<D>(s);
#pragma unroll
  for (int t = 0; t < D / 32; ++t) tr_frag_off<D>(t, vlo[t], vhi[t]);

  f32x16 o[D / 32];
  float m = 0.f, lsum = 0.f;
  const uint32_t dlb = drop_hash_in(a, n, hd, q, h);   // this lane's query, this half's key group
  const uint32_t dthr = attn_thr(a.drop_p);

  // one pass over the keys; SAFE: online softmax with the running maximum m
  auto pass = [&](auto safe) {
    constexpr bool SAFE = decltype(safe)::value;
    zero_acc(o);
    m = SAFE ? NEG_BIG : 0.f;
    lsum = 0.f;
    kv.prime();
    ragged_tiles<KT>(a.L, [&](int k0, auto rag) {   // one key tile
      constexpr bool RAGGED = decltype(rag)::value;
      kv.enter(k0, lk, lv);
      if (!wact) return;
      // ragged tile: the second 32-key half has no key below L when <= 32 keys remain (its
      // scores are masked to -inf below either way): no MFMAs for it
      const bool half1 = !RAGGED || k0 + 32 < a.L;
      f32x16 st[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        zero_acc(st[u]);
        if (u == 1 && !half1) continue;
#pragma unroll
        for (int s = 0; s < D / 16; ++s)
          st[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_b128(lk, koff[s] + u * RB), qf[s], st[u], 0, 0, 0);
      }
      if constexpr (RAGGED) {   // keys past L: P = exp2(-huge) = 0
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (k0 + 32 * u + acc_row(r, h) >= a.L) st[u][r] = NEG_BIG;
      }
      float alpha = 1.f, mn = 0.f;
      bool grow = false;
      if constexpr (SAFE) {
        float mt = NEG_BIG;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[u][r]);
        mt = halves_max(mt);
        // rescale only when some row's max grew (exact: alpha == 1 otherwise)
        grow = mt > m;
        mn = grow ? mt : m;
        alpha = grow ? __builtin_amdgcn_exp2f(m - mn) : 1.f;
        m = mn;
      }
      float ps = 0.f;
      uint32_t pw[2][4][2];   // bf16 pairs of P (dropout applied): [u][g][keys 4g+0,1 | 4g+2,3]
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float p4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            p4[j] = __builtin_amdgcn_exp2f(SAFE ? st[u][4 * g + j] - mn : st[u][4 * g + j]);
            ps += p4[j];
          }
          uint32_t w0 = pack_bf16x2(p4[0], p4[1]), w1 = pack_bf16x2(p4[2], p4[3]);
          if (DROP) {   // keys k0+32u+8g+4h+j, j = 0..3, share one hash; masks on the packed pairs
            const uint32_t y = keep_flags(mix24(dlb + drop_groups((k0 >> 2) + 8 * u + 2 * g)), dthr);
            w0 &= keep_mask01(y);
            w1 &= keep_mask23(y);
          }
          pw[u][g][0] = w0;
          pw[u][g][1] = w1;
        }
      }
      if constexpr (SAFE) {
        lsum = lsum * alpha + ps;
        if (__any(grow)) {
#pragma unroll
          for (int t = 0; t < D / 32; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[t][r] *= alpha;
        }
      } else {
        lsum += ps;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          if (u == 1 && !half1) continue;   // P = 0 there
          const bf16x8 pf = __builtin_bit_cast(
              bf16x8, make_uint4(pw[u][2 * s][0], pw[u][2 * s][1], pw[u][2 * s + 1][0], pw[u][2 * s + 1][1]));
#pragma unroll
          for (int t = 0; t < D / 32; ++t)
            o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                lds_tr(lv, vlo[t] + u * RB + s * (RB / 2), vhi[t] + u * RB + s * (RB / 2)), pf, o[t], 0, 0, 0);
        }
    });
    lsum = halves_sum(lsum);
  };
  pass(std::false_type{});
  bool bad = !(lsum >= 0x1p-100f && lsum <= 0x1p100f);
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) bad |= !__builtin_isfinite(o[t][r]);
  if (wact && __any(bad && q < a.L) && l == 0) lbad = 1;
  __syncthreads();
  if (lbad) pass(std::true_type{});   // block-uniform: the rerun's barriers are safe
  store_acc32(hv.out(a, q, hv.C), o, (DROP ? attn_drop_scale(a.drop_p) : 1.f) / lsum, q < a.L, h);
  if (q < a.L && h == 0) a.lse[hv.lrow + q] = (m + log2f(lsum)) * LN2;
}

// =============================================================== delta = rowsum(dO*O)  (f32 backward)
__global__ void attn_delta_kernel(AttnArgs a, int D) {
  // one wave per (n, l) row: H*D values; lanes split over heads
  const int64_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  if (row >= (int64_t)a.N * a.L) return;
  const int C = a.H * D;
  const float* o = (const float*)a.o + row * C;
  const float* dout = (const float*)a.dout + row * C;
  const int n = (int)(row / a.L), q = (int)(row % a.L);
  for (int hd = 0; hd < a.H; ++hd) {
    float s = 0.f;
    for (int d = l; d < D; d += 64) s += o[hd * D + d] * dout[hd * D + d];
    s = wave_sum(s);
    if (l == 0) a.delta[((int64_t)n * a.H + hd) * a.L + q] = s;
  }
}

// =============================================================== bf16 backward dK, dV
// Keys on lanes (32 per wave, 128 per block); Q / dO tiles (64 rows) staged to LDS
// with register prefetch and read both row-wise (S, dP) and transposed (dV, dK).
// Software-pipelined form: per 64-row tile the wave's two 32-row halves u = 0, 1 run
// as  S,dP(0)  S,dP(1) | softmax(0) | dV,dK(0) | softmax(1) | dV,dK(1)  so each
// half's exp / dropout / dS VALU stream has the other half's MFMAs to hide under.
// Row constants (folded into the LDS copies of LSE and Delta): dkdv_lkeep / dkdv_dkeep, QdoPipe.
//
// The Q tiles are the dQ kernel's bf16(Q * scale * log2 e) (a.qc, row stride C) and the S
// accumulator starts at -LSE2 of its query row: the MFMA leaves the exp2 argument itself (one
// VALU op per score fewer than exp2(fma(S, c, -LSE2))), and S is formed from exactly the
// rounded operand the forward and the dQ kernel use (bf16(Q c) . K), so the rebuilt P rows
// match the forward's normalisation.  dK = dS^T Q scale = dS^T Qc ln 2.
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_bwd_dkdv_bf16(AttnArgs a) {
  constexpr int QT = 64;
  constexpr int RB = 32 * D * 2;
  constexpr int KB = 32 * NW;   // keys per block
  __shared__ __attribute__((aligned(16))) char lq[QT * D * 2];
  __shared__ __attribute__((aligned(16))) char ldo[QT * D * 2];
  __shared__ __attribute__((aligned(16))) float llse[QT];
  __shared__ __attribute__((aligned(16))) float ldel[QT];
  const AttnTile tl((a.L + KB - 1) / KB, a.H);
  const int n = tl.n, hd = tl.hd;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
  const HeadView<__bf16, D> hv(a, n, hd);
  const int key = tl.qb * KB + w * 32 + (l & 31);
  const bool wact = tl.qb * KB + w * 32 < a.L;   // else: only stages tiles (see the forward)

  bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    if (key < a.L) {
      kf[s] = *(const bf16x8*)(hv.k + (int64_t)key * hv.ldq + 16 * s + 8 * h);
      vf[s] = *(const bf16x8*)(hv.v + (int64_t)key * hv.ldq + 16 * s + 8 * h);
    } else {
      for (int j = 0; j < 8; ++j) { kf[s][j] = (__bf16)0.f; vf[s][j] = (__bf16)0.f; }
    }
  }
  int roff[D / 16], tlo[D / 32], thi[D / 32];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) roff[s] = row_frag_off<D>(s);
#pragma unroll
  for (int t = 0; t < D / 32; ++t) tr_frag_off<D>(t, tlo[t], thi[t]);

  f32x16 dk[D / 32] = {}, dv[D / 32] = {};
  const int kq = l & 3;
  const float lkeep = dkdv_lkeep<DROP>(attn_drop_scale(a.drop_p));
  // dkdv_dkeep's expression, kept inline: through the helper (or with the scale in a local) this
  // kernel's compare comes out with the other sense or a VGPR more (profiles/attn_cleanup_isa_and_ab.txt)
  const float dkeep = DROP ? (attn_drop_scale(a.drop_p) > 0.f ? 1.f / attn_drop_scale(a.drop_p) : 0.f) : -1.f;
  const uint32_t dthr = attn_thr(a.drop_p), sel1 = quad_sel1(kq), sel2 = quad_sel2(kq);
  const uint32_t dlb = drop_hash_in(a, n, hd, 4 * h + kq, key >> 2);

  // S = Q K^T and dP = dO V^T for query rows q0 + 32u .. +31 (keys on lanes)
  auto sdp = [&](int u, f32x16& sa, f32x16& da) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {   // -LSE2 of rows 32u + 8g + 4h + j (stored negated: no VALU)
      const float4 a4 = *(const float4*)&llse[32 * u + 8 * g + 4 * h];
      sa[4 * g] = a4.x; sa[4 * g + 1] = a4.y; sa[4 * g + 2] = a4.z; sa[4 * g + 3] = a4.w;
    }
    if (DROP) {
      zero_acc(da);
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) {   // -Delta of rows 32u + 8g + 4h + j
        const float4 b4 = *(const float4*)&ldel[32 * u + 8 * g + 4 * h];
        da[4 * g] = b4.x; da[4 * g + 1] = b4.y; da[4 * g + 2] = b4.z; da[4 * g + 3] = b4.w;
      }
    }
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_b128(lq, roff[s] + u * RB), kf[s], sa, 0, 0, 0);
      da = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_b128(ldo, roff[s] + u * RB), vf[s], da, 0, 0, 0);
    }
  };
  // P (dropped, x the keep scale) and dS as bf16 B-operand fragments
  auto softmax = [&](int q0, int u, const f32x16& sa, const f32x16& da, bf16x8 (&pf)[2], bf16x8 (&sf)[2]) {
    f32x16 pv, dsv;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint32_t kb4 = 0;
      if (DROP) kb4 = dkdv_keep4(dlb + drop_rows(q0 + 32 * u + 8 * g), sel1, sel2, dthr);
      float del4[4] = {0.f, 0.f, 0.f, 0.f};
      if (DROP) {
        const float4 b4 = *(const float4*)&ldel[32 * u + 8 * g + 4 * h];
        del4[0] = b4.x; del4[1] = b4.y; del4[2] = b4.z; del4[3] = b4.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 4 * g + j;
        const float p = __builtin_amdgcn_exp2f(sa[r]);
        if (DROP) {
          const float pk = keep_sel(p, kb4, j);
          pv[r] = pk;
          dsv[r] = fmaf(pk, da[r], -(p * del4[j]));
        } else {
          pv[r] = p;
          dsv[r] = p * da[r];
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) { pf[s] = acc_to_frag(pv, s); sf[s] = acc_to_frag(dsv, s); }
  };
  auto dvdk = [&](int u, const bf16x8 (&pf)[2], const bf16x8 (&sf)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < D / 32; ++t) {
        const int ob = u * RB + s * (RB / 2);
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_tr(ldo, tlo[t] + ob, thi[t] + ob), pf[s], dv[t], 0, 0, 0);
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_tr(lq, tlo[t] + ob, thi[t] + ob), sf[s], dk[t], 0, 0, 0);
      }
  };

  QdoPipe<D, 64 * NW, false> pipe;
  pipe.init(a.qc + hv.orow, (const __bf16*)a.dout + hv.orow, hv.C, a.L);
  pipe.prime(a.lse + hv.lrow, a.delta + hv.lrow);
  for (int q0 = 0; q0 < a.L; q0 += QT) {
    pipe.enter(q0, lq, ldo, llse, ldel, lkeep, dkeep);
    if (!wact) continue;
    f32x16 s0, p0, s1, p1;
    bf16x8 pf0[2], sf0[2], pf1[2], sf1[2];
    sdp(0, s0, p0);
    sdp(1, s1, p1);
    softmax(q0, 0, s0, p0, pf0, sf0);
    dvdk(0, pf0, sf0);
    softmax(q0, 1, s1, p1, pf1, sf1);
    dvdk(1, pf1, sf1);
  }
  __bf16* out = hv.out(a, key, hv.ldq);
  store_acc32(out + hv.C, dk, LN2, key < a.L, h);
  store_acc32(out + 2 * hv.C, dv, 1.f, key < a.L, h);
}

// =============================================================== bf16 backward dQ
// The dQ kernels' prologue for query row q, whose lane holds columns CS s + col0 .. + 7 of
// fragment s (CS = D / NF): loads the Q and dO fragments; forms this lane's part of Delta =
// rowsum(dO * O), combines the row's lanes with `rowsum` and has the row's `writer` lane
// store it for the dK/dV kernel, which runs after this one -- no separate Delta pass over O
// and dO; then pre-scales Q by scale * log2(e) in registers (S starts at -LSE2, so the MFMA
// leaves the exp2 argument, as in the dK/dV kernel; dQ = dS K needs no Q) and writes that
// rounded operand to a.qc for the dK/dV kernel's S.  Returns Delta.
template <int D, int NF, typename Sum>
SM_DEV float dq_prologue(const AttnArgs& a, const HeadView<__bf16, D>& hv, int q, int col0, bool writer, Sum rowsum,
                         bf16x8 (&qf)[NF], bf16x8 (&df)[NF]) {
  constexpr int CS = D / NF;
  const bool qok = q < a.L;
  // this lane's first 8 columns of row q in qkv's q, dO, O and qc
  const __bf16* qr = hv.q + (int64_t)q * hv.ldq + col0;
  const __bf16* dor = (const __bf16*)a.dout + hv.orow + (int64_t)q * hv.C + col0;
  const __bf16* orw = (const __bf16*)a.o + hv.orow + (int64_t)q * hv.C + col0;
  __bf16* qcr = a.qc + hv.orow + (int64_t)q * hv.C + col0;
  float dpart = 0.f;
#pragma unroll
  for (int s = 0; s < NF; ++s) {
    if (qok) {
      qf[s] = *(const bf16x8*)(qr + CS * s);
      df[s] = *(const bf16x8*)(dor + CS * s);
      const bf16x8 of = *(const bf16x8*)(orw + CS * s);
#pragma unroll
      for (int j = 0; j < 8; ++j) dpart = fmaf((float)df[s][j], (float)of[j], dpart);
    } else {
      for (int j = 0; j < 8; ++j) { qf[s][j] = (__bf16)0.f; df[s][j] = (__bf16)0.f; }
    }
  }
  const float dl = rowsum(dpart);
  if (qok && writer) a.delta[hv.lrow + q] = dl;
#pragma unroll
  for (int s = 0; s < NF; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[s][j] = (__bf16)((float)qf[s][j] * (a.scale * LOG2E));
    if (qok) *(bf16x8*)(qcr + CS * s) = qf[s];
  }
  return dl;
}

// Queries on lanes; K / V tiles staged with prefetch; dQ^T = K^T dS^T.
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_bwd_dq_bf16(AttnArgs a) {
  constexpr int KT = 64;
  constexpr int RB = 32 * D * 2;
  constexpr int QB = 32 * NW;   // queries per block
  __shared__ __attribute__((aligned(16))) char lk[KT * D * 2];
  __shared__ __attribute__((aligned(16))) char lv[KT * D * 2];
  const AttnTile tl((a.L + QB - 1) / QB, a.H);
  const int n = tl.n, hd = tl.hd;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, h = l >> 5;
  const HeadView<__bf16, D> hv(a, n, hd);
  const int q = tl.qb * QB + w * 32 + (l & 31);
  const bool qok = q < a.L;
  const bool wact = tl.qb * QB + w * 32 < a.L;   // else: only stages tiles (see the forward)
  const float lse2 = qok ? a.lse[hv.lrow + q] * LOG2E : 1e30f;

  bf16x8 qf[D / 16], df[D / 16];
  const float dl = dq_prologue(a, hv, q, 8 * h, h == 0, halves_sum, qf, df);
  TilePipe<D, 64 * NW, false> kv;
  kv.init(hv.k, hv.v, hv.ldq, a.L);
  int roff[D / 16], tlo[D / 32], thi[D / 32];
#pragma unroll
  for (int s = 0; s < D / 16; ++s) roff[s] = row_frag_off<D>(s);
#pragma unroll
  for (int t = 0; t < D / 32; ++t) tr_frag_off<D>(t, tlo[t], thi[t]);
  f32x16 dq[D / 32] = {};
  const float ks = DROP ? attn_drop_scale(a.drop_p) : 1.f;
  const uint32_t dlb = drop_hash_in(a, n, hd, q, h);   // this lane's query, this half's key group
  const uint32_t dthr = attn_thr(a.drop_p);

  kv.prime();
  ragged_tiles<KT>(a.L, [&](int k0, auto rag) {   // one key tile
    constexpr bool RAGGED = decltype(rag)::value;
    kv.enter(k0, lk, lv);
    if (!wact) return;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (RAGGED && u == 1 && k0 + 32 >= a.L) continue;   // no key below L in this half
      f32x16 sacc, dpacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = -lse2; dpacc[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < D / 16; ++s) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_b128(lk, roff[s] + u * RB), qf[s], sacc, 0, 0, 0);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_b128(lv, roff[s] + u * RB), df[s], dpacc, 0, 0, 0);
      }
      if constexpr (RAGGED) {   // keys past L: P = exp2(-huge) = 0 (last tile only)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + 32 * u + acc_row(r, h) >= a.L) sacc[r] = NEG_BIG;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint32_t hv4 = 0;
        if (DROP) hv4 = keep_bytes(keep_flags(mix24(dlb + drop_groups((k0 >> 2) + 8 * u + 2 * g)), dthr));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j;
          const float p = __builtin_amdgcn_exp2f(sacc[r]);
          const float dp = dpacc[r];
          if (DROP) dpacc[r] = p * fmaf(keep_sel(dp, hv4, j), ks, -dl);
          else dpacc[r] = p * (dp - dl);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 sf = acc_to_frag(dpacc, s);
#pragma unroll
        for (int t = 0; t < D / 32; ++t) {
          const int ob = u * RB + s * (RB / 2);
          dq[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_tr(lk, tlo[t] + ob, thi[t] + ob), sf, dq[t], 0, 0, 0);
        }
      }
    }
  });
  store_acc32(hv.out(a, q, hv.ldq), dq, a.scale, qok, h);
}

// =============================================================== bf16 backward on 16x16x32
// The same two kernels (dK/dV with keys on lanes, dQ with queries on lanes) on
// v_mfma_f32_16x16x32_bf16 instead of 32x32x16: equal MFMA cycles per FLOP, equal LDS
// bytes and registers per wave, but the chip holds a higher clock on this shape
// (MI355X_MICROARCH.md 'DVFS give-back' item 7: 1.12-1.15x the FLOP/s of the 32x32x16
// loop on random data), and each product is a quarter of the size, so the softmax / dS
// VALU of one 16x16 score block can start while the others are still in the matrix core.
//
// Fragment maps (lane l, c = l & 15, g = l >> 4): A[row c][k = 8g + j], B[k = 8g + j][col c],
// D[row 4g + i][col c].  A wave owns 32 keys (dK/dV) or 32 queries (dQ) as two 16-column
// groups.  A 16x16 accumulator feeds the next product as its B operand over its ROW index,
// two blocks per 32-deep k-step: element j < 4 is row 4g + j of the first block, j >= 4 row
// 4g + j - 4 of the second (16 rows further); the A operand of that product reads the same
// k order with two ds_read_b64_tr_b16 (rows 4g.. and 16 + 4g..).
template <int D>
SM_DEV int tr16_off(int dt) {    // transposed A fragment (first block): rows 4g + (c>>2), cols 16 dt + 4 (c&3)
  const int l = threadIdx.x & 63, c = l & 15;
  return tile_off<D, true>(4 * (l >> 4) + (c >> 2), 16 * dt + 4 * (c & 3));
}
SM_DEV f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
SM_DEV bf16x8 pack_frag16(const f32x4& lo, const f32x4& hi) {
  return __builtin_bit_cast(bf16x8, make_uint4(pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]),
                                               pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3])));
}

// dK, dV: keys on lanes (key = kbase + 16 kg + c), Q / dO tiles of 64 rows in LDS, per
// 32-row half u: S, dP for the 2 x 2 (query group, key group) blocks, then P / dS packed
// as B fragments per key group and dV^T / dK^T += dO^T P, Qc^T dS over 16-wide d tiles.
// Row constants, dropout (quad byte transpose: the four keys of a hash are the four lanes
// of a DPP quad) and the pipelined order are the 32x32x16 kernel's.
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_bwd_dkdv16_bf16(AttnArgs a) {
  constexpr int QT = 64;
  constexpr int RB = 16 * D * 2;   // bytes of 16 tile rows
  constexpr int KB = 32 * NW;      // keys per block
  constexpr int KS = D / 32, DT = D / 16;
  __shared__ __attribute__((aligned(16))) char lq[QT * D * 2];
  __shared__ __attribute__((aligned(16))) char ldo[QT * D * 2];
  __shared__ __attribute__((aligned(16))) float llse[QT];
  __shared__ __attribute__((aligned(16))) float ldel[QT];
  const AttnTile tl((a.L + KB - 1) / KB, a.H);
  const int n = tl.n, hd = tl.hd;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const HeadView<__bf16, D> hv(a, n, hd);
  const int kbase = tl.qb * KB + w * 32;
  const bool wact = kbase < a.L;

  bf16x8 kf[2][KS], vf[2][KS];
#pragma unroll
  for (int kg = 0; kg < 2; ++kg) {
    const int key = kbase + 16 * kg + c;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (key < a.L) {
        kf[kg][ks] = *(const bf16x8*)(hv.k + (int64_t)key * hv.ldq + 32 * ks + 8 * g);
        vf[kg][ks] = *(const bf16x8*)(hv.v + (int64_t)key * hv.ldq + 32 * ks + 8 * g);
      } else {
        for (int j = 0; j < 8; ++j) { kf[kg][ks][j] = (__bf16)0.f; vf[kg][ks][j] = (__bf16)0.f; }
      }
    }
  }
  int roff[KS], toff[DT];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) roff[ks] = row_frag_off<D, 16>(ks);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) toff[dt] = tr16_off<D>(dt);

  f32x4 dk[2][DT] = {}, dv[2][DT] = {};
  const int kq = l & 3;
  const float ksc = DROP ? attn_drop_scale(a.drop_p) : 1.f;
  const float lkeep = dkdv_lkeep<DROP>(ksc), dkeep = dkdv_dkeep<DROP>(ksc);
  const uint32_t dthr = attn_thr(a.drop_p), sel1 = quad_sel1(kq), sel2 = quad_sel2(kq);
  // hash input of row q0 + 32u + 16qg + 4g + kq, key group (kbase + 16kg + c) >> 2 (+ 4 kg, scalar)
  const uint32_t dlb = drop_hash_in(a, n, hd, 4 * g + kq, (kbase + c) >> 2);

  auto sdp = [&](int u, f32x4 (&sa)[2][2], f32x4 (&da)[2][2]) {
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      const float4 a4 = *(const float4*)&llse[32 * u + 16 * qg + 4 * g];   // -LSE2 of rows 4g + i
      float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!DROP) b4 = *(const float4*)&ldel[32 * u + 16 * qg + 4 * g];     // -Delta
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        sa[qg][kg][0] = a4.x; sa[qg][kg][1] = a4.y; sa[qg][kg][2] = a4.z; sa[qg][kg][3] = a4.w;
        da[qg][kg][0] = b4.x; da[qg][kg][1] = b4.y; da[qg][kg][2] = b4.z; da[qg][kg][3] = b4.w;
      }
    }
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 aq = lds_b128(lq, roff[ks] + (2 * u + qg) * RB);
        const bf16x8 ad = lds_b128(ldo, roff[ks] + (2 * u + qg) * RB);
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
          sa[qg][kg] = mfma16(aq, kf[kg][ks], sa[qg][kg]);
          da[qg][kg] = mfma16(ad, vf[kg][ks], da[qg][kg]);
        }
      }
  };
  auto softmax = [&](int q0, int u, const f32x4 (&sa)[2][2], const f32x4 (&da)[2][2], bf16x8 (&pf)[2],
                     bf16x8 (&sf)[2]) {
    f32x4 pv[2][2], dsv[2][2];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      float del4[4] = {0.f, 0.f, 0.f, 0.f};
      if (DROP) {
        const float4 b4 = *(const float4*)&ldel[32 * u + 16 * qg + 4 * g];
        del4[0] = b4.x; del4[1] = b4.y; del4[2] = b4.z; del4[3] = b4.w;
      }
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        uint32_t kb4 = 0;
        if (DROP) kb4 = dkdv_keep4(dlb + drop_rows(q0 + 32 * u + 16 * qg) + drop_groups(4 * kg), sel1, sel2, dthr);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = __builtin_amdgcn_exp2f(sa[qg][kg][i]);
          if (DROP) {
            const float pk = keep_sel(p, kb4, i);
            pv[qg][kg][i] = pk;
            dsv[qg][kg][i] = fmaf(pk, da[qg][kg][i], -(p * del4[i]));
          } else {
            pv[qg][kg][i] = p;
            dsv[qg][kg][i] = p * da[qg][kg][i];
          }
        }
      }
    }
#pragma unroll
    for (int kg = 0; kg < 2; ++kg) {
      pf[kg] = pack_frag16(pv[0][kg], pv[1][kg]);
      sf[kg] = pack_frag16(dsv[0][kg], dsv[1][kg]);
    }
  };
  auto dvdk = [&](int u, const bf16x8 (&pf)[2], const bf16x8 (&sf)[2]) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const int o = toff[dt] + 2 * u * RB;
      const bf16x8 ado = lds_tr(ldo, o, o + RB);
      const bf16x8 aq = lds_tr(lq, o, o + RB);
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        dv[kg][dt] = mfma16(ado, pf[kg], dv[kg][dt]);
        dk[kg][dt] = mfma16(aq, sf[kg], dk[kg][dt]);
      }
    }
  };

  QdoPipe<D, 64 * NW, true> pipe;
  pipe.init(a.qc + hv.orow, (const __bf16*)a.dout + hv.orow, hv.C, a.L);
  pipe.prime(a.lse + hv.lrow, a.delta + hv.lrow);
  for (int q0 = 0; q0 < a.L; q0 += QT) {
    pipe.enter(q0, lq, ldo, llse, ldel, lkeep, dkeep);
    if (!wact) continue;
    f32x4 s0[2][2], p0[2][2], s1[2][2], p1[2][2];
    bf16x8 pf0[2], sf0[2], pf1[2], sf1[2];
    sdp(0, s0, p0);
    sdp(1, s1, p1);
    softmax(q0, 0, s0, p0, pf0, sf0);
    dvdk(0, pf0, sf0);
    softmax(q0, 1, s1, p1, pf1, sf1);
    dvdk(1, pf1, sf1);
  }
#pragma unroll
  for (int kg = 0; kg < 2; ++kg) {
    const int key = kbase + 16 * kg + c;
    if (key >= a.L) continue;
    __bf16* out = hv.out(a, key, hv.ldq) + 4 * g;
    store_acc16(out + hv.C, dk[kg], LN2);
    store_acc16(out + 2 * hv.C, dv[kg], 1.f);
  }
}

// dQ: queries on lanes (q = qbase + 16 qg + c), K / V tiles of 64 keys in LDS; per 32-key
// half s the 2 x 2 (key group, query group) blocks of S^T, dP^T, then dS^T packed per
// query group and dQ^T += K^T dS^T over 16-wide d tiles.  The prologue (dq_prologue; the
// row's four d groups live in lanes c, c + 16, c + 32, c + 48) is the 32x32x16 kernel's.
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, 8 / NW) void attn_bwd_dq16_bf16(AttnArgs a) {
  constexpr int KT = 64;
  constexpr int RB = 16 * D * 2;
  constexpr int QB = 32 * NW;
  constexpr int KS = D / 32, DT = D / 16;
  __shared__ __attribute__((aligned(16))) char lk[KT * D * 2];
  __shared__ __attribute__((aligned(16))) char lv[KT * D * 2];
  const AttnTile tl((a.L + QB - 1) / QB, a.H);
  const int n = tl.n, hd = tl.hd;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, g = l >> 4;
  const HeadView<__bf16, D> hv(a, n, hd);
  const int qbase = tl.qb * QB + w * 32;
  const bool wact = qbase < a.L;

  bf16x8 qf[2][KS], df[2][KS];
  float lse2[2], dl[2];
  uint32_t dlb[2];   // hash input of this lane's row, key group (k0 + 32 s + 16 kk + 4 g) >> 2 minus its scalar part
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int q = qbase + 16 * qg + c;
    lse2[qg] = q < a.L ? a.lse[hv.lrow + q] * LOG2E : 1e30f;
    dl[qg] = dq_prologue(a, hv, q, 8 * g, g == 0, quarters_sum, qf[qg], df[qg]);
  }
  TilePipe<D, 64 * NW, true> kv;
  kv.init(hv.k, hv.v, hv.ldq, a.L);
  int roff[KS], toff[DT];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) roff[ks] = row_frag_off<D, 16>(ks);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) toff[dt] = tr16_off<D>(dt);
  f32x4 dq[2][DT] = {};
  const float ksc = DROP ? attn_drop_scale(a.drop_p) : 1.f;
  const uint32_t dthr = attn_thr(a.drop_p);
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) dlb[qg] = drop_hash_in(a, n, hd, qbase + 16 * qg + c, g);

  kv.prime();
  ragged_tiles<KT>(a.L, [&](int k0, auto rag) {   // one key tile
    constexpr bool RAGGED = decltype(rag)::value;
    kv.enter(k0, lk, lv);
    if (!wact) return;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (RAGGED && s == 1 && k0 + 32 >= a.L) continue;   // no key below L in this half
      f32x4 sacc[2][2], dpacc[2][2];   // [key group kk][query group]
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg)
#pragma unroll
          for (int i = 0; i < 4; ++i) { sacc[kk][qg][i] = -lse2[qg]; dpacc[kk][qg][i] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const bf16x8 ak = lds_b128(lk, roff[ks] + (2 * s + kk) * RB);
          const bf16x8 av = lds_b128(lv, roff[ks] + (2 * s + kk) * RB);
#pragma unroll
          for (int qg = 0; qg < 2; ++qg) {
            sacc[kk][qg] = mfma16(ak, qf[qg][ks], sacc[kk][qg]);
            dpacc[kk][qg] = mfma16(av, df[qg][ks], dpacc[kk][qg]);
          }
        }
      if constexpr (RAGGED) {   // keys past L: P = exp2(-huge) = 0 (last tile only)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int qg = 0; qg < 2; ++qg)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (k0 + 32 * s + 16 * kk + 4 * g + i >= a.L) sacc[kk][qg][i] = NEG_BIG;
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
          uint32_t hv4 = 0;
          if (DROP) hv4 = keep_bytes(keep_flags(mix24(dlb[qg] + drop_groups((k0 >> 2) + 8 * s + 4 * kk)), dthr));
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float p = __builtin_amdgcn_exp2f(sacc[kk][qg][i]);
            const float dp = dpacc[kk][qg][i];
            if (DROP) dpacc[kk][qg][i] = p * fmaf(keep_sel(dp, hv4, i), ksc, -dl[qg]);
            else dpacc[kk][qg][i] = p * (dp - dl[qg]);
          }
        }
      bf16x8 sf[2];
#pragma unroll
      for (int qg = 0; qg < 2; ++qg) sf[qg] = pack_frag16(dpacc[0][qg], dpacc[1][qg]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const int o = toff[dt] + 2 * s * RB;
        const bf16x8 ak = lds_tr(lk, o, o + RB);
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) dq[qg][dt] = mfma16(ak, sf[qg], dq[qg][dt]);
      }
    }
  });
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int q = qbase + 16 * qg + c;
    if (q < a.L) store_acc16(hv.out(a, q, hv.ldq) + 4 * g, dq[qg], a.scale);
  }
}

// =============================================================== f32 kernels
// rows r0 .. r0 + ROWS - 1 of two [L][ld] operands (zeros past L) into LDS, by the block's 128 threads
template <int ROWS, int D>
SM_DEV void stage2_f32(float (&la)[ROWS][D], const float* a, int64_t lda, float (&lb)[ROWS][D], const float* b,
                       int64_t ldb, int r0, int L) {
  for (int i = threadIdx.x; i < ROWS * D; i += 128) {
    const int r = i / D, d = i % D, row = r0 + r;
    la[r][d] = row < L ? a[(int64_t)row * lda + d] : 0.f;
    lb[r][d] = row < L ? b[(int64_t)row * ldb + d] : 0.f;
  }
}

template <int D>
__global__ __launch_bounds__(128) void attn_fwd_f32(AttnArgs a) {
  constexpr int KT = 32;
  __shared__ float lk[KT][D], lv[KT][D];
  const int n = blockIdx.z, hd = blockIdx.y;
  const HeadView<float, D> hv(a, n, hd);
  const int q = blockIdx.x * 128 + threadIdx.x;
  const bool qok = q < a.L;
  float qv[D], o[D];
  for (int d = 0; d < D; ++d) { qv[d] = qok ? hv.q[(int64_t)q * hv.ldq + d] : 0.f; o[d] = 0.f; }
  float m = NEG_BIG, lsum = 0.f;
  for (int k0 = 0; k0 < a.L; k0 += KT) {
    __syncthreads();
    stage2_f32(lk, hv.k, hv.ldq, lv, hv.v, hv.ldq, k0, a.L);
    __syncthreads();
    for (int r = 0; r < KT && k0 + r < a.L; ++r) {
      float s = 0.f;
      for (int d = 0; d < D; ++d) s += qv[d] * lk[r][d];
      s *= a.scale;
      const float mn = fmaxf(m, s);
      const float al = __expf(m - mn);
      float p = __expf(s - mn);
      lsum = lsum * al + p;
      if (a.drop_p > 0.f) p *= drop_keep_scale(a, n, hd, q, k0 + r);
      for (int d = 0; d < D; ++d) o[d] = o[d] * al + p * lv[r][d];
      m = mn;
    }
  }
  if (qok) {
    float* ob = hv.out(a, q, hv.C);
    for (int d = 0; d < D; ++d) ob[d] = o[d] / lsum;
    a.lse[hv.lrow + q] = m + logf(lsum);
  }
}

template <int D>
__global__ __launch_bounds__(128) void attn_bwd_dq_f32(AttnArgs a) {
  constexpr int KT = 32;
  __shared__ float lk[KT][D], lv[KT][D];
  const int n = blockIdx.z, hd = blockIdx.y;
  const HeadView<float, D> hv(a, n, hd);
  const float* dob = (const float*)a.dout + hv.orow;
  const int q = blockIdx.x * 128 + threadIdx.x;
  const bool qok = q < a.L;
  float qv[D], dov[D], dq[D];
  for (int d = 0; d < D; ++d) {
    qv[d] = qok ? hv.q[(int64_t)q * hv.ldq + d] : 0.f;
    dov[d] = qok ? dob[(int64_t)q * hv.C + d] : 0.f;
    dq[d] = 0.f;
  }
  const float lse = qok ? a.lse[hv.lrow + q] : 0.f;
  const float dl = qok ? a.delta[hv.lrow + q] : 0.f;
  for (int k0 = 0; k0 < a.L; k0 += KT) {
    __syncthreads();
    stage2_f32(lk, hv.k, hv.ldq, lv, hv.v, hv.ldq, k0, a.L);
    __syncthreads();
    for (int r = 0; r < KT && k0 + r < a.L; ++r) {
      float s = 0.f, dp = 0.f;
      for (int d = 0; d < D; ++d) { s += qv[d] * lk[r][d]; dp += dov[d] * lv[r][d]; }
      const float p = __expf(s * a.scale - lse);
      if (a.drop_p > 0.f) dp *= drop_keep_scale(a, n, hd, q, k0 + r);
      const float ds = p * (dp - dl);
      for (int d = 0; d < D; ++d) dq[d] += ds * lk[r][d];
    }
  }
  if (qok) {
    float* out = hv.out(a, q, hv.ldq);
    for (int d = 0; d < D; ++d) out[d] = dq[d] * a.scale;
  }
}

template <int D>
__global__ __launch_bounds__(128) void attn_bwd_dkdv_f32(AttnArgs a) {
  constexpr int QT = 32;
  __shared__ float lq[QT][D], ldo[QT][D], llse[QT], ldel[QT];
  const int n = blockIdx.z, hd = blockIdx.y;
  const HeadView<float, D> hv(a, n, hd);
  const int key = blockIdx.x * 128 + threadIdx.x;
  const bool kok = key < a.L;
  float kv[D], vv[D], dk[D], dv[D];
  for (int d = 0; d < D; ++d) {
    kv[d] = kok ? hv.k[(int64_t)key * hv.ldq + d] : 0.f;
    vv[d] = kok ? hv.v[(int64_t)key * hv.ldq + d] : 0.f;
    dk[d] = 0.f; dv[d] = 0.f;
  }
  for (int q0 = 0; q0 < a.L; q0 += QT) {
    __syncthreads();
    stage2_f32(lq, hv.q, hv.ldq, ldo, (const float*)a.dout + hv.orow, hv.C, q0, a.L);
    if (threadIdx.x < QT) {
      const int qq = q0 + threadIdx.x;
      llse[threadIdx.x] = qq < a.L ? a.lse[hv.lrow + qq] : 0.f;
      ldel[threadIdx.x] = qq < a.L ? a.delta[hv.lrow + qq] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < QT && q0 + r < a.L; ++r) {
      float s = 0.f, dp = 0.f;
      for (int d = 0; d < D; ++d) { s += lq[r][d] * kv[d]; dp += ldo[r][d] * vv[d]; }
      const float p = __expf(s * a.scale - llse[r]);
      float pd = p;
      if (a.drop_p > 0.f) {
        const float ks = drop_keep_scale(a, n, hd, q0 + r, key);
        pd = p * ks;
        dp *= ks;
      }
      const float ds = p * (dp - ldel[r]);
      for (int d = 0; d < D; ++d) { dv[d] += pd * ldo[r][d]; dk[d] += ds * lq[r][d]; }
    }
  }
  if (kok) {
    float* out = hv.out(a, key, hv.ldq);
    for (int d = 0; d < D; ++d) { out[hv.C + d] = dk[d] * a.scale; out[2 * hv.C + d] = dv[d]; }
  }
}

// =============================================================== host side
// MFMA shape of the bf16 backward per head dim (sm_attn_tuning: 32 = v_mfma_f32_32x32x16_bf16,
// 16 = v_mfma_f32_16x16x32_bf16); key 0: D = 64 (decoder), key 1: D = 32 (encoder).
int g_attn_bwd_shape[2] = {16, 32};   // measured: profiles/r06cd_attn_bwd16_variants.txt

// workspace of sm_attn_bwd: Delta [N][H][L] fp32, then (bf16) bf16(Q scale log2 e) [N][L][H][D]
int64_t attn_delta_bytes(int N, int L, int H) { return ((int64_t)N * H * L * 4 + 255) / 256 * 256; }

// Validates one call of sm_attn_fwd (delta_ws = nullptr) / sm_attn_bwd and fills its AttnArgs
// (out, o, dout stay the caller's).  Returns 0: launch; 1: nothing to do (success); -2: refused.
int attn_args(AttnArgs& a, int N, int L, int H, int D, const void* qkv, const float* lse, float* delta_ws, float scale,
              float drop_p, uint64_t seed) {
  if (N <= 0 || L <= 0) return 1;
  if (D != 32 && D != 64) return -2;
  if (((uintptr_t)delta_ws) & 255) return -2;
  a = AttnArgs{};
  a.qkv = qkv; a.lse = (float*)lse; a.N = N; a.L = L; a.H = H; a.scale = scale; a.drop_p = drop_p; a.seed = seed;
  if (delta_ws) {
    a.delta = delta_ws;
    a.qc = (__bf16*)((char*)delta_ws + attn_delta_bytes(N, L, H));
  }
  return 0;
}

// Every kernel takes 128 queries (or keys) of one (sample, head) per block: the bf16 kernels on
// a 1-D grid (XCD-remapped, AttnTile), the f32 kernels on (block, head, sample).
template <typename K>
void attn_launch(K kernel, int dtype, const AttnArgs& a, hipStream_t st) {
  const unsigned nb = (unsigned)((a.L + 127) / 128);
  if (dtype == SM_BF16) hipLaunchKernelGGL(kernel, dim3(nb * (unsigned)(a.H * a.N)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(kernel, dim3(nb, a.H, a.N), dim3(128), 0, st, a);
}

// run-time (D, drop) -> template arguments: f(integral_constant<int, D>, bool_constant<DROP>)
template <typename F>
void attn_dispatch(int D, bool drop, F&& f) {
  using D32 = std::integral_constant<int, 32>;
  using D64 = std::integral_constant<int, 64>;
  if (D == 32) { if (drop) f(D32{}, std::true_type{}); else f(D32{}, std::false_type{}); }
  else { if (drop) f(D64{}, std::true_type{}); else f(D64{}, std::false_type{}); }
}

}  // namespace

extern "C" int sm_attn_fwd(int dtype, int N, int L, int H, int D, const void* qkv, void* out,
                           float* lse, float scale, float drop_p, uint64_t seed, hipStream_t st) {
  AttnArgs a;
  if (const int rc = attn_args(a, N, L, H, D, qkv, lse, nullptr, scale, drop_p, seed)) return rc < 0 ? rc : 0;
  a.out = out;
  attn_dispatch(D, drop_p > 0.f, [&](auto d, auto drop) {
    constexpr int HD = decltype(d)::value;
    constexpr bool DROP = decltype(drop)::value;
    if (dtype == SM_BF16) attn_launch(attn_fwd_bf16<HD, DROP>, dtype, a, st);
    else attn_launch(attn_fwd_f32<HD>, dtype, a, st);
  });
  SM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t sm_attn_bwd_workspace_bytes(int dtype, int N, int L, int H, int D) {
  if (N <= 0 || L <= 0) return 0;
  return attn_delta_bytes(N, L, H) + (dtype == SM_BF16 ? (int64_t)N * L * H * D * 2 : 0);
}

extern "C" int sm_attn_bwd(int dtype, int N, int L, int H, int D, const void* qkv, const void* o,
                           const void* dout, const float* lse, float* delta_ws, void* dqkv,
                           float scale, float drop_p, uint64_t seed, hipStream_t st) {
  AttnArgs a;
  if (const int rc = attn_args(a, N, L, H, D, qkv, lse, delta_ws, scale, drop_p, seed)) return rc < 0 ? rc : 0;
  a.o = o; a.dout = dout; a.out = dqkv;
  attn_dispatch(D, drop_p > 0.f, [&](auto d, auto drop) {
    constexpr int HD = decltype(d)::value;
    constexpr bool DROP = decltype(drop)::value;
    if (dtype == SM_BF16) {
      // dQ first: it forms Delta = rowsum(dO*O) in its prologue and writes bf16(Q scale log2 e)
      // for the dK/dV kernel.  (8-wave blocks and a static s_setprio for one wave of each SIMD
      // pair measured 1-10 % slower, profiles/r04c_attn_bwd_variants.txt.)
      if (g_attn_bwd_shape[HD == 64 ? 0 : 1] == 16) {
        attn_launch(attn_bwd_dq16_bf16<HD, DROP>, dtype, a, st);
        attn_launch(attn_bwd_dkdv16_bf16<HD, DROP>, dtype, a, st);
      } else {
        attn_launch(attn_bwd_dq_bf16<HD, DROP>, dtype, a, st);
        attn_launch(attn_bwd_dkdv_bf16<HD, DROP>, dtype, a, st);
      }
    } else {
      hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)(((int64_t)N * L + 3) / 4)), dim3(256), 0, st, a, D);
      attn_launch(attn_bwd_dkdv_f32<HD>, dtype, a, st);
      attn_launch(attn_bwd_dq_f32<HD>, dtype, a, st);
    }
  });
  SM_CHECK_LAUNCH();
  return 0;
}

// A/B switch of the bf16 backward's MFMA shape (see sm_attn_bwd): key 0 = D 64, 1 = D 32;
// *prev <- current shape; set > 0 stores value (16 or 32), set < 0 restores the default.  Host-side only.
extern "C" int sm_attn_tuning(int key, int set, int value, int* prev) {
  if (key < 0 || key > 1) return -2;
  int& v = g_attn_bwd_shape[key];
  if (prev) *prev = v;
  if (set > 0) {
    if (value != 16 && value != 32) return -2;
    v = value;
  } else if (set < 0) {
    v = key == 0 ? 16 : 32;
  }
  return 0;
}

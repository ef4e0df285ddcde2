/* C ABI of libsslmae.so — the MI355X (gfx950) kernels of the video-MAE
 * pretraining step of lzc452/SSL-VIT-VIDEO-ANALYTICS.
 *
 * The reference has no FFI: its path is the Python module API used by
 * src/train_ssl_mae.py:13-16 (tiny_vit_21m_variant, TinyVideoMAE, get_tube_mask,
 * patchify) on stock aten ops.  Each entry point below replaces one aten op (or
 * a fused group of them) on that path; the citation is the reference line whose
 * computation it performs.  The host mirror of the reference API
 * (ssl-vit-video-analytics_amd/ssl_mae_amd) binds these with ctypes.
 *
 * Conventions: raw device pointers, element counts, row strides in ELEMENTS,
 * dtype enum (0 = f32, 1 = bf16), the caller's hipStream_t; kernels never
 * allocate — scratch comes from the caller (`*_workspace_bytes`).  Every
 * function returns 0 on success, a hipError_t (>0) on launch failure, or a
 * negative code: -2 unsupported shape/alignment, -3 unsupported dtype combo,
 * -4 workspace too small.  No exceptions cross the ABI; no host syncs.
 */
#ifndef SM_API_H
#define SM_API_H
#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- GEMM: every nn.Linear / 1x1 Conv2d and their dX/dW products.
 * Replaces aten::addmm/mm of tiny_vit.py:79,81,93,94 (Mlp, Attention qkv/proj),
 * tiny_vit.py:43,49 (MBConv 1x1 convs), mae_vit_adapter.py:24,53 (enc_to_dec,
 * decoder_pred) and torch TransformerEncoderLayer in_proj/out_proj/linear1/2.
 * C = alpha*op(A)op(B) + bias (+ beta*R, R = C when null); epi bit0 = exact GELU
 * (aux <- pre-activation), bit1 = round the branch to bf16 before adding R (autocast).
 * Branch regularisers of the training step: elementwise dropout (drop_p, counter-hash
 * RNG keyed by seed and the element index, nn.Dropout semantics with the keep rate quantised
 * to 8 bits: dropped w.p. round(256 p)/256, kept values scaled by drop_scale(p) =
 * 256/(256 - round(256 p))) and DropPath (branch *= row_scale[row / rows_per_group]).
 * a_layout 0: A[M][K], 1: A[K][M];  b_layout 0: B[N][K], 1: B[K][N]. */
int64_t sm_gemm_workspace_bytes(int ab_dtype, int M, int N, int K);
int sm_gemm(int ab_dtype, int c_dtype, int a_layout, int b_layout, int M, int N, int K,
            const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
            const float* bias, float alpha, float beta, int epi, void* aux, const void* R,
            float drop_p, uint64_t seed, const float* row_scale, int64_t rows_per_group,
            void* workspace, int64_t ws_bytes, hipStream_t stream);
/* Form of the non-split bf16 GEMMs with a K-major A and a plain bf16 epilogue (every
 * forward / data-gradient Linear of the step): 1 = persistent blocks with each tile's
 * output stores drained under the next tile's K loop (default), 0 = one tile per block.
 * Outputs are bit-identical either way.  mode < 0 only queries.  Returns the previous mode.
 * (= sm_gemm_tuning key 0.) */
int sm_gemm_persistent(int mode);
/* GEMM dispatch tuning for A/B measurement scripts (never changed by the product path):
 * key 0 persistent form on/off,
 * 1 / 2 persistent form's minimum N / maximum K at K > 128, 3 tiles per persistent block
 * (-1 = per-K rule, 0 = fully persistent), 4 / 5 tiles per block at K <= 128 / above,
 * 6 minimum K per block for the v_mfma_f32_16x16x32_bf16 K loop of K-major-A tiles
 * (default 1 << 30 = off: measured neutral), 7 the 384 x 128 pipelined weight-gradient tile
 * (gemm_dw384) for outputs it divides (default 1 = on), 8 keep such outputs untransposed in
 * sm_linear_dw_bias (fused bias gradient; default 1).
 * *prev <- the current value; set > 0 stores value, set < 0 restores the default.
 * Returns 0, or -2 for an unknown key.  Host-side only (no launch). */
int sm_gemm_tuning(int key, int set, int value, int* prev);
/* Weight + bias gradient of y = x W^T + b (Linear / 1x1 conv backward, e.g.
 * tiny_vit.py:74-84 Mlp, mae_vit_adapter.py:40-48 decoder layers): dW[nout][nin]
 * (+)= dy^T x and db[nout] += sum_rows dy in one GEMM pass over dy (bf16 dy, x;
 * fp32 dW, db).  Replaces sm_gemm (dW) followed by sm_colsum (db). */
int64_t sm_linear_dw_bias_workspace_bytes(int rows, int nout, int nin);
int sm_linear_dw_bias(int rows, int nout, int nin, const void* dy, const void* x, float* dW, float* db,
                      int accumulate, void* ws, int64_t ws_bytes, hipStream_t stream);
/* The fc2 data gradient through dropout(GELU(pre)) with the fc2 weight gradient's operand
 * as a side output (Mlp tiny_vit.py:74-84, decoder FF mae_vit_adapter.py:40-48): dx = (dy w)
 * * keep * drop_scale(p) * GELU'(pre) and h = bf16(GELU(pre) * keep * drop_scale(p)) (= sm_gelu_fwd(pre))
 * from one epilogue.  dy [M][N], w [N][K], pre / dx / h [M][K] bf16; N, K % 8 == 0. */
int sm_linear_dx_gelu(int M, int N, int K, const void* dy, const void* w, const void* pre, void* dx, void* h,
                      float drop_p, uint64_t seed, hipStream_t stream);
/* fc2's weight gradient with the activation formed in the GEMM's operand loads:
 * dW[nout][nin] (+)= dy^T dropout(GELU(pre)), db += colsum(dy); pre = the fc1
 * pre-activation [rows][nin] bf16, (drop_p, seed) the fc1 output's dropout (the Mlp of
 * tiny_vit.py:74-84, the decoder feed-forward).  Bit-identical to sm_gelu_fwd followed by
 * sm_linear_dw_bias without the recompute pass; workspace as
 * sm_linear_dw_bias_workspace_bytes. */
int sm_linear_dw_bias_gelu(int rows, int nout, int nin, const void* dy, const void* pre, float drop_p,
                           uint64_t seed, float* dW, float* db, int accumulate, void* ws, int64_t ws_bytes,
                           hipStream_t stream);
/* y = x W^T (bf16, no bias) plus the train-mode BatchNorm statistics of y (Conv2d_BN,
 * tiny_vit.py:12-18, of the MBConv expand conv tiny_vit.py:43): the GEMM epilogue sums the
 * stored values per 64-row slab; fixed-order fp64 reduction, mean / rstd and the running
 * statistics update (`updates` times) as sm_bn_stats -- replaces sm_gemm + sm_bn_stats
 * (one read pass of y fewer).  x [M][K], w [N][K] bf16. */
int64_t sm_linear_bn_stats_workspace_bytes(int M, int N);
int sm_linear_bn_stats(int M, int N, int K, const void* x, const void* w, void* y, float* mean, float* rstd,
                       float* run_mean, float* run_var, int64_t* num_batches_tracked, float momentum, float eps,
                       int updates, void* ws, int64_t ws_bytes, hipStream_t stream);
/* The MBConv projection's forward over the SE output (tiny_vit.py:29-34, 53): y[rows][nout]
 * bf16 = h3 W^T, h3 = bf16(bf16(act(a2)) * gate[r / hw][c]) formed in the GEMM's operand
 * loads exactly as sm_se_fwd stores it (bit-identical to sm_se_fwd's y + sm_gemm), w
 * [nout][nin] bf16; hw % 128 == 0, nin % 64 == 0, nin <= 1536. */
int sm_linear_se(int rows, int nout, int nin, const void* a2, const void* w, const float* act_mean,
                 const float* act_rstd, const float* act_w, const float* act_b, int act_gelu, const float* gate,
                 int hw, void* y, hipStream_t stream);
/* The MBConv projection's weight gradient over the SE output (tiny_vit.py:29-34, 53,
 * replacing the Conv2d weight-gradient autograd node fed by SELayer.forward's product):
 * dW[nout][nin] (+)= dy^T h3, h3[r][c] = bf16(bf16(act(a2[r][c])) * gate[r / hw][c]),
 * act = BatchNorm(mean, rstd, w, b) + GELU (act_gelu) of the depthwise output a2
 * [rows][nin] bf16, gate [rows / hw][nin] fp32 (the SE sigmoid), dy [rows][nout] bf16,
 * fp32 dW.  h3 is formed in the GEMM's operand loads exactly as sm_se_scale stores it:
 * bit-identical to sm_se_scale + sm_gemm.  hw % 64 == 0. */
/* ---- the stem's BN2 folded into stage 0's first MBConv (tiny_vit.py:62-72 feeding :43;
 * replaces the aten batch_norm output the reference materialises between PatchEmbed and
 * stages[0][0]): y = x W^T with x = bf16(a sc + sh), sc = a_rstd a_w, sh = a_b - a_mean sc,
 * formed in the A-operand loads exactly as sm_bn_apply stores x (bit-identical to
 * sm_bn_apply + sm_gemm / sm_linear_bn_stats).  a [M][K] bf16, K % 8 == 0, K <= 256, w [N][K]
 * bf16, y [M][N] bf16.  _bn_stats: plus the output's train-mode BatchNorm statistics
 * (workspace sm_linear_bn_stats_workspace_bytes). */
int sm_linear_bnin(int M, int N, int K, const void* a, const float* a_mean, const float* a_rstd,
                   const float* a_w, const float* a_b, const void* w, void* y, hipStream_t stream);
int sm_linear_bnin_bn_stats(int M, int N, int K, const void* a, const float* a_mean, const float* a_rstd,
                            const float* a_w, const float* a_b, const void* w, void* y, float* mean,
                            float* rstd, float* run_mean, float* run_var, int64_t* num_batches_tracked,
                            float momentum, float eps, int updates, void* ws, int64_t ws_bytes,
                            hipStream_t stream);
/* sm_bn_apply whose residual R is stored before its own BatchNorm (r_*): R's value is the
 * BN output bf16(R r_sc + r_sh) exactly as sm_bn_apply stores it (the MBConv residual of
 * stages[0][0] over the stem's BN2, tiny_vit.py:54-56). */
int sm_bn_apply_res_bn(int x_dtype, int y_dtype, int64_t M, int C, const void* x, const float* mean,
                       const float* rstd, const float* w, const float* b, void* y, int gelu, const void* R,
                       const float* r_mean, const float* r_rstd, const float* r_w, const float* r_b,
                       const float* row_scale, int64_t rows_per_group, hipStream_t st);
/* sm_linear_dw_se with gate == NULL: the B operand is the BatchNorm output act(a2) (act_gelu
 * 0: x = bf16(a2 sc + sh)); rows need not be a multiple of hw. */
int64_t sm_linear_dw_se_workspace_bytes(int rows, int nout, int nin);
int sm_linear_dw_se(int rows, int nout, int nin, const void* dy, const void* a2, const float* act_mean,
                    const float* act_rstd, const float* act_w, const float* act_b, int act_gelu, const float* gate,
                    int hw, float* dW, int accumulate, void* ws, int64_t ws_bytes, hipStream_t stream);
/* Data gradient over an A operand made of two buffers: dx[M][N] = [a1 | a2] w (+ bias[n])
 * (+ residual[M][N]); a1 [M][K1] (row stride lda1), a2 [M][K2] (row stride lda2), w [K1 + K2][N],
 * dx / residual [M][N], all bf16; bias fp32, nullable like residual.  Bit-identical to the plain
 * data gradient of a materialised concatenation.  K1 % 64 == 0, K2 % 8 == 0, N % 8 == 0
 * (else -2). */
int sm_linear_dx2(int M, int N, int K1, int K2, const void* a1, int64_t lda1, const void* a2, int64_t lda2,
                  const void* w, const float* bias, const void* residual, void* dx, hipStream_t stream);
/* BN0's backward dx map folded into the MBConv expand conv's gradient GEMMs (tiny_vit.py:43-48).
 * With a1 = x W^T, xhat = (a1 - mean) rstd, dz and coef = (k0, k1) [2][mid] from
 * sm_dwconv_bn_bwd_dz:  da1 = omega dz - delta a1 + c  per channel, omega = bn_w rstd,
 * delta = omega rstd k1, c = omega (rstd k1 mean - k0).  Then
 *   dX  = dz W' - x T + r0,  W' = diag(omega) W, T = W^T diag(delta) W, r0 = c^T W
 *   dW += diag(omega) P - diag(delta) (W G) + c s^T,  P = dz^T x, G = x^T x, s = column sums of x.
 * _prep: w [mid][Cin] bf16 -> wst [mid + Cin][Cin] bf16 = [W'; -T] (T summed in fp32), r0 [Cin],
 * vec [3][mid] = omega, delta, c.  _dw: P [mid][Cin], G [Cin][Cin], s [Cin] fp32 over the M rows,
 * combined in fp64 into dW [mid][Cin] (+=).  x_mean .. x_b (all or none): the block input is
 * x = BN(xs) of a stored xs (no GELU); the data-gradient GEMM, G and s then read xs (P the
 * BatchNorm output) and the affine goes into -T, r0 and the combination.
 * mid <= 2048, Cin <= 1024. */
int sm_mbconv_fold_prep(int mid, int Cin, const float* coef, const float* bn_mean, const float* bn_rstd,
                        const float* bn_w, const void* w, const float* x_mean, const float* x_rstd,
                        const float* x_w, const float* x_b, void* wst, float* r0, float* vec, hipStream_t st);
int sm_mbconv_fold_dw(int mid, int Cin, int64_t M, const float* vec, const void* w, const float* P, const float* G,
                      const float* s, const float* x_mean, const float* x_rstd, const float* x_w, const float* x_b,
                      float* dW, hipStream_t st);

/* ---- fused attention (tiny_vit.py:103 F.scaled_dot_product_attention;
 * torch MultiheadAttention core of the decoder, mae_vit_adapter.py:40-48).
 * qkv packed [N][L][3][H][D] bf16|f32, out O [N][L][H][D], lse [N][H][L].  D = 32 or 64
 * (else -2).  drop_p > 0: dropout on the attention probabilities, mask a pure function of
 * (seed, n, head, query, key) with the keep rate quantised to 7 bits: dropped w.p.
 * round(128 p)/128, kept probabilities scaled by 128/(128 - round(128 p)); sm_attn_bwd
 * regenerates the same mask from the same (drop_p, seed). */
int sm_attn_fwd(int dtype, int N, int L, int H, int D, const void* qkv, void* out, float* lse,
                float scale, float drop_p, uint64_t seed, hipStream_t st);
/* delta_ws: workspace of sm_attn_bwd_workspace_bytes (256-B aligned): rowsum(dO * O)
 * [N][H][L] fp32, then for bf16 the dQ kernel's bf16(Q * scale * log2 e) [N][L][H][D], the
 * operand the dK/dV kernel's scores are formed from (the forward's and dQ's S exactly). */
int64_t sm_attn_bwd_workspace_bytes(int dtype, int N, int L, int H, int D);
int sm_attn_bwd(int dtype, int N, int L, int H, int D, const void* qkv, const void* o,
                const void* dout, const float* lse, float* delta_ws, void* dqkv,
                float scale, float drop_p, uint64_t seed, hipStream_t st);
/* MFMA shape of the bf16 attention backward (A/B and tests; the default is the measured best):
 * key 0 = head dim 64, key 1 = head dim 32; value 32 (v_mfma_f32_32x32x16_bf16) or 16
 * (v_mfma_f32_16x16x32_bf16).  *prev <- the current shape; set > 0 stores value, set < 0
 * restores the default.  Returns 0, or -2 for an unknown key / shape.  Host-side only. */
int sm_attn_tuning(int key, int set, int value, int* prev);

/* ---- LayerNorm (tiny_vit.py:112,115; decoder norm1/norm2; mae_vit_adapter.py:50) */
int sm_layernorm_fwd(int x_dtype, int y_dtype, int64_t M, int C, const void* x, const float* gamma,
                     const float* beta, void* y, float* mean, float* rstd, float eps, hipStream_t st);
int64_t sm_layernorm_bwd_workspace_bytes(int64_t M, int C);
int sm_layernorm_bwd(int x_dtype, int dy_dtype, int dx_dtype, int64_t M, int C, const void* dy,
                     const void* x, const float* mean, const float* rstd, const float* gamma,
                     void* dx, const void* dres, float* dgamma, float* dbeta, void* ws,
                     int64_t ws_bytes, hipStream_t st);
/* sm_layernorm_bwd plus the block branch's copy of dx (C = 192 or 384): dxb [M][C] bf16 =
 * bf16(bf16(dx) * row_scale[row / rows_per_group] * keep(row, col) / (1 - drop_p)) with
 * sm_dropout_bwd's mask (row_scale may be null, drop_p 0): the cast / dropout-backward
 * passes over dx that feed the branch's Linear backward (tiny_vit.py:126-128 DropPath,
 * mae_vit_adapter.py:40-48 dropout1) folded into the LayerNorm backward; bit-identical. */
int sm_layernorm_bwd_branch(int x_dtype, int dy_dtype, int dx_dtype, int64_t M, int C, const void* dy,
                            const void* x, const float* mean, const float* rstd, const float* gamma, void* dx,
                            const void* dres, float* dgamma, float* dbeta, void* dxb, float drop_p, uint64_t seed,
                            const float* row_scale, int64_t rows_per_group, void* ws, int64_t ws_bytes,
                            hipStream_t st);

/* ---- BatchNorm2d, train mode (tiny_vit.py:16 Conv2d_BN), channels-last [M][C] */
int64_t sm_bn_workspace_bytes(int64_t M, int C);
int sm_bn_stats(int x_dtype, int64_t M, int C, const void* x, float* mean, float* rstd,
                float* run_mean, float* run_var, int64_t* num_batches_tracked, float momentum, float eps,
                int updates, void* ws, int64_t ws_bytes, hipStream_t st);
/* eval mode (running statistics; tiny_vit.py:16 BatchNorm2d under model.eval(),
 * train_finetune.py:127-138 evaluate): mean = run_mean, rstd = 1/sqrt(run_var + eps),
 * the form every BN consumer takes.  sm_bn_stats / sm_bn_bwd process C > 1024
 * (stage-4 MBConv, 1536 channels) in column slices. */
int sm_bn_eval_params(const float* run_mean, const float* run_var, int C, float eps, float* mean, float* rstd,
                      hipStream_t st);
/* statistics from per-block partials [nrows][2][C] written by a fused producer */
int64_t sm_bn_partials_workspace_bytes(int C);
int sm_bn_stats_from_partials(const float* part, int64_t nrows, int C, int64_t M, float* mean, float* rstd,
                              float* run_mean, float* run_var, int64_t* num_batches_tracked, float momentum,
                              float eps, int updates, void* ws, int64_t ws_bytes, hipStream_t st);
/* y = R + row_scale[row/rows_per_group] * act(BN(x)) (R / row_scale nullable: MBConv
 * residual with DropPath, tiny_vit.py:53-56) */
int sm_bn_apply(int x_dtype, int y_dtype, int64_t M, int C, const void* x, const float* mean,
                const float* rstd, const float* w, const float* b, void* y, int gelu, const void* R,
                const float* row_scale, int64_t rows_per_group, hipStream_t st);
int sm_bn_bwd(int x_dtype, int g_dtype, int64_t M, int C, const void* dy, const void* x,
              const float* mean, const float* rstd, const float* w, const float* b, int gelu,
              const float* row_scale, int64_t rows_per_group, void* dx, float* dw, float* db, void* ws,
              int64_t ws_bytes, hipStream_t st);

/* ---- elementwise (GELU tiny_vit.py:44,47,68,80; residual adds; casts) */
int sm_gelu_bwd(int pre_dtype, int g_dtype, int64_t n, int ncols, const void* pre, const void* dy, void* dx,
                float drop_p, uint64_t seed, hipStream_t st);
int sm_add(int a_dtype, int o_dtype, int64_t n, const void* a, const void* b, void* o, hipStream_t st);
int sm_cast(int a_dtype, int o_dtype, int64_t n, const void* a, void* o, hipStream_t st);
int sm_fill(float* p, int64_t n, float v, hipStream_t st);
int sm_gelu_fwd(int dtype, int64_t n, int ncols, const void* x, void* y, float drop_p, uint64_t seed,
                hipStream_t st);
/* backward of the branch regularisers: dx = dy * dropout-mask * row_scale[row/rows_per_group]
 * (nn.Dropout of the decoder layers; timm DropPath of tiny_vit.py:52,114) */
int sm_dropout_bwd(int dtype, int64_t n, int ncols, const void* dy, void* dx, float drop_p, uint64_t seed,
                   const float* row_scale, int64_t rows_per_group, hipStream_t st);
/* sm_cast (fp32 -> bf16) and sm_dropout_bwd in one pass: dx_bf16 = bf16(bf16(dy) *
 * row_scale * keep * drop_scale(p)); the decoder block's fp32 residual-stream gradient entering
 * its bf16 branch (torch.autocast's cast + nn.Dropout backward, mae_vit_adapter.py:40-48). */
int sm_cast_dropout_bwd(int64_t n, int ncols, const float* dy, void* dx_bf16, float drop_p, uint64_t seed,
                        const float* row_scale, int64_t rows_per_group, hipStream_t st);
/* DropPath per-sample keep scales: out[i] = keep ? drop_scale(p) = 256/(256 - round(256 p)) : 0 */
int sm_droppath_scale(int n, float p, uint64_t seed, float* out, hipStream_t st);
/* column sums (Linear bias gradients): out[c] (+)= sum_m x[m][c] */
int64_t sm_colsum_workspace_bytes(int64_t M, int C);
int sm_colsum(int dtype, int64_t M, int C, const void* x, float* out, int accumulate, void* ws,
              int64_t ws_bytes, hipStream_t st);

/* ---- convolutions (PatchEmbed tiny_vit.py:62-72; depthwise 3x3 tiny_vit.py:46)
 * stem im2col folds the frame permute of mae_vit_adapter.py:84 into its loads. */
int sm_stem_im2col(int out_dtype, const float* clip, int B, int T, int H, int W, int64_t sB,
                   int64_t sC, int64_t sT, int64_t sH, int64_t sW, int stride, void* col, hipStream_t st);
int sm_im2col3(int dtype, const void* x, int F, int H, int W, int C, int stride, void* col, hipStream_t st);
int sm_col2im3(int dtype, const void* dcol, int F, int H, int W, int C, int stride, void* dx, hipStream_t st);
int sm_conv_wpack(int out_dtype, const float* src, void* dst, int Cout, int Cin, int Kpad, int order,
                  hipStream_t st);
int sm_conv_wunpack_add(const float* packed, float* grad, int Cout, int Cin, int Kpad, int order,
                        hipStream_t st);
/* Stem conv1 (tiny_vit.py:67: 3 -> 48, 3x3, stride 2, pad 1) straight from the fp32 clip
 * (strides as sm_stem_im2col) on the matrix cores, plus the train-mode BatchNorm statistics
 * of its bf16 output y [B*T*Ho*Wo][48] (tiny_vit.py:68, as sm_linear_bn_stats): replaces
 * sm_stem_im2col + sm_linear_bn_stats (y bit-identical), no [pixels][32] buffer.
 * wpack = sm_conv_wpack order 0 [48][32] bf16. */
int64_t sm_stem_conv1_workspace_bytes(void);
int sm_stem_conv1_bn_stats(const float* clip, int B, int T, int H, int W, int64_t sB, int64_t sC, int64_t sT,
                           int64_t sH, int64_t sW, const void* wpack, void* y, float* mean, float* rstd,
                           float* run_mean, float* run_var, int64_t* num_batches_tracked, float momentum, float eps,
                           int updates, void* ws, int64_t ws_bytes, hipStream_t st);
/* Stem conv2 over h1 = act(BN1(a1)) (tiny_vit.py:68-70: BN1 + GELU, 3x3 48 -> 96 stride 1
 * pad 1) plus the train-mode BatchNorm statistics of its bf16 output, one frame per
 * workgroup: BN1 + GELU applied once per element into an LDS ring of h1 rows, so h1 is
 * never written (y bit-identical to sm_bn_apply + sm_conv3x3_fwd).  a1 [F*H*W][48] bf16,
 * wpack = sm_conv_wpack order 1 [96][432] bf16, y [F*H*W][96] bf16, W <= 128; BN1 =
 * (mean, rstd, weight, bias), gelu = act is GELU.  Workspace sm_stem_conv2_workspace_bytes(F). */
int64_t sm_stem_conv2_workspace_bytes(int F);
int sm_stem_conv2_bn_stats(const void* a1, int F, int H, int W, const float* bn1_mean, const float* bn1_rstd,
                           const float* bn1_w, const float* bn1_b, int gelu, const void* wpack, void* y, float* mean,
                           float* rstd, float* run_mean, float* run_var, int64_t* num_batches_tracked, float momentum,
                           float eps, int updates, void* ws, int64_t ws_bytes, hipStream_t st);
/* Stem conv2 (tiny_vit.py:69, 3x3 / stride 1 / pad 1, bf16, channels-last) as GEMMs over
 * the implicit im2col matrix -- no [pixels][9C] buffer in HBM.  wpack = sm_conv_wpack
 * order 1 ([Cout][9*Cin]); wpack_t = order 2 ([Cin][9*Cout]); Cin, Cout % 8 == 0.
 * fwd: y = conv(x); dgrad: dx = conv^T(dy); wgrad: dw[Cout][9*Cin] (+)= fp32 weight
 * gradient (unpack with sm_conv_wunpack_add order 1). */
int sm_conv3x3_fwd(const void* x, const void* wpack, void* y, int F, int H, int W, int Cin, int Cout, hipStream_t st);
/* conv fwd + the train-mode BatchNorm statistics of y (tiny_vit.py:69-70, the stem's conv2
 * -> BN) from the GEMM epilogue, as sm_linear_bn_stats (workspace =
 * sm_linear_bn_stats_workspace_bytes(F*H*W, Cout)); replaces sm_conv3x3_fwd + sm_bn_stats. */
int sm_conv3x3_fwd_bn_stats(const void* x, const void* wpack, void* y, int F, int H, int W, int Cin, int Cout,
                            float* mean, float* rstd, float* run_mean, float* run_var, int64_t* num_batches_tracked,
                            float momentum, float eps, int updates, void* ws, int64_t ws_bytes, hipStream_t st);
int sm_conv3x3_dgrad(const void* dy, const void* wpack_t, void* dx, int F, int H, int W, int Cin, int Cout,
                     hipStream_t st);
int64_t sm_conv3x3_wgrad_workspace_bytes(int F, int H, int W, int Cin, int Cout);
int sm_conv3x3_wgrad(const void* dy, const void* x, float* dw, int accumulate, int F, int H, int W, int Cin, int Cout,
                     void* ws, int64_t ws_bytes, hipStream_t st);
int sm_dwconv_fwd(int dtype, const void* x, const float* w, void* y, int F, int H, int W, int C,
                  int stride, hipStream_t st);
int64_t sm_dwconv_wgrad_workspace_bytes(int F, int H, int W, int C, int stride);
/* Fused MBConv depthwise path (tiny_vit.py:48-51, bf16): y = dwconv3x3(act(x)) with the
 * producer's BN + GELU folded into the loads (in_mean == NULL: identity) and per-block
 * BN statistics partials of y written to part[sm_dwconv_fused_partial_rows][2][C]
 * (part nullable); backward: dx = dL/d act(x), dw += weight gradient with act(x)
 * recomputed. C % 32 == 0, stride 1 or 2. */
int64_t sm_dwconv_fused_partial_rows(int F, int H, int stride);
int sm_dwconv_fused_fwd(int F, int H, int W, int C, int stride, const void* x, const float* in_mean,
                        const float* in_rstd, const float* in_w, const float* in_b, int in_gelu,
                        const float* w, void* y, float* part, hipStream_t st);
int64_t sm_dwconv_fused_bwd_workspace_bytes(int F, int H, int W, int C, int stride);
int sm_dwconv_fused_bwd(int F, int H, int W, int C, int stride, const void* dy, const void* x,
                        const float* in_mean, const float* in_rstd, const float* in_w, const float* in_b,
                        int in_gelu, const float* w, void* dx, float* dw, void* ws, int64_t ws_bytes,
                        hipStream_t st);
// Depthwise conv (stride 1 or 2) + BatchNorm + GELU backward that never stores the depthwise
// data gradient (one pass over dy forming dw, dz = g GELU' and the BN sums, one
// streaming pass dz -> dx, dx doubling as the dz buffer): dx = dL/dx for y = dwconv3x3(GELU(BN(x))), dw += dL/dw,
// dgamma / dbeta += the BatchNorm's (MBConv conv1 -> act -> conv2, tiny_vit.py:36-56;
// replaces sm_dwconv_fused_bwd + sm_bn_bwd on that path).  F, H, W, C are the input's, dy is
// [F][(H-1)/stride+1][(W-1)/stride+1][C] (stride 2: the MBConv opening stages 1-3).  The GELU
// is built into the kernels: bn_gelu == 0 is refused (-2), here and in sm_dwconv_bn_bwd_dz.
int64_t sm_dwconv_bn_bwd_workspace_bytes(int F, int H, int W, int C);
int sm_dwconv_bn_bwd(int stride, int F, int H, int W, int C, const void* dy, const void* x, const float* bn_mean,
                     const float* bn_rstd, const float* bn_w, const float* bn_b, int bn_gelu, const float* w,
                     void* dx, float* dw, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes,
                     hipStream_t st);
/* The first pass alone (stride 1 or 2; same shapes, outputs and workspace): dz = g GELU'(BN(x))
 * stays in dz [F][H][W][C], coef [2][C] = mean(dz), mean(dz xhat); the BatchNorm's dx map
 * dx = bn_w rstd (dz - coef[0] - xhat coef[1]) is left to the consumer (sm_mbconv_fold_prep). */
int sm_dwconv_bn_bwd_dz(int stride, int F, int H, int W, int C, const void* dy, const void* x, const float* bn_mean,
                        const float* bn_rstd, const float* bn_w, const float* bn_b, int bn_gelu, const float* w,
                        void* dz, float* dw, float* dgamma, float* dbeta, float* coef, void* ws, int64_t ws_bytes,
                        hipStream_t st);
int sm_dwconv_bwd(int dtype, const void* dy, const void* x, const float* w, void* dx, float* dw, int F,
                  int H, int W, int C, int stride, void* ws, int64_t ws_bytes, hipStream_t st);

/* ---- SELayer (tiny_vit.py:20-34).  The SE input h = act(x) is recomputed from the
 * pre-BatchNorm tensor x by every kernel that reads it (act = BN2 + GELU of MBConv,
 * tiny_vit.py:50-51; act_mean == NULL: h = x). */
int64_t sm_se_workspace_bytes(int F, int HW, int C);
int sm_se_fwd(int dtype, const void* x, const float* act_mean, const float* act_rstd, const float* act_w,
              const float* act_b, int act_gelu, int F, int HW, int C, int R, const float* w1, const float* w2,
              float* pooled, float* z1, float* s, void* y, void* ws, int64_t ws_bytes, hipStream_t st);
int sm_se_bwd(int dtype, const void* dy, const void* x, const float* act_mean, const float* act_rstd,
              const float* act_w, const float* act_b, int act_gelu, int F, int HW, int C, int R,
              const float* w1, const float* w2, const float* s, const float* z1, float* dz2, float* dz1,
              void* dx, void* ws, int64_t ws_bytes, hipStream_t st);
int sm_se_scale(int dtype, const void* x, const float* act_mean, const float* act_rstd, const float* act_w,
                const float* act_b, int act_gelu, const float* s, void* y, int F, int HW, int C, hipStream_t st);
/* Fused backward of SE(GELU(BN2(x))) -- sm_se_bwd followed by sm_bn_bwd(gelu) on its
 * dx (tiny_vit.py:50-53), in two passes over (dy, x); dh2 is never materialised.
 * dw / db accumulate BN2's weight / bias gradients. */
int64_t sm_se_bn_bwd_workspace_bytes(int F, int HW, int C);
int sm_se_bn_bwd(int dtype, const void* dy, const void* x, const float* bn_mean, const float* bn_rstd,
                 const float* bn_w, const float* bn_b, int bn_gelu, int F, int HW, int C, int R, const float* w1,
                 const float* w2, const float* s, const float* z1, float* dz2, float* dz1, void* dx, float* dw,
                 float* db, void* ws, int64_t ws_bytes, hipStream_t st);

/* ---- MAE glue: tube mask (mae_loader.py:80-90) + masked-token compaction
 * (train_ssl_mae.py:105), pos-embed/mask-token blend (mae_vit_adapter.py:97-104),
 * fused patchify + norm_pix + masked MSE (train_ssl_mae.py:26-31,74-84). */
int sm_tube_mask(const float* noise, int B, int T, int L, int n_mask, uint8_t* mask, int32_t* idx,
                 hipStream_t st);
int sm_pos_blend_fwd(int y_dtype, int x_dtype, const void* y, const float* tpos, const float* spos,
                     const float* tok, const uint8_t* mask, void* x, int B, int T, int L, int D,
                     hipStream_t st);
int sm_pos_blend_bwd(int g_dtype, int y_dtype, const void* dx, const uint8_t* mask, void* dy,
                     float* dtpos, float* dspos, float* dtok, float* ws, int B, int T, int L, int D,
                     hipStream_t st);
int64_t sm_loss_workspace_bytes(int B, int T, int L);
int sm_mae_loss_fwd(int pred_dtype, const void* pred, const float* clip, int64_t sB, int64_t sC,
                    int64_t sT, int64_t sH, int64_t sW, const uint8_t* mask, int B, int T, int H, int W,
                    int norm_pix, float* loss, float* denom, void* ws, int64_t ws_bytes, hipStream_t st);
int sm_mae_loss_bwd(int pred_dtype, const void* pred, const float* clip, int64_t sB, int64_t sC,
                    int64_t sT, int64_t sH, int64_t sW, const uint8_t* mask, int B, int T, int H, int W,
                    int norm_pix, const float* grad_out, const float* denom, void* dpred, hipStream_t st);
int sm_patchify(const float* imgs, int B, int C, int T, int H, int W, int64_t sB, int64_t sC, int64_t sT,
                int64_t sH, int64_t sW, int p, float* out, hipStream_t st);
int sm_unpatchify(const float* tokens, int B, int C, int T, int H, int W, int p, float* imgs, hipStream_t st);
int sm_gather_rows(int dtype, const void* src, const int32_t* idx, int64_t nrows, int C, void* dst,
                   hipStream_t st);
int64_t sm_std_workspace_bytes(void);
int sm_std(int dtype, const void* x, int64_t n, float* out, void* ws, int64_t ws_bytes, hipStream_t st);

/* ---- fine-tune head (BASELINE config 4; src/train_finetune.py:19-40 VideoClassifier):
 * out[g][c] = mean_r x[g][r][c] for x [G][R][C] -- per-frame embedding pooling of the
 * channels-last encoder tokens (F.adaptive_avg_pool2d(feat, 1), mobilevit.py:164-165)
 * and the temporal mean of the fp32 embeddings (feats.mean(dim=1), :38); backward
 * dx[g][r][c] = dy[g][c] / R. */
int sm_segment_mean(int dtype, const void* x, int G, int R, int C, float* out, hipStream_t st);
int sm_segment_mean_bwd(int dtype, const float* dy, int G, int R, int C, void* dx, hipStream_t st);

/* ---- streaming dynamic inference (src/models/dynamic_infer.py; csrc/dynamic.hip), all fp32.
 * clip = fp32 [B][C][T][H][W] read through its five element strides (no permute copy),
 * 16-byte loads when sW == 1, W % 4 == 0 and the base and the other strides are 16-byte
 * multiples, scalar loads otherwise (same pixel ownership and summation order: same bits).
 *
 * sm_motion_scores (dynamic_infer.py:34-49 motion_scores_l1): scores[b][0] = 0,
 * scores[b][t] = mean over (c, h, w) of |x[b][c][t] - x[b][c][t-1]|; T == 1 gives zeros.
 * One pass over the clip (a block walks t over a band of one (b, c) plane with the previous
 * frame in registers); per-lane fp32 partials, wave reduce, then the per-wave partials summed
 * in fp64 in a fixed order: deterministic, no atomics.  Workspace
 * sm_motion_scores_workspace_bytes. */
int64_t sm_motion_scores_workspace_bytes(int B, int C, int T, int H, int W);
int sm_motion_scores(const float* clip, int B, int C, int T, int H, int W, int64_t sB, int64_t sC, int64_t sT,
                     int64_t sH, int64_t sW, float* scores, void* ws, int64_t ws_bytes, hipStream_t st);
/* dynamic_infer.py:66-71 (scores.topk(k).indices.sort()): idx int32 [B][k_eff], k_eff =
 * min(k, T), the indices of the k_eff largest scores of each row in ascending index order.
 * Where the reference leaves ties to torch.topk this defines them: among equal scores the
 * lower frame index ranks first (-0 == +0), and NaN ranks after every number (NaNs among
 * themselves by index).  T <= 256 and k >= 1, else -2. */
int sm_topk_frames(const float* scores, int B, int T, int k, int32_t* idx, hipStream_t st);
/* out fp32 dense [n][C][H][W], out[i] = clip[b_i][:, t_i] (dynamic_infer.py:80-81 torch.gather
 * of the selected frames; :175 clip[:, :, t] of the samples still active):
 * b_i = b_idx[i], or i / rows_per_b when b_idx is null; t_i = t_idx[i], or t_fixed when t_idx
 * is null.  An index outside the clip yields a zero frame. */
int sm_gather_frames(const float* clip, int B, int C, int T, int H, int W, int64_t sB, int64_t sC, int64_t sT,
                     int64_t sH, int64_t sW, const int32_t* b_idx, int rows_per_b, const int32_t* t_idx,
                     int t_fixed, int n, float* out, hipStream_t st);
/* One frame's update + decision of streaming_early_exit (dynamic_infer.py:152-186), one block
 * per active row i, s = active[i] (distinct, < B): if emb (fp32 [n][D], nullable) sum[s] +=
 * emb[i], cnt[s] += 1; mean = sum[s] / max(cnt[s], 1); logits = w mean + bias (w [K][D], fixed
 * reduction order); c = max softmax = 1 / sum_k exp(l_k - max l).  The sample is decided when
 * final_pass (the reference's closing pass over the undecided, :180-186), or when c >= threshold
 * and cnt[s] >= min_frames; a decided sample writes final_logits[s] [K], used[s] = cnt[s],
 * conf[s] = c, decided[s] = 1.  State: sum [B][D], cnt int32 [B], decided uint8 [B],
 * final_logits [B][K], used int32 [B], conf [B].  (D + K) * 4 bytes of LDS <= 64 KiB. */
int sm_exit_step(const float* emb, const int32_t* active, int n, int B, int D, int K, const float* w,
                 const float* bias, float threshold, int min_frames, int final_pass, float* sum, int32_t* cnt,
                 uint8_t* decided, float* final_logits, int32_t* used, float* conf, hipStream_t st);
/* The samples still undecided (the reference's ~decided mask, dynamic_infer.py:172, as an
 * index list): active int32 [B] <- ascending s with decided[s] == 0, *count <- their number. */
int sm_active_compact(const uint8_t* decided, int B, int32_t* active, int32_t* count, hipStream_t st);

/* ---- feature-privacy evaluation (src/run_privacy.py:229-348 run_feature_privacy; csrc/privacy.hip),
 * all fp32; 16-byte accesses when the shapes and pointers allow, scalar ones otherwise (same bits).
 *
 * sm_privacy_perturb (src/privacy/feature_noise.py:4-15, run_privacy.py:299-300): z [N][D] ->
 * out [G][N][D], out[g] = (z + sigma_g n_g(r, c)) keep_g(r, c), 1 <= G <= SM_PRIVACY_MAX_CONFIGS,
 * one launch that reads z once.  Noise first, then the 0/1 mask with no 1 / keep rescale;
 * sigma_g <= 0 adds nothing and thresholds[g] == 0 keeps everything (both bit-exact).  sigmas,
 * thresholds, seeds are HOST arrays of G.  The draws are a pure function of (seed, r, c):
 *   s32 = lo32(seed) ^ hi32(seed);  rb = fmix32(s32 + r * 0x9E3779B1)
 *   h_k = fmix32(fmix32(rb + K_k) + c * 0x7FEB352D),  K = {0x68E31DA4, 0xB5297A4D, 0x1B56C4E9}
 *   u1 = ((h0 >> 8) + 1) 2^-24 in (0, 1], u2 = (h1 >> 8) 2^-24, n = sqrt(-2 ln u1) cos(2 pi u2)
 *   keep = (uint64)h2 >= thresholds[g], thresholds[g] = min(round(ratio 2^32), 2^32) (> 2^32: -2)
 * so slice g of a grid call equals a G = 1 call with the same (sigma, threshold, seed) bit for bit.
 * N < 2^31. */
#define SM_PRIVACY_MAX_CONFIGS 64
int sm_privacy_perturb(const float* z, int64_t N, int D, int G, const float* sigmas, const uint64_t* thresholds,
                       const uint64_t* seeds, float* out, hipStream_t st);
/* Classification metrics of logits [rows][C], rows = S * N, the label of row i = labels[i % N]
 * (int64 [N]); one wave per row, C <= SM_LOGITS_MAX_CLASSES (else -2).  Per row: loss = logsumexp(l)
 * - l_y (nn.CrossEntropyLoss, run_privacy.py:312), entropy = -sum_j p_j log(p_j + 1e-12)
 * (metrics_privacy.py:5-8), hit1 / hitk = rank_y < 1 / < k with rank_y = #{j : l_j > l_y} +
 * #{j < y : l_j == l_y} (metrics_privacy.py:15-16, run_privacy.py:306; where torch leaves ties
 * open the lower index wins, as sm_topk_frames).  A NaN or +inf logit (or a label outside [0, C))
 * makes the row's loss NaN and the row a miss.  out fp64 [S][4] = sum loss, sum entropy, #hit1,
 * #hitk over each segment's N rows, added in fp64 in a fixed order.  dlogits (nullable) [rows][C]
 * <- (softmax(l) - onehot(y)) * grad_scale.  Workspace sm_logits_metrics_workspace_bytes(rows),
 * 16-byte aligned (else -4). */
#define SM_LOGITS_MAX_CLASSES 4096
int64_t sm_logits_metrics_workspace_bytes(int64_t rows);
int sm_logits_metrics(const float* logits, int64_t rows, int C, const int64_t* labels, int64_t N, int k,
                      float* dlogits, float grad_scale, double* out, void* ws, int64_t ws_bytes, hipStream_t st);
/* Cross-entropy of logits [N][C] against a two-label, smoothed target (Mixup / CutMix and label
 * smoothing in fine-tuning; the reference has neither), sm_logits_metrics' row kernel with another
 * target: t_c = lam_i s(ya_i)_c + (1 - lam_i) s(yb_i)_c, s(y)_c = eps / C + (1 - eps) [c == y], ya =
 * labels_a, yb = labels_b (int64 [N]), lam fp32 [N]; a null labels_b or a null lam means lam_i = 1.
 * loss_i = -sum_c t_c (l_c - logsumexp(l)), formed as (logsumexp(l) - l_ya) - sum_c d_c (l_c - max l)
 * with d = t - onehot(ya) (sum_c d_c = 0): finite for large logits, and exactly sm_logits_metrics'
 * loss when the target is the one-hot of ya.  dlogits (nullable) [N][C] <- (softmax(l) - t) *
 * grad_scale.  out fp64 [2] = sum of the row losses, number of rows whose arg-max is ya_i (ties to
 * the lower index: the rank rule above with k = 1), the row values added in fp64 in
 * sm_logits_metrics' order.  With eps == 0 and no labels_b / lam, out[0], out[1] and dlogits equal
 * those of sm_logits_metrics(..., k = 1, ...) bit for bit.  A label outside [0, C), or a NaN or +inf
 * logit, makes the row's loss NaN and the row a miss.  -2: C > SM_LOGITS_MAX_CLASSES, eps outside
 * [0, 1), N < 1 or a null pointer; workspace sm_soft_ce_workspace_bytes(N), 16-byte aligned (else -4). */
int64_t sm_soft_ce_workspace_bytes(int64_t N);
int sm_soft_ce(const float* logits, int64_t N, int C, const int64_t* labels_a, const int64_t* labels_b,
               const float* lam, float eps, float* dlogits, float grad_scale, double* out, void* ws, int64_t ws_bytes,
               hipStream_t st);
/* The attacker's hidden layer (src/privacy/attacker.py:11-15 nn.ReLU between two Linears):
 * h[i] = max(pre[i], 0) (NaN stays NaN); backward dpre = dh * (h > 0) and db[c] = sum over the M
 * rows of dpre[.][c] (the first Linear's bias gradient) in the same pass: fp32 partial sums over
 * chunks of 32 rows, the chunks added in fp64 in a fixed order.  Workspace
 * sm_relu_bias_bwd_workspace_bytes; M <= 32 * 65535. */
int sm_relu_fwd(const float* pre, int64_t n, float* h, hipStream_t st);
int64_t sm_relu_bias_bwd_workspace_bytes(int64_t M, int C);
int sm_relu_bias_bwd(const float* dh, const float* h, int64_t M, int C, float* dpre, float* db, void* ws,
                     int64_t ws_bytes, hipStream_t st);

/* ---- MAE reconstruction evaluation (src/visualize_mae.py:162-208, the token-error map of
 * src/mae/visualize.py:47-58; csrc/recon.hip).  p = 8, C = 3 as the loss; H % 8 or W % 8: -2.
 *
 * sm_mae_reconstruct: one launch over pred [B][T*L][192] (fp32 or bf16 by pred_dtype, as
 * sm_mae_loss_fwd), clip fp32 [B][3][T][H][W] through its five element strides and mask uint8
 * [B][T][L]; the target and the reconstruction are never stored as token tensors.  Per token, x
 * the 192 clip values of its patch in feature order f = (p * 8 + q) * 3 + c:
 *   target   norm_pix: mu = mean(x), var = sum((x - mu)^2) / 191, tgt = (x - mu) / sqrt(var + 1e-6)
 *            (the loss's operations, train_ssl_mae.py:74-77); otherwise tgt = x
 *   recon    r = pred * sqrt(var + 1e-6) + mu (norm_pix) or pred: the prediction in clip space;
 *            with paste_visible a visible token (mask == 0) shows r = x instead
 *   display  clip channel c is source channel s = 2 - c when bgr_swap, else c (the inverse of
 *            sm_frames_normalize); v = value * std3[s] + mean3[s], written at RGB position s
 *   byte     floor(clamp(v, 0, 1) * 255), the reference's (x * 255).astype(uint8)
 * Outputs:
 *   panels    uint8 [B][T][H][3 * W][3]: original | masked original | reconstruction, HWC RGB
 *             strips ready for an image file; the pixels of masked patches are 0 in the middle panel
 *   recon     (nullable) fp32 [B][3][T][H][W], dense: the display value v of the reconstruction,
 *             not clamped, RGB channel order
 *   token_err fp32 [B * T * L][2]: [0] = mean_f (pred - tgt)^2, the loss map entry
 *             (train_ssl_mae.py:81-82); [1] = mean_f (clamp(v_r, 0, 1) - clamp(v_x, 0, 1))^2 with
 *             v_r from r before paste_visible and v_x from x (where neither clamps, the difference
 *             is formed as (pred - tgt) sqrt(var + 1e-6) std3[s], which does not cancel)
 * mean3 / std3 are HOST arrays of 3 floats indexed by RGB position.  One wave per four tokens,
 * fixed reduction order, no atomics: bitwise reproducible.  The panels are stored as packed
 * dwords when their base is 4-byte aligned, as bytes otherwise (same bits).  T * L < 2^31 and
 * B * T * L < 2^35 (else -2); a null pred, clip, mask, mean3, std3,
 * panels or token_err, or a pred_dtype that is neither, is -2; nothing is launched on -2.
 *
 * sm_recon_clip_metrics: token_err and mask as above -> out fp32 [B][4] = mean of token_err[.][0]
 * over the clip's masked tokens, mean of token_err[.][1] over them (mse_pix), PSNR =
 * 10 log10(1 / mse_pix) dB, n_masked.  n_masked == 0 gives means 0; mse_pix == 0 gives PSNR +inf.
 * One block per clip, fp64 sums in a fixed order, no atomics: bitwise reproducible. */
int sm_mae_reconstruct(int pred_dtype, const void* pred, const float* clip, int64_t sB, int64_t sC, int64_t sT,
                       int64_t sH, int64_t sW, const uint8_t* mask, int B, int T, int H, int W, const float* mean3,
                       const float* std3, int norm_pix, int paste_visible, int bgr_swap, uint8_t* panels,
                       float* recon, float* token_err, hipStream_t st);
int sm_recon_clip_metrics(const float* token_err, const uint8_t* mask, int B, int T, int L, float* out,
                          hipStream_t st);

/* ---- optimizer (train_ssl_mae.py:163 AdamW, :87-89 GradScaler inf-skip) */
int sm_nonfinite(const float* g, int64_t n, int* flag, hipStream_t st);
/* p *= a (data-parallel gradient averaging after a SUM all-reduce) */
int sm_scale(float* p, int64_t n, float a, hipStream_t st);
int sm_adamw(float* p, const float* g, float* m, float* v, void* bf16_shadow, int64_t n, float lr,
             float b1, float b2, float eps, float wd, const int* found_inf, int64_t* step,
             int advance_step, hipStream_t st);

/* ---- grouped AdamW: one launch updates any number of fp32 ranges, each with the learning rate
 * and weight decay of its parameter group (fine-tuning with a head / backbone learning rate,
 * layer-wise learning-rate decay, no decay on biases and norms).
 *
 * AdamW segment table (DEVICE memory, 16-byte aligned, built once per set of S segments; a
 * segment is one contiguous fp32 range with its gradient and its two moment ranges):
 *   SmAdamwTableHeader                     64 bytes
 *   uint64_t addr[4][S]                    device addresses of segment s: row 0 the parameters,
 *                                          1 the gradients, 2 exp_avg, 3 exp_avg_sq; each a
 *                                          multiple of 4, not necessarily of 16
 *   int64_t  seg_len[S]                    elements (0 allowed: such a segment has no chunk)
 *   int64_t  chunk_off[C]                  first element of the chunk within its segment,
 *                                          a multiple of SM_ADAMW_CHUNK_ELEMS
 *   int32_t  chunk_seg[C]                  the chunk's segment; a chunk covers
 *                                          min(SM_ADAMW_CHUNK_ELEMS, seg_len - chunk_off) elements
 *   int32_t  seg_group[S]                  the segment's parameter group
 *   zero padding to a multiple of 16 bytes
 * total_bytes = 64 + 44 S + 12 C rounded up to 16.  The chunks together cover every element of
 * every segment once.
 *
 * sm_adamw_table: sm_adamw's update (the same device function, bit for bit) of every element of
 * every segment, segment s with fp32(lr[seg_group[s]] * lr_mult) and wd[seg_group[s]]; lr and wd
 * are HOST arrays of num_groups (1..SM_ADAMW_MAX_GROUPS) floats, passed to the kernel by value.
 * check_finite != 0: *found_inf is reset, then set to 1 when any gradient element of any segment
 * is not finite; the update then writes nothing and *step keeps its value.  Otherwise every
 * segment is updated at step *step + 1 and *step advances once.  check_finite == 0: found_inf is
 * neither read nor written (may be NULL).  At most three operations are enqueued on the stream
 * (the flag's reset, the flag pass, the update pass) and the host is never synchronised: the
 * header was validated when the table was built and is not read back (the kernels compare its
 * magic and counts with the arguments and touch nothing on a mismatch).  A chunk moves as 16-byte
 * vectors when its four bases are 16-byte aligned, else element by element; each segment's
 * len % 4 tail is scalar; the update is element-wise, so both forms give the same bits.  No
 * atomics in the update pass.
 * Returns -2, with nothing launched, for a NULL table, lr, wd, step (or found_inf with
 * check_finite), a table that is not 16-byte aligned, negative counts, num_groups outside
 * 1..SM_ADAMW_MAX_GROUPS or a table_bytes that is not the formula's value for the counts; 0, with
 * nothing launched, for zero segments (or zero chunks). */
#define SM_ADAMW_MAX_GROUPS 64
#define SM_ADAMW_CHUNK_ELEMS 2048
#define SM_ADAMW_TABLE_MAGIC 0x314254574D414441LL /* "ADAMWTB1" */
typedef struct SmAdamwTableHeader {
  int64_t magic, num_segments, num_chunks, chunk_elems, total_bytes, reserved[3];
} SmAdamwTableHeader;
int sm_adamw_table(const void* table, int64_t table_bytes, int64_t num_segments, int64_t num_chunks,
                   int num_groups, const float* lr, const float* wd, float lr_mult, float b1, float b2,
                   float eps, int* found_inf, int64_t* step, int check_finite, hipStream_t st);

/* ---- temporal SSL pretraining (src/train_ssl.py; csrc/temporal.hip).  No atomics: every
 * reduction has a fixed partition and order, results are bitwise reproducible.
 *
 * sm_mfm_loss_fwd: the masked-frame objective (train_ssl.py:26-34, :215-220) over the N rows idx
 * (int32, ascending, each in [0, R)) of pred [R][D] (fp32 or bf16) and teacher [R][D] (fp32), both
 * contiguous.  With s_i = pred_i / max(|pred_i|, 1e-12) and u_i the same of the teacher row:
 *   mfm     = 2 - (2 / N) sum_i s_i . u_i
 *   sigma_c = sqrt(biased var_i(s_ic) + eps),  var = mean_c max(0, target_std - sigma_c)
 *   out[3]  = mfm, var, w_mfm mfm + w_var var
 * (the reference normalises a second time inside cosine_loss: the identity up to rounding).
 * stats (fp32, 3 N + 2 D elements) receives what the backward reuses: per masked row the two
 * inverse norms and the cosine, per column the mean and the hinge's factor.  Workspace
 * sm_mfm_loss_workspace_bytes (8-byte aligned; -4 if short).  Row dot products are fp32 fmas in
 * a fixed lane ownership, sums over rows / columns fp64.
 * sm_mfm_loss_bwd: dpred [R][D] (fp32 or bf16) = grad_out[0] (device scalar) x d out[2] / d pred;
 * rows not in idx are written as exact zeros.
 * Both have a 16-byte form (D a multiple of 16 bytes of the pred dtype, bases 16-byte aligned)
 * and a scalar form with the same element ownership: same bits.  -2 on a bad shape (N > R,
 * N > 32 * 65535), dtype or null pointer; nothing is launched then. */
int64_t sm_mfm_loss_workspace_bytes(int N, int D);
int sm_mfm_loss_fwd(int pred_dtype, const void* pred, const float* teacher, const int32_t* idx, int R, int N,
                    int D, float w_mfm, float w_var, float target_std, float eps, float* out, float* stats,
                    void* ws, int64_t ws_bytes, hipStream_t st);
int sm_mfm_loss_bwd(int pred_dtype, int dpred_dtype, const void* pred, const float* teacher, const int32_t* idx,
                    int R, int N, int D, const float* stats, const float* grad_out, float w_mfm, float w_var,
                    void* dpred, hipStream_t st);
/* update_ema (train_ssl.py:36-39) over flat fp32 buffers: dst = m dst + one_minus_m src, the
 * product rounded and the sum one fma; one launch.  The caller passes fp32(m) and
 * fp32(1.0 - m), the difference formed in double, as torch rounds the two scalars. */
int sm_ema_update(float* dst, const float* src, int64_t n, float m, float one_minus_m, hipStream_t st);
/* torch.nn.utils.clip_grad_norm_ (train_ssl.py:258-259) over the element ranges
 * [starts[i], ends[i]) of grad (HOST arrays): norm_out[0] = the L2 norm of the ranges' elements
 * (squares added in fp64: per 8192-element chunk of a range, then over the chunks in order),
 * then grad *= coef, coef = min(1, max_norm / (norm + 1e-6)) formed in fp32 on the device (no
 * host synchronise; coef == 1 writes nothing).  A non-finite norm leaves non-finite values in
 * grad, as torch with error_if_nonfinite=False.  Workspace sm_grad_clip_workspace_bytes (-1 on
 * a bad range), 8-byte aligned. */
int64_t sm_grad_clip_workspace_bytes(const int64_t* starts, const int64_t* ends, int nranges);
int sm_grad_clip(float* grad, const int64_t* starts, const int64_t* ends, int nranges, float max_norm,
                 float* norm_out, void* ws, int64_t ws_bytes, hipStream_t st);
/* nn.TransformerEncoderLayer's ReLU + dropout on [n / ncols][ncols] (fp32 or bf16, ncols % 8 == 0,
 * 16-byte aligned): y = max(x, 0) keep(row, col) drop_scale16(p), the mask csrc/common.h's counter
 * hash of (seed, row, col) with the 16-bit threshold round(65536 p) (keep rate 0.899994 at
 * p = 0.1, kept values scaled by its inverse); drop_p == 0 is ReLU bit for bit (NaN stays NaN).
 * Backward: dx = dy keep drop_scale16(p) where ref > 0, the mask regenerated from the seed; ref is
 * the forward's x or its y. */
int sm_relu_dropout_fwd(int dtype, int64_t n, int ncols, const void* x, void* y, float drop_p, uint64_t seed,
                        hipStream_t st);
int sm_relu_dropout_bwd(int dtype, int64_t n, int ncols, const void* ref, const void* dy, void* dx, float drop_p,
                        uint64_t seed, hipStream_t st);

/* ---- federated averaging (src/federated/fed_loop.py:14-62 fedavg_aggregate).
 * out[i] = sum_j client_bufs[j][i] * weights[j], accumulated from +0 in client order
 * with the product and the sum rounded separately (fed_loop.py:46-49, weights[j] =
 * fp32(w_j / total_w)): bit-identical to the reference's CPU loop.  client_bufs is a
 * HOST array of num_clients device pointers (1 <= num_clients <= SM_FEDAVG_MAX_CLIENTS),
 * each holding one client's floating-point state_dict entries flattened in key order.
 * sm_fedavg_counters_max: out[i] = max_j client_counters[j][i] (num_batches_tracked,
 * fed_loop.py:52-55). */
#define SM_FEDAVG_MAX_CLIENTS 32
int sm_fedavg_weighted_sum(int num_clients, const float* const* client_bufs, const float* weights, int64_t n,
                           float* out, hipStream_t st);
int sm_fedavg_counters_max(int num_clients, const int64_t* const* client_counters, int64_t n, int64_t* out,
                           hipStream_t st);

/* ---- FedAvg round exchange over a cohort's state entries where they live: one launch
 * reads every source model's tensors and writes the result into every destination model's.
 *
 * FedAvg exchange table (DEVICE memory, 16-byte aligned, built once per cohort of P models,
 * 1 <= P <= SM_FEDAVG_MAX_CLIENTS + 1; a segment is one state entry, laid out identically --
 * same length, contiguous -- in every model):
 *   SmFedTableHeader                       64 bytes
 *   uint64_t addr[P][S]                    device address of segment s in model p
 *   int64_t  seg_len[S]                    elements
 *   int64_t  chunk_off[C]                  first element of the chunk within its segment,
 *                                          a multiple of SM_FEDAVG_CHUNK_ELEMS
 *   int32_t  chunk_seg[C]                  the chunk's segment; a chunk covers
 *                                          min(SM_FEDAVG_CHUNK_ELEMS, seg_len - chunk_off) elements
 *   zero padding to a multiple of 16 bytes
 * total_bytes = 64 + 8 P S + 8 S + 12 C rounded up to 16.  The chunks together cover every
 * element of every segment once.  elem_bytes is 4 (fp32 segments, sm_fedavg_exchange) or 8
 * (int64 segments, sm_fedavg_exchange_counters); every address is a multiple of elem_bytes.
 *
 * sm_fedavg_exchange: for every element i of every segment, acc = +0, then in src order
 * acc = fadd_rn(acc, fmul_rn(x_j[i], weights[j])) -- sm_fedavg_weighted_sum's operations in
 * its order, so bit-identical to it -- stored to element i of the segment in every dst model.
 * copy_only = 1 needs num_src == 1 and stores x_0[i] unchanged (a bit copy: -0 and NaN
 * payloads survive; weights may be NULL).  src_models / dst_models (model indices into the
 * table, 1 <= num_src <= SM_FEDAVG_MAX_CLIENTS, 1 <= num_dst <= SM_FEDAVG_MAX_CLIENTS + 1) and
 * weights are HOST arrays.  A destination may also be a source: the lane that writes element i
 * has loaded it from every source first.  A chunk moves as 16-byte vectors when its segment's
 * base is 16-byte aligned in every model of the launch, else element by element; each segment's
 * len % 4 tail is scalar.
 * sm_fedavg_exchange_counters: the int64 max over the sources instead.
 * Both read the table's header back (64 bytes, a stream synchronisation) and return -2 for bad
 * counts, NULL arrays or table, a header that does not match table_bytes / the element size /
 * the chunk size, or a model index outside [0, P). */
#define SM_FEDAVG_CHUNK_ELEMS 2048
#define SM_FEDAVG_TABLE_MAGIC 0x31424154444546LL /* "FEDTAB1" */
typedef struct SmFedTableHeader {
  int64_t magic, num_models, num_segments, num_chunks, elem_bytes, chunk_elems, total_bytes, reserved;
} SmFedTableHeader;
int sm_fedavg_exchange(int num_src, const int32_t* src_models, const float* weights, int num_dst,
                       const int32_t* dst_models, const void* table, int64_t table_bytes, int copy_only,
                       hipStream_t st);
int sm_fedavg_exchange_counters(int num_src, const int32_t* src_models, int num_dst, const int32_t* dst_models,
                                const void* table, int64_t table_bytes, hipStream_t st);

/* ---- DP-FedAvg round exchange (McMahan et al. 2018; not in the reference) over the fp32 FedAvg
 * exchange table above: every source's update x_c - theta is clipped to an L2 bound, the clipped
 * updates are averaged onto theta and Gaussian noise is added; the result goes into every dst model.
 * src_models, weights (already normalised) and dst_models are HOST arrays as for sm_fedavg_exchange;
 * global_model is theta's model index and may be a destination.  seg_clip (DEVICE, one byte per
 * segment of the table): 1 = clipped and noised, 0 = sm_fedavg_exchange's plain weighted sum of the
 * sources, bit for bit.  stats (DEVICE, float [2 num_src]) receives norm_c, then scale_c.
 * Three launches, no atomics, no host synchronise beyond the header read:
 *   norms     norm_c = sqrt(sum over the clipped segments' elements of (x_c[i] - theta[i])^2): the
 *             fp32 differences squared, a lane adding at most 8 of them (one chunk's share) in fp32,
 *             everything above a lane in fp64 in a fixed order -- the same bits on every call
 *   finalise  scale_c = min(1, clip_norm / (norm_c + 1e-6f)) in fp32 on the device (the form of
 *             sm_grad_clip's coefficient; a non-finite norm_c goes through the same expression),
 *             ws_c = fmul_rn(weights[c], scale_c)
 *   update    clipped segment s, element i: acc = theta[i]; in src order acc = fadd_rn(acc,
 *             fmul_rn(ws_c, fsub_rn(x_c[i], theta[i]))); then, when noise_std > 0,
 *             acc = fmaf(noise_std, n, acc) with n sm_privacy_perturb's Gaussian of (seed, row = s,
 *             column = i)
 * A lane loads its elements from theta and every source before its first store, so destinations
 * may alias sources and theta.  A chunk moves as 16-byte vectors when it is 16-byte aligned in every
 * model of the launch, else element by element, with the same bits.
 * Workspace sm_fedavg_dp_exchange_workspace_bytes (-1 for a bad count), 16-byte aligned.
 * Returns -2 as sm_fedavg_exchange does, and for NULL weights / seg_clip / stats, global_model
 * outside [0, P), clip_norm <= 0 or NaN, noise_std < 0 or NaN, a clipped segment of more than 2^32
 * elements (the draw's column is 32 bits; the lengths are read back only from a table large enough
 * to hold such a segment) or more than 2^32 segments; -4 for a NULL, short or misaligned workspace.
 * Nothing is written in either case. */
int64_t sm_fedavg_dp_exchange_workspace_bytes(int num_src, int64_t num_chunks);
int sm_fedavg_dp_exchange(int num_src, const int32_t* src_models, const float* weights, int global_model,
                          int num_dst, const int32_t* dst_models, const void* table, int64_t table_bytes,
                          const uint8_t* seg_clip, float clip_norm, float noise_std, uint64_t seed, float* stats,
                          void* ws, int64_t ws_bytes, hipStream_t st);

/* ---- Compressed FedAvg round exchange (int8 block quantisation with error feedback: Seide et al.
 * 2014, Karimireddy et al. 2019; not in the reference) over the fp32 FedAvg exchange table above, in
 * one launch with no workspace.  src_models, weights (already normalised), global_model and dst_models
 * as for sm_fedavg_dp_exchange; every source is a client model: a source equal to global_model is -2.
 * seg_mode (DEVICE, one byte per segment): 1 = quantised, 0 = sm_fedavg_exchange's plain weighted sum
 * of the sources, bit for bit.
 * resid (DEVICE, fp32 [num_rows][num_chunks * SM_FEDAVG_CHUNK_ELEMS], 16-byte aligned): the sources'
 * quantisation residuals, row = model index - 1, element c * SM_FEDAVG_CHUNK_ELEMS + i = element i of
 * chunk c; read and updated in place for the quantised chunks' elements, nothing else is touched.
 * A block is SM_FEDAVG_Q8_BLOCK consecutive elements of a chunk.  For every element of a quantised
 * segment, for every source j in source order, every operation rounded on its own (no fma):
 *   v    = fadd_rn(fsub_rn(x_j, theta), e_j)
 *   m    = max over the block of |v| (exact; a NaN in the block makes m NaN; slots past the chunk's
 *          end count as 0)
 *   live = m >= 1e-30f and m finite
 *   s    = live ? fdiv_rn(m, 127) : 0,  inv = live ? fdiv_rn(127, m) : 0
 *   q    = live ? clamp(rint(fmul_rn(v, inv)), -127, 127) : 0      (round-half-even)
 *   d    = fmul_rn((float)q, s);  e_j = fsub_rn(v, d)             (a dead block keeps all of v)
 *   acc  = theta, then acc = fadd_rn(acc, fmul_rn(weights[j], d)) in source order
 * and acc goes to the element in every dst model.  What a client uploads is (q, s): one byte per
 * element and one fp32 per block.  The payload is optional -- with codes or scales NULL neither is
 * written: codes (DEVICE, int8 [num_src][num_chunks][SM_FEDAVG_CHUNK_ELEMS], 4-byte aligned) and
 * scales (DEVICE, fp32 [num_src][num_chunks][SM_FEDAVG_CHUNK_ELEMS / SM_FEDAVG_Q8_BLOCK]), written in
 * full: zeros for slots past a chunk's end and for chunks of mode-0 segments.
 * part (DEVICE, double [num_src][num_chunks][2]) receives, for every chunk, (max |v| of the chunk,
 * sum of the squares of the chunk's new residual): the squares are fp32, a lane adds its 8 in fp32
 * in ascending order, everything above a lane is fp64 in a fixed order -- the same bits on every
 * call; (0, 0) for the chunks of mode-0 segments.  No atomics.
 * A lane loads its elements from theta and every source before its first store into a model, so
 * destinations may alias sources and theta; resid, codes, scales and part overlap no model.  A chunk
 * moves as 16-byte vectors when it is 16-byte aligned in every model of the launch, else element by
 * element, with the same bits.
 * Returns -2 as sm_fedavg_exchange does, and for NULL weights / seg_mode / resid / part, global_model
 * outside [0, P), num_rows < 1, or a source that is global_model or whose row is outside
 * [0, num_rows); -4 for a misaligned resid, part, codes or scales.  Nothing is written in either case. */
#define SM_FEDAVG_Q8_BLOCK 256
int sm_fedavg_q8_exchange(int num_src, const int32_t* src_models, const float* weights, int global_model,
                          int num_dst, const int32_t* dst_models, const void* table, int64_t table_bytes,
                          const uint8_t* seg_mode, float* resid, int num_rows, int8_t* codes, float* scales,
                          double* part, hipStream_t st);

/* ---- clip input pipeline (src/train_ssl_mae.py:137-141 PILToTensor + ConvertImageDtype +
 * Normalize; src/datasets/mae_loader.py:70-77 BGR swap img[[2,1,0]] and [C,T,H,W] stack).
 * frames uint8 [B][T][H][W][3] (decoded RGB) -> out fp32 [B][3][T][H][W],
 * out = (u / 255 - mean[s]) / std[s] with s = 2 - c when bgr_swap (IEEE division,
 * bit-identical to the CPU transform); valid[b] == 0 (nullable) writes a zero clip
 * (mae_loader.py:35-43).  mean3 / std3 are HOST arrays of 3 floats. */
int sm_frames_normalize(const uint8_t* frames, const uint8_t* valid, int B, int T, int H, int W, const float* mean3,
                        const float* std3, int bgr_swap, float* out, hipStream_t st);

/* Resize + flip + normalise a batch of decoded clips that each keep their own frame size
 * (src/datasets/mae_dataset.py:84-90 u8 / 255 -> F.interpolate(bilinear, align_corners=False)
 * -> clip-level horizontal flip -> Normalize), one launch, no workspace, no host sync.
 * packed uint8: clip b is [T][Hs_b][Ws_b][3] (RGB, HWC) starting at byte desc[b][0];
 * desc int64 [B][4] (DEVICE) = {byte offset, Hs, Ws, flags}, flags bit 0 = flip horizontally,
 * bit 1 = invalid clip.  out fp32 [B][3][T][Ho][Wo], Ho, Wo <= 4096.  A clip is written as
 * zeros when it is flagged invalid, when Hs or Ws is outside [1, 8192] or when its byte range
 * leaves [0, packed_bytes); nothing outside `packed` is read.  Per axis (n_in source, n_out
 * output samples, output index d): n_in == n_out takes sample d; otherwise scale = fp32(n_in) /
 * fp32(n_out), src = max(fma(scale, d + 0.5, -0.5), 0), i0 = min((int)src, n_in - 1),
 * l1 = clamp(src - i0, 0, 1), i1 = i0 + (i0 < n_in - 1), l0 = 1 - l1.  With p = fp32(u) / 255:
 * r = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11), every product and sum rounded on its
 * own; a flipped clip writes column x's r to column Wo-1-x; out[c] = (r - mean[s]) / std[s],
 * s = 2 - c when bgr_swap (source channel s).  A clip already at (Ho, Wo), not flipped, equals
 * sm_frames_normalize bit for bit.  mean3 / std3 are HOST arrays of 3 floats.  Returns 0 (also
 * for an empty output), -2 for a null pointer or a bad count (nothing launched), or the
 * hipError_t of the launch. */
int sm_frames_resize_normalize(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int B, int T, int Ho,
                               int Wo, const float* mean3, const float* std3, int bgr_swap, float* out,
                               hipStream_t st);

/* The same launch with a source window per clip (random-resized crop): desc int64 [B][8] =
 * {byte offset, Hs, Ws, flags, y0, x0, Hc, Wc}; clip b is still [T][Hs][Ws][3] in `packed`.  The
 * result equals, bit for bit, sm_frames_resize_normalize applied to a buffer that holds only
 * rows [y0, y0 + Hc) x columns [x0, x0 + Wc) of every frame: each axis runs with n_in = Hc
 * (resp. Wc), so i1 = i0 + (i0 < Hc - 1) clamps at the window's edge and no pixel outside the
 * window contributes, and y0 / x0 are added to i0 and i1.  The flip is within the window.  The
 * window (0, 0, Hs, Ws) gives the bits of sm_frames_resize_normalize.  A clip is written as zeros
 * under every rule above and also when y0 < 0, x0 < 0, Hc < 1, Wc < 1, y0 + Hc > Hs or
 * x0 + Wc > Ws; nothing outside `packed` is read.  Arguments and return values as above. */
int sm_frames_crop_resize_normalize(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int B, int T,
                                    int Ho, int Wo, const float* mean3, const float* std3, int bgr_swap, float* out,
                                    hipStream_t st);

/* ---- mixing regularisation for fine-tuning (csrc/mix.hip): Mixup and CutMix of a batch with its own
 * flip in ONE pass (the reference has no augmentation; the pairing is the usual batch-flip rule).
 * x, out fp32 [B][planes][H][W] contiguous (planes = 3 * T; only the product is used).  Clip b is paired
 * with clip B - 1 - b: P = B / 2 pairs, lam_px device fp32 [P], box device int32 [P][4] = (y0, x0, h, w),
 * shared by both clips of a pair.  Per element, a the clip's own pixel and q the partner's pixel at
 * the same position:
 *   inside the box, rows [y0, y0 + h) x columns [x0, x0 + w) of EVERY plane (so of every frame: the
 *   mix is clip-consistent)                     out = q
 *   outside the box and lam_px == 1             out = a   (a select: a non-finite q does not leak
 *                                                          through a 0 * q)
 *   outside the box otherwise                   out = fl(fl(lam_px a) + fl(fl(1 - lam_px) q))
 * every operation rounded on its own (no fma), so clip b gets lam x[b] + (1 - lam) x[B-1-b] and its
 * partner lam x[B-1-b] + (1 - lam) x[b]; bit for bit tests/mix_mirror.py.  The middle clip of an odd
 * batch is copied unchanged.  One thread owns the same element of both clips of a pair, reads each
 * source element once and writes each output element once, so out == x (in place) is legal; any
 * other overlap of x and out is not.  16-byte accesses when W % 4 == 0 and x and out are 16-byte
 * aligned, scalar ones otherwise (same bits).  The box is only a predicate on (row, column), never
 * an address; a box that leaves the frame or has a negative side must be refused on the host
 * BEFORE the upload (kernels.clip_mix does), since the table lives on the device.  B == 0: 0.
 * -2: a null pointer, planes / H / W < 1, B < 0, planes * H * W >= 2^31 or more than 65535 pairs
 * (the launch's grid limits). */
int sm_clip_mix(const float* x, int64_t B, int64_t planes, int H, int W, const float* lam_px, const int32_t* box,
                float* out, hipStream_t st);

/* ---- visual privacy (csrc/anonymize.hip; the anonymisation half of the reference's
 * src/run_privacy.py:118-226 run_visual_privacy: cv2.GaussianBlur over detected boxes.  The detector
 * is not part of this build: the boxes are an input).  One kernel launch each (the statistics after
 * a memset of their output on the same stream), no workspace, no host sync.
 *
 * packed uint8: frame n is [H_n][W_n][3] (RGB, HWC) starting at byte desc[n][0]; desc int64 [N][3]
 * (DEVICE) = {byte offset, H, W}; frames of one call may differ in size, offsets need no alignment.
 * boxes int32 [num_boxes][4] (DEVICE) = {x, y, w, h}; box_start int32 [N + 1] (DEVICE): frame n
 * owns boxes [box_start[n], box_start[n + 1]).  max_h / max_w are host upper bounds on the frame
 * sizes of the call: the grid is N x ceil(max_h / SM_BOX_TILE_H) x ceil(max_w / SM_BOX_TILE_W)
 * blocks, so the host never reads desc back.
 *
 * Validity is decided in the kernel; nothing outside packed, boxes or box_start is read.  A frame
 * is skipped (its bytes of `out` are not written, its stats row is zeros) when H or W is outside
 * [1, 8192], when H > max_h or W > max_w, or when its byte range leaves [0, packed_bytes).  The ends
 * of a box range are clamped into [0, num_boxes]; a reversed range is empty.  A box is clipped to
 * its frame, x0 = max(x, 0), x1 = min(x + w, W), likewise y, the sums in 64 bits; it is empty when
 * w <= 0, h <= 0 or nothing remains.  (The reference's numpy slice img[y:y+h, x:x+w] drops a box
 * that starts at a negative coordinate; this build clips it.)
 *
 * sm_frames_box_blur: with U the union of a frame's clipped boxes, a pixel outside U keeps its
 * input bytes; a pixel in U gets, per channel, the separable Gaussian of the ORIGINAL frame.
 * weights is a HOST array of ksize floats, ksize odd in [3, 63], r = (ksize - 1) / 2.  refl(i, n) is
 * the reflect-101 index (no edge repetition), periodic and so defined for n <= r too: 0 for
 * n == 1; otherwise p = 2 (n - 1), i = i mod p (non-negative), and i >= n maps to p - i.
 *   h(y, x) = acc after acc = acc + weights[i] * fp32(u[y][refl(x + i - r, W)]) for i = 0 .. ksize - 1
 *             ascending from acc = 0, every product and every sum rounded to fp32 on its own (no fma)
 *   v(y, x) = the same over weights[i] * h(refl(y + i - r, H), x)
 *   out     = (uint8) min(255, max(0, rintf(v))), round-half-even
 * A pixel has one summation order: the result does not depend on the tiling, on the number of
 * boxes, their order or their overlap, and two calls give the same bits.  For one box this is
 * cv2.GaussianBlur(roi, (k, k), 0) on a ROI view in exact arithmetic (OpenCV too reads the parent
 * image beyond the ROI and reflects only at the frame's edge).  Two documented deviations from the
 * reference: its sequential loop blurs already-blurred pixels where two boxes lie closer than r,
 * this does not; and OpenCV's 8-bit path is fixed-point: agreement within one grey level is
 * expected but NOT MEASURED (no OpenCV where this was built).
 *
 * sm_box_region_stats: a and b are two buffers of the layout above (packed_bytes each, one desc).
 * stats int64 [N][4] = {P, SSE, Ea, Eb} per frame: P = pixels in U; SSE = sum over U and 3
 * channels of (a - b)^2; E_img = sum over pixels (y, x) in U and 3 channels of
 * [x + 1 < W] (img[y][x+1] - img[y][x])^2 + [y + 1 < H] (img[y+1][x] - img[y][x])^2 (a neighbour may
 * lie outside U); Ea = E_a, Eb = E_b.  All exact integers (64-bit atomics, the order is free); the
 * call zeroes stats itself, on the stream.
 *
 * Both return 0 (also for N == 0, nothing launched), -2 with nothing launched for N < 0, N x the
 * tile counts above 2^31 - 1 blocks, max_h or max_w outside [1, 8192], an even ksize or one outside
 * [3, 63], num_boxes < 0, packed_bytes < 0 and, for N > 0, a null pointer (boxes may be null when
 * num_boxes == 0) or an `out` whose packed_bytes overlap those of `packed` (the blur reads halos of
 * the original frame while other blocks write: the buffers must be disjoint); otherwise the
 * hipError_t of the launch.  Every thread of a tile walks all of its frame's boxes (twice where the
 * tile meets one), the copy tiles included: the cost per tile is linear in the boxes per frame, meant
 * for a few boxes per frame, not for dense box files.  With num_boxes == 0 the launch reserves no LDS. */
#define SM_BOX_TILE_H 32
#define SM_BOX_TILE_W 64
int sm_frames_box_blur(const uint8_t* packed, const int64_t* desc, int64_t packed_bytes, int N, int max_h, int max_w,
                       const int32_t* boxes, const int32_t* box_start, int64_t num_boxes, const float* weights,
                       int ksize, uint8_t* out, hipStream_t st);
int sm_box_region_stats(const uint8_t* a, const uint8_t* b, const int64_t* desc, int64_t packed_bytes, int N, int max_h,
                        int max_w, const int32_t* boxes, const int32_t* box_start, int64_t num_boxes, int64_t* stats,
                        hipStream_t st);

/* ---- box calibration (bench.py; csrc/calib.hip): `blocks` workgroups of 4 waves, each wave
 * `iters` x 8 v_mfma_f32_32x32x16_bf16 (shape 32) or the same FLOPs as 16
 * v_mfma_f32_16x16x32_bf16 (shape 16) on random register operands.  stamps [blocks][2] int64:
 * wave 0's s_memtime / s_memrealtime deltas (clock = d_mem / d_real x 100 MHz); sink
 * [blocks * 256] fp32 receives the accumulators.  Returns 0 or -2 (unknown shape). */
int sm_calibrate_mfma(int shape, int iters, int blocks, int64_t* stamps, float* sink, hipStream_t st);

/* ---- weighted k-nearest-neighbour evaluation of frozen features (Wu et al. 2018; csrc/knn.hip;
 * no counterpart in the reference).  All fp32, rows contiguous, every pointer 4-byte aligned
 * (else -2); no atomics, no host sync.
 *
 * sm_row_rnorm: x [N][D] -> rn [N], rn_i = ss_i > 0 ? 1.0f / sqrtf(ss_i) : 0 (a zero row has
 * similarity 0 to everything, not NaN).  ss_i: 64 partial sums p_l = sum of x_id^2 over d = l,
 * l + 64, ... ascending, one fmaf each, then five pairwise rounds p_l += p_(l xor o), o = 32, 16,
 * 8, 4, 2, 1.
 *
 * sm_knn_topk: queries q [Nq][D], bank b [Nb][D] -> idx int32 [Nq][k], sim [Nq][k]: row i holds
 * the first k bank rows under the total order below, with their similarities.
 *   similarity  dot_ij = the fmaf chain acc = fmaf(q_id, b_jd, acc) from acc = +0 over d = 0, 1,
 *               ..., D - 1 and on through zero products up to the next multiple of 32 (the
 *               single-accumulator K loop of v_mfma_f32_32x32x2_f32): one order per pair, whatever
 *               the tile, the partition or the load form.  rq [Nq] and rb [Nb] both given:
 *               sim_ij = fl(fl(dot_ij * rq_i) * rb_j) (cosine, with sm_row_rnorm's vectors); both
 *               null: sim_ij = dot_ij; exactly one null: -2.
 *   order       larger sim first; equal sims (-0 == +0) by lower bank index; NaN after every
 *               number, NaNs among themselves by index (the rule of sm_topk_frames and
 *               sm_logits_metrics).  -inf is an ordinary value.
 *   leave-one-out  self_offset >= 0 removes bank row i + self_offset from query i's candidates.
 *   padding     with fewer than k candidates the remaining slots are idx = -1, sim = -inf.
 *   splits      the bank is searched in `splits` partitions of ceil(Nb / splits) consecutive rows
 *               by different blocks (0 = chosen from Nq and Nb; at most 1024), the partial lists
 *               go to the workspace and a second launch merges them.  The order is total and
 *               every sim has one summation order: the outputs are the same bits for every splits.
 * 1 <= k <= 64, D >= 1, 1 <= Nq, Nb <= 2^31 - 256, else -2.  16-byte loads when D % 4 == 0 and
 * q and b are 16-byte aligned, scalar loads otherwise (same bits).  Workspace
 * sm_knn_topk_workspace_bytes(Nq, Nb, k, splits) (0 when one partition is searched), 16-byte
 * aligned (else -4).
 *
 * sm_knn_vote: idx, sim [Nq][k], labels int64 [Nb], ks a HOST array of nk <= SM_KNN_MAX_KS
 * strictly ascending values in [1, k] (else -2) -> scores [nk][Nq][C],
 *   scores[s][i][c] = sum over r < ks[s] with labels[idx_ir] == c of expf(sim_ir * inv_temperature),
 * added in rank order r ascending in fp32 (the table of ks[s] is a prefix of that of ks[s + 1]).
 * A slot with idx outside [0, Nb), a label outside [0, C) or a NaN sim adds nothing.  C <=
 * SM_LOGITS_MAX_CLASSES.  [nk * Nq][C] is the [S * N][C] layout sm_logits_metrics takes with S = nk. */
#define SM_KNN_MAX_KS 8
int sm_row_rnorm(const float* x, int64_t N, int D, float* rn, hipStream_t st);
int64_t sm_knn_topk_workspace_bytes(int64_t Nq, int64_t Nb, int k, int splits);
int sm_knn_topk(const float* q, int64_t Nq, const float* b, int64_t Nb, int D, const float* rq, const float* rb, int k,
                int64_t self_offset, int splits, int32_t* idx, float* sim, void* ws, int64_t ws_bytes, hipStream_t st);
int sm_knn_vote(const int32_t* idx, const float* sim, int64_t Nq, int k, const int64_t* labels, int64_t Nb, int C,
                float inv_temperature, const int32_t* ks, int nk, float* scores, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif /* SM_API_H */

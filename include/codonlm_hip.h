/*
 * codonlm_hip.h -- C-ABI of the MI355X-native codon-LM hot path (libcodonlm_hip.so).
 *
 * The reference (AvishaiBarnoy/genomics-lm) is pure PyTorch: its "boundary" is the
 * nn.Module API of src/codonlm/model_tiny_gpt.py and the op calls inside it.  Every
 * entry point below replaces one such call site (cited per function), with plain
 * pointers + sizes, no torch types.  All functions are stream-ordered on the
 * caller's hipStream_t (passed as void*), never allocate, never synchronise, and
 * return CG_OK (0) or a negative cg_status.  Buffers are caller-owned device memory.
 *
 * dtype codes: CG_F32 = fp32 storage/compute (parity mode), CG_BF16 = bf16 storage
 * with fp32 accumulation (throughput mode), CG_BF16X2 = split bf16 (a value v stored as
 * hi = bf16(v) and lo = bf16(v - hi) in the two halves of a row: [hi(ldd/2) | lo(ldd/2)]),
 * accepted where noted (gradient operands whose later sums cancel).
 */
#ifndef CODONLM_HIP_H
#define CODONLM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CG_F32 = 0, CG_BF16 = 1, CG_BF16X2 = 2 };
enum { CG_OK = 0, CG_EINVAL = -1, CG_EUNSUPPORTED = -2, CG_ELAUNCH = -3 };

/* GEMM epilogue flags (bit set) */
enum {
  CG_EPI_BIAS = 1,       /* + bias[n] (fp32)                                           */
  CG_EPI_GELU = 2,       /* out = gelu(v); aux_out (dtype of C) receives v (pre-act)   */
  CG_EPI_DGELU = 4,      /* out = v * gelu'(aux[m,n]) (aux in dtype of C)              */
  CG_EPI_RESID = 8,      /* out = resid[m,n] + v   (resid fp32, may alias C)           */
  CG_EPI_DROPOUT = 16,   /* v = v * keep(seed, m, n) / (1-p) before RESID              */
  CG_EPI_ACCUM = 32,     /* out (fp32) += v                                            */
  CG_EPI_COLSUM = 64,    /* also column sums of the final values into `workspace` as    */
                         /* [ceil(M/64)][N] fp32 partials (reduce: cg_colsum_reduce) --  */
                         /* a fused bias gradient; needs split_k == 1                     */
  /* SwiGLU (model_tiny_gpt.py:47-57), bf16 persistent tile only (else CG_EUNSUPPORTED): */
  CG_EPI_SWIGLU = 128,   /* B = [w_gate; w_up] (2N rows): aux_out [M][2N] receives the  */
                         /* pre-activations g|u, C [M][N] = silu(g) * u (0 for n >= n_valid) */
  CG_EPI_DSWIGLU = 256,  /* v = dL/ds; aux = g|u [M][2N]: C [M][2N] = d(g|u)             */
                         /* (0 for n >= n_valid)                                         */
  CG_EPI_GELU_DERIV = 512, /* modifies GELU / DGELU: the forward's aux_out receives gelu'(v) */
                         /* instead of v, and the backward's aux holds gelu' (out = v*aux): */
                         /* the derivative is formed once, from the unrounded pre-activation */
  CG_EPI_ROPE = 1024     /* (with or without BIAS) rotate-half RoPE of the q / k heads after */
                         /* the bias (model_tiny_gpt.py:91-93): columns [0, rope_heads*rope_hd) */
                         /* of row m rotated at position m % rope_T by the rope_cos / rope_sin */
                         /* [>= rope_T][rope_hd/2] tables (16-B aligned); bf16 in / out, the */
                         /* loader-wave persistent tile only (else CG_EUNSUPPORTED); rope_hd */
                         /* % 16 == 0 and N % 16 == 0                                   */
};

/*
 * C[m,n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )
 *   A(m,k) = a_kcontig ? A[m*lda + k] : A[k*lda + m]
 *   B(n,k) = b_kcontig ? B[n*ldb + k] : B[k*ldb + n]
 * Replaces nn.Linear / matmul call sites of model_tiny_gpt.py:85-93,132,143-148,50-57,327
 * and their autograd (dX = dY W, dW = dY^T X).  Inputs are `in_dtype`; C is c_dtype.
 * Contiguous extents must be multiples of 8 and leading dims multiples of 8 elements.
 * split_k > 1 needs `workspace` of split_k*M*N floats (dW GEMMs); CG_EPI_COLSUM needs
 * ceil(M/64)*N floats.  ws_bytes is the workspace's size: a short one is CG_EINVAL.
 */
typedef struct {
  int in_dtype, c_dtype;
  int M, N, K;
  const void* A; long long lda; int a_kcontig;
  const void* B; long long ldb; int b_kcontig;
  void* C; long long ldc;
  int epilogue;
  float alpha;
  const float* bias;
  const float* resid; long long ldr;
  const void* aux; void* aux_out; long long ld_aux;
  uint32_t drop_seed; float drop_p;
  int split_k; float* workspace;
  int n_valid; /* SWIGLU / DSWIGLU: columns < n_valid are live (0 = all N) */
  size_t ws_bytes; /* bytes at `workspace` */
  /* CG_EPI_ROPE (ABI 0.3): tables and geometry */
  const float* rope_cos; const float* rope_sin;
  int rope_T, rope_hd, rope_heads;
  /* ABI 0.4: kernel choice per call (the library holds no mutable process-wide settings).
   * tile: CG_TILE_AUTO (0, what the engine uses) or a forced bf16 kernel for tests / A/B runs
   * (CG_EUNSUPPORTED where it cannot run the product); max_wg: cap on the persistent grid
   * (0 = one workgroup per CU; N > 0 = at most N workgroups, each walking more tiles). */
  int tile, max_wg;
} cg_gemm_desc;
enum {
  CG_TILE_AUTO = 0,    /* persistent 256x128 (loader-wave variant where measured faster), else    */
                       /* 256x128 LDS-DMA tile for large K-contiguous products, else 128x128      */
  CG_TILE_VEC = 1,     /* 128x128 register-staged tile                                           */
  CG_TILE_WIDE = 2,    /* 256x128 LDS-DMA tile, one tile per workgroup                           */
  CG_TILE_PERS = 3,    /* persistent 256x128, 8 waves issuing their own LDS-DMA (gemm_pers.h)    */
  CG_TILE_PERS_LW = 4  /* persistent 256x128 with 4 dedicated loader waves (gemm_lw.h)           */
};
int cg_gemm(const cg_gemm_desc* d, void* stream);
/* the CU count the persistent launches (and the dW planner) spread over */
int cg_pers_cus(void);

/* Grouped weight-gradient GEMM: for every product p of the group
 *   C_p[n][k] (+)= alpha_p * sum_{m < K} A_p[m*lda_p + n] * B_p[m*ldb_p + k]
 * (dW = dY^T X of the nn.Linear call sites, A = dY and B = X both token-major bf16, C fp32).
 * Each output tile is reduced over all K rows inside one workgroup (no split-K partials);
 * the tiles of all products form one persistent launch (tile_m codes: 128 = 128x128 (0 = this),
 * 129 = the same with a 5-stage ring, 256 = 256x128, 512 = 256x256 on a ring of five 32-token
 * stages).  Any K >= 1 (a ragged last 64-row k-step is zero-filled);
 * N_out, K_out, lda, ldb % 8 == 0; ldc % 4. */
#define CG_DW_MAX 32
typedef struct {
  const void* A; long long lda;
  const void* B; long long ldb;
  float* C; long long ldc;
  int N_out, K_out;
  float alpha; int accumulate;
  float* col_sum;  /* ABI 0.5, optional: [N_out] fp32 (+)= alpha * sum_m A_p[m][n] (the bias gradient */
                   /* of the nn.Linear whose output gradient A_p is), from the A fragments the tiles  */
                   /* already stream; NULL = none; needs ksplit <= 1 (else CG_EUNSUPPORTED)           */
} cg_dw_product;
typedef struct {
  int n, K, tile_m;
  cg_dw_product p[CG_DW_MAX];
  /* ABI 0.3: ksplit > 1 (<= 8) splits every tile's token range over ksplit workgroups (more work
   * items where a group's tiles do not fill the CUs); slices 1.. write fp32 slabs into workspace
   * (ws_bytes >= cg_gemm_dw_grouped_workspace(grp), 16-B aligned, else CG_EINVAL) and one
   * reduction launch adds them into C in slice order -- deterministic.  0 / 1 = no split. */
  int ksplit;
  float* workspace; size_t ws_bytes;
  int max_wg; /* ABI 0.4: grid cap (0 = one workgroup per CU) */
} cg_dw_group;
int cg_gemm_dw_grouped(const cg_dw_group* grp, void* stream);
size_t cg_gemm_dw_grouped_workspace(const cg_dw_group* grp);
/* tiles one product contributes at tile_m */
int cg_gemm_dw_tiles(int tile_m, int N_out, int K_out);

/* LayerNorm (nn.LayerNorm, biased var, eps) -- model_tiny_gpt.py:137,139,216 */
int cg_layernorm_fwd(int out_dtype, const float* x, long long ldx, const float* gamma,
                     const float* beta, void* y, long long ldy, float* mean, float* rstd,
                     int rows, int cols, float eps, void* stream);
/* ABI 0.5: cg_layernorm_fwd and cg_attn_drop_mask(B, T, H, drop_seed, drop_p, mask) in one launch
 * (the LayerNorm of a block's input is HBM-bound, the keep words of the same block's attention
 * dropout VALU-bound: their workgroups alternate in one grid and run side by side).  Results are
 * those of the two calls, bit for bit; drop_p in (0, 1) and mask non-NULL (else CG_EINVAL). */
int cg_layernorm_fwd_mask(int out_dtype, const float* x, long long ldx, const float* gamma,
                          const float* beta, void* y, long long ldy, float* mean, float* rstd,
                          int rows, int cols, float eps, int B, int T, int H, uint32_t drop_seed,
                          float drop_p, void* mask, void* stream);
/* dx = LN backward(dy) [+ g_in]; writes g_out (fp32) and optionally g_out_t (out_dtype,
 * optionally multiplied by a dropout keep mask (seed,p) for the consumer branch);
 * per-block column partials for dgamma/dbeta go to `partials` [nblk][2*cols]
 * (nblk = cg_layernorm_bwd_blocks(rows)), reduced into dgamma/dbeta (accumulate flag).
 * dcolsum (optional, needs g_out_t): column sums of g_out_t before rounding = the bias
 * gradient of the Linear that produced the branch g_out_t feeds (partials then [nblk][3*cols]).
 * partials_bytes: the partials buffer's size, at least cg_layernorm_bwd_workspace(rows, cols,
 * want_col = dcolsum != NULL), else CG_EINVAL.  g_in may equal g_out (in-place accumulation). */
int cg_layernorm_bwd_blocks(int rows);
size_t cg_layernorm_bwd_workspace(int rows, int cols, int want_col);
int cg_layernorm_bwd(int dy_dtype, const void* dy, long long lddy, const float* x, long long ldx,
                     const float* mean, const float* rstd, const float* gamma,
                     const float* g_in, float* g_out, int out_dtype, void* g_out_t,
                     uint32_t drop_seed, float drop_p, float* partials, size_t partials_bytes,
                     float* dgamma, float* dbeta, float* dcolsum, int accumulate, int rows, int cols,
                     float eps, void* stream);
/* the same backward without the reduction: only the partial rows are written,
 * [nblk][(2 + want_col) * cols] = dgamma | dbeta | (consumer column sums); they are reduced
 * later, batched with other layers' partials, by cg_reduce_columns (the engine defers the
 * per-layer parameter-gradient reductions of a dW group to one launch) */
int cg_layernorm_bwd_partials(int dy_dtype, const void* dy, long long lddy, const float* x,
                              long long ldx, const float* mean, const float* rstd,
                              const float* gamma, const float* g_in, float* g_out, int out_dtype,
                              void* g_out_t, uint32_t drop_seed, float drop_p, float* partials,
                              size_t partials_bytes, int want_col, int rows, int cols, void* stream);

/* batched column reductions of partial rows (parameter / bias gradients, the backward of the
 * sums autograd performs per nn.Parameter): per job, dst[c] (+)= sum_r part[r * ld + c],
 * c < cols, r < nrows, in a fixed summation order; all jobs in one launch */
typedef struct {
  const float* part;
  long long ld;
  int nrows, cols;
  float* dst;
  int accumulate;
  int first_block; /* filled by cg_reduce_columns */
} cg_reduce_job;
#define CG_REDUCE_MAX 48
typedef struct {
  int n;
  cg_reduce_job j[CG_REDUCE_MAX];
} cg_reduce_batch;
int cg_reduce_columns(const cg_reduce_batch* batch, void* stream);

/* token + position embedding (+dropout) -- model_tiny_gpt.py:305-312 */
int cg_embed_fwd(const int64_t* idx, const float* tok_emb, const float* pos_emb, float* x,
                 int B, int T, int d, uint32_t drop_seed, float drop_p, void* stream);
/* scatter-add backward into tok_emb grad (V rows) and pos grad; with dtok, ws of ws_bytes >=
 * cg_embed_bwd_workspace(B,T,V,d) bytes (else CG_EINVAL) */
size_t cg_embed_bwd_workspace(int B, int T, int V, int d);
int cg_embed_bwd(const int64_t* idx, const float* g, float* dtok, float* dpos, int B, int T,
                 int V, int d, uint32_t drop_seed, float drop_p, int accumulate, void* ws,
                 size_t ws_bytes, void* stream);

/* segment starts from SEP ids: segstart[b,t] = last p<=t with idx[b,p]==sep (else 0);
 * build_attention_mask's cumsum(idx==sep) equality, model_tiny_gpt.py:289-294 */
int cg_segment_starts(const int64_t* idx, int32_t* segstart, int B, int T, int sep_id,
                      void* stream);

/* RoPE (half-split rotate_half) applied in place to the q and k column blocks of the
 * packed qkv rows -- model_tiny_gpt.py:9-45,98-100.  cos_tab/sin_tab: fp32 [T][hd/2]
 * built on the host exactly like RotaryEmbedding._set_cos_sin_cache.  inverse=1
 * applies R^T (backward of the rotation). */
int cg_rope_tab(int dtype, void* qkv, long long ldqkv, int B, int T, int H, int KV, int hd,
                const float* cos_tab, const float* sin_tab, int inverse, void* stream);

/* Fused causal + SEP-segment (+window) attention with GQA and attention-prob
 * dropout, flash-style (no T x T materialisation) -- model_tiny_gpt.py:102-131.
 * qkv rows: [q(H*hd) | k(KV*hd) | v(KV*hd)] with leading dim ldqkv; y: [B*T, H*hd];
 * lse: [B*H*T] fp32 (natural-log logsumexp of the scaled scores). window<=0: none. */
int cg_attn_fwd(int dtype, const void* qkv, long long ldqkv, const int32_t* segstart,
                void* y, long long ldy, float* lse, int B, int T, int H, int KV, int hd,
                int window, uint32_t drop_seed, float drop_p, const void* drop_mask, void* stream);
/* Attention-dropout keep bits (the same keep(seed, (b*H+h)*T + q, key) as the in-kernel hash),
 * precomputed once per (layer, step) so the bf16 MFMA kernels test one bit per (query, key):
 * a tile-major bit array ([b*H][key tile][query][2 words]) over the causal lower triangle, in a buffer of
 * cg_attn_drop_mask_bytes(B, T, H) bytes.  drop_mask (fwd / bwd): such a buffer made with the
 * same seed and p, or NULL to hash in the kernels (identical keep decisions). */
size_t cg_attn_drop_mask_bytes(int B, int T, int H);
int cg_attn_drop_mask(int B, int T, int H, uint32_t drop_seed, float drop_p, void* mask, void* stream);
/* cg_attn_fwd with dropout (0 < drop_p < 1) whose forward also writes the keep bits into mask_out
 * (a cg_attn_drop_mask_bytes buffer) for the backward: the bf16 MFMA forward hashes the keep
 * decisions itself and stores, for every (query, key) pair a query can see, the bits
 * cg_attn_drop_mask would store (bits of pairs no query sees are left as they are); other paths
 * run cg_attn_drop_mask and then cg_attn_fwd.  Replaces the drop_mask + fwd pair of
 * model_tiny_gpt.py:104-114 (SDPA dropout_p) in the training forward. */
int cg_attn_fwd_keep(int dtype, const void* qkv, long long ldqkv, const int32_t* segstart, void* y,
                     long long ldy, float* lse, int B, int T, int H, int KV, int hd, int window,
                     uint32_t drop_seed, float drop_p, void* mask_out, void* stream);
/* Attention probabilities materialised (the manual path's `last_attn`, model_tiny_gpt.py:117-128):
 * out fp32 [B][H][T][T] = exp(S/sqrt(hd) - lse) on visible (query, key), 0 elsewhere, from the
 * forward's qkv rows (post-RoPE) and lse.  Inspection path. */
int cg_attn_probs(int dtype, const void* qkv, long long ldqkv, const int32_t* segstart, const float* lse,
                  float* out, int B, int T, int H, int KV, int hd, int window, void* stream);
/* backward: writes dqkv (dtype) for q,k,v column blocks.  ws: ws_bytes >= cg_attn_bwd_workspace()
 * bytes (else CG_EINVAL; 2 B H T + 4096 B H ceil(T/64) floats: the per-query rows and the fused pass's
 * dQ accumulator).
 * bias_part (optional, bf16 MFMA path only -- CG_EUNSUPPORTED otherwise): fp32 column sums of
 * dqkv (before bf16 rounding) per (batch, 128-row tile), rows b*ceil(T/128) + tile, leading dim
 * ld_part >= (H + 2 KV) hd; reduced by cg_colsum_reduce into the q/k/v bias gradients. */
size_t cg_attn_bwd_workspace(int B, int T, int H);
int cg_attn_bwd(int dtype, const void* qkv, long long ldqkv, const int32_t* segstart,
                const void* y, long long ldy, const void* dy, long long lddy, const float* lse,
                void* dqkv, long long lddqkv, int B, int T, int H, int KV, int hd, int window,
                uint32_t drop_seed, float drop_p, const void* drop_mask, float* bias_part,
                long long ld_part, void* ws, size_t ws_bytes, void* stream);
/* cg_attn_bwd for RoPE models (ABI 0.3): qkv holds the ROTATED q / k (model_tiny_gpt.py:91-93
 * applies RotaryEmbedding after the projection), and the dQ / dK outputs -- and bias_part -- are
 * rotated back to the gradients w.r.t. the un-rotated projections in the kernels' registers
 * (the inverse rotation at each row's position), replacing a separate inverse-rotation pass.
 * rope_cos / rope_sin: 16-B aligned fp32 [>= T][hd/2] tables as cg_rope_tab takes; both NULL =
 * cg_attn_bwd.  Tables with a non-MFMA configuration (fp32, hd not 32/48/64): CG_EUNSUPPORTED. */
int cg_attn_bwd_rope(int dtype, const void* qkv, long long ldqkv, const int32_t* segstart,
                     const void* y, long long ldy, const void* dy, long long lddy, const float* lse,
                     void* dqkv, long long lddqkv, int B, int T, int H, int KV, int hd, int window,
                     uint32_t drop_seed, float drop_p, const void* drop_mask, float* bias_part,
                     long long ld_part, const float* rope_cos, const float* rope_sin, void* ws,
                     size_t ws_bytes, void* stream);
/* ABI 0.5: cg_attn_bwd_rope with the bf16 MFMA backward's algorithm chosen per call.
 *   CG_ATTN_BWD_AUTO  (0): the split pass (measured faster in the step at every benchmarked geometry,
 *                          profiles/round6/attn_bwd_fused_ab.txt)
 *   CG_ATTN_BWD_SPLIT (1): two kernels -- dQ (S, dP, dQ per query tile), then dK / dV (S, dP, dV,
 *                          dK per key tile): seven MFMA products per tile
 *   CG_ATTN_BWD_FUSED (2): one pass per (batch, kv head) -- S, dP, dV, dK and dQ, five products per
 *                          tile, dQ summed over the key blocks in an fp32 part of ws that only that
 *                          workgroup writes (no atomics: bitwise reproducible) -- between a row-
 *                          statistics pre-pass and a pass that writes the bf16 dQ columns
 * Both replace the autograd of model_tiny_gpt.py:102-131 with the same results up to fp32
 * summation order.  FUSED needs the bf16 MFMA configuration and, with dropout, drop_mask
 * (CG_EUNSUPPORTED otherwise); AUTO and SPLIT run every configuration. */
enum { CG_ATTN_BWD_AUTO = 0, CG_ATTN_BWD_SPLIT = 1, CG_ATTN_BWD_FUSED = 2 };
int cg_attn_bwd_algo(int algo, int dtype, const void* qkv, long long ldqkv, const int32_t* segstart,
                     const void* y, long long ldy, const void* dy, long long lddy, const float* lse,
                     void* dqkv, long long lddqkv, int B, int T, int H, int KV, int hd, int window,
                     uint32_t drop_seed, float drop_p, const void* drop_mask, float* bias_part,
                     long long ld_part, const float* rope_cos, const float* rope_sin, void* ws,
                     size_t ws_bytes, void* stream);

/* Label-smoothed, class-weighted, ignore_index cross-entropy fwd+bwd over logits rows
 * (F.cross_entropy at model_tiny_gpt.py:343-349).  logits fp32 [rows][ldl], V used
 * columns; writes loss (1 float, mean per the reference weighting), dlogits (d_dtype
 * CG_F32 / CG_BF16 / CG_BF16X2, pad columns [V, ldd) -- per half for CG_BF16X2 -- zeroed)
 * scaled by `grad_scale`.  ws: ws_bytes >= cg_ce_workspace(rows) bytes (else CG_EINVAL) */
size_t cg_ce_workspace(int rows);
int cg_cross_entropy(const float* logits, long long ldl, const int64_t* targets, int rows,
                     int V, float eps, const float* class_w, int ignore_index,
                     float grad_scale, int d_dtype, void* dlogits, long long ldd,
                     float* loss, void* ws, size_t ws_bytes, void* stream);

/* SwiGLU: s = silu(gu[:, :H]) * gu[:, Hp:Hp+H] (model_tiny_gpt.py:57) and backward */
int cg_swiglu_fwd(int dtype, const void* gu, long long ldgu, int Hp, void* s, long long lds,
                  int rows, int H, void* stream);
int cg_swiglu_bwd(int dtype, const void* gu, long long ldgu, int Hp, const void* ds,
                  long long ldds, void* dgu, long long lddgu, int rows, int H, void* stream);

/* column sums (bias gradients): out[n] (+)= sum_m X[m*ldx+n]; ws of ws_bytes >=
 * cg_colsum_workspace(rows, cols) bytes (else CG_EINVAL) */
size_t cg_colsum_workspace(int rows, int cols);
int cg_colsum(int dtype, const void* X, long long ldx, int rows, int cols, float* out,
              int accumulate, void* ws, size_t ws_bytes, void* stream);
/* the first stage alone: *nparts partial rows [*nparts][cols] fp32 into part (part_bytes >=
 * cg_colsum_workspace), for a reduction batched with others (cg_reduce_columns) */
int cg_colsum_partials(int dtype, const void* X, long long ldx, int rows, int cols, float* part,
                       size_t part_bytes, int* nparts, void* stream);

/* out[c] (+)= sum_i part[i*cols + c] over nparts partial rows (the second stage of the fused
 * bias-gradient column sums, e.g. CG_EPI_COLSUM GEMM partials) */
int cg_colsum_reduce(const float* part, int nparts, int cols, float* out, int accumulate, void* stream);

/* batched transpose of 2-byte matrices: dst[c][r] = src[r][c]; rows, cols, lds, ldd multiples
 * of 8, 16-B aligned pointers.  Used to give the backward dX products K-contiguous weight
 * operands (bf16 shadow weights transposed once per step). */
#define CG_TRANSPOSE_MAX 64
typedef struct {
  const void* src; void* dst;
  long long lds, ldd;
  int rows, cols;
} cg_transpose_item;
typedef struct {
  int n;
  cg_transpose_item items[CG_TRANSPOSE_MAX];
} cg_transpose_batch;
int cg_transpose16_batch(const cg_transpose_batch* tb, void* stream);

/* elementwise casts / utilities */
int cg_cast_f32_to_bf16(const float* src, uint16_t* dst, long long n, void* stream);
int cg_cast_bf16_to_f32(const uint16_t* src, float* dst, long long n, void* stream);
/* x[r][c] *= *scale (device float; exactly 1 is a no-op) for dtype CG_F32 / CG_BF16 / CG_BF16X2 */
int cg_scale_dev(int dtype, void* x, long long ld, int rows, int cols, const float* scale, void* stream);
/* dst[r][c] = src[r][c] (c < cols), 0 for cols <= c < dcols; dst in `dtype` (CG_BF16X2: hi in
 * columns [0, dcols), lo in [dcols, 2 dcols); ldd >= 2 dcols) */
int cg_cast_pad_2d(const float* src, long long lds, int rows, int cols, int dtype, void* dst,
                   long long ldd, int dcols, void* stream);

/* Device-resident batches (src/codonlm/data_loading.py): the token arrays live in HBM and a
 * batch is one gather launch (no per-step host->device copy of tokens).  elem_bytes: 1
 * (uint8), 2 (int16), 4 (int32) or 8 (int64) storage, widened to int64.
 * fixed windows (PackedDataset X/Y :43-129): out[b][t] = X[rows[b]][t]
 * dynamic sequences (flat X + lengths, dynamic_lm_collate_fn :380-393): x[b][t] = seq[t],
 * y[b][t] = seq[t+1] for t < len-1, PAD (0) beyond; seq = flat[starts[r] .. +lens[r]).
 * rows: device int64 sample indices; out-of-range rows give PAD rows. */
int cg_gather_windows(int elem_bytes, const void* X, long long ldx, long long nrows,
                      const int64_t* rows, int B, int T, int64_t* out, void* stream);
int cg_gather_sequences(int elem_bytes, const void* flat, const int64_t* starts,
                        const int64_t* lens, long long nseq, const int64_t* rows, int B, int Tout,
                        int64_t* x, int64_t* y, void* stream);

/* Sequence embeddings from hidden states (scripts/extract_embeddings.py _pool_state :94-114):
 * h: [B*T rows][ldh] (dtype) as cg_model_hidden returns; out fp32 [B][d].
 * mode 0 = mean over idx != pad_id, 1 = mean over ids set in content_mask (host, 8 x 32-bit
 * words = ids 0..255), 2 = the state at position (#non-PAD - 1, clamped at 0). */
enum { CG_POOL_MEAN_NONPAD = 0, CG_POOL_MEAN_CONTENT = 1, CG_POOL_EOS = 2 };
int cg_pool_hidden(int dtype, const void* h, long long ldh, const int64_t* idx, int B, int T,
                   int d, int pad_id, int mode, const uint32_t* content_mask, float* out,
                   void* stream);

/* Auxiliary objectives' label construction (src/codonlm/training/objectives.py).
 * offset targets (offset_target_mask :6-23): out[b][t] = y[b][t+k-1] where that target is
 * valid (t+k-1 < T, not PAD, no boundary id among y[b][t..t+k-2]), else 0 (= ignored by the
 * PAD-ignoring cross-entropy); *n_valid (device int, optional) += number of valid targets. */
int cg_offset_targets(const int64_t* y, int B, int T, int offset, const int* boundary_ids,
                      int n_boundary, int64_t* out, int* n_valid, void* stream);
/* termination_distance_bucket_labels (:63-91): distance to the next stop id bucketed by
 * the sorted edges (count of edges < distance); no later stop -> n_edges; PAD -> ignore. */
int cg_termination_labels(const int64_t* y, int B, int T, const int* stop_ids, int n_stop,
                          const int* edges, int n_edges, int ignore_index, int64_t* labels,
                          void* stream);

/* Fused AdamW over the flat parameter buffer (torch.optim.AdamW semantics,
 * loop.py:681-731): up to 4 contiguous segments with their own (lr, wd); grads are
 * multiplied by grad_scale (1/(n_micro*world)) first; optionally refreshes the bf16
 * shadow copy used by the bf16 GEMMs.  step is the 1-based AdamW step count. */
typedef struct { long long begin, end; float lr, wd; } cg_adamw_segment;
int cg_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
             uint16_t* shadow_bf16, const cg_adamw_segment* segs, int nseg, float beta1,
             float beta2, float eps, int step, float grad_scale, void* stream);
/* nonfinite flag: flag |= any(!isfinite(x[0..n))) (device int) */
int cg_nonfinite_flag(const float* x, long long n, int* flag, void* stream);

/* ------------------------------------------------------------------------------
 * Whole-model engine: the TinyGPT forward/backward sequence as one native call per
 * phase (replaces TinyGPT.forward + loss.backward(), model_tiny_gpt.py:297-352,
 * loop.py:1067-1233).  Parameters live in ONE flat fp32 buffer whose layout is owned
 * by the library (cg_model_param_layout); grads use the same layout.
 * ----------------------------------------------------------------------------*/
/* engine options (ABI 0.4): all zero = the defaults the engine was measured fastest with; each
 * field selects a measured alternative for tests and same-box A/B runs.  They are part of the
 * model's configuration (fixed for its lifetime), so the workspace size and the dW plan that
 * cg_model_workspace_bytes / cg_model_dw_plan report are the ones forward / backward use. */
typedef struct {
  int dw_group;           /* blocks per grouped dW launch (0 = the planner's choice)            */
  int dw_ksplit;          /* token-range split of the grouped dW tiles, 1..3 (0 = planner);     */
                          /* out of range -> CG_EINVAL                                          */
  int dw_remainder_first; /* 1: the short remainder dW group runs first from the top (0: last) */
  int head_dw_separate;   /* 1: the tied head's dW as its own split-K product in backward phase */
                          /* 0 (0: inside the first grouped dW launch)                          */
  int rope_tables;        /* 1: RoPE as separate cg_rope_tab passes (0: fused into the qkv      */
                          /* projection's epilogue and the attention backward)                  */
  int attn_mask_kernel;   /* 1: the attention dropout keep bits by cg_attn_drop_mask before     */
                          /* each block's forward (0: written by the attention forward itself); */
                          /* 2 (ABI 0.5): made in the block's LN1 launch, cg_layernorm_fwd_mask */
  int dw_plan_tokens;     /* > 0: plan the grouped dW as for steps of this many tokens (a small  */
                          /* parity step then runs a large step's plan); 0: the step's own B*T  */
  int attn_bwd_algo;      /* ABI 0.5: CG_ATTN_BWD_* for every block's attention backward (0 auto) */
  int pers_max_wg;        /* ABI 0.5: grid cap of every persistent launch (grouped dW, persistent */
                          /* fwd / dX GEMMs); 0 = one workgroup per CU.  A data-parallel run sets */
                          /* cg_pers_cus() - R to leave R CUs to the bucket all-reduce's kernels  */
} cg_model_opts;
typedef struct {
  int vocab_size, block_size, n_layer, n_head, n_kv_head, n_embd;
  int use_swiglu, use_rope, sep_id /* <0: none */, tie_embeddings;
  int termination_aux, termination_n_classes;
  int n_offsets; int offsets[8];
  float dropout, label_smoothing, ln_eps;
  int dtype; /* CG_F32 or CG_BF16 */
  cg_model_opts opts;
} cg_model_cfg;

/* parameter tensor kinds (layer = -1 for global tensors) */
enum {
  CG_P_TOK_EMB = 0, CG_P_POS_EMB, CG_P_LN1_W, CG_P_LN1_B, CG_P_Q_W, CG_P_K_W, CG_P_V_W,
  CG_P_Q_B, CG_P_K_B, CG_P_V_B, CG_P_PROJ_W, CG_P_PROJ_B, CG_P_LN2_W, CG_P_LN2_B,
  CG_P_FC1_W, CG_P_FC1_B, CG_P_FC2_W, CG_P_FC2_B, CG_P_GATE_W, CG_P_UP_W, CG_P_DOWN_W,
  CG_P_LNF_W, CG_P_LNF_B, CG_P_HEAD_W, CG_P_TERM_W, CG_P_TERM_B, CG_P_OFF1_W, CG_P_OFF1_B,
  CG_P_OFF2_W, CG_P_OFF2_B, CG_P_NKINDS
};
typedef struct {
  int kind, layer;        /* layer: block index, offset index (OFF*), or -1 */
  long long offset;       /* element offset into the flat buffer */
  int rows, cols;         /* logical (state_dict) shape; cols=0 for 1-D */
  long long ld;           /* row stride in elements (>= cols) */
} cg_param_entry;
/* returns number of entries (<= max) and the flat buffer size in *total_elems */
int cg_model_param_layout(const cg_model_cfg* cfg, cg_param_entry* out, int max,
                          long long* total_elems);
size_t cg_model_workspace_bytes(const cg_model_cfg* cfg, int B, int T);
/* the grouped weight-gradient plan of the bf16 engine for a (B, T) step on the current device:
 * blocks per grouped dW launch, the tile code of a full group and its token-range split (the plan
 * forward / backward use at that B * T; it depends on the token count) */
int cg_model_dw_plan(const cg_model_cfg* cfg, int B, int T, int* group_layers, int* tile_m, int* ksplit);

typedef struct {
  cg_model_cfg cfg;
  float* params;            /* flat fp32 master */
  const uint16_t* shadow;   /* flat bf16 copy (dtype==CG_BF16) */
  float* grads;             /* flat fp32 grads, same layout */
  const float* loss_weights;/* [V] or NULL (uniform) */
  const float* rope_cos;    /* [block_size][hd/2] (use_rope) */
  const float* rope_sin;
  void* workspace; size_t workspace_bytes;
  /* filled by cg_model_forward, consumed by cg_model_backward / cg_model_hidden */
  int B, T, training, window;
  uint32_t seed;
  const int64_t* idx;
  const int64_t* targets;
  float* logits;
  /* auxiliary heads (model_tiny_gpt.py:329-337).  cg_model_forward resets these to
   * (0, 1, NULL...); the caller sets the gradients of the aux outputs between
   * cg_model_aux_forward and cg_model_backward phase 0. */
  int aux_ready;                    /* set by cg_model_aux_forward                      */
  float head_grad_scale;            /* d(objective)/d(next-codon loss)                  */
  const float* head_grad_scale_dev; /* optional device float multiplying it (no host sync) */
  const float* d_term_logits;       /* fp32 [B*T][ld_d_term] or NULL                    */
  long long ld_d_term;
  const float* d_offset_logits[8];  /* fp32 [B*T][V] per offset head, or NULL           */
  /* set by cg_model_backward: the weight gradients of blocks are produced in groups (one
   * grouped dW launch per group of blocks, bf16 engine); after each call every parameter
   * gradient of blocks >= dw_done_layer (and of the head / ln_f after phase 0) is final --
   * the point a data-parallel caller may start that bucket's all-reduce. */
  int dw_done_layer;
  /* engine-private backward state (zero-initialise; the caller never writes it): the tied
   * head's weight gradient deferred from phase 0 into the first grouped dW launch (bf16, tied,
   * no aux heads).  Phase 0 sets it, the first dW group or phase 2 consumes it. */
  long long head_dw_off;
  float head_dw_alpha;
  int head_dw_accumulate;
  int head_dw_pending;
  /* engine-private: the parameter / bias gradient column reductions deferred to the end of the
   * current dW group (one cg_reduce_columns launch per group) */
  cg_reduce_batch reduce_pending;
  /* termination-loss additions (zero-initialise).  cg_model_term_loss sets term_fused and the two
   * pointers; between it and the backward the caller may set term_scale (host, 1 by default) and
   * term_scale_dev (an optional device float multiplying it), the way head_grad_scale /
   * head_grad_scale_dev scale the next-codon gradient.  Every forward resets all five. */
  int term_fused;
  const int64_t* term_labels;
  const float* term_class_w;
  float term_scale;
  const float* term_scale_dev;
} cg_model;

/* forward: logits (fp32 [B*T][V] contiguous; NULL => internal buffer), loss (device
 * float; targets NULL => no loss).  With targets, d(loss)/d(logits) is produced here
 * (fused CE fwd+bwd).  training enables dropout with `seed`; window<=0: no window. */
int cg_model_forward(cg_model* m, const int64_t* idx, const int64_t* targets, int B, int T,
                     int training, uint32_t seed, int window, float* logits, float* loss,
                     void* stream);
/* the same forward through ln_f and no further: no head product, no logits, no cross-entropy
 * (m->logits and m->targets are NULL afterwards).  cg_model_aux_forward, cg_model_term_loss,
 * cg_model_hidden and the backward work after it as after a forward without targets: the second
 * forward of a replay microbatch (loop.py:1113-1142), whose only loss sits on the termination head. */
int cg_model_forward_trunk(cg_model* m, const int64_t* idx, int B, int T, int training, uint32_t seed,
                           int window, void* stream);
/* termination_aux_loss (objectives.py:94-105, ignore_index -100) of the termination head on the ln_f
 * output of the last forward, without the logits: cg_term_ce_fwd with the fp32 master head weights.
 * labels device int64 [B*T], class_w fp32 [termination_n_classes] or NULL, loss a device float; both
 * arrays must stay alive until the backward.  It marks the model (term_fused) so that the backward's
 * aux step runs cg_term_ce_bwd -- the head's weight and bias gradients and dxf += -- instead of the
 * dense path over d_term_logits; setting d_term_logits as well makes the backward return CG_EINVAL.
 * CG_EINVAL: no termination head, no forward yet, NULL labels. */
int cg_model_term_loss(cg_model* m, const int64_t* labels, const float* class_w, float* loss, void* stream);
/* auxiliary heads on the ln_f output of the last forward (model_tiny_gpt.py:329-337):
 * termination logits fp32 [B*T][ld_term] = xf W_t^T + b_t (termination_aux), and per
 * offset head i: logits_i fp32 [B*T][ld_off] = head(W2 gelu(W1 xf + b1) + b2) (tied head);
 * ld_off >= V; with ld_off >= round_up(V, 16) the zero pad columns are computed too (the
 * product then takes the vector / persistent GEMM tiles).
 * The offset activations stay in the workspace for the backward.  After cg_model_term_loss
 * term_logits may be NULL: the termination logits are then not computed. */
int cg_model_aux_forward(cg_model* m, float* term_logits, long long ld_term,
                         float* const* offset_logits, long long ld_off, void* stream);
/* backward in phases so the caller can overlap per-bucket gradient all-reduce:
 *   phase 0: head (+ aux heads) + ln_f; phase 1: one block `layer` (call L-1 .. 0; block
 *   weight gradients complete per dW group, see cg_model.dw_done_layer);
 *   phase 2: embeddings.  Phase 0 scales the next-codon head gradient by head_grad_scale
 *   and adds the aux-head gradients given in d_term_logits / d_offset_logits; aux
 *   parameters without a gradient are zeroed when accumulate=0.
 * accumulate=0 overwrites grads (first microbatch of a group), 1 adds. */
int cg_model_backward(cg_model* m, int phase, int layer, int accumulate, void* stream);
/* the backward of a frozen backbone (loop.py:656-667, freeze_backbone): only the gradients of the aux
 * parameters -- the termination head from the fused path or d_term_logits, each offset head's two
 * Linears and biases from d_offset_logits (the head weight is an operand only).  No LM-head dW, no
 * d(head) product of the offset heads, no dxf product, no ln_f backward, no block weight transposes,
 * no phase 1 / 2: no element of grads outside the aux parameters' range is written.  accumulate and
 * the zeroing of unused aux parameters as in phase 0. */
int cg_model_backward_heads(cg_model* m, int accumulate, void* stream);
/* pointer to hidden state `which` (0 = embedding output, 1..L = block outputs,
 * L+1 = ln_f output) inside the workspace after a forward; dtype in *dtype_out */
const void* cg_model_hidden(const cg_model* m, int which, int* dtype_out, long long* ld);
/* attention probabilities of block `layer` of the last forward: fp32 [B][H][T][T] (cg_attn_probs) */
int cg_model_attn_probs(const cg_model* m, int layer, float* out, void* stream);

/* Incremental decoding with a KV cache (query_model.py generate / next_token :160-214 without
 * re-running the whole prefix).  The cache holds, per layer and sequence, the post-RoPE K and
 * V rows of every position: layout [L][B][Tmax][2*kv_dim] in the model dtype.  Valid while
 * the context fits block_size (the reference then slides its window and recomputes).
 *   cg_model_prefill: full eval forward of idx [B][T] (logits [B*T][V]), fills cache rows
 *     0..T-1 and segstate[b] (start of the last SEP segment; 0 without sep masking).
 *   cg_model_decode: one new token per sequence at position pos (= current length): writes
 *     its cache rows and logits [B][V].  dec_ws: cg_decode_workspace_bytes(cfg, B). */
size_t cg_kv_cache_bytes(const cg_model_cfg* cfg, int B, int Tmax);
size_t cg_decode_workspace_bytes(const cg_model_cfg* cfg, int B);
int cg_model_prefill(cg_model* m, const int64_t* idx, int B, int T, int window, void* cache, int Tmax,
                     int32_t* segstate, float* logits, void* stream);
int cg_model_decode(cg_model* m, const int64_t* tok, int B, int pos, void* cache, int Tmax,
                    int32_t* segstate, void* dec_ws, size_t dec_ws_bytes, float* logits, void* stream);
/* the decode step's attention: query rows q [B][ldq] (head h at column h*hd), cache rows of
 * one layer [B][Tmax][ldc] (K at kv_head*hd, V at KV*hd + kv_head*hd), keys
 * max(segstate[b], pos-window+1) .. pos; y [B][ldy] */
int cg_attn_decode(int dtype, const void* q, long long ldq, const void* cache, long long ldc, int Tmax,
                   int pos, const int32_t* segstate, int window, int B, int H, int KV, int hd, void* y,
                   long long ldy, void* stream);
/* segstate[b] = pos where tok[b] == sep_id (the SEP token opens its segment) */
int cg_segstate_step(const int64_t* tok, int B, int sep_id, int pos, int32_t* segstate, void* stream);

/* Ragged decoding (ABI 0.6): every sequence of the batch at its own position, read from a device
 * int32 pos[B].  A row with pos[b] < 0 or pos[b] >= Tmax is INACTIVE: it writes nothing to the
 * cache and its outputs (logits, term_logits, segstate) are left untouched.  Same cache layout.
 *   cg_model_prefill_ragged: eval forward of the right-padded prompts idx [B][T] (pad with any
 *     token but sep_id; the causal mask keeps rows < len[b] independent of the padding), len[b]
 *     in 1..T on the device.  Fills cache rows 0..len[b]-1 (one launch per layer), segstate[b]
 *     as of row len[b]-1 and last_logits [B][V] from row len[b]-1.  The aux heads of the same
 *     forward are available from cg_model_aux_forward afterwards.
 *   cg_model_decode_ragged: token tok[b] enters at row pos[b]: the layer sequence of
 *     cg_model_decode with the per-row ops below.  term_logits (fp32 [B][ld_term], optional,
 *     needs cfg.termination_aux) receives the termination head of the new row.
 *     dec_ws: cg_decode_ragged_workspace_bytes(cfg, B). */
size_t cg_decode_ragged_workspace_bytes(const cg_model_cfg* cfg, int B);
int cg_model_prefill_ragged(cg_model* m, const int64_t* idx, const int32_t* len, int B, int T, int window,
                            void* cache, int Tmax, int32_t* segstate, float* last_logits, void* stream);
int cg_model_decode_ragged(cg_model* m, const int64_t* tok, const int32_t* pos, int B, void* cache, int Tmax,
                           int32_t* segstate, void* dec_ws, size_t dec_ws_bytes, float* logits,
                           float* term_logits, long long ld_term, void* stream);
/* The decode step's attention, one workgroup per (kv head, sequence) serving all H/KV query heads
 * of the group from each K / V row; rows are read 16 bytes per lane, each wave runs an online
 * softmax over its share of the keys max(segstate[b], pos[b]-window+1) .. pos[b] and the waves
 * merge through LDS (no score buffer, any Tmax).  Same operand layout as cg_attn_decode.
 * fp32 and bf16, hd <= 64, hd a multiple of 8 (bf16) / 4 (fp32), q and cache rows 16-byte
 * aligned; anything else CG_EUNSUPPORTED. */
int cg_attn_decode_ragged(int dtype, const void* q, long long ldq, const void* cache, long long ldc, int Tmax,
                          const int32_t* pos, const int32_t* segstate, int window, int B, int H, int KV, int hd,
                          void* y, long long ldy, void* stream);
/* x[b] = tok_emb[tok[b]] (+ pos_emb[pos[b]]), fp32 [B][d] */
int cg_embed_fwd_pos(const int64_t* tok, const float* tok_emb, const float* pos_emb, const int32_t* pos, float* x,
                     int B, int d, int V, int Tmax, void* stream);
/* rotate-half RoPE of the q and k heads of row b of qkv [B][ldqkv] with table row pos[b] */
int cg_rope_pos(int dtype, void* qkv, long long ldqkv, const int32_t* pos, int B, int H, int KV, int hd,
                const float* cos_tab, const float* sin_tab, int Tmax, void* stream);
/* cache[b][pos[b]][0..n) = src[b][0..n): one layer's cache [B][Tmax][ldc], src rows lds apart */
int cg_kv_append(int dtype, const void* src, long long lds, void* cache, long long ldc, int Tmax,
                 const int32_t* pos, int B, int n, void* stream);
/* cache[b][t][0..n) = src[b*T + t][0..n) for t < len[b]: a prefill's cache fill of one layer */
int cg_kv_scatter(int dtype, const void* src, long long lds, int T, void* cache, long long ldc, int Tmax,
                  const int32_t* len, int B, int n, void* stream);
/* segstate[b] = pos[b] where tok[b] == sep_id */
int cg_segstate_step_ragged(const int64_t* tok, const int32_t* pos, int B, int sep_id, int Tmax, int32_t* segstate,
                            void* stream);
/* dst[b][0..n) = src[row][0..n), fp32.  T > 0: row = b*T + sel[b]-1 (sel = prompt lengths), and
 * seg_dst[b] = seg_src[row] (0 without seg_src) when seg_dst is given.  T == 0: row = b, only
 * where sel[b] is an active position. */
int cg_gather_rows(const float* src, long long lds, const int32_t* sel, int T, int Tmax, float* dst, long long ldd,
                   int n, const int32_t* seg_src, int32_t* seg_dst, int B, void* stream);
/* out[b][c] = xf[b] . w[c] + bias[c] (w fp32 [nc][d]) on the active rows */
int cg_row_head(int dtype, const void* xf, long long ldx, const float* w, const float* bias, const int32_t* pos,
                int Tmax, int B, int d, int nc, float* out, long long ldo, void* stream);

/* Multi-offset priors in batched generation (ABI 0.6; the reference's generate.py :130-150,
 * :203-212): the offset head k of a step reads the ln_f output of cache row ctx_len - k, so the
 * ragged decode keeps that output per row.
 * ln_f history of a ragged batch: [B][Tmax][d] in the model dtype, row t of sequence b = the
 * ln_f output of cache row t.  cg_xf_hist_bytes = B*Tmax*d*elem (0 for B <= 0). */
size_t cg_xf_hist_bytes(const cg_model_cfg* cfg, int B, int Tmax);
/* after cg_model_prefill_ragged (same m, B, T): hist[b][t] = ln_f row b*T+t for t < len[b] */
int cg_model_prefill_hist(cg_model* m, const int32_t* len, int B, int T, void* hist, int Tmax, void* stream);
/* cg_model_decode_ragged, and the new row's ln_f output appended at hist[b][pos[b]] on the
 * active rows (one cg_kv_append more).  hist NULL = exactly cg_model_decode_ragged. */
int cg_model_decode_ragged_hist(cg_model* m, const int64_t* tok, const int32_t* pos, int B, void* cache, int Tmax,
                                int32_t* segstate, void* dec_ws, size_t dec_ws_bytes, float* logits,
                                float* term_logits, long long ld_term, void* hist, void* stream);
typedef struct { int n; int head[8]; float weight[8]; } cg_offset_prior; /* head[i] indexes cfg.offsets */
size_t cg_offset_prior_workspace(const cg_model_cfg* cfg, int B);
/* For every active row (0 <= pos[b] < Tmax; pos[b] = the last cached row, so ctx_len = pos[b]+1),
 * for i = 0..n-1 in this order: k = cfg.offsets[head[i]], src = pos[b] + 1 - k; if weight[i] != 0
 * and src >= 0:  logits[b][0..V) += weight[i] * head(W2_k gelu(W1_k hist[b][src] + b1_k) + b2_k).
 * Inactive rows, rows no head applies to and columns >= V are not touched.  `head` is the decode
 * step's linear (tied or not, no bias).  Three launches whatever n is (all W1 products, all W2
 * products, the head products with the weighted sum); one owner per logits element, no atomics,
 * every dot product in a fixed order that does not depend on B: a row's result is bitwise the
 * same alone and in any batch.  fp32: exact FMA chains; bf16: the operand rounding of
 * cg_model_aux_forward (shadow weights, bf16 activations, fp32 accumulation and logits).
 * CG_EINVAL: a NULL m / p / hist / pos / logits / ws, B <= 0, n outside 0..8, a head[i] outside
 * [0, cfg.n_offsets) or with an offset < 1, ldl < V, Tmax outside 1..block_size, ws_bytes below
 * cg_offset_prior_workspace(cfg, B), bf16 without the shadow weights.  n == 0: CG_OK, no launch.
 * CG_EUNSUPPORTED: n_embd above 4864 (a workgroup keeps its 8 x n_embd fp32 weight slice in LDS). */
int cg_offset_prior_add(cg_model* m, const cg_offset_prior* p, const void* hist, int Tmax, const int32_t* pos,
                        int B, float* logits, long long ldl, void* ws, size_t ws_bytes, void* stream);

/* The fused sampler and stop-rule step of batched generation (ABI 0.6; the rules of the
 * reference's generate.py :51-59, :111-127, :193-260): one launch per generated token, one
 * workgroup per sequence, V <= 1024 (else CG_EUNSUPPORTED).  tok_class[v] is a bit set of
 * CG_TOK_*; a stop codon is CG_TOK_CODON | CG_TOK_STOP.  For each sequence not yet CG_GEN_DONE:
 *  1. termination bias, only with term_logits, stop_bias > 0 and
 *     n_codons >= max(0, target_codons - bias_window): cls = argmax(term_logits[b][:n_term_classes])
 *     (lowest index on ties), last_term_class = cls; if cls <= trigger_class_max every
 *     CG_TOK_STOP token's logit gains stop_bias and bias_steps grows by one;
 *  2. tokens with allowed[v] == 0 get weight 0 (at least one token must stay allowed);
 *  3. w_v = exp((l_v - max) / max(1e-6, temperature)), max over the allowed tokens;
 *  4. topk > 0: the min(topk, V) largest weights are kept, ties to the lower token index;
 *  5. the draw: u = (h >> 8) * 2^-24 with
 *         h = fmix32(row_hash(seed, state.stream) + n_tokens * 0x9E3779B1u),
 *     fmix32 the murmur3 finaliser and row_hash(s, r) = fmix32(s ^ (r * 0x9E3779B1u)) (csrc/common.h
 *     cg_fmix32 / cg_row_hash), all in uint32 arithmetic.  The token is the first index, in
 *     ascending token order, whose inclusive cumulative weight exceeds u * total, else the last
 *     kept index with a positive weight.  Steps 1-5 are evaluated in fp64 from the fp32 logits.
 *     A sequence's draws depend on (seed, stream, n_tokens) only, not on its place in a batch;
 *  6. next_tok[b] = out_ids[b][n_tokens] = token; n_tokens++; n_codons++ for a CG_TOK_CODON token;
 *  7. stop rules, the first that fires ends the sequence:
 *     CG_TOK_STOP with stop_on_bio_stop: n_codons < target_codons sets EARLY_STOP and, unless
 *       require_terminal_stop, TERMINAL_STOP|DONE; n_codons >= target_codons sets TERMINAL_STOP|DONE;
 *     CG_TOK_EOS with stop_on_eos: EOS|DONE if n_codons >= target_codons or !require_terminal_stop;
 *     n_codons >= target_codons and !require_terminal_stop: TARGET|DONE;
 *     n_codons >= max_codons or n_tokens >= max_tokens: CAP|DONE;
 *  8. not DONE: pos = pos0 + n_tokens - 1, the cache row the next cg_model_decode_ragged writes this
 *     token to (pos0 = the prompt length); pos >= Tmax sets CONTEXT_FULL|DONE.  DONE: pos = -1;
 *  9. n_active (optional, device) = number of sequences still running after the step.
 * A DONE sequence's state, next_tok and out_ids are not touched. */
enum { CG_TOK_CODON = 1, CG_TOK_STOP = 2, CG_TOK_EOS = 4 };
enum { CG_GEN_DONE = 1, CG_GEN_TERMINAL_STOP = 2, CG_GEN_EARLY_STOP = 4, CG_GEN_EOS = 8,
       CG_GEN_TARGET = 16, CG_GEN_CAP = 32, CG_GEN_CONTEXT_FULL = 64 };
typedef struct {
  int V;
  const uint8_t* tok_class; /* device [V] */
  const uint8_t* allowed;   /* device [V] or NULL = every token */
  float temperature;
  int topk;
  int target_codons, max_codons, max_tokens; /* INT_MAX = off */
  int require_terminal_stop, stop_on_eos, stop_on_bio_stop;
  float stop_bias;
  int trigger_class_max, bias_window, n_term_classes;
  uint32_t seed;
  int Tmax;
} cg_sample_params;
typedef struct {
  int32_t pos0, pos, n_tokens, n_codons, flags, bias_steps, last_term_class; /* last_term_class -1 = none */
  uint32_t stream;
} cg_gen_state;
int cg_sample_step(const cg_sample_params* p, const float* logits, long long ldl, const float* term_logits,
                   long long ld_term, cg_gen_state* state, int64_t* next_tok, int64_t* out_ids, long long ld_out,
                   int32_t* n_active, int B, void* stream);

/* cg_sample_step with a token set per step of every sequence and the log-probability of what it
 * drew (ABI 0.6 addition; the reference's generate_cds_synonymous, generate.py :617-753, whose
 * allowed set changes with every residue).  One workgroup per sequence; thread t reads the four
 * adjacent bytes 4t .. 4t+3 of the step's set row.  For a sequence not yet CG_GEN_DONE, with
 * j = n_tokens before the draw:
 *  set choice: s = plan[b][j] when j < plan_len[b], otherwise none.  If 0 <= s < n_sets and
 *     sets[s] allows at least one token < V (one block-wide OR), sets[s] replaces p->allowed in
 *     step 2.  An empty set, or an s outside [0, n_sets), means p->allowed applies (the reference's
 *     fallback, :675-676).  Steps 1 and 3-6 are cg_sample_step's, the draw the same u from
 *     (seed, stream, n_tokens);
 *  log-probabilities, fp64 from the fp32 logits, written by one thread of the sequence's own
 *     workgroup (no floating-point atomics):
 *       logp[b][0] += l_tok - logsumexp over all V raw logits: the model's own log-probability,
 *                     no bias, no mask, no temperature;
 *       logp[b][1] += log(w_tok / total) under the distribution drawn from, after bias, mask,
 *                     temperature and top-k;
 *       tok_logp[b][j] = the fp32 rounding of the first term, when j < ld_tok_logp;
 *  stop rules: step 7 unchanged; after its last rule, if the sequence is not DONE, end_with_plan
 *     is set, plan_len[b] > 0 and n_tokens >= plan_len[b]: CG_GEN_PLAN_END|DONE.  Steps 8-9
 *     unchanged.
 * A DONE sequence's state, next_tok, out_ids, logp and tok_logp rows are not touched.
 * V > 1024: CG_EUNSUPPORTED.  A NULL plan struct, n_sets < 0, or with n_sets > 0 a NULL sets /
 * plan / plan_len, ld_sets < V or ld_plan < 0: CG_EINVAL.  n_sets == 0 is plain sampling that can
 * still report log-probabilities: sets and plan are not read, and a NULL plan_len counts as all
 * zeros.  Plan entries at or past ld_plan are never read. */
enum { CG_GEN_PLAN_END = 128 }; /* cg_gen_state.flags */
typedef struct {
  const uint8_t* sets; int n_sets; long long ld_sets; /* device [n_sets][ld_sets], ld_sets >= V; non-zero = allowed */
  const int32_t* plan; long long ld_plan;             /* device [B][ld_plan]: plan[b][j] = set for generated token j */
  const int32_t* plan_len;                            /* device [B], 0 <= plan_len[b] <= ld_plan */
  int end_with_plan;                                  /* 1: a sequence ends when its plan is used up */
  double* logp;                                       /* device [B][2], optional, += */
  float* tok_logp; long long ld_tok_logp;             /* device [B][ld_tok_logp], optional */
} cg_sample_plan;
int cg_sample_step_plan(const cg_sample_params* p, const cg_sample_plan* plan, const float* logits, long long ldl,
                        const float* term_logits, long long ld_term, cg_gen_state* state, int64_t* next_tok,
                        int64_t* out_ids, long long ld_out, int32_t* n_active, int B, void* stream);

/* Batched scoring (ABI 0.6 addition): one fused pass over fp32 logits rows [rows][ldl], of which
 * only the first V columns are read (V <= 1024, else CG_EUNSUPPORTED).  It replaces the
 * log_softmax / gather / F.cross_entropy passes of the reference's scoring scripts
 * (score_mutations.py :95-157, evaluate_test.py :86-171, benchmark_zero_shot_mutations.py :25-41).
 * All row arithmetic is fp64 from the fp32 logits; every fp32 output is the single rounding of
 * the fp64 value.  Every output pointer is optional (NULL = not wanted).
 *   Row r with logits z: y = targets[r] (when targets is given); the row is VALID when targets !=
 *   NULL, y != ignore_index and 0 <= y < V.
 *     lse[r]     = log sum_c exp z_c
 *     logp[r]    = z_y - lse on a valid row, else 0
 *     entropy[r] = lse - sum_c p_c z_c (columns with p_c == 0, i.e. z_c = -inf, add 0)
 *     argmax[r]  = the lowest index among the maxima
 *     rank[r]    = #{c : z_c > z_y} + #{c < y : z_c == z_y} on a valid row (0 = top-1), else -1
 *   Selected classes (the mutation map): sel = device int32 [n_sel], delta fp32 [rows][ld_delta]:
 *     delta[r][j] = (z_sel[j] - lse) - base_r, base_r = the row's fp64 logp (0 on an invalid row);
 *     -inf where sel[j] < 0 or sel[j] >= V.
 *   Per-sequence sums, T > 0 and rows = B * T: seq_logp[b] (fp64) = sum of logp over the valid rows
 *     of sequence b, seq_count[b] = their number.  Lane t % 64 of one wave adds row t of the
 *     sequence in order and a fixed butterfly follows; invalid rows add exactly 0: a sequence's
 *     sum is bitwise independent of its padding and of the rest of the batch.
 *   acc (device fp64 [4], += across launches): [0] sum of nll = -logp over the valid rows,
 *     [1] sum of (1 - smoothing) nll + (smoothing / V) sum_c (lse - z_c) (F.cross_entropy with
 *     label_smoothing, ignore_index, reduction="sum", no class weights), [2] the number of valid
 *     rows, [3] the number of valid rows with argmax == y.  Per-workgroup fp64 partials go to the
 *     workspace and one single-workgroup launch adds them in a fixed order (no floating-point
 *     atomics): the same inputs give the same bits.
 * workspace: 8-byte aligned, ws_bytes >= cg_score_workspace of the row count (else CG_EINVAL).
 * rows == 0 is CG_OK and touches nothing. */
typedef struct {
  const float* logits; long long ldl;
  int rows, V;
  const int64_t* targets;  /* device [rows] or NULL */
  int ignore_index;
  float smoothing;
  float* lse; float* logp; float* entropy;
  int32_t* argmax; int32_t* rank;
  const int32_t* sel; int n_sel;
  float* delta; long long ld_delta;
  int T;
  double* seq_logp; int32_t* seq_count;
  double* acc;
  void* workspace; size_t ws_bytes;
} cg_score_desc;
size_t cg_score_workspace(int rows);
int cg_score_rows(const cg_score_desc* d, void* stream);

/* Input attribution (ABI 0.6 addition): gradient x input saliency and per-target dependency maps
 * on the native engine.  Replaces the tok_emb forward hook + retain_grad() + loss.backward() of the
 * reference's scripts/analyze_saliency.py :48-81, whose only use of the backward is the gradient at
 * the embedding output: cg_model_input_grad runs the dX chain alone, from a caller-chosen seed.
 *
 * cg_attr_seed: d(objective)/d(logits) of rows of fp32 logits [rows][ldl] (V used columns), written
 * in the engine's dlogits layouts: d_dtype CG_F32 [rows][ldd], ldd >= V, or CG_BF16X2 (split hi | lo
 * halves of ldd / 2 >= V columns, as cg_cross_entropy writes them); the pad columns [V, ldd) -- of
 * each half -- are zero.  Row r has the class y[r] (device int64) and the weight w[r] (device fp32;
 * w NULL = 1):
 *   CG_ATTR_LOGPROB: d[r][c] = w (delta_{c,y} - softmax(z_r)_c), the gradient of the objective
 *     sum_r w_r log p(y_r | row r) -- a sum, not a mean, so a row's seed does not depend on the
 *     other rows;
 *   CG_ATTR_LOGIT:   d[r][c] = w delta_{c,y} (logits is not read and may be NULL).
 * A row with y < 0, y >= V or w == 0 is all zero.  The softmax is evaluated in fp64 from the fp32
 * logits and every stored value is the single rounding of the fp64 one.  One wave per row, any V.
 * rows == 0: CG_OK, nothing touched.  CG_EINVAL: NULL y / d, LOGPROB without logits, ldl < V, a
 * short ldd, another mode; CG_EUNSUPPORTED: another d_dtype. */
enum { CG_ATTR_LOGPROB = 0, CG_ATTR_LOGIT = 1 };
int cg_attr_seed(const float* logits, long long ldl, const int64_t* y, const float* w, int rows, int V,
                 int mode, int d_dtype, void* d, long long ldd, void* stream);
/* cg_attr_reduce: the per-token reductions of an input gradient g fp32 [rows][ldg] over its d
 * columns, each output optional (NULL = not wanted), fp32 [rows]:
 *   gxt[r]   = sum_k g[r][k] tok_emb[idx[r]][k]  (tok_emb fp32 [V][ld_e]; 0 where idx[r] is outside
 *              [0, V)) -- what analyze_saliency.py :79-81 computes: its hook sits on tok_emb, so the
 *              position embedding is not part of the activation;
 *   gxi[r]   = sum_k g[r][k] x0[r][k]            (x0 fp32 [rows][ldx]: the embedding output, tok + pos);
 *   gnorm[r] = sqrt(sum_k g[r][k]^2).
 * One wave per row; lane l adds elements 4 (l + 64 j) .. + 3, j ascending, as one FMA chain per
 * output and a fixed butterfly follows (16-byte loads when d % 4 == 0 and every operand's rows are
 * 16-byte aligned, element loads otherwise -- the same order either way): a row's values are bitwise
 * independent of the other rows and of the row count.  rows == 0: CG_OK, nothing touched.
 * CG_EINVAL (before any launch): NULL g / idx, gxt without tok_emb, gxi without x0, a stride < d. */
int cg_attr_reduce(const float* g, long long ldg, const int64_t* idx, const float* tok_emb, long long ld_e,
                   int V, const float* x0, long long ldx, int rows, int d, float* gxt, float* gxi,
                   float* gnorm, void* stream);
/* cg_model_input_grad: d(objective)/d(embedding output) of the last forward, which must have been
 * an eval forward (training == 0), and its per-token reductions.
 *   seed: y != NULL -- cg_attr_seed(mode, y [B*T], w [B*T] or NULL) over the forward's logits: the
 *     objective is sum_r w_r log p(y_r) (or the weighted logits).  y == NULL -- the dlogits the
 *     forward's fused cross-entropy left, i.e. the model's own mean loss with its label smoothing
 *     and class weights (the loss analyze_saliency.py :57-70 differentiates); the forward must have
 *     had targets, and no seeded call may have run since (a seeded call overwrites that buffer).
 *   outputs, all optional: gxt / gxi / gnorm fp32 [B*T] (cg_attr_reduce of the gradient with the
 *     forward's idx, the fp32 master tok_emb and hidden state 0), dx0 fp32 [B*T][ld_dx0 >= n_embd]
 *     (the gradient itself).
 * It runs the dX products, LayerNorm and attention backward kernels of cg_model_backward with the
 * same operands (window, SEP segments, GQA, RoPE), block L-1 down to 0, and none of the parameter
 * gradient work: no dW product, no bias column sum, no LayerNorm parameter reduction, no embedding
 * scatter.  The aux heads contribute nothing (the seed is on the next-codon head).  m->grads may be
 * NULL and is never written; head_dw_pending, reduce_pending and dw_done_layer are left as they
 * are; the workspace of cg_model_workspace_bytes suffices.  The forward's activations and logits
 * stay intact, so it can be called again with another seed.
 * CG_EINVAL: NULL m / a, no forward yet, a training forward, y == NULL after a forward without
 * targets, an unknown mode, dx0 with ld_dx0 < n_embd. */
typedef struct {
  const int64_t* y;  /* device [B*T] or NULL */
  const float* w;    /* device [B*T] or NULL (= 1) */
  int mode;          /* CG_ATTR_LOGPROB / CG_ATTR_LOGIT (read with y) */
  float* gxt; float* gxi; float* gnorm;
  float* dx0; long long ld_dx0;
} cg_attr_desc;
int cg_model_input_grad(cg_model* m, const cg_attr_desc* a, void* stream);

/* Motif mining (ABI 0.6 addition): sliding-window pooling of hidden states and a deterministic
 * k-means step.  Replaces the per-window Python loop of the reference's src/eval/motif_extractor.py
 * and the host sklearn.KMeans of src/eval/motif_clusterer.py (scripts/mine_motifs.py).
 * Windows: nwin = T >= window ? (T - window) / stride + 1 : 0 per sequence, window j of sequence b
 * covers positions j*stride .. j*stride + window - 1.
 *
 * cg_window_keep (motif_extractor.py:71-77): keep[b*nwin + j] = 1 when no token of the window is in
 * exclude_mask (host, 8 x 32-bit words = ids 0..255, the convention of cg_pool_hidden's
 * content_mask), else 0.  An id outside 0..255 is never excluded.  idx device int64 [B][T].
 * B == 0 or nwin == 0: CG_OK, nothing touched.  CG_EINVAL: NULL idx / exclude_mask / keep, B or T
 * negative, window < 1, stride < 1. */
int cg_window_keep(const int64_t* idx, int B, int T, int window, int stride, const uint32_t* exclude_mask,
                   int32_t* keep, void* stream);
/* cg_window_pool (motif_extractor.py:80-83): h is a hidden-state buffer as cg_model_hidden returns it
 * ([B*T rows][ldh], CG_F32 or CG_BF16).  For window (b, j) with r = dst_row[b*nwin + j] (device
 * int32): r < 0 or r >= out_rows writes nothing; otherwise out[r][c] (fp32 [out_rows][ldo]), c < d,
 * is the sum over t = j*stride .. j*stride + window - 1 of h[b*T + t][c], taken in fp32 in ascending
 * t, divided by window.  The pad columns [d, ldh) and [d, ldo) are neither read nor written.  The
 * caller makes dst_row from cg_window_keep's flags with a prefix sum, so the kept windows of many
 * forwards land back to back in one [N][d] matrix in (sequence, window start) order.
 * B == 0, d == 0 or nwin == 0: CG_OK, nothing touched.  CG_EINVAL: NULL h / dst_row / out, ldh < d,
 * ldo < d, window < 1, stride < 1, a negative size; CG_EUNSUPPORTED: another dtype. */
int cg_window_pool(int dtype, const void* h, long long ldh, int B, int T, int d, int window, int stride,
                   const int32_t* dst_row, float* out, long long ldo, long long out_rows, void* stream);
/* cg_kmeans_step: the E-step of Lloyd's algorithm and the sufficient statistics of its M-step for
 * fp32 points x [n][ldx] (d used columns) and centres [k][ldc] (KMeans.fit of motif_clusterer.py:37-48).
 *   labels[i] (required) = the nearest centre in squared Euclidean distance, ranked by
 *     |c|^2 - 2 x.c with the products on the exact-fp32 MFMA; an exact tie of that score (two
 *     identical centres among them) goes to the lowest index.
 *   dist2[i] (optional) = sum_j (x[i][j] - c[label][j])^2 formed directly in fp32 (not from the
 *     ranking score): lane l of one wave adds columns l, l + 64, ... in order, a fixed butterfly follows.
 *   sums (optional, fp64 [k][d] contiguous) and counts (long long [k], required with sums): the sum and
 *     the number of the points labelled c; a cluster without points gets 0 and a zero row.  Rows are
 *     taken in chunks of CG_KMEANS_CHUNK: a chunk is cut into 1..16 equal row ranges (a number fixed by
 *     k), a range's values of a column are added in row order into an fp32 word of shared memory that
 *     one thread alone touches, the ranges' words are added in range order (fp32: at most
 *     CG_KMEANS_CHUNK additions per partial) and the chunks' partials in chunk order in fp64.
 *   inertia (optional, device fp64) = the sum of dist2, per-workgroup fp64 partials added in a fixed
 *     order.
 * No floating-point atomics anywhere; every sum is taken in an order fixed by (n, d, k): the same
 * inputs give the same bits.  The pad columns of x and centres are never read.
 * n == 0: CG_OK, nothing touched.  CG_EUNSUPPORTED: k outside 1..256 or d outside 1..1024.
 * CG_EINVAL: a NULL desc / x / centers / labels / workspace, n < 0, ldx < d, ldc < d, sums without
 * counts, ws_bytes below cg_kmeans_workspace(n, d, k) (workspace 16-byte aligned). */
#define CG_KMEANS_CHUNK 4096
typedef struct {
  const float* x; long long ldx; long long n; int d;
  const float* centers; long long ldc; int k;
  int32_t* labels;
  float* dist2;
  double* sums;
  long long* counts;
  double* inertia;
  void* workspace; size_t ws_bytes;
} cg_kmeans_desc;
size_t cg_kmeans_workspace(long long n, int d, int k);
int cg_kmeans_step(const cg_kmeans_desc* k, void* stream);

/* Fused termination-head loss (ABI 0.6 addition): the linear head, its class-weighted cross-entropy and their
 * backward over the LABELLED rows only.  Replaces termination_head(x) (model_tiny_gpt.py:329-337)
 * followed by termination_aux_loss (src/codonlm/training/objectives.py:94-105) and their autograd
 * where the labels are sparse (a replay batch labels at most replay_window positions of a row) or
 * the logits themselves are not wanted (a frozen-backbone step).
 *   x [rows][ldx] (x_dtype CG_F32 or CG_BF16, widened exactly; the ln_f output), W fp32 [C][ldw],
 *   bias fp32 [C], labels device int64 [rows], class_w fp32 [C] or NULL (= 1).
 *   Row r is LABELLED when labels[r] != ignore_index and 0 <= labels[r] < C.  Any other label --
 *   ignore_index or out of range -- is ignored (torch would raise a device assert on the latter;
 *   callers validate their labels on the host).  A row without a label costs its label read and
 *   nothing else: x is read for labelled rows only.
 * cg_term_ce_fwd: per labelled row z = x W^T + b (fp32 fma chains: lane l of a wave takes columns
 *   4 (l + 64 i) .. + 3 in ascending i -- 16-byte loads where ldx, ldw % 4 == 0 and the bases are
 *   aligned -- and an element tail, then a fixed butterfly), lse = log sum_c exp z_c and
 *   nll = lse - z_y.  loss (device float, optional) = sum_r w_y nll / sum_r w_y; sums (device
 *   float[2], optional) = the numerator and the denominator.  Without a labelled row the loss is NaN
 *   (torch's weighted mean over nothing).  The rows' probabilities and the two sums stay in the
 *   workspace for the backward.
 * cg_term_ce_bwd (after cg_term_ce_fwd with the same x, W, bias, labels, class_w and workspace):
 *   g[r][c] = scale * (scale_dev ? *scale_dev : 1) * w_y (softmax(z_r)_c - [c == y]) / sum_r w_y on
 *   labelled rows (scale_dev: an optional device float, read in the kernel -- no host sync), and
 *     dW[c][j] (+)= sum_r g[r][c] x[r][j]   (fp32 [C][lddw], optional)
 *     db[c]    (+)= sum_r g[r][c]           (fp32 [C], optional)
 *     dx[r][j] (+)= sum_c g[r][c] W[c][j]   (fp32 [rows][lddx], optional)
 *   each with its own accumulate flag.  Without acc_dx the unlabelled rows of dx are written as zero;
 *   with it they are not touched.  Without a labelled row the backward contributes exactly zero.
 * Reproducible bit for bit: rows are taken in chunks of 64; a chunk's share of a dW / db element is
 * summed in row order by one thread (fp32), the chunks' shares in chunk order (fp64) by one thread;
 * the loss sums are fp64 from the per-row fp32 terms in a fixed order.  No floating-point atomics.
 * The pad columns of x, W, dW and dx are neither read nor written.
 * rows == 0: CG_OK, nothing touched.  CG_EUNSUPPORTED: C > 16, another x_dtype.  CG_EINVAL: NULL
 * desc / x / W / bias / labels / workspace, C < 1, d < 1, rows < 0, ldx / ldw / lddw / lddx < d,
 * ws_bytes below cg_term_ce_workspace(rows, d, C) (workspace 16-byte aligned). */
typedef struct {
  int x_dtype; const void* x; long long ldx;
  long long rows; int d, C;
  const float* W; long long ldw;
  const float* bias;
  const int64_t* labels; int ignore_index;
  const float* class_w;
  float* loss; float* sums;                 /* forward outputs */
  float scale; const float* scale_dev;      /* backward */
  float* dW; long long lddw; int acc_dW;
  float* db; int acc_db;
  float* dx; long long lddx; int acc_dx;
  void* workspace; size_t ws_bytes;
} cg_term_ce_desc;
size_t cg_term_ce_workspace(long long rows, int d, int C);
int cg_term_ce_fwd(const cg_term_ce_desc* p, void* stream);
int cg_term_ce_bwd(const cg_term_ce_desc* p, void* stream);

/* Context diagnostic (ABI 0.6 addition): segment-aware n-gram baselines and the sliced loss /
 * calibration pass of the reference's leakage-controlled revalidation scripts, each of which is a
 * Python loop per token there.  Shared conventions: x, y are device int64 [B][T] (inputs and
 * next-token targets, as the engine takes them); V <= CG_NGRAM_MAX_V = 128, else CG_EUNSUPPORTED
 * (the dense trigram table is V^3 int64); pad_id (0 <= pad_id < V, the reference's is 0) is the
 * ignored target; reset_mask is cg_window_keep's id mask (host, 8 x 32-bit words = ids 0..255): the
 * tokens after which the n-gram history restarts (<SEP>).  All row arithmetic is fp64 and an fp32
 * output is the single rounding of the fp64 value.  No floating-point atomics: per-workgroup fp64
 * partials go to the workspace and one single-workgroup launch adds them in a fixed order, so the same
 * inputs give the same bits; the integer tables use integer atomics, which are order-independent.
 * B == 0 or T == 0: CG_OK, nothing touched.  CG_EINVAL: a NULL required pointer, a negative size,
 * pad_id outside [0, V), a misaligned (8 bytes) or short workspace.
 *
 * cg_ngram_count (fit_baselines, scripts/eval_ppl_baselines.py:61-84): position (b, t) counts when
 * y != pad_id.  previous = x[b][t]; previous2 = pad_id when t == 0 or previous is a reset token,
 * else x[b][t-1].  A counted position whose y, previous or (read) previous2 lies outside [0, V)
 * adds 1 to n_bad[0] (optional) and is skipped; any other adds 1 to uni[y], bi[previous][y] and
 * tri[previous2][previous][y].  uni [V], bi [V][V], tri [V][V][V] are device int64 and += across
 * launches (the caller zeroes them).  Bigram counts are taken in a per-workgroup 32-bit LDS table and
 * its non-zero cells flushed with 64-bit global integer adds (the unigram counts are that table's
 * column sums); trigram adds go straight to global memory without a returned value.  More than
 * 2^40 positions in one launch: CG_EUNSUPPORTED.
 *
 * cg_ngram_totals (_probability, :87-90): uni_total[0], bi_total[p] and tri_total[p2][p] = the sum
 * of the row's counts over the targets 1 .. V-1 (the reference leaves column 0 out), device int64
 * [1], [V], [V][V]; overwritten. */
#define CG_NGRAM_MAX_V 128
int cg_ngram_count(const int64_t* x, const int64_t* y, int B, int T, int V, int pad_id, const uint32_t* reset_mask,
                   long long* uni, long long* bi, long long* tri, long long* n_bad, void* stream);
int cg_ngram_totals(const long long* uni, const long long* bi, const long long* tri, int V, long long* uni_total,
                    long long* bi_total, long long* tri_total, void* stream);
/* cg_ngram_nll (evaluate_baselines, scripts/eval_ppl_baselines.py:93-137, and _trigram_nll,
 * scripts/diagnose_context_learning.py:78-105): with active = V - 1,
 *   p = (count + alpha) / (total + alpha * active), nll = -log p
 * for the unigram row, the bigram row of previous, and the trigram row of (previous2, previous) when
 * its total is non-zero, else the bigram row of previous (the reference's trigram.get(...) is None
 * back-off: with pad_id = 0 column 0 is never counted, so a context exists exactly when its total is
 * non-zero).  An unseen context gives alpha / (alpha * active); the uniform model gives log(active).
 * A position counts as in cg_ngram_count; one with a token outside [0, V) is skipped.
 * Outputs, all optional:
 *   tok_tri   fp32 [B][T]: the trigram nll, 0 where not counted;
 *   row_sums  fp64 [B][4]: the row's uniform, unigram, bigram and trigram nll sums (lane t % 64 of one
 *             wave adds position t in order, a fixed butterfly follows), row_count int32 [B];
 *   acc       fp64 [5], += across launches: the four sums and the number of counted positions.
 * workspace: cg_ngram_nll_workspace(B) bytes.  alpha <= 0 (or not finite): CG_EINVAL. */
typedef struct {
  const int64_t* x; const int64_t* y;
  int B, T, V, pad_id;
  const uint32_t* reset_mask;
  double alpha;
  const long long* uni; const long long* bi; const long long* tri;
  const long long* uni_total; const long long* bi_total; const long long* tri_total;
  float* tok_tri;
  double* row_sums; int32_t* row_count;
  double* acc;
  void* workspace; size_t ws_bytes;
} cg_ngram_nll_desc;
size_t cg_ngram_nll_workspace(int B);
int cg_ngram_nll(const cg_ngram_nll_desc* d, void* stream);
/* cg_diag_rows: one pass over the fp32 logits [B*T][ldl] (the first V columns are read) of a forward
 * over x with the targets y.  It replaces the slice loop of scripts/diagnose_context_learning.py
 * :322-357 and ece_from_logits / brier_from_logits of scripts/calibration_metrics.py:35-75.
 * Position (b, t) is VALID when y != pad_id and 0 <= y < V.  Per valid position, in fp64:
 *   lse = log sum_c exp z_c, nll = lse - z_y, conf = exp(zmax - lse) = 1 / sum_c exp(z_c - zmax),
 *   correct = (the lowest-index argmax == y), brier = sum_c p_c^2 - 2 p_y + 1.
 * Segment position (the reference's counter): it runs over the valid positions of a row from 0, is
 * set to 0 at a valid position whose input is sep_id, and grows by 1 after each valid position; an
 * invalid position neither resets nor advances it, even when its input is the separator.  One
 * workgroup per row scans it, for any T.
 * slices fp64 [CG_DIAG_SLICES][2] = (sum of nll, count), += across launches, in the order of the
 * CG_DIAG_* enumerators: all; after_separator (valid and x == sep_id); row_flag set, row_flag clear
 * (row_flag device uint8 [B], NULL = clear: the chunk-continuation windows); the segment-position
 * bins 0, 1-3, 4-15, 16-63, 64+; the four target classes of tok_class (device uint8 [V] of
 * CG_DIAG_CLS_*, NULL = no class slices; a value above 3 joins none).
 * Calibration: edges device fp32 [n_bins + 1], 1 <= n_bins <= CG_DIAG_MAX_BINS; conf rounded to fp32
 * falls in bin i when conf > edges[i] && conf <= edges[i+1] (the lowest such i; none: not binned).
 * calib fp64 [n_bins][3] = (count, sum of conf, sum of correct), brier_acc fp64 [2] = (sum, count),
 * both += across launches.  edges NULL: no calibration (calib must be NULL too).
 * Optional per-token outputs [B][T]: nll fp32 (0 where invalid), segpos int32 (-1 where invalid),
 * conf fp32 (0 where invalid).  Optional per-row outputs: row_nll fp64 [B] and row_count int32 [B],
 * summed as cg_score_rows sums seq_logp (lane t % 64 of one wave adds position t in order, a fixed
 * butterfly follows; invalid positions add exactly 0).
 * workspace: cg_diag_workspace(B) bytes (needed with slices, calib or brier_acc). */
enum {
  CG_DIAG_ALL = 0, CG_DIAG_AFTER_SEP = 1, CG_DIAG_FLAG_SET = 2, CG_DIAG_FLAG_CLEAR = 3,
  CG_DIAG_POS_0 = 4, CG_DIAG_POS_1_3 = 5, CG_DIAG_POS_4_15 = 6, CG_DIAG_POS_16_63 = 7, CG_DIAG_POS_64_PLUS = 8,
  CG_DIAG_CLS_SPECIAL_SLICE = 9, CG_DIAG_CLS_START_SLICE = 10, CG_DIAG_CLS_STOP_SLICE = 11,
  CG_DIAG_CLS_ORDINARY_SLICE = 12, CG_DIAG_SLICES = 13
};
enum { CG_DIAG_CLS_SPECIAL = 0, CG_DIAG_CLS_START = 1, CG_DIAG_CLS_STOP = 2, CG_DIAG_CLS_ORDINARY = 3 };
#define CG_DIAG_MAX_BINS 32
typedef struct {
  const float* logits; long long ldl;
  const int64_t* x; const int64_t* y;
  int B, T, V, pad_id, sep_id;
  const uint8_t* row_flag;
  const uint8_t* tok_class;
  const float* edges; int n_bins;
  double* slices; double* calib; double* brier_acc;
  float* nll; int32_t* segpos; float* conf;
  double* row_nll; int32_t* row_count;
  void* workspace; size_t ws_bytes;
} cg_diag_desc;
size_t cg_diag_workspace(int B);
int cg_diag_rows(const cg_diag_desc* d, void* stream);

/* cg_attn_stats: per-head statistics of the attention probabilities P of one layer, over any number
 * of sequences, without a T x T tensor reaching memory.  It replaces the per-head reductions of
 * scripts/conference_attention.py:41-66 (_head_stats: entropy, start- and stop-column bias) and the
 * row reductions scripts/analyze_attention.py and scripts/report_top_saliency.py take from the
 * captured `attn` tensor of collect_artifacts_yaml.py, which cg_attn_probs could only serve by
 * writing B*H*T*T floats per layer.
 * qkv as cg_attn_fwd (rows [B*T], q | k | v, RoPE already applied).  Key k is visible to query q iff
 * lo(q) <= k <= q, lo = max(segstart[b,q], q - window + 1) (the forward's mask); query head h reads
 * KV head h / (H/KV); scale 1/sqrt(hd).  The op is self-normalised: it takes each row's maximum and
 * normaliser itself in fp32 (pass A over the row's key tiles) and adds p = exp(s - lse) into every
 * sum in fp32 (pass B), for bf16 inputs too; the forward's saved LSE is not read.
 * A row (b, q) is KEPT iff (idx == NULL or idx[b,q] != pad_id) and (row_keep == NULL or
 * row_keep[b,q] != 0).  The class of key k is tok_class[idx[b,k]]; a class above 3 or a token
 * outside [0, V) joins no class; tok_class without idx is CG_EINVAL.
 * Outputs, all optional: rows (0 on rows not kept), nvis (every row), received[b][h][k] = the sum
 * over the kept queries q of p[q][k], head_acc[h][s] += the fp64 sum over the kept rows of the fp32
 * row statistics, n_rows += the kept (b, q) count.  Every sum has a fixed order (per 128-query tile
 * in query order, then the tiles in ascending order): two runs give identical bits, no atomics.
 * bf16 with hd % 8 == 0 runs on v_mfma_f32_32x32x16_bf16 with the forward's K-tile DMA; fp32 and
 * other head dims on a vector kernel.  hd in 1..64 (more: CG_EUNSUPPORTED).  B == 0 or T == 0:
 * CG_OK, nothing written.  CG_EINVAL: H % KV != 0, a NULL qkv, ldqkv below (H + 2 KV) hd, a workspace
 * (always needed, 8-byte aligned) smaller than cg_attn_stats_workspace(B, T, H). */
enum { CG_AS_ENTROPY = 0,            /* -sum p ln p over the visible keys, nats            */
       CG_AS_NORM_ENTROPY = 1,       /* entropy / ln(nvis); 0 when nvis == 1                */
       CG_AS_MASS_SPECIAL = 2, CG_AS_MASS_START = 3, CG_AS_MASS_STOP = 4, CG_AS_MASS_ORDINARY = 5,
                                     /* sum of p over keys of class CG_DIAG_CLS_* (same order) */
       CG_AS_DIST_0 = 6, CG_AS_DIST_1_3 = 7, CG_AS_DIST_4_15 = 8, CG_AS_DIST_16_63 = 9, CG_AS_DIST_64_PLUS = 10,
                                     /* sum of p over keys at distance q - k in the bin      */
       CG_AS_MEAN_DIST = 11,         /* sum p (q - k)                                        */
       CG_AS_MAX_PROB = 12,          /* max p                                                */
       CG_AS_FIRST = 13,             /* p at the first visible key lo(q) (the "sink")        */
       CG_AS_NSTAT = 14 };
typedef struct {
  int dtype; const void* qkv; long long ldqkv;          /* as cg_attn_fwd: rows [B*T], q | k | v, RoPE already applied */
  const int32_t* segstart;                              /* NULL = no SEP mask */
  int B, T, H, KV, hd, window;
  const int64_t* idx; int pad_id;                       /* idx NULL = every row kept, no classes */
  const uint8_t* tok_class; int V;                      /* uint8 [V] of CG_DIAG_CLS_*; NULL = class masses are 0 */
  const uint8_t* row_keep;                              /* uint8 [B][T], NULL = all */
  float* rows;                                          /* optional fp32 [B][H][T][CG_AS_NSTAT], 0 on rows not kept */
  int32_t* nvis;                                        /* optional int32 [B][T] = q - lo(q) + 1 */
  float* received;                                      /* optional fp32 [B][H][T]: sum over kept queries q of p[q][k] */
  double* head_acc;                                     /* optional fp64 [H][CG_AS_NSTAT], += across launches */
  double* n_rows;                                       /* optional fp64 [1], += the kept (b, q) count */
  void* workspace; size_t ws_bytes;
} cg_attn_stats_desc;
size_t cg_attn_stats_workspace(int B, int T, int H);
int cg_attn_stats(const cg_attn_stats_desc* d, void* stream);
/* cg_attn_stats on block `layer` of the last forward: dtype, qkv, ldqkv, segstart, B, T, H, KV, hd,
 * window and idx come from the model (as cg_model_attn_probs takes them), every other field from d */
int cg_model_attn_stats(const cg_model* m, int layer, const cg_attn_stats_desc* d, void* stream);

/* Structural regression probes (ABI 0.6 addition): per-codon DNAshape targets from token ids and the
 * grouped augmented Gram matrix of hidden states and targets, from which every ridge fit, fold metric
 * and principal component of the probes follows on a (d + m + 1)^2 matrix.  Replaces the per-sequence
 * host copies and the N x d regression matrix of the reference's scripts/probe_structural_regression.py
 * (:88-128) and scripts/probe_structural_awareness.py.
 *
 * cg_shape_targets (probe_structural_awareness.py:8-167 get_theoretical_shape, and the per-codon
 * pooling of probe_structural_regression.py:116-121): idx device int64 [B][T]; codon_of host int32 [V],
 * V <= 256: 6 bits = three 2-bit nucleotides, the first in the high bits, A, C, G, T = 0..3; negative =
 * not a codon; an id outside 0..V-1 is not a codon.  A run is a maximal stretch of codon tokens inside
 * one row of idx, its DNA the concatenation of its codons.  Nucleotide i of a run of L nucleotides
 * sees the window dna[max(0, i-2) : min(L, i+3)] (never across a run or row boundary); each of the
 * CG_SHAPE_TARGETS values of a nucleotide is the first rule whose word occurs in the window:
 *    0 MGW      AAAA 3.5;  GGGG | CCCC 5.8;  else 4.5       7 Shift    AA | TT 0.0;  GC 0.2;  else -0.1
 *    1 Roll     GC | CG 5.0;  AA | TT 0.0;  else 2.5        8 Tilt     AA 0.0;  CG 0.5;  else -0.2
 *    2 EP       AAAA -10;  GGCC -2;  else -5                9 Buckle   GC -12;  AT 0;  else -6
 *    3 ProT     GC -11;  AT -18;  else -14                 10 Opening  AT 2.0;  GC 0.5;  else 1.0
 *    4 HelT     CG 36;  TA 32;  else 34                    11 Shear    GC 0.0;  else 0.1
 *    5 Slide    AAAA -0.8;  GC | CG 0.2;  else -0.3        12 Stagger  AA 0.1;  else -0.1
 *    6 Rise     CG 3.2;  AA 3.4;  else 3.3                 13 Stretch  CG -0.1;  else 0.0
 * y[b*T + t][k] (fp32 [B*T][ldy]) = ((v0 + v1) + v2) / 3 of the codon's three nucleotides in fp64,
 * rounded once to fp32; valid[b*T + t] = 1.  A position that holds no codon gets valid = 0 and its y
 * row is not written; columns [CG_SHAPE_TARGETS, ldy) are never written.
 * B == 0 or T == 0: CG_OK, nothing touched.  CG_EINVAL: NULL idx / y / valid / codon_of (V > 0), a
 * negative size, V > 256, a table entry above 63, ldy < CG_SHAPE_TARGETS. */
#define CG_SHAPE_TARGETS 14
int cg_shape_targets(const int64_t* idx, int B, int T, const int32_t* codon_of, int V, float* y, long long ldy,
                     int32_t* valid, void* stream);
/* cg_gram_accum: h is a hidden-state buffer as cg_model_hidden returns it ([rows][ldh], CG_F32 or
 * CG_BF16, d used columns), y fp32 [rows][ldy] with m >= 0 used columns, grp device int32 [rows].
 * Row r belongs to group grp[r] when 0 <= grp[r] < G; any other row is skipped and its h and y are
 * never read (they may hold NaN).  With z_r = (h[r][0..d), y[r][0..m), 1) and P = d + m + 1,
 *   gram[g][i][j] (fp64 [G][P][ldg]) (+)= sum over the rows r of group g of z_r[i] * z_r[j],
 * so gram[g][P-1][P-1] counts the group's rows (X^T X, X^T y, y^T y and the column sums of
 * probe_structural_regression.py:165-178 for every fold at once).  accumulate = 1 adds the call's sums
 * to what gram holds, accumulate = 0 overwrites all G * P * P entries (zeros for an empty group).
 * The inputs are widened exactly to fp64; products and sums are fp64 on v_mfma_f64_16x16x4_f64.
 * Order: the rows of a group, ascending, are cut into S slices of equal length (S fixed by rows, P
 * and G); a slice's rows are added in order, four to an MFMA step, into one partial per 64 x 64
 * block of the upper triangle, and the partials in slice order.  Element (i, j) and (j, i) are the same
 * sum, so the call's sums are symmetric bitwise, and the same calls give the same bits.  No
 * floating-point atomics.  The pad columns of h, y and gram are neither read nor written.
 * rows == 0: CG_OK; with accumulate = 1 nothing is touched, otherwise gram is zeroed.
 * CG_EINVAL: NULL gram, NULL h (d > 0) / y (m > 0) / grp / workspace with rows > 0, a negative size,
 * rows above 2^30, G < 1, ldh < d, ldy < m, ldg < P, accumulate outside 0 / 1, ws_bytes below
 * cg_gram_workspace(rows, d, m, G) or a workspace not 256-byte aligned.  CG_EUNSUPPORTED: another
 * dtype, P > 8192 or G > 4096 (cg_gram_workspace returns 0 for those and for invalid sizes). */
size_t cg_gram_workspace(long long rows, int d, int m, int G);
int cg_gram_accum(int dtype, const void* h, long long ldh, int d, const float* y, long long ldy, int m,
                  const int32_t* grp, long long rows, int G, int accumulate, double* gram, long long ldg,
                  void* workspace, size_t ws_bytes, void* stream);

/* Memorization audit (ABI 0.6 addition): an exact window-membership index over byte symbols.  It replaces
 * the Python set of n-gram tuples of the reference's scripts/eval_generation_prefix.py
 * (_build_train_ngram_set :164-206, capped at 10M tokens "to prevent RAM bloat", and
 * _training_match_coverage :472-482) and the window index of src/codonlm/leakage_audit.py
 * (matching_substring_coverage, _coverage_from_index, _matched_query_windows), which runs over nucleotide
 * windows of 30 and protein windows of 10.
 * Symbols are uint8: token ids below 256, or the ASCII bytes of a nucleotide / protein string.  A sequence
 * set is a flat device uint8 buffer (4-byte aligned) of n_sym symbols plus device int64 offsets[n_seq + 1],
 * non-decreasing, offsets[n_seq] <= n_sym <= CG_NGRAM_INDEX_MAX_SYM = 2^32 - 2; sequence s is
 * [offsets[s], offsets[s+1]).  Packed rows [R][T] are the case offsets[r] = r * T.  A window is n
 * consecutive symbols of one sequence, 1 <= n <= CG_NGRAM_INDEX_MAX_N = 32; it never crosses a sequence
 * boundary.  Offsets outside [0, n_sym] are clamped, so no call reads past a buffer it was given.
 *
 * cg_ngram_index_build inserts every window of the sequences [seq_lo, seq_hi) into table, an
 * open-addressing table uint32 [capacity]: capacity a power of two (2 .. 2^32), strictly greater than the
 * number of windows ever inserted; empty = 0xFFFFFFFF, which the caller fills the table with before the
 * first build.  A slot holds the flat start position of one occurrence of its window.  Insertion: hash the
 * n symbols (the hash is internal, a function of the symbols and n only), probe linearly with wrap-around;
 * an empty slot is claimed with a 32-bit agent-scope compare-and-swap (the slot is read first, so a heavily
 * duplicated window -- a pad run, low-complexity sequence -- does not hammer one address with atomics); at
 * an occupied slot the n symbols at the stored position are compared with the window's own: equal = a
 * duplicate, stop; different = the next slot.  Stored positions never change once written, which is all
 * the synchronisation there is.  n_unique (optional, device int64 [1], 8-byte aligned) += the number of
 * claims, reduced per workgroup into one integer atomic; several launches over disjoint sequence ranges of
 * the same sym buffer give the same set and the same n_unique as one launch.  n_dropped (optional, as
 * n_unique) += the windows that found no slot in `capacity` probes: 0 unless the caller broke the capacity
 * rule.  WHICH duplicate's position a slot holds, and in WHICH slot a window lies, is not defined (it
 * depends on the order the hardware ran the threads in); n_unique, n_dropped and every output of
 * cg_ngram_coverage are defined, exact integers, the same in every run.
 * seq_lo == seq_hi or n_sym < n: CG_OK, nothing touched.  CG_EINVAL: n < 1, a negative size, a sequence
 * range outside [0, n_seq], NULL or misaligned sym / offsets / table, a capacity that is no power of two in
 * 2 .. 2^32.  CG_EUNSUPPORTED: n > CG_NGRAM_INDEX_MAX_N, n_sym > CG_NGRAM_INDEX_MAX_SYM. */
#define CG_NGRAM_INDEX_MAX_N 32
#define CG_NGRAM_INDEX_MAX_SYM 4294967294ll
#define CG_NGRAM_MAX_QUERY 16384
typedef struct {
  const uint8_t* sym; long long n_sym;
  const int64_t* offsets; int n_seq;
  int seq_lo, seq_hi;
  int n;
  uint32_t* table; long long capacity;
  long long* n_unique;
  long long* n_dropped;
} cg_ngram_index_desc;
int cg_ngram_index_build(const cg_ngram_index_desc* d, void* stream);
/* cg_ngram_coverage: the query set (qsym [n_qsym], qoffsets [n_q + 1], as above) against a built table
 * and the sym it was built over.  For query q of length len, every start s with s + n <= len is a HIT
 * iff its window is in the table (probe until an equal window = hit, or an empty slot = miss).  Outputs,
 * each optional:
 *   hit      uint8, one per query symbol (the layout of qsym): 1 at hit starts, 0 elsewhere in the query;
 *            bytes of qsym that belong to no query are not written;
 *   n_hit    int32 [n_q]: the number of hit starts;
 *   covered  int32 [n_q]: the number of positions t with a hit start s, s <= t < s + n (the reference's
 *            coverage is covered / len, a division the caller makes).
 * A query shorter than n gives 0 / 0.  One workgroup per query: lookups into a bit mask in LDS, a barrier,
 * then cover and reduce.  max_qlen is the longest query as the caller states it: above CG_NGRAM_MAX_QUERY =
 * 16384 the call is CG_EUNSUPPORTED; a query longer than max_qlen is read as its first max_qlen symbols.
 * n_q == 0: CG_OK, nothing touched.  Otherwise the errors of cg_ngram_index_build. */
typedef struct {
  const uint8_t* sym; long long n_sym;
  int n;
  const uint32_t* table; long long capacity;
  const uint8_t* qsym; long long n_qsym;
  const int64_t* qoffsets; int n_q;
  int max_qlen;
  uint8_t* hit; int32_t* n_hit; int32_t* covered;
} cg_ngram_coverage_desc;
int cg_ngram_coverage(const cg_ngram_coverage_desc* d, void* stream);

/* Live probe of one kernel class during a real run: HIP events are recorded on the
 * launching stream around each launch of the selected kernel together with its
 * algorithmic work (FLOPs for MFMA kernels).  kind 0 disables.  cg_probe_read
 * synchronises on the recorded events and returns (work, total device ms, launches). */
enum {
  CG_PROBE_NONE = 0,
  CG_PROBE_GEMM_DW = 1,      /* bf16 dW GEMM main kernel (A,B MN-contiguous)       */
  CG_PROBE_GEMM_FWD = 2,     /* bf16 forward GEMM main kernel (A,B K-contiguous)   */
  CG_PROBE_GEMM_DX = 3,      /* bf16 dX GEMM main kernel                           */
  CG_PROBE_ATTN_FWD = 4,     /* attn_fwd_mfma                                      */
  CG_PROBE_ATTN_DQ = 5,      /* attn_bwd_dq_mfma                                   */
  CG_PROBE_ATTN_DKDV = 6,    /* attn_bwd_dkdv_mfma                                 */
  CG_PROBE_GEMM_DW_GROUPED = 7, /* grouped weight-gradient GEMM (gemm_dw_kernel)     */
  CG_PROBE_GEMM_PERS = 8,      /* persistent fwd / dX GEMM (gemm_bf16_pers_kernel, all */
                               /* epilogue specialisations: one kernel class)           */
  CG_PROBE_ATTN_BWD = 9,       /* attn_bwd_fused_mfma (the fused dQ / dK / dV pass)     */
  CG_PROBE_DW_SLAB = 10        /* dw_slab_reduce_kernel: the k-split slab sum after the */
                               /* grouped dW (HBM-bound; work = its adds, bytes = slabs */
                               /* read + dW read and written)                           */
};
int cg_probe_enable(int kind);
/* record 1 of every `every` launches of the probed kernel (default 1 = all); the launch
 * count and work returned by cg_probe_read cover the recorded launches only */
int cg_probe_sample(int every);
int cg_probe_read(double* work, double* ms, long long* launches);
/* algorithmic HBM bytes (operands once + outputs once) of the same recorded launches */
int cg_probe_bytes(double* bytes);

/* diagnostic: occupy n_cus CUs (one 1024-thread workgroup holding all 160 KiB of LDS each) for
 * `usec` microseconds on `stream` -- stands in for kernels that run beside the step (an RCCL
 * all-reduce) when measuring the persistent launches' sensitivity to busy CUs */
int cg_diag_occupy(int n_cus, int usec, void* stream);

/* sizeof the named ABI struct ("cg_gemm_desc", "cg_dw_product", "cg_dw_group", "cg_reduce_job",
 * "cg_reduce_batch", "cg_transpose_item", "cg_transpose_batch", "cg_adamw_segment",
 * "cg_model_cfg", "cg_param_entry", "cg_model", "cg_model_opts", "cg_sample_params", "cg_gen_state",
 * "cg_score_desc", "cg_sample_plan", "cg_offset_prior", "cg_attr_desc", "cg_kmeans_desc",
 * "cg_term_ce_desc", "cg_ngram_nll_desc", "cg_diag_desc", "cg_attn_stats_desc", "cg_ngram_index_desc",
 * "cg_ngram_coverage_desc"), 0 for
 * another name: lets a binding that mirrors
 * the layouts check them against the library it loaded. */
size_t cg_struct_bytes(const char* name);

/* "codonlm_hip <abi> gfx950".  ABI 0.2 (round 3): cg_gemm_desc.ws_bytes and the size_t
 * workspace-size argument after every workspace pointer.  ABI 0.3 (round 4): cg_model gained
 * the engine-private head_dw_* fields at its end.  ABI 0.4 (round 5): no process-wide setters --
 * cg_gemm_desc.tile / max_wg, cg_dw_group.max_wg and cg_model_cfg.opts replace the cg_set_* /
 * cg_gemm_set_* calls and the environment switches; cg_model_dw_plan takes (B, T) and reports the
 * token split; cg_model.embed_done is gone.  ABI 0.5 (round 6): the fused attention backward --
 * cg_attn_bwd_algo, cg_model_opts.attn_bwd_algo, CG_PROBE_ATTN_BWD; cg_attn_bwd_workspace also
 * covers the fused pass's dQ accumulator.  ABI 0.6: batched on-device generation, additions only --
 * the ragged decode entry points (cg_model_prefill_ragged, cg_model_decode_ragged,
 * cg_decode_ragged_workspace_bytes and their per-row ops, cg_attn_decode_ragged among them) and
 * cg_sample_step with cg_sample_params / cg_gen_state.  ABI 0.6, additions: batched scoring --
 * cg_score_rows with cg_score_desc, and cg_score_workspace.  ABI 0.6, additions: per-step token
 * sets and drawn-token log-probabilities -- cg_sample_step_plan with cg_sample_plan, CG_GEN_PLAN_END.
 * ABI 0.6, additions: multi-offset priors in batched generation -- cg_xf_hist_bytes,
 * cg_model_prefill_hist, cg_model_decode_ragged_hist, cg_offset_prior_workspace and
 * cg_offset_prior_add with cg_offset_prior.  ABI 0.6, additions: input attribution -- cg_attr_seed,
 * cg_attr_reduce and cg_model_input_grad with cg_attr_desc.  ABI 0.6, additions: motif mining --
 * cg_window_keep, cg_window_pool, cg_kmeans_step with cg_kmeans_desc, and cg_kmeans_workspace.
 * ABI 0.6, additions: termination-head correction -- cg_term_ce_fwd / cg_term_ce_bwd with
 * cg_term_ce_desc and cg_term_ce_workspace, cg_model_forward_trunk, cg_model_term_loss,
 * cg_model_backward_heads, and the term_* fields at the end of cg_model.  ABI 0.6, additions: context
 * diagnostic -- cg_ngram_count, cg_ngram_totals, cg_ngram_nll with cg_ngram_nll_desc and
 * cg_ngram_nll_workspace, cg_diag_rows with cg_diag_desc and cg_diag_workspace.  ABI 0.6, additions:
 * attention head analysis -- cg_attn_stats with cg_attn_stats_desc, cg_attn_stats_workspace and
 * cg_model_attn_stats.  ABI 0.6, additions: structural regression probes -- cg_shape_targets,
 * cg_gram_accum and cg_gram_workspace.  ABI 0.6, additions: memorization audit -- cg_ngram_index_build
 * with cg_ngram_index_desc, cg_ngram_coverage with cg_ngram_coverage_desc. */
const char* cg_version(void);

#ifdef __cplusplus
}
#endif
#endif

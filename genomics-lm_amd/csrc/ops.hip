// Memory-bound kernels of the TinyGPT step: LayerNorm fwd/bwd, embedding fwd/bwd,
// SEP segment starts, RoPE, SwiGLU, bias column sums, label-smoothed CE, AdamW,
// casts.  All are HBM-bound; rows are processed one 64-lane wave per row with
// coalesced lane-strided access, cross-row reductions go through per-block partial
// slabs reduced in a fixed order (bitwise reproducible, no float atomics).
#include "common.h"
#include <algorithm>

// ===========================================================================
// LayerNorm  (nn.LayerNorm(d), eps=1e-5, biased variance; model_tiny_gpt.py:137-152,216)
// ===========================================================================
constexpr int LN_MAXV = 32;  // cols <= 2048

template <typename TO>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, long long ldx,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, TO* __restrict__ y,
                                                     long long ldy, float* __restrict__ mean,
                                                     float* __restrict__ rstd, int rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + (long long)row * ldx;
  float v[LN_MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = lane + 64 * i;
    v[i] = (c < cols) ? xr[c] : 0.f;
    s += v[i];
  }
  const float mu = wave_sum(s) / (float)cols;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = lane + 64 * i;
    const float dlt = (c < cols) ? v[i] - mu : 0.f;
    q += dlt * dlt;
  }
  const float var = wave_sum(q) / (float)cols;
  const float rs = rsqrtf(var + eps);
  TO* yr = y + (long long)row * ldy;
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) {
    const int c = lane + 64 * i;
    if (c < cols) st_act<TO>(yr + c, (v[i] - mu) * rs * gamma[c] + beta[c]);
  }
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

// Vectorised fast path: cols = 64*W*NV, each lane owns NV runs of W consecutive columns at
// W*(lane + 64 i) (every wave-instruction moves 64*W contiguous elements; W = 4 -> 1 KiB of
// fp32 x per wave-instruction, W = 2 for widths that are not a multiple of 256): ld_vec<W> /
// st_vec<W> of common.h.
// the residual-gradient row: read again only by the next LayerNorm backward, several kernels
// later, so it is stored nontemporal (round 5, same-box A/B of the C4 step: 14.57 -> 14.50 ms,
// profiles/round5/nt_stores_ab.txt)
template <int W>
__device__ __forceinline__ void stw_g(float* p, const float* v) {
  if constexpr (W == 4) {
    typedef float f4_nt __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store((f4_nt){v[0], v[1], v[2], v[3]}, (f4_nt*)p);
  } else {
    typedef float f2_nt __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store((f2_nt){v[0], v[1]}, (f2_nt*)p);
  }
}

// LayerNorm row prefetch: the backward keeps two rows in flight per wave; the forward runs 4 rows
// per wave with the next row's x loaded before the current row's reductions at W = 2 (d 384) only.
// rocprofv3 per kernel (profiles/round4/ln_prefetch.txt): backward 23.88 -> 23.7 us at d 512,
// 34.39 -> 34.05 at d 384; forward 15.09 -> 14.11 at d 384 (W = 2) but 10.24 -> 10.44 at d 512.
static inline bool ln_pf_bwd() { return true; }
static inline bool ln_pf_fwd(int W) { return W == 2; }

// PF rows per wave of the prefetching forward
constexpr int LN_FWD_RPW = 4;
template <typename TO, int W, int NV>
__global__ __launch_bounds__(256) void ln_fwd_pf(const float* __restrict__ x, long long ldx,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 TO* __restrict__ y, long long ldy, float* __restrict__ mean,
                                                 float* __restrict__ rstd, int rows, float eps) {
  constexpr int cols = 64 * W * NV;
  const int lane = threadIdx.x & 63;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_FWD_RPW;
  if (r0 >= rows) return;
  const int r1 = min(rows, r0 + LN_FWD_RPW);
  float gm[NV][W], bt[NV][W], v[NV][W];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ld_vec<W>(gamma + W * (lane + 64 * i), gm[i]);
    ld_vec<W>(beta + W * (lane + 64 * i), bt[i]);
    ld_vec<W>(x + (long long)r0 * ldx + W * (lane + 64 * i), v[i]);
  }
  for (int row = r0; row < r1; ++row) {
    float nv[NV][W];
    const int nr = min(row + 1, r1 - 1);  // the last row's reload is unused
#pragma unroll
    for (int i = 0; i < NV; ++i) ld_vec<W>(x + (long long)nr * ldx + W * (lane + 64 * i), nv[i]);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) s += v[i][j];
    const float mu = wave_sum(s) * (1.0f / cols);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float a = v[i][j] - mu;
        q += a * a;
      }
    const float rs = rsqrtf(wave_sum(q) * (1.0f / cols) + eps);
    TO* yr = y + (long long)row * ldy;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float o[W];
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = (v[i][j] - mu) * rs * gm[i][j] + bt[i][j];
      st_vec<W>(yr + W * (lane + 64 * i), o);
    }
    if (lane == 0) {
      if (mean) mean[row] = mu;
      if (rstd) rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int j = 0; j < W; ++j) v[i][j] = nv[i][j];
  }
}

// one LayerNorm row per wave (ln_fwd_vec; ln_fwd_mask_kernel)
template <typename TO, int W, int NV>
__device__ __forceinline__ void ln_fwd_row(const float* __restrict__ x, long long ldx, const float* __restrict__ gamma,
                                           const float* __restrict__ beta, TO* __restrict__ y, long long ldy,
                                           float* __restrict__ mean, float* __restrict__ rstd, int row, float eps,
                                           int lane) {
  constexpr int cols = 64 * W * NV;
  const float* xr = x + (long long)row * ldx;
  float v[NV][W];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ld_vec<W>(xr + W * (lane + 64 * i), v[i]);
#pragma unroll
    for (int j = 0; j < W; ++j) s += v[i][j];
  }
  const float mu = wave_sum(s) * (1.0f / cols);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float a = v[i][j] - mu;
      q += a * a;
    }
  const float rs = rsqrtf(wave_sum(q) * (1.0f / cols) + eps);
  TO* yr = y + (long long)row * ldy;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = W * (lane + 64 * i);
    float gm[W], bt[W], o[W];
    ld_vec<W>(gamma + c, gm);
    ld_vec<W>(beta + c, bt);
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = (v[i][j] - mu) * rs * gm[j] + bt[j];
    st_vec<W>(yr + c, o);
  }
  if (lane == 0) {
    if (mean) mean[row] = mu;
    if (rstd) rstd[row] = rs;
  }
}

template <typename TO, int W, int NV>
__global__ __launch_bounds__(256) void ln_fwd_vec(const float* __restrict__ x, long long ldx,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  TO* __restrict__ y, long long ldy, float* __restrict__ mean,
                                                  float* __restrict__ rstd, int rows, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  ln_fwd_row<TO, W, NV>(x, ldx, gamma, beta, y, ldy, mean, rstd, row, eps, threadIdx.x & 63);
}

// The LayerNorm rows of a block's input (HBM-bound) and the attention-dropout keep words of the same
// block's attention (VALU-bound: cg_drop_mask_block) in one launch: LayerNorm and keep-word
// workgroups alternate in the grid, so every CU runs both kinds side by side and the keep words
// ride on the LayerNorm's memory time.  nln LayerNorm workgroups (4 rows each), nmask keep-word
// workgroups (4 causal 64x64 blocks each, mbx per (b, h) row).
template <typename TO, int W, int NV>
__global__ __launch_bounds__(256) void ln_fwd_mask_kernel(const float* __restrict__ x, long long ldx,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, TO* __restrict__ y,
                                                          long long ldy, float* __restrict__ mean,
                                                          float* __restrict__ rstd, int rows, float eps, int nln,
                                                          uint32_t* __restrict__ qmask, int T, int wpr, uint32_t seed,
                                                          uint32_t thr, int nbt, int mbx, int nmask) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = min(nln, nmask);
  int role, k;
  if (b < 2 * pair) {
    role = b & 1;
    k = b >> 1;
  } else {
    role = nln > nmask ? 0 : 1;
    k = pair + (b - 2 * pair);
  }
  if (role == 0) {
    const int row = k * 4 + wave;
    if (row < rows) ln_fwd_row<TO, W, NV>(x, ldx, gamma, beta, y, ldy, mean, rstd, row, eps, lane);
  } else {
    const int i = (k % mbx) * 4 + wave;
    if (i < nbt) cg_drop_mask_block(qmask, T, wpr, seed, thr, i, (long long)(k / mbx), lane);
  }
}

// W = 4 when cols is a multiple of 256 and every row start is 16-B aligned, else W = 2
static inline int ln_width(int cols, const void* a, long long lda, const void* b, long long ldb, int b_bytes) {
  if (cols % 256 == 0 && cols <= 1024 && lda % 4 == 0 && ldb % 4 == 0 && ((uintptr_t)a & 15) == 0 &&
      ((uintptr_t)b & (4 * b_bytes - 1)) == 0)
    return 4;
  if (cols % 128 == 0 && cols <= 1024 && lda % 2 == 0 && ldb % 2 == 0) return 2;
  return 0;
}

template <typename TO>
static bool ln_fwd_fast(int W, int cols, dim3 g, hipStream_t s, const float* x, long long ldx, const float* gamma,
                        const float* beta, TO* y, long long ldy, float* mean, float* rstd, int rows, float eps) {
#define LNF(WW, N)                                                                                                  \
  case N:                                                                                                          \
    if (ln_pf_fwd(WW))                                                                                             \
      hipLaunchKernelGGL((ln_fwd_pf<TO, WW, N>), dim3(cg_cdiv(rows, 4 * LN_FWD_RPW)), dim3(256), 0, s, x, ldx, gamma, \
                         beta, y, ldy, mean, rstd, rows, eps);                                                        \
    else                                                                                                           \
      hipLaunchKernelGGL((ln_fwd_vec<TO, WW, N>), g, dim3(256), 0, s, x, ldx, gamma, beta, y, ldy, mean, rstd, rows, eps); \
    return true;
  if (W == 4) {
    switch (cols / 256) { LNF(4, 1) LNF(4, 2) LNF(4, 3) LNF(4, 4) default: return false; }
  }
  if (W == 2) {
    switch (cols / 128) { LNF(2, 1) LNF(2, 2) LNF(2, 3) LNF(2, 4) LNF(2, 6) LNF(2, 8) default: return false; }
  }
  return false;
#undef LNF
}

extern "C" int cg_layernorm_fwd(int out_dtype, const float* x, long long ldx, const float* gamma,
                                const float* beta, void* y, long long ldy, float* mean, float* rstd,
                                int rows, int cols, float eps, void* stream) {
  if (cols <= 0 || cols > 64 * LN_MAXV || rows < 0) return CG_EUNSUPPORTED;
  if (rows == 0) return CG_OK;
  dim3 g(cg_cdiv(rows, 4));
  const int W = ln_width(cols, x, ldx, y, ldy, out_dtype == CG_BF16 ? 2 : 4);
  if (W) {
    const bool ok = out_dtype == CG_BF16
                        ? ln_fwd_fast<bf16_t>(W, cols, g, (hipStream_t)stream, x, ldx, gamma, beta, (bf16_t*)y,
                                              ldy, mean, rstd, rows, eps)
                        : ln_fwd_fast<float>(W, cols, g, (hipStream_t)stream, x, ldx, gamma, beta, (float*)y, ldy,
                                             mean, rstd, rows, eps);
    if (ok) {
      CG_LAUNCH_CHECK();
      return CG_OK;
    }
  }
  if (out_dtype == CG_BF16)
    hipLaunchKernelGGL(ln_fwd_kernel<bf16_t>, g, dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta,
                       (bf16_t*)y, ldy, mean, rstd, rows, cols, eps);
  else
    hipLaunchKernelGGL(ln_fwd_kernel<float>, g, dim3(256), 0, (hipStream_t)stream, x, ldx, gamma, beta,
                       (float*)y, ldy, mean, rstd, rows, cols, eps);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

template <typename TO>
static bool ln_fwd_mask_fast(int W, int cols, hipStream_t s, const float* x, long long ldx, const float* gamma,
                             const float* beta, TO* y, long long ldy, float* mean, float* rstd, int rows, float eps,
                             uint32_t* qmask, int B, int T, int H, uint32_t seed, uint32_t thr) {
  const int nb = cg_cdiv(T, 64), nbt = nb * (nb + 1) / 2, mbx = cg_cdiv(nbt, 4);
  const long long nmask = (long long)mbx * B * H, nln = cg_cdiv(rows, 4);
  if (nmask + nln > 0x7fffffffLL) return false;
  const dim3 g((unsigned)(nmask + nln));
#define LNFM(WW, N)                                                                                                 \
  case N:                                                                                                          \
    hipLaunchKernelGGL((ln_fwd_mask_kernel<TO, WW, N>), g, dim3(256), 0, s, x, ldx, gamma, beta, y, ldy, mean, rstd, \
                       rows, eps, (int)nln, qmask, T, 2 * nb, seed, thr, nbt, mbx, (int)nmask);                       \
    return true;
  if (W == 4) {
    switch (cols / 256) { LNFM(4, 1) LNFM(4, 2) LNFM(4, 3) LNFM(4, 4) default: return false; }
  }
  if (W == 2) {
    switch (cols / 128) { LNFM(2, 1) LNFM(2, 2) LNFM(2, 3) LNFM(2, 4) LNFM(2, 6) LNFM(2, 8) default: return false; }
  }
  return false;
#undef LNFM
}

extern "C" int cg_layernorm_fwd_mask(int out_dtype, const float* x, long long ldx, const float* gamma,
                                     const float* beta, void* y, long long ldy, float* mean, float* rstd, int rows,
                                     int cols, float eps, int B, int T, int H, uint32_t drop_seed, float drop_p,
                                     void* mask, void* stream) {
  if (!(drop_p > 0.f) || drop_p >= 1.f || !mask || B < 0 || T < 0 || H <= 0) return CG_EINVAL;
  if (cols <= 0 || cols > 64 * LN_MAXV || rows < 0) return CG_EUNSUPPORTED;
  const uint32_t thr = cg_drop_threshold(drop_p);
  const int W = ln_width(cols, x, ldx, y, ldy, out_dtype == CG_BF16 ? 2 : 4);
  if (W && rows > 0 && B > 0 && T > 0) {
    const bool ok = out_dtype == CG_BF16
                        ? ln_fwd_mask_fast<bf16_t>(W, cols, (hipStream_t)stream, x, ldx, gamma, beta, (bf16_t*)y, ldy,
                                                   mean, rstd, rows, eps, (uint32_t*)mask, B, T, H, drop_seed, thr)
                        : ln_fwd_mask_fast<float>(W, cols, (hipStream_t)stream, x, ldx, gamma, beta, (float*)y, ldy,
                                                  mean, rstd, rows, eps, (uint32_t*)mask, B, T, H, drop_seed, thr);
    if (ok) {
      CG_LAUNCH_CHECK();
      return CG_OK;
    }
  }
  // shapes outside the vector LayerNorm: the two launches (the same results)
  const int rc = cg_layernorm_fwd(out_dtype, x, ldx, gamma, beta, y, ldy, mean, rstd, rows, cols, eps, stream);
  if (rc != CG_OK) return rc;
  return cg_attn_drop_mask(B, T, H, drop_seed, drop_p, mask, stream);
}

extern "C" int cg_layernorm_bwd_blocks(int rows) {
  // 32 rows per block (8 per wave), at most 1024 blocks.  Round 2 measured 16 rows faster (C4:
  // 29.7 vs 38.2 us); with the round-2/3 kernel the two run alike (24.1 vs 24.5 us) and 32 halves
  // the partial rows the deferred column reduction reads (18.9 -> 14.9 us per group): C4 step
  // -23..-46 us (3 interleaved same-box runs); 64 rows was slower again.
  constexpr int rpb = 32, maxb = 1024;
  int b = cg_cdiv(rows, rpb);
  return b > maxb ? maxb : (b < 1 ? 1 : b);
}
extern "C" size_t cg_layernorm_bwd_workspace(int rows, int cols, int want_col) {
  return (size_t)cg_layernorm_bwd_blocks(rows) * (size_t)(want_col ? 3 : 2) * (size_t)(cols > 0 ? cols : 0) * sizeof(float);
}

// Vectorised backward: cols = 64*W*NV (runs as in ln_fwd_vec); one wave per row, per-lane
// dgamma/dbeta partials in registers, combined across the block's 4 waves in LDS (fixed order).
// g_in may alias g_out (the engine accumulates the residual gradient in place): each row's g_in
// values are read before that row's g_out is written, and no other row touches them.
// PF: the next row's dy / x / residual-gradient loads are issued before the current row's
// reductions (two rows in flight per wave)
template <typename TD, typename TO, int W, int NV, bool PF = false>
__global__ __launch_bounds__(256) void ln_bwd_vec(const TD* __restrict__ dy, long long lddy, const float* __restrict__ x,
                                                  long long ldx, const float* __restrict__ mean,
                                                  const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                  const float* g_in, float* g_out,
                                                  TO* __restrict__ g_out_t, uint32_t seed, uint32_t thr, float dscale,
                                                  float* __restrict__ partials, int rows, int want_col) {
  constexpr int cols = 64 * W * NV;
  __shared__ __attribute__((aligned(16))) float red[4][3 * cols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (rows + gridDim.x - 1) / gridDim.x;
  const int r_begin = blockIdx.x * per, r_end = min(rows, r_begin + per);
  float gm[NV][W], dg[NV][W], db[NV][W], dc[NV][W];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    ld_vec<W>(gamma + W * (lane + 64 * i), gm[i]);
#pragma unroll
    for (int j = 0; j < W; ++j) dg[i][j] = db[i][j] = dc[i][j] = 0.f;
  }
  // one row's operands: the residual-gradient row is loaded with dy and x, before the reductions
  struct RowIn { float mu, rs, g2[NV][W], d[NV][W], xv[NV][W]; };
  auto load_row = [&](int row, RowIn& in) __attribute__((always_inline)) {
    in.mu = mean[row];
    in.rs = rstd[row];
    if (g_in) {
#pragma unroll
      for (int i = 0; i < NV; ++i) ld_vec<W>(g_in + (long long)row * cols + W * (lane + 64 * i), in.g2[i]);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = W * (lane + 64 * i);
      ld_vec<W>(dy + (long long)row * lddy + c, in.d[i]);
      ld_vec<W>(x + (long long)row * ldx + c, in.xv[i]);
    }
  };
  RowIn cur;
  if (PF && r_begin + wave < r_end) load_row(r_begin + wave, cur);
  for (int row = r_begin + wave; row < r_end; row += 4) {
    if constexpr (!PF) {
      load_row(row, cur);
    }
    RowIn nxt;
    if constexpr (PF) {
      if (row + 4 < r_end) load_row(row + 4, nxt);  // wave-uniform: rows past r_end belong to no wave here
    }
    const float mu = cur.mu, rs = cur.rs;
    const float* gi = g_in ? g_in + (long long)row * cols : nullptr;
    float xh[NV][W], gy[NV][W];
    float s1 = 0.f, s2 = 0.f;
    float (&g2)[NV][W] = cur.g2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float d = cur.d[i][j];
        xh[i][j] = (cur.xv[i][j] - mu) * rs;
        gy[i][j] = d * gm[i][j];
        dg[i][j] += d * xh[i][j];
        db[i][j] += d;
        s1 += gy[i][j];
        s2 += gy[i][j] * xh[i][j];
      }
    }
    s1 = wave_sum(s1) * (1.0f / cols);
    s2 = wave_sum(s2) * (1.0f / cols);
    float* go = g_out + (long long)row * cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = W * (lane + 64 * i);
      float o[W];
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = rs * (gy[i][j] - s1 - xh[i][j] * s2);
      if (gi) {
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] += g2[i][j];
      }
      stw_g<W>(go + c, o);
      if (g_out_t) {
        if (thr) {
#pragma unroll
          for (int j = 0; j < W; j += 2) {
            const uint32_t h = cg_hash_pair(seed, (uint32_t)row, (uint32_t)(c + j) >> 1);
            o[j] = (h & 0xFFFFu) >= thr ? o[j] * dscale : 0.f;
            o[j + 1] = (h >> 16) >= thr ? o[j + 1] * dscale : 0.f;
          }
        }
        st_vec<W>(g_out_t + (long long)row * cols + c, o);
#pragma unroll
        for (int j = 0; j < W; ++j) dc[i][j] += o[j];  // column sum of the consumer's dY (its bias gradient)
      }
    }
    if constexpr (PF) cur = nxt;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = W * (lane + 64 * i);
    st_vec<W>(&red[wave][c], dg[i]);
    st_vec<W>(&red[wave][cols + c], db[i]);
    st_vec<W>(&red[wave][2 * cols + c], dc[i]);
  }
  __syncthreads();
  const int nw = (want_col ? 3 : 2);
  for (int e = threadIdx.x; e < nw * cols; e += 256)
    partials[(long long)blockIdx.x * nw * cols + e] = red[0][e] + red[1][e] + red[2][e] + red[3][e];
}

template <typename TD, typename TO>
static bool ln_bwd_fast(int W, int cols, int nblk, hipStream_t s, const TD* dy, long long lddy, const float* x,
                        long long ldx, const float* mean, const float* rstd, const float* gamma, const float* g_in,
                        float* g_out, TO* g_out_t, uint32_t seed, uint32_t thr, float dscale, float* partials,
                        int rows, int want_col) {
#define LNB(WW, N)                                                                                                  \
  case N:                                                                                                          \
    if (ln_pf_bwd())                                                                                               \
      hipLaunchKernelGGL((ln_bwd_vec<TD, TO, WW, N, true>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, mean, rstd, \
                         gamma, g_in, g_out, g_out_t, seed, thr, dscale, partials, rows, want_col);                   \
    else                                                                                                           \
      hipLaunchKernelGGL((ln_bwd_vec<TD, TO, WW, N>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, mean, rstd, gamma, \
                         g_in, g_out, g_out_t, seed, thr, dscale, partials, rows, want_col);                          \
    return true;
  if (W == 4) {
    switch (cols / 256) { LNB(4, 1) LNB(4, 2) LNB(4, 3) LNB(4, 4) default: return false; }
  }
  if (W == 2) {
    switch (cols / 128) { LNB(2, 1) LNB(2, 2) LNB(2, 3) LNB(2, 4) LNB(2, 6) LNB(2, 8) default: return false; }
  }
  return false;
#undef LNB
}

// Column sums of a [nrows][ld] fp32 partial-row block for the 32 columns c0 .. c0+31, one
// 1024-thread block, in a fixed order: row lane v in [0, 64) sums rows v + 64u + 256k in 4 chains
// u (the tail rows into chain 0), the chains combine as (0+1)+(2+3), the lanes in 8 groups of 8,
// then the 8 group sums.  Thread (tx, ty) serves lanes ty and ty + 32 of column c0 + tx, so every
// wave load covers two 128-B row segments.  The result is valid in threads ty == 0.
__device__ __forceinline__ float colred32(const float* __restrict__ part, long long ld, int nrows, int ncols, int c0,
                                          float (*red)[33]) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c = c0 + tx;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int v = ty + 32 * h;
    float s = 0.f;
    if (c < ncols) {
      float s4[4] = {0.f, 0.f, 0.f, 0.f};
      int b = v;
      for (; b + 192 < nrows; b += 256)
#pragma unroll
        for (int u = 0; u < 4; ++u) s4[u] += part[(long long)(b + 64 * u) * ld + c];
      for (; b < nrows; b += 64) s4[0] += part[(long long)b * ld + c];
      s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    }
    red[v][tx] = s;
  }
  __syncthreads();
  float g = 0.f;
  if (ty < 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) g += red[ty * 8 + i][tx];
  }
  __syncthreads();
  if (ty < 8) red[ty][tx] = g;
  __syncthreads();
  float t = 0.f;
  if (ty == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][tx];
  }
  return t;
}

// sum the per-block partial rows of the LayerNorm backward (colred32 order)
// (nw = 2: dgamma|dbeta, nw = 3: dgamma|dbeta|dcol)
__global__ __launch_bounds__(1024) void ln_param_reduce2(const float* __restrict__ partials, int nblk, int cols,
                                                         int nw, float* __restrict__ dgamma,
                                                         float* __restrict__ dbeta, float* __restrict__ dcol,
                                                         int accumulate) {
  __shared__ float red[64][33];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  const float t = colred32(partials, (long long)nw * cols, nblk, nw * cols, blockIdx.x * 32, red);
  if ((threadIdx.x >> 5) == 0 && c < nw * cols) {
    float* dst = c < cols ? dgamma + c : c < 2 * cols ? dbeta + (c - cols) : dcol + (c - 2 * cols);
    *dst = accumulate ? *dst + t : t;
  }
}

// dx = rstd * (dy*g - mean(dy*g) - xhat*mean(dy*g*xhat));  g_out = g_in + dx
template <typename TD, typename TO>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const TD* __restrict__ dy, long long lddy,
                                                     const float* __restrict__ x, long long ldx,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* g_in,
                                                     float* g_out, TO* __restrict__ g_out_t,
                                                     uint32_t seed, uint32_t thr, float dscale,
                                                     float* __restrict__ partials, int rows, int cols,
                                                     int want_col) {
  __shared__ float red[4][3 * 64 * 8];  // per-wave column partials, chunked
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_blk = (rows + gridDim.x - 1) / gridDim.x;
  const int r_begin = blockIdx.x * rows_per_blk;
  const int r_end = min(rows, r_begin + rows_per_blk);
  float dg[LN_MAXV], db[LN_MAXV], dc[LN_MAXV];
#pragma unroll
  for (int i = 0; i < LN_MAXV; ++i) { dg[i] = 0.f; db[i] = 0.f; dc[i] = 0.f; }
  for (int row = r_begin + wave; row < r_end; row += 4) {
    const float mu = mean[row], rs = rstd[row];
    const float* xr = x + (long long)row * ldx;
    const TD* dyr = dy + (long long)row * lddy;
    float xh[LN_MAXV], gy[LN_MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < cols) {
        const float d = ld_act<TD>(dyr + c);
        xh[i] = (xr[c] - mu) * rs;
        gy[i] = d * gamma[c];
        dg[i] += d * xh[i];
        db[i] += d;
      } else {
        xh[i] = 0.f; gy[i] = 0.f;
      }
      s1 += gy[i];
      s2 += gy[i] * xh[i];
    }
    s1 = wave_sum(s1) / (float)cols;
    s2 = wave_sum(s2) / (float)cols;
    const float* gi = g_in ? g_in + (long long)row * cols : nullptr;
    float* go = g_out + (long long)row * cols;
    TO* got = g_out_t ? g_out_t + (long long)row * cols : nullptr;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < cols) {
        float v = rs * (gy[i] - s1 - xh[i] * s2);
        if (gi) v += gi[c];
        go[c] = v;
        if (got) {
          float w = v;
          if (thr) w = cg_keep(seed, (uint32_t)row, (uint32_t)c, thr) ? w * dscale : 0.f;
          st_act<TO>(got + c, w);
          dc[i] += w;
        }
      }
    }
  }
  // reduce the 4 waves' column partials in fixed order, 64*8 columns at a time
#pragma unroll
  for (int cb = 0; cb < LN_MAXV; cb += 8) {
    if (cb * 64 >= cols) continue;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[wave][i * 64 + lane] = dg[cb + i];
      red[wave][512 + i * 64 + lane] = db[cb + i];
      red[wave][1024 + i * 64 + lane] = dc[cb + i];
    }
    __syncthreads();
    const int nw = want_col ? 3 : 2;
    for (int e = threadIdx.x; e < nw * 512; e += 256) {
      const int which = e >> 9, rem = e & 511, i = rem >> 6, l = rem & 63;
      const int c = l + 64 * (cb + i);
      if (c < cols) {
        const float v = red[0][e] + red[1][e] + red[2][e] + red[3][e];
        partials[(long long)blockIdx.x * nw * cols + which * cols + c] = v;
      }
    }
    __syncthreads();
  }
}

__global__ void ln_param_reduce_kernel(const float* __restrict__ partials, int nblk, int cols, int nw,
                                       float* __restrict__ dgamma, float* __restrict__ dbeta,
                                       float* __restrict__ dcol, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nw * cols) return;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += partials[(long long)b * nw * cols + c];
  float* dst = c < cols ? dgamma + c : c < 2 * cols ? dbeta + (c - cols) : dcol + (c - 2 * cols);
  *dst = accumulate ? *dst + s : s;
}

// the row pass (g_out, g_out_t, per-block partial rows); *fast: the vectorised kernel ran
static int ln_bwd_rows(int dy_dtype, const void* dy, long long lddy, const float* x, long long ldx, const float* mean,
                       const float* rstd, const float* gamma, const float* g_in, float* g_out, int out_dtype,
                       void* g_out_t, uint32_t drop_seed, float drop_p, float* partials, int want_col, int rows,
                       int cols, hipStream_t s, bool* fast_out) {
  const int nblk = cg_layernorm_bwd_blocks(rows);
  const uint32_t thr = drop_p > 0.f ? cg_drop_threshold(drop_p) : 0u;
  const float dscale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  bool fast = false;
  // W = 4 also needs 16-B aligned g_in / g_out rows (stride cols) and 8-B aligned branch rows
  int W = ln_width(cols, x, ldx, dy, lddy, dy_dtype == CG_BF16 ? 2 : 4);
  if (W == 4 && (((uintptr_t)g_out | (uintptr_t)g_in | (uintptr_t)g_out_t) & 15)) W = 2;
  if (W) {
    if (dy_dtype == CG_BF16) {
      fast = out_dtype == CG_BF16
                 ? ln_bwd_fast<bf16_t, bf16_t>(W, cols, nblk, s, (const bf16_t*)dy, lddy, x, ldx, mean, rstd, gamma, g_in,
                                               g_out, (bf16_t*)g_out_t, drop_seed, thr, dscale, partials, rows, want_col)
                 : ln_bwd_fast<bf16_t, float>(W, cols, nblk, s, (const bf16_t*)dy, lddy, x, ldx, mean, rstd, gamma, g_in,
                                              g_out, (float*)g_out_t, drop_seed, thr, dscale, partials, rows, want_col);
    } else {
      fast = out_dtype == CG_BF16
                 ? ln_bwd_fast<float, bf16_t>(W, cols, nblk, s, (const float*)dy, lddy, x, ldx, mean, rstd, gamma, g_in,
                                              g_out, (bf16_t*)g_out_t, drop_seed, thr, dscale, partials, rows, want_col)
                 : ln_bwd_fast<float, float>(W, cols, nblk, s, (const float*)dy, lddy, x, ldx, mean, rstd, gamma, g_in,
                                             g_out, (float*)g_out_t, drop_seed, thr, dscale, partials, rows, want_col);
    }
  }
  if (!fast) {
#define LNB(TD, TO)                                                                                  \
  hipLaunchKernelGGL((ln_bwd_kernel<TD, TO>), dim3(nblk), dim3(256), 0, s, (const TD*)dy, lddy, x, ldx, \
                     mean, rstd, gamma, g_in, g_out, (TO*)g_out_t, drop_seed, thr, dscale, partials, rows, cols, want_col)
    if (dy_dtype == CG_BF16) {
      if (out_dtype == CG_BF16) LNB(bf16_t, bf16_t); else LNB(bf16_t, float);
    } else {
      if (out_dtype == CG_BF16) LNB(float, bf16_t); else LNB(float, float);
    }
#undef LNB
  }
  CG_LAUNCH_CHECK();
  *fast_out = fast;
  return CG_OK;
}

extern "C" int cg_layernorm_bwd(int dy_dtype, const void* dy, long long lddy, const float* x, long long ldx,
                                const float* mean, const float* rstd, const float* gamma, const float* g_in,
                                float* g_out, int out_dtype, void* g_out_t, uint32_t drop_seed, float drop_p,
                                float* partials, size_t partials_bytes, float* dgamma, float* dbeta,
                                float* dcolsum, int accumulate, int rows, int cols, float eps, void* stream) {
  (void)eps;
  if (cols <= 0 || cols > 64 * LN_MAXV) return CG_EUNSUPPORTED;
  if (dcolsum && (!g_out_t || !dgamma || !dbeta)) return CG_EINVAL;
  const int want_col = dcolsum ? 1 : 0;
  if (rows <= 0) return CG_OK;
  if (!partials || partials_bytes < cg_layernorm_bwd_workspace(rows, cols, want_col)) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = cg_layernorm_bwd_blocks(rows);
  bool fast = false;
  const int rc = ln_bwd_rows(dy_dtype, dy, lddy, x, ldx, mean, rstd, gamma, g_in, g_out, out_dtype, g_out_t, drop_seed,
                             drop_p, partials, want_col, rows, cols, s, &fast);
  if (rc != CG_OK) return rc;
  if (dgamma && dbeta) {
    if (fast)
      hipLaunchKernelGGL(ln_param_reduce2, dim3(cg_cdiv((2 + want_col) * cols, 32)), dim3(1024), 0, s, partials, nblk,
                         cols, 2 + want_col, dgamma, dbeta, dcolsum, accumulate);
    else
      hipLaunchKernelGGL(ln_param_reduce_kernel, dim3(cg_cdiv((2 + want_col) * cols, 256)), dim3(256), 0, s, partials,
                         nblk, cols, 2 + want_col, dgamma, dbeta, dcolsum, accumulate);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

extern "C" int cg_layernorm_bwd_partials(int dy_dtype, const void* dy, long long lddy, const float* x, long long ldx,
                                         const float* mean, const float* rstd, const float* gamma, const float* g_in,
                                         float* g_out, int out_dtype, void* g_out_t, uint32_t drop_seed, float drop_p,
                                         float* partials, size_t partials_bytes, int want_col, int rows, int cols,
                                         void* stream) {
  if (cols <= 0 || cols > 64 * LN_MAXV) return CG_EUNSUPPORTED;
  if (!partials || (want_col && !g_out_t)) return CG_EINVAL;
  if (rows <= 0) return CG_OK;
  if (partials_bytes < cg_layernorm_bwd_workspace(rows, cols, want_col)) return CG_EINVAL;
  bool fast = false;
  return ln_bwd_rows(dy_dtype, dy, lddy, x, ldx, mean, rstd, gamma, g_in, g_out, out_dtype, g_out_t, drop_seed, drop_p,
                     partials, want_col ? 1 : 0, rows, cols, (hipStream_t)stream, &fast);
}

// Batched column reductions (cg_reduce_columns): one 1024-thread block = 32 columns of one job in
// the colred32 order (the order of ln_param_reduce2, so a deferred LayerNorm reduction is bitwise
// the in-call one); the block finds its job by a scan over the (<= CG_REDUCE_MAX) first-block offsets
__global__ __launch_bounds__(1024) void reduce_columns_kernel(cg_reduce_batch bt) {
  __shared__ float red[64][33];
  int j = 0;
  while (j + 1 < bt.n && bt.j[j + 1].first_block <= (int)blockIdx.x) ++j;
  const cg_reduce_job& jb = bt.j[j];
  const int c0 = ((int)blockIdx.x - jb.first_block) * 32, c = c0 + (threadIdx.x & 31);
  const float t = colred32(jb.part, jb.ld, jb.nrows, jb.cols, c0, red);
  if ((threadIdx.x >> 5) == 0 && c < jb.cols) jb.dst[c] = jb.accumulate ? jb.dst[c] + t : t;
}

extern "C" int cg_reduce_columns(const cg_reduce_batch* batch, void* stream) {
  if (!batch || batch->n < 0 || batch->n > CG_REDUCE_MAX) return CG_EINVAL;
  cg_reduce_batch bt = *batch;
  int nb = 0, k = 0;
  for (int i = 0; i < batch->n; ++i) {
    const cg_reduce_job& q = batch->j[i];
    if (q.cols < 0 || q.nrows < 0 || ((!q.part || !q.dst) && q.cols > 0)) return CG_EINVAL;
    if (q.cols == 0) continue;
    bt.j[k] = q;
    bt.j[k].first_block = nb;
    nb += cg_cdiv(q.cols, 32);
    ++k;
  }
  bt.n = k;
  if (nb == 0) return CG_OK;
  hipLaunchKernelGGL(reduce_columns_kernel, dim3(nb), dim3(1024), 0, (hipStream_t)stream, bt);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Embedding (model_tiny_gpt.py:305-312)
// ===========================================================================
__global__ __launch_bounds__(256) void embed_fwd_kernel(const int64_t* __restrict__ idx, const float* __restrict__ tok,
                                                        const float* __restrict__ pos, float* __restrict__ x,
                                                        int B, int T, int d, uint32_t seed, uint32_t thr, float dscale) {
  const long long total = (long long)B * T * d;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long m = e / d;
    const int c = (int)(e - m * d);
    const int t = (int)(m % T);
    float v = tok[idx[m] * d + c];
    if (pos) v += pos[(long long)t * d + c];
    if (thr) v = cg_keep(seed, (uint32_t)m, (uint32_t)c, thr) ? v * dscale : 0.f;
    x[e] = v;
  }
}

// d % 4 == 0: one wave per token row, 16-B column runs (no per-element index division)
__global__ __launch_bounds__(256) void embed_fwd_rows_kernel(const int64_t* __restrict__ idx, const float* __restrict__ tok,
                                                             const float* __restrict__ pos, float* __restrict__ x,
                                                             int rows, int T, int d, uint32_t seed, uint32_t thr,
                                                             float dscale) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= rows) return;
  const int t = m % T;
  const float4* tr = (const float4*)(tok + idx[m] * (long long)d);
  const float4* pr = pos ? (const float4*)(pos + (long long)t * d) : nullptr;
  float4* xr = (float4*)(x + (long long)m * d);
  for (int q = lane; q < d / 4; q += 64) {
    float4 v = tr[q];
    if (pr) {
      const float4 p = pr[q];
      v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    if (thr) {
      const uint32_t c = 4u * (uint32_t)q;
      v.x = cg_keep(seed, (uint32_t)m, c, thr) ? v.x * dscale : 0.f;
      v.y = cg_keep(seed, (uint32_t)m, c + 1, thr) ? v.y * dscale : 0.f;
      v.z = cg_keep(seed, (uint32_t)m, c + 2, thr) ? v.z * dscale : 0.f;
      v.w = cg_keep(seed, (uint32_t)m, c + 3, thr) ? v.w * dscale : 0.f;
    }
    xr[q] = v;
  }
}

extern "C" int cg_embed_fwd(const int64_t* idx, const float* tok_emb, const float* pos_emb, float* x, int B,
                            int T, int d, uint32_t drop_seed, float drop_p, void* stream) {
  const long long total = (long long)B * T * d;
  if (total == 0) return CG_OK;
  const uint32_t thr = drop_p > 0.f ? cg_drop_threshold(drop_p) : 0u;
  if (d % 4 == 0 && ((uintptr_t)tok_emb & 15) == 0 && ((uintptr_t)x & 15) == 0 &&
      (!pos_emb || ((uintptr_t)pos_emb & 15) == 0)) {
    const int rows = B * T;
    hipLaunchKernelGGL(embed_fwd_rows_kernel, dim3(cg_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, idx, tok_emb,
                       pos_emb, x, rows, T, d, drop_seed, thr, drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f);
    CG_LAUNCH_CHECK();
    return CG_OK;
  }
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(embed_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, idx, tok_emb, pos_emb, x,
                     B, T, d, drop_seed, thr, drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

constexpr int EMB_RCHUNKS = 32;   // row chunks of embed_bwd_tok_kernel (64 columns per workgroup)
constexpr int EMB_RCHUNKS2 = 64;  // row chunks of embed_bwd_tok2_kernel (128 columns per workgroup)
constexpr int EMB_V2 = 80;        // largest vocabulary of the latter (4 [V][128] fp32 slabs in LDS)
extern "C" size_t cg_embed_bwd_workspace(int B, int T, int V, int d) {
  (void)B; (void)T;
  return (size_t)(V <= EMB_V2 ? EMB_RCHUNKS2 : EMB_RCHUNKS) * V * d * sizeof(float);
}

// per (64-column chunk, row chunk): each wave accumulates its own rows into its own LDS
// [V][64] slab (no atomics), the 4 slabs are summed in order into a global partial slab.
__global__ __launch_bounds__(256) void embed_bwd_tok_kernel(const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                            float* __restrict__ part, int rows, int V, int d,
                                                            uint32_t seed, uint32_t thr, float dscale) {
  extern __shared__ __attribute__((aligned(16))) float acc[];  // [4][V][64]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  for (int e = threadIdx.x; e < 4 * V * 64; e += 256) acc[e] = 0.f;
  __syncthreads();
  const int per = (rows + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  float* mine = acc + wave * V * 64;
  if (c < d) {
    int r = r0 + wave;
    for (; r + 28 < r1; r += 32) {  // 8 rows' loads in flight, added in row order
      int tk[8];
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        tk[u] = (int)idx[r + 4 * u];
        v[u] = g[(long long)(r + 4 * u) * d + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (thr) v[u] = cg_keep(seed, (uint32_t)(r + 4 * u), (uint32_t)c, thr) ? v[u] * dscale : 0.f;
        mine[tk[u] * 64 + lane] += v[u];
      }
    }
    for (; r < r1; r += 4) {
      const int tkn = (int)idx[r];
      float v = g[(long long)r * d + c];
      if (thr) v = cg_keep(seed, (uint32_t)r, (uint32_t)c, thr) ? v * dscale : 0.f;
      mine[tkn * 64 + lane] += v;
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < V * 64; e += 256) {
    const int v = e >> 6, l = e & 63, cc = blockIdx.x * 64 + l;
    if (cc < d) {
      const float s = acc[e] + acc[V * 64 + e] + acc[2 * V * 64 + e] + acc[3 * V * 64 + e];
      part[((long long)blockIdx.y * V + v) * d + cc] = s;
    }
  }
}

// V <= EMB_V2: each lane owns two adjacent columns (one float2 load and one keep hash per row:
// the pair is the hash's column pair), a wave spans 128 columns and keeps 16 rows' loads in
// flight -- 4x the bytes in flight of the kernel above, whose 4-byte lanes left the C4 pass
// latency-bound (24 us for 34 MB).  Same fixed order: rows of a wave in order, slabs 0..3, chunks.
__global__ __launch_bounds__(256) void embed_bwd_tok2_kernel(const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                             float* __restrict__ part, int rows, int V, int d,
                                                             uint32_t seed, uint32_t thr, float dscale) {
  extern __shared__ __attribute__((aligned(16))) float acc[];  // [4][V][128]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 128 + 2 * lane;
  for (int e = threadIdx.x; e < V * 128; e += 256) *(float4*)(acc + 4 * e) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  const int per = (rows + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  float* mine = acc + wave * V * 128 + 2 * lane;
  auto add = [&](int r, int tk, float2 v) {
    if (thr) {
      const uint32_t h = cg_hash_pair(seed, (uint32_t)r, (uint32_t)c >> 1);
      v.x = (h & 0xFFFFu) >= thr ? v.x * dscale : 0.f;
      v.y = (h >> 16) >= thr ? v.y * dscale : 0.f;
    }
    float2* a = (float2*)(mine + tk * 128);
    float2 t = *a;
    t.x += v.x;
    t.y += v.y;
    *a = t;
  };
  if (c < d) {
    int r = r0 + wave;
    for (; r + 60 < r1; r += 64) {  // 16 rows' loads in flight, added in row order
      int tk[16];
      float2 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        tk[u] = (int)idx[r + 4 * u];
        v[u] = *(const float2*)(g + (long long)(r + 4 * u) * d + c);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) add(r + 4 * u, tk[u], v[u]);
    }
    for (; r < r1; r += 4) add(r, (int)idx[r], *(const float2*)(g + (long long)r * d + c));
  }
  __syncthreads();
  for (int e = threadIdx.x; e < V * 128; e += 256) {
    const int v = e >> 7, l = e & 127, cc = blockIdx.x * 128 + l;
    if (cc < d) {
      const float sm = acc[e] + acc[V * 128 + e] + acc[2 * V * 128 + e] + acc[3 * V * 128 + e];
      part[((long long)blockIdx.y * V + v) * d + cc] = sm;
    }
  }
}

__global__ void embed_bwd_tok_reduce(const float* __restrict__ part, float* __restrict__ dtok, int nch, int V, int d,
                                     int accumulate) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= V * d) return;
  float s = 0.f;
#pragma unroll 8
  for (int ch = 0; ch < nch; ++ch) s += part[(long long)ch * V * d + e];
  dtok[e] = accumulate ? dtok[e] + s : s;
}

// d % 4 == 0: each thread sums 4 adjacent columns (one float4 per batch row, the B rows' loads
// independent), per element in the same b order as the scalar kernel
__global__ void embed_bwd_pos4_kernel(const float* __restrict__ g, float* __restrict__ dpos, int B, int T, int d,
                                      uint32_t seed, uint32_t thr, float dscale, int accumulate) {
  const long long e4 = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e4 * 4 >= (long long)T * d) return;
  const long long e = e4 * 4;
  const int t = (int)(e / d), c = (int)(e % d);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = 0; b < B; ++b) {
    const long long m = (long long)b * T + t;
    float4 v = *(const float4*)(g + m * d + c);
    if (thr) {
      const uint32_t h0 = cg_hash_pair(seed, (uint32_t)m, (uint32_t)c >> 1);
      const uint32_t h1 = cg_hash_pair(seed, (uint32_t)m, ((uint32_t)c >> 1) + 1u);
      v.x = (h0 & 0xFFFFu) >= thr ? v.x * dscale : 0.f;
      v.y = (h0 >> 16) >= thr ? v.y * dscale : 0.f;
      v.z = (h1 & 0xFFFFu) >= thr ? v.z * dscale : 0.f;
      v.w = (h1 >> 16) >= thr ? v.w * dscale : 0.f;
    }
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  float4* o = (float4*)(dpos + e);
  if (accumulate) {
    const float4 a = *o;
    s = make_float4(a.x + s.x, a.y + s.y, a.z + s.z, a.w + s.w);
  }
  *o = s;
}

__global__ void embed_bwd_pos_kernel(const float* __restrict__ g, float* __restrict__ dpos, int B, int T, int d,
                                     uint32_t seed, uint32_t thr, float dscale, int accumulate) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= (long long)T * d) return;
  const int t = (int)(e / d), c = (int)(e % d);
  float s = 0.f;
  for (int b = 0; b < B; ++b) {
    const long long m = (long long)b * T + t;
    float v = g[m * d + c];
    if (thr) v = cg_keep(seed, (uint32_t)m, (uint32_t)c, thr) ? v * dscale : 0.f;
    s += v;
  }
  dpos[e] = accumulate ? dpos[e] + s : s;
}

extern "C" int cg_embed_bwd(const int64_t* idx, const float* g, float* dtok, float* dpos, int B, int T, int V,
                            int d, uint32_t drop_seed, float drop_p, int accumulate, void* ws, size_t ws_bytes,
                            void* stream) {
  if (V > 256) return CG_EUNSUPPORTED;
  const int rows = B * T;
  if (rows == 0) return CG_OK;
  if (dtok && (!ws || ws_bytes < cg_embed_bwd_workspace(B, T, V, d))) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t thr = drop_p > 0.f ? cg_drop_threshold(drop_p) : 0u;
  const float dscale = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  if (dtok && V <= EMB_V2 && d % 2 == 0 && ((uintptr_t)g & 7) == 0) {
    const int nch = EMB_RCHUNKS2 > rows ? rows : EMB_RCHUNKS2;
    const size_t sh = (size_t)4 * V * 128 * sizeof(float);
    cg_func_lds((const void*)embed_bwd_tok2_kernel, 160 * 1024);
    hipLaunchKernelGGL(embed_bwd_tok2_kernel, dim3(cg_cdiv(d, 128), nch), dim3(256), sh, s, idx, g, (float*)ws, rows,
                       V, d, drop_seed, thr, dscale);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_bwd_tok_reduce, dim3(cg_cdiv(V * d, 256)), dim3(256), 0, s, (const float*)ws, dtok,
                       nch, V, d, accumulate);
    CG_LAUNCH_CHECK();
  } else if (dtok) {
    int nch = EMB_RCHUNKS;
    if (nch > rows) nch = rows;
    const size_t sh = (size_t)4 * V * 64 * sizeof(float);
    if (sh > 160 * 1024) return CG_EUNSUPPORTED;
    cg_func_lds((const void*)embed_bwd_tok_kernel, 160 * 1024);
    hipLaunchKernelGGL(embed_bwd_tok_kernel, dim3(cg_cdiv(d, 64), nch), dim3(256), sh, s, idx, g, (float*)ws, rows,
                       V, d, drop_seed, thr, dscale);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_bwd_tok_reduce, dim3(cg_cdiv(V * d, 256)), dim3(256), 0, s, (const float*)ws, dtok,
                       nch, V, d, accumulate);
    CG_LAUNCH_CHECK();
  }
  if (dpos) {
    if (d % 4 == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)dpos & 15) == 0)
      hipLaunchKernelGGL(embed_bwd_pos4_kernel, dim3(cg_cdiv((long long)T * d / 4, 256)), dim3(256), 0, s, g, dpos, B,
                         T, d, drop_seed, thr, dscale, accumulate);
    else
      hipLaunchKernelGGL(embed_bwd_pos_kernel, dim3(cg_cdiv((long long)T * d, 256)), dim3(256), 0, s, g, dpos, B, T,
                       d, drop_seed, thr, dscale, accumulate);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

// ===========================================================================
// SEP segment starts: segstart[b,t] = max{p <= t : idx[b,p] == sep} (0 if none)
// (same-segment test of build_attention_mask, model_tiny_gpt.py:289-294)
// ===========================================================================
__global__ __launch_bounds__(256) void segstart_kernel(const int64_t* __restrict__ idx, int32_t* __restrict__ out,
                                                       int T, int sep) {
  __shared__ int tot[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = (T + 255) / 256;
  const int t0 = tid * per, t1 = min(T, t0 + per);
  int run = 0;
  for (int t = t0; t < t1; ++t)
    if (sep >= 0 && idx[(long long)b * T + t] == sep) run = t;
  tot[tid] = run;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int v = (tid >= off) ? tot[tid - off] : 0;
    __syncthreads();
    tot[tid] = max(tot[tid], v);
    __syncthreads();
  }
  run = tid > 0 ? tot[tid - 1] : 0;
  for (int t = t0; t < t1; ++t) {
    if (sep >= 0 && idx[(long long)b * T + t] == sep) run = t;
    out[(long long)b * T + t] = run;
  }
}

extern "C" int cg_segment_starts(const int64_t* idx, int32_t* segstart, int B, int T, int sep_id, void* stream) {
  if (B == 0 || T == 0) return CG_OK;
  hipLaunchKernelGGL(segstart_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, idx, segstart, T, sep_id);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// RoPE in place on packed qkv rows (rotate_half form; model_tiny_gpt.py:35-45)
// cos/sin tables [T][hd/2] are built on the host exactly like RotaryEmbedding.
// ===========================================================================
template <typename T_>
__global__ __launch_bounds__(256) void rope_kernel(T_* __restrict__ qkv, long long ld, int rows, int T, int nh, int hd,
                                                   const float* __restrict__ cosb, const float* __restrict__ sinb,
                                                   int inverse) {
  const int half = hd >> 1;
  const long long total = (long long)rows * nh * half;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int i = (int)(e % half);
    const long long rh = e / half;
    const int h = (int)(rh % nh);
    const long long m = rh / nh;
    const int t = (int)(m % T);
    T_* base = qkv + m * ld + (long long)h * hd;
    const float x1 = ld_act<T_>(base + i), x2 = ld_act<T_>(base + i + half);
    const float c = cosb[(long long)t * half + i], s = sinb[(long long)t * half + i];
    float y1, y2;
    if (!inverse) { y1 = x1 * c - x2 * s; y2 = x2 * c + x1 * s; }
    else          { y1 = x1 * c + x2 * s; y2 = x2 * c - x1 * s; }
    st_act<T_>(base + i, y1);
    st_act<T_>(base + i + half, y2);
  }
}

// Vectorised forms (8 consecutive elements per thread: 16-B bf16 / 2x16-B fp32 accesses, one
// 32-bit row division per 8 elements instead of 64-bit divisions per element) -- the scalar
// kernels above ran at 2.5-4 TB/s on C3 (d384, hd48), these are HBM-bound.  ld_vec<8> / st_vec<8>
// of common.h; 8-element runs are usable where every row start is 16-B aligned (cg_rows16) and
// the run length is a multiple of 8.

// rotate-half RoPE, one thread = 8 consecutive i of one (row, head) and their partners i + half
template <typename T_>
__global__ __launch_bounds__(256) void rope_vec_kernel(T_* __restrict__ qkv, long long ld, int rows, int T, int nh,
                                                       int hd, const float* __restrict__ cosb,
                                                       const float* __restrict__ sinb, int inverse) {
  const int half = hd >> 1, cph = half >> 3, cpr = nh * cph;
  const int total = rows * cpr;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int m = e / cpr, c = e - m * cpr;
    const int h = c / cph, i = 8 * (c - h * cph);
    const int t = m % T;
    T_* base = qkv + (long long)m * ld + (long long)h * hd;
    float x1[8], x2[8], cs[8], sn[8], y1[8], y2[8];
    ld_vec<8>(base + i, x1);
    ld_vec<8>(base + i + half, x2);
    ld_vec<8>(cosb + (long long)t * half + i, cs);
    ld_vec<8>(sinb + (long long)t * half + i, sn);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (!inverse) { y1[k] = x1[k] * cs[k] - x2[k] * sn[k]; y2[k] = x2[k] * cs[k] + x1[k] * sn[k]; }
      else          { y1[k] = x1[k] * cs[k] + x2[k] * sn[k]; y2[k] = x2[k] * cs[k] - x1[k] * sn[k]; }
    }
    st_vec<8>(base + i, y1);
    st_vec<8>(base + i + half, y2);
  }
}

extern "C" int cg_rope_tab(int dtype, void* qkv, long long ldqkv, int B, int T, int H, int KV, int hd,
                           const float* cos_tab, const float* sin_tab, int inverse, void* stream) {
  if (hd & 1) return CG_EUNSUPPORTED;
  const int rows = B * T, nh = H + KV;  // q heads then k heads are contiguous column blocks
  const long long total = (long long)rows * nh * (hd / 2);
  if (total == 0) return CG_OK;
  const int es = dtype == CG_BF16 ? 2 : 4;
  if ((hd / 2) % 8 == 0 && cg_rows16(qkv, ldqkv, es) && ((uintptr_t)cos_tab | (uintptr_t)sin_tab) % 16 == 0 &&
      total / 8 < (1LL << 31)) {
    int vb = (int)((total / 8 + 255) / 256);
    if (vb > 16384) vb = 16384;
    if (dtype == CG_BF16)
      hipLaunchKernelGGL(rope_vec_kernel<bf16_t>, dim3(vb), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, ldqkv,
                         rows, T, nh, hd, cos_tab, sin_tab, inverse);
    else
      hipLaunchKernelGGL(rope_vec_kernel<float>, dim3(vb), dim3(256), 0, (hipStream_t)stream, (float*)qkv, ldqkv,
                         rows, T, nh, hd, cos_tab, sin_tab, inverse);
    CG_LAUNCH_CHECK();
    return CG_OK;
  }
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(rope_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, ldqkv,
                       rows, T, nh, hd, cos_tab, sin_tab, inverse);
  else
    hipLaunchKernelGGL(rope_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)qkv, ldqkv,
                       rows, T, nh, hd, cos_tab, sin_tab, inverse);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// SwiGLU (model_tiny_gpt.py:47-57): s = silu(g) * u, gate at cols [0,H), up at [Hp,Hp+H)
// ===========================================================================
template <typename T_>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T_* __restrict__ gu, long long ldgu, int Hp,
                                                         T_* __restrict__ s, long long lds, int rows, int H) {
  const long long total = (long long)rows * Hp;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long m = e / Hp;
    const int j = (int)(e - m * Hp);
    float v = 0.f;
    if (j < H) {
      const float g = ld_act<T_>(gu + m * ldgu + j), u = ld_act<T_>(gu + m * ldgu + Hp + j);
      v = silu_f(g) * u;
    }
    st_act<T_>(s + m * lds + j, v);
  }
}
template <typename T_>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T_* __restrict__ gu, long long ldgu, int Hp,
                                                         const T_* __restrict__ ds, long long ldds,
                                                         T_* __restrict__ dgu, long long lddgu, int rows, int H) {
  const long long total = (long long)rows * Hp;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long m = e / Hp;
    const int j = (int)(e - m * Hp);
    float dg = 0.f, du = 0.f;
    if (j < H) {
      const float g = ld_act<T_>(gu + m * ldgu + j), u = ld_act<T_>(gu + m * ldgu + Hp + j);
      const float d = ld_act<T_>(ds + m * ldds + j);
      const float sg = 1.0f / (1.0f + __expf(-g));
      const float sl = g * sg;
      du = d * sl;
      dg = d * u * sg * (1.0f + g * (1.0f - sg));
    }
    st_act<T_>(dgu + m * lddgu + j, dg);
    st_act<T_>(dgu + m * lddgu + Hp + j, du);
  }
}

template <typename T_>
__global__ __launch_bounds__(256) void swiglu_fwd_vec_kernel(const T_* __restrict__ gu, long long ldgu, int Hp,
                                                             T_* __restrict__ s, long long lds, int rows, int H) {
  const int cpr = Hp >> 3, total = rows * cpr;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int m = e / cpr, j = 8 * (e - m * cpr);
    float g[8], u[8], v[8];
    ld_vec<8>(gu + (long long)m * ldgu + j, g);
    ld_vec<8>(gu + (long long)m * ldgu + Hp + j, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = j + k < H ? silu_f(g[k]) * u[k] : 0.f;
    st_vec<8>(s + (long long)m * lds + j, v);
  }
}
template <typename T_>
__global__ __launch_bounds__(256) void swiglu_bwd_vec_kernel(const T_* __restrict__ gu, long long ldgu, int Hp,
                                                             const T_* __restrict__ ds, long long ldds,
                                                             T_* __restrict__ dgu, long long lddgu, int rows, int H) {
  const int cpr = Hp >> 3, total = rows * cpr;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < total; e += gridDim.x * 256) {
    const int m = e / cpr, j = 8 * (e - m * cpr);
    float g[8], u[8], d[8], dg[8], du[8];
    ld_vec<8>(gu + (long long)m * ldgu + j, g);
    ld_vec<8>(gu + (long long)m * ldgu + Hp + j, u);
    ld_vec<8>(ds + (long long)m * ldds + j, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      dg[k] = du[k] = 0.f;
      if (j + k < H) {
        const float sg = 1.0f / (1.0f + __expf(-g[k]));
        const float sl = g[k] * sg;
        du[k] = d[k] * sl;
        dg[k] = d[k] * u[k] * sg * (1.0f + g[k] * (1.0f - sg));
      }
    }
    st_vec<8>(dgu + (long long)m * lddgu + j, dg);
    st_vec<8>(dgu + (long long)m * lddgu + Hp + j, du);
  }
}
static inline int vec_blocks(long long chunks) { return cg_grid_cap((chunks + 255) / 256, 16384); }

extern "C" int cg_swiglu_fwd(int dtype, const void* gu, long long ldgu, int Hp, void* s, long long lds, int rows,
                             int H, void* stream) {
  const long long total = (long long)rows * Hp;
  if (total == 0) return CG_OK;
  const int es = dtype == CG_BF16 ? 2 : 4;
  if (Hp % 8 == 0 && cg_rows16(gu, ldgu, es) && cg_rows16(s, lds, es) && total / 8 < (1LL << 31)) {
    if (dtype == CG_BF16)
      hipLaunchKernelGGL(swiglu_fwd_vec_kernel<bf16_t>, dim3(vec_blocks(total / 8)), dim3(256), 0,
                         (hipStream_t)stream, (const bf16_t*)gu, ldgu, Hp, (bf16_t*)s, lds, rows, H);
    else
      hipLaunchKernelGGL(swiglu_fwd_vec_kernel<float>, dim3(vec_blocks(total / 8)), dim3(256), 0,
                         (hipStream_t)stream, (const float*)gu, ldgu, Hp, (float*)s, lds, rows, H);
    CG_LAUNCH_CHECK();
    return CG_OK;
  }
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(swiglu_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)gu, ldgu, Hp, (bf16_t*)s, lds, rows, H);
  else
    hipLaunchKernelGGL(swiglu_fwd_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)gu,
                       ldgu, Hp, (float*)s, lds, rows, H);
  CG_LAUNCH_CHECK();
  return CG_OK;
}
extern "C" int cg_swiglu_bwd(int dtype, const void* gu, long long ldgu, int Hp, const void* ds, long long ldds,
                             void* dgu, long long lddgu, int rows, int H, void* stream) {
  const long long total = (long long)rows * Hp;
  if (total == 0) return CG_OK;
  const int es = dtype == CG_BF16 ? 2 : 4;
  if (Hp % 8 == 0 && cg_rows16(gu, ldgu, es) && cg_rows16(ds, ldds, es) && cg_rows16(dgu, lddgu, es) &&
      total / 8 < (1LL << 31)) {
    if (dtype == CG_BF16)
      hipLaunchKernelGGL(swiglu_bwd_vec_kernel<bf16_t>, dim3(vec_blocks(total / 8)), dim3(256), 0,
                         (hipStream_t)stream, (const bf16_t*)gu, ldgu, Hp, (const bf16_t*)ds, ldds, (bf16_t*)dgu,
                         lddgu, rows, H);
    else
      hipLaunchKernelGGL(swiglu_bwd_vec_kernel<float>, dim3(vec_blocks(total / 8)), dim3(256), 0,
                         (hipStream_t)stream, (const float*)gu, ldgu, Hp, (const float*)ds, ldds, (float*)dgu, lddgu,
                         rows, H);
    CG_LAUNCH_CHECK();
    return CG_OK;
  }
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(swiglu_bwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)gu, ldgu, Hp, (const bf16_t*)ds, ldds, (bf16_t*)dgu, lddgu, rows, H);
  else
    hipLaunchKernelGGL(swiglu_bwd_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)gu,
                       ldgu, Hp, (const float*)ds, ldds, (float*)dgu, lddgu, rows, H);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Column sums for bias gradients: out[n] (+)= sum_m X[m, n]
// ===========================================================================
constexpr int COLSUM_R = 64;
extern "C" size_t cg_colsum_workspace(int rows, int cols) {
  (void)rows;
  const int nrb = rows > 0 ? (rows + 127) / 128 : 1;  // colsum_vec_kernel's 128-row blocks
  return (size_t)(nrb > COLSUM_R ? nrb : COLSUM_R) * cols * sizeof(float);
}
template <typename T_>
__global__ __launch_bounds__(256) void colsum_part_kernel(const T_* __restrict__ X, long long ldx, int rows, int cols,
                                                          float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  const int per = (rows + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * per, r1 = min(rows, r0 + per);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += ld_act<T_>(X + (long long)r * ldx + c);
  part[(long long)blockIdx.y * cols + c] = s;
}
// out[c] (+)= sum_i part[i][c]: 32 columns x 8 row lanes per block (fixed summation order)
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ part, int nch, int cols,
                                                            float* __restrict__ out, int accumulate) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < cols) {   // four independent chains keep 4 loads in flight per lane
    float s4[4] = {0.f, 0.f, 0.f, 0.f};
    int i = rl;
    for (; i + 24 < nch; i += 32)
#pragma unroll
      for (int u = 0; u < 4; ++u) s4[u] += part[(long long)(i + 8 * u) * cols + c];
    for (; i < nch; i += 8) s4[0] += part[(long long)i * cols + c];
    s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) v += red[i][cl];
    out[c] = accumulate ? out[c] + v : v;
  }
}
extern "C" int cg_colsum_reduce(const float* part, int nparts, int cols, float* out, int accumulate, void* stream) {
  if (cols <= 0) return CG_OK;
  if (!part || !out || nparts < 0) return CG_EINVAL;
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3(cg_cdiv(cols, 32)), dim3(256), 0, (hipStream_t)stream, part, nparts,
                     cols, out, accumulate);
  CG_LAUNCH_CHECK();
  return CG_OK;
}
// Fast path: 8 columns (one 16-B bf16 chunk / two float4) per thread, 32 column chunks x
// 8 row lanes per 256-thread block, COLSUM_RB rows per block; partial rows reduced by
// colsum_reduce_kernel.
// 128-row x 128-column blocks: 16 column chunks of 8 x 16 row lanes (C5's d = 384 bias sums ran
// as 64 workgroups of 512 rows x 256 columns, half of them half empty)
constexpr int COLSUM_RB = 128;
template <typename T_>
__global__ __launch_bounds__(256) void colsum_vec_kernel(const T_* __restrict__ X, long long ldx, int rows, int cols,
                                                         float* __restrict__ part) {
  __shared__ float red[16][128 + 4];
  const int ch = threadIdx.x & 15, rs = threadIdx.x >> 4;
  const int c0 = blockIdx.x * 128 + ch * 8;
  const int r0 = blockIdx.y * COLSUM_RB;
  const int r1 = min(rows, r0 + COLSUM_RB);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (c0 < cols) {
#pragma unroll 4
    for (int r = r0 + rs; r < r1; r += 16) {
      const T_* p = X + (long long)r * ldx + c0;
      if (sizeof(T_) == 2) {
        const uint4 u = *(const uint4*)p;
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[2 * j] += __uint_as_float(w[j] << 16);
          acc[2 * j + 1] += __uint_as_float(w[j] & 0xFFFF0000u);
        }
      } else {
        const float4 a = *(const float4*)p, b = *(const float4*)((const float*)p + 4);
        acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
        acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[rs][ch * 8 + j] = acc[j];
  __syncthreads();
  if (threadIdx.x < 128) {  // one output column per thread, fixed order
    const int c = threadIdx.x;
    if (blockIdx.x * 128 + c < cols) {
      float v = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) v += red[i][c];
      part[(long long)blockIdx.y * cols + blockIdx.x * 128 + c] = v;
    }
  }
}

static inline bool colsum_vec_ok(const void* X, long long ldx, int cols) {
  return cols % 8 == 0 && ldx % 8 == 0 && ((uintptr_t)X & 15) == 0;
}

extern "C" int cg_colsum_partials(int dtype, const void* X, long long ldx, int rows, int cols, float* part,
                                  size_t part_bytes, int* nparts, void* stream) {
  if (!nparts || (cols > 0 && (!X || !part))) return CG_EINVAL;
  *nparts = 0;
  if (cols <= 0 || rows <= 0) return CG_OK;
  if (part_bytes < cg_colsum_workspace(rows, cols)) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (colsum_vec_ok(X, ldx, cols)) {
    const int nrb = cg_cdiv(rows, COLSUM_RB);
    dim3 g(cg_cdiv(cols, 128), nrb);
    if (dtype == CG_BF16)
      hipLaunchKernelGGL(colsum_vec_kernel<bf16_t>, g, dim3(256), 0, s, (const bf16_t*)X, ldx, rows, cols, part);
    else
      hipLaunchKernelGGL(colsum_vec_kernel<float>, g, dim3(256), 0, s, (const float*)X, ldx, rows, cols, part);
    *nparts = nrb;
  } else {
    const int nch = rows < COLSUM_R ? rows : COLSUM_R;
    dim3 g(cg_cdiv(cols, 256), nch);
    if (dtype == CG_BF16)
      hipLaunchKernelGGL(colsum_part_kernel<bf16_t>, g, dim3(256), 0, s, (const bf16_t*)X, ldx, rows, cols, part);
    else
      hipLaunchKernelGGL(colsum_part_kernel<float>, g, dim3(256), 0, s, (const float*)X, ldx, rows, cols, part);
    *nparts = nch;
  }
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_colsum(int dtype, const void* X, long long ldx, int rows, int cols, float* out, int accumulate,
                         void* ws, size_t ws_bytes, void* stream) {
  if (cols == 0) return CG_OK;
  int np = 0;
  const int rc = cg_colsum_partials(dtype, X, ldx, rows > 0 ? rows : 0, cols, (float*)ws, ws_bytes, &np, stream);
  if (rc != CG_OK) return rc;
  if (np == 0) {  // no rows: the sum is 0
    if (!accumulate && hipMemsetAsync(out, 0, (size_t)cols * 4, (hipStream_t)stream) != hipSuccess) return CG_ELAUNCH;
    return CG_OK;
  }
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3(cg_cdiv(cols, 32)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, np, cols, out, accumulate);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Cross-entropy: label smoothing + class weights + ignore_index (F.cross_entropy,
// model_tiny_gpt.py:343-349). L = sum_valid[(1-e) w_y nll_y + e/V sum_c w_c nll_c] / sum_valid w_y
// ===========================================================================
constexpr int CE_BLK = 4096;  // rows per block = 4 waves x 1 row, grid-strided beyond 16384 rows
// sum_valid w_y: 1024 threads, 4 independent sums each, fixed-order tree.  16 rows per thread and
// round: all 16 targets are loaded before any class-weight gather (two load latencies per round
// instead of eight dependent pairs: C4's 16384 rows took 10.5 us in 4-row rounds)
__global__ __launch_bounds__(1024) void ce_denom_kernel(const int64_t* __restrict__ tg, int rows, const float* __restrict__ w,
                                                        int ignore, float* __restrict__ ws) {
  __shared__ float red[1024];
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  int r = threadIdx.x;
  for (; r + 15 * 1024 < rows; r += 16 * 1024) {
    int64_t t[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) t[u] = tg[r + 1024 * u];
    float wt[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) wt[u] = t[u] == ignore ? 0.f : (w ? w[t[u]] : 1.0f);
#pragma unroll
    for (int u = 0; u < 16; ++u) s4[u & 3] += wt[u];
  }
  for (; r + 3072 < rows; r += 4096)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t t = tg[r + 1024 * u];
      if (t != ignore) s4[u] += w ? w[t] : 1.0f;
    }
  for (; r < rows; r += 1024) {
    const int64_t t = tg[r];
    if (t != ignore) s4[0] += w ? w[t] : 1.0f;
  }
  block_sum_1024((s4[0] + s4[1]) + (s4[2] + s4[3]), red);
  if (threadIdx.x == 0) ws[0] = red[0];
}

// (dlogits element layouts: st_grad of common.h)
template <typename TD, bool SPLIT = false>
__global__ __launch_bounds__(256) void ce_main_kernel(const float* __restrict__ logits, long long ldl,
                                                      const int64_t* __restrict__ tg, int rows, int V, float eps,
                                                      const float* __restrict__ w, int ignore, float grad_scale,
                                                      TD* __restrict__ dl, long long ldd, float* __restrict__ ws) {
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float denom = ws[0];
  const float inv = grad_scale / denom;
  float acc = 0.f;
  // total class weight W
  float Wt = 0.f;
  for (int c = lane; c < V; c += 64) Wt += w ? w[c] : 1.0f;
  Wt = wave_sum(Wt);
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const float* z = logits + (long long)row * ldl;
    const int64_t t = tg[row];
    const bool valid = (t != ignore);
    float z0 = lane < V ? z[lane] : -INFINITY;
    float z1 = (lane + 64) < V ? z[lane + 64] : -INFINITY;
    const float mx = wave_max(fmaxf(z0, z1));
    float e0 = lane < V ? __expf(z0 - mx) : 0.f;
    float e1 = (lane + 64) < V ? __expf(z1 - mx) : 0.f;
    const float se = wave_sum(e0 + e1);
    const float lse = mx + __logf(se);
    TD* dr = dl ? dl + (long long)row * ldd : nullptr;
    const long long half = SPLIT ? ldd / 2 : ldd;
    if (valid) {
      const float wy = w ? w[t] : 1.0f;
      // smoothing term sum_c w_c (lse - z_c)
      float sm = 0.f;
      if (lane < V) sm += (w ? w[lane] : 1.f) * (lse - z0);
      if (lane + 64 < V) sm += (w ? w[lane + 64] : 1.f) * (lse - z1);
      sm = wave_sum(sm);
      const float zy = z[t];
      acc += (1.0f - eps) * wy * (lse - zy) + (eps / (float)V) * sm;
      if (dr) {
        const float rse = 1.0f / se;
        for (int k = 0; k < 2; ++k) {
          const int c = lane + 64 * k;
          if (c < V) {
            const float p = (k == 0 ? e0 : e1) * rse;
            const float wc = w ? w[c] : 1.f;
            float g = (1.0f - eps) * wy * (p - (c == t ? 1.f : 0.f)) + (eps / (float)V) * (Wt * p - wc);
            st_grad<TD, SPLIT>(dr, c, half, g * inv);
          }
        }
      }
    } else if (dr) {
      for (int c = lane; c < V; c += 64) st_grad<TD, SPLIT>(dr, c, half, 0.f);
    }
    if (dr)
      for (int c = V + lane; c < half; c += 64) st_grad<TD, SPLIT>(dr, c, half, 0.f);
  }
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[1 + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// loss = sum of the per-block partials (fixed-order tree) / denominator
__global__ __launch_bounds__(1024) void ce_final_kernel(const float* __restrict__ ws, int nblk, float* __restrict__ loss) {
  __shared__ float red[1024];
  float s = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 1024) s += ws[1 + b];
  block_sum_1024(s, red);
  if (threadIdx.x == 0) *loss = red[0] / ws[0];
}

static int ce_blocks(int rows) { return cg_grid_cap(cg_cdiv(rows, 4), CE_BLK); }
extern "C" size_t cg_ce_workspace(int rows) { return (size_t)(1 + ce_blocks(rows)) * sizeof(float); }

extern "C" int cg_cross_entropy(const float* logits, long long ldl, const int64_t* targets, int rows, int V,
                                float eps, const float* class_w, int ignore_index, float grad_scale, int d_dtype,
                                void* dlogits, long long ldd, float* loss, void* ws, size_t ws_bytes,
                                void* stream) {
  if (V > 128 || V <= 0) return CG_EUNSUPPORTED;
  if (!ws || ws_bytes < cg_ce_workspace(rows)) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = ce_blocks(rows);
  hipLaunchKernelGGL(ce_denom_kernel, dim3(1), dim3(1024), 0, s, targets, rows, class_w, ignore_index, (float*)ws);
  CG_LAUNCH_CHECK();
  if (d_dtype == CG_BF16X2 && (ldd & 1 || ldd / 2 < V)) return CG_EINVAL;
  if (d_dtype == CG_BF16)
    hipLaunchKernelGGL(ce_main_kernel<bf16_t>, dim3(nblk), dim3(256), 0, s, logits, ldl, targets, rows, V, eps,
                       class_w, ignore_index, grad_scale, (bf16_t*)dlogits, ldd, (float*)ws);
  else if (d_dtype == CG_BF16X2)
    hipLaunchKernelGGL((ce_main_kernel<bf16_t, true>), dim3(nblk), dim3(256), 0, s, logits, ldl, targets, rows, V,
                       eps, class_w, ignore_index, grad_scale, (bf16_t*)dlogits, ldd, (float*)ws);
  else
    hipLaunchKernelGGL(ce_main_kernel<float>, dim3(nblk), dim3(256), 0, s, logits, ldl, targets, rows, V, eps,
                       class_w, ignore_index, grad_scale, (float*)dlogits, ldd, (float*)ws);
  CG_LAUNCH_CHECK();
  if (loss) {
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(1024), 0, s, (const float*)ws, nblk, loss);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

// ===========================================================================
// AdamW over the flat parameter buffer (torch.optim.AdamW, loop.py:681-731)
// ===========================================================================
struct AdamSegs { long long begin[4], end[4]; float lr[4], wd[4]; int n; };

__device__ __forceinline__ void adamw_elem(float& pi, float gi, float& mi, float& vi, float lr, float wd, float b1,
                                           float b2, float eps, float step_size, float bc2_sqrt) {
  pi = pi * (1.0f - lr * wd);
  mi = b1 * mi + (1.0f - b1) * gi;
  vi = b2 * vi + (1.0f - b2) * gi * gi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  pi = pi - step_size * (mi / denom);
}
// 16-B loads / stores over each segment's 4-aligned interior (the scalar form moved 30 B per
// parameter in 4-B accesses), the unaligned head / tail elementwise; same arithmetic per element
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ shadow, AdamSegs segs, float b1, float b2,
                                                    float eps, float bc1, float bc2_sqrt, float gscale, int vec) {
  const long long tid = blockIdx.x * 256ll + threadIdx.x, nth = (long long)gridDim.x * 256;
  for (int si = 0; si < segs.n; ++si) {
    const long long b = segs.begin[si], e = segs.end[si];
    const float lr = segs.lr[si], wd = segs.wd[si];
    const float step_size = lr / bc1;
    const long long a0 = (b + 3) & ~3ll, a1 = e & ~3ll;
    auto one = [&](long long i) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_elem(pi, g[i] * gscale, mi, vi, lr, wd, b1, b2, eps, step_size, bc2_sqrt);
      m[i] = mi;
      v[i] = vi;
      p[i] = pi;
      if (shadow) shadow[i] = f2bf(pi);
    };
    if (!vec || a0 >= a1) {  // !vec: a base pointer the 16-B (shadow: 8-B) accesses cannot use
      for (long long i = b + tid; i < e; i += nth) one(i);
      continue;
    }
    if (tid < a0 - b) one(b + tid);
    if (tid < e - a1) one(a1 + tid);
    for (long long q = a0 / 4 + tid; q < a1 / 4; q += nth) {
      float4 pv = ((const float4*)p)[q], mv = ((const float4*)m)[q], vv = ((const float4*)v)[q];
      const float4 gv = ((const float4*)g)[q];
      adamw_elem(pv.x, gv.x * gscale, mv.x, vv.x, lr, wd, b1, b2, eps, step_size, bc2_sqrt);
      adamw_elem(pv.y, gv.y * gscale, mv.y, vv.y, lr, wd, b1, b2, eps, step_size, bc2_sqrt);
      adamw_elem(pv.z, gv.z * gscale, mv.z, vv.z, lr, wd, b1, b2, eps, step_size, bc2_sqrt);
      adamw_elem(pv.w, gv.w * gscale, mv.w, vv.w, lr, wd, b1, b2, eps, step_size, bc2_sqrt);
      ((float4*)m)[q] = mv;
      ((float4*)v)[q] = vv;
      ((float4*)p)[q] = pv;
      if (shadow)
        ((uint2*)shadow)[q] = make_uint2((uint32_t)f2bf(pv.x) | ((uint32_t)f2bf(pv.y) << 16),
                                         (uint32_t)f2bf(pv.z) | ((uint32_t)f2bf(pv.w) << 16));
    }
  }
}

extern "C" int cg_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, uint16_t* shadow_bf16,
                        const cg_adamw_segment* segs, int nseg, float beta1, float beta2, float eps, int step,
                        float grad_scale, void* stream) {
  if (nseg < 1 || nseg > 4 || step < 1) return CG_EINVAL;
  AdamSegs s{};
  long long total = 0;
  for (int i = 0; i < nseg; ++i) {
    s.begin[i] = segs[i].begin; s.end[i] = segs[i].end; s.lr[i] = segs[i].lr; s.wd[i] = segs[i].wd;
    total += segs[i].end - segs[i].begin;
  }
  s.n = nseg;
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  // the float4 / packed-bf16 interior needs 16-B aligned fp32 bases and an 8-B aligned shadow
  // (the engine's flat buffers are; an offset view through the C ABI may not be)
  auto al = [](const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; };
  const int vec = al(param, 16) && al(grad, 16) && al(exp_avg, 16) && al(exp_avg_sq, 16) &&
                  (!shadow_bf16 || al(shadow_bf16, 8));
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                     (bf16_t*)shadow_bf16, s, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale, vec);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

__global__ void nonfinite_kernel(const float* __restrict__ x, long long n, int* __restrict__ flag) {
  int bad = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    bad |= !isfinite(x[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
extern "C" int cg_nonfinite_flag(const float* x, long long n, int* flag, void* stream) {
  if (n <= 0) return CG_OK;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(nonfinite_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, n, flag);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// casts
// ===========================================================================
__global__ void cast_f2b_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, long long n) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) d[i] = f2bf(s[i]);
}
__global__ void cast_b2f_kernel(const bf16_t* __restrict__ s, float* __restrict__ d, long long n) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) d[i] = bf2f(s[i]);
}
extern "C" int cg_cast_f32_to_bf16(const float* src, uint16_t* dst, long long n, void* stream) {
  if (n <= 0) return CG_OK;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cast_f2b_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
  CG_LAUNCH_CHECK();
  return CG_OK;
}
extern "C" int cg_cast_bf16_to_f32(const uint16_t* src, float* dst, long long n, void* stream) {
  if (n <= 0) return CG_OK;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cast_b2f_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, dst, n);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// x[r][c] *= *s for a gradient buffer (dtype F32 / BF16 / BF16X2 split pairs, ld in elements;
// BF16X2 rows hold hi in [0, ld/2) and lo in [ld/2, ld)).  The scale is read on the device (the
// autograd output gradient d(objective)/d(loss)), so no host synchronisation is needed; a
// scale of exactly 1 returns at once.
__global__ __launch_bounds__(256) void scale_dev_kernel(int dtype, void* __restrict__ x, long long ld, int rows,
                                                        int cols, const float* __restrict__ sp) {
  const float sc = *sp;
  if (sc == 1.0f) return;
  const long long total = (long long)rows * cols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / cols;
    const int c = (int)(i - r * cols);
    if (dtype == CG_F32) {
      float* p = (float*)x + r * ld + c;
      *p *= sc;
    } else if (dtype == CG_BF16) {
      bf16_t* p = (bf16_t*)x + r * ld + c;
      *p = f2bf(bf2f(*p) * sc);
    } else {
      bf16_t* p = (bf16_t*)x + r * ld;
      const float v = (bf2f(p[c]) + bf2f(p[ld / 2 + c])) * sc;
      st_grad<bf16_t, true>(p, c, ld / 2, v);
    }
  }
}
extern "C" int cg_scale_dev(int dtype, void* x, long long ld, int rows, int cols, const float* scale, void* stream) {
  if (!x || !scale || rows < 0 || cols < 0) return CG_EINVAL;
  if (dtype != CG_F32 && dtype != CG_BF16 && dtype != CG_BF16X2) return CG_EINVAL;
  if (ld < (dtype == CG_BF16X2 ? 2LL * cols : cols)) return CG_EINVAL;
  const long long total = (long long)rows * cols;
  if (!total) return CG_OK;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_dev_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dtype, x, ld, rows, cols, scale);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// fp32 [rows][cols] -> dtype [rows][dcols] with zero pad columns (aux-head logit grads into
// the padded GEMM operand layout)
template <typename T_, bool SPLIT = false>
__global__ __launch_bounds__(256) void cast_pad_kernel(const float* __restrict__ src, long long lds, int rows, int cols,
                                                       T_* __restrict__ dst, long long ldd, int dcols) {
  const long long total = (long long)rows * dcols;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / dcols;
    const int c = (int)(i - r * dcols);
    st_grad<T_, SPLIT>(dst + r * ldd, c, dcols, c < cols ? src[r * lds + c] : 0.f);
  }
}
extern "C" int cg_cast_pad_2d(const float* src, long long lds, int rows, int cols, int dtype, void* dst, long long ldd,
                              int dcols, void* stream) {
  if (rows < 0 || cols < 0 || dcols < cols || lds < cols || ldd < (dtype == CG_BF16X2 ? 2 * dcols : dcols))
    return CG_EINVAL;
  const long long total = (long long)rows * dcols;
  if (total == 0) return CG_OK;
  if (!src || !dst) return CG_EINVAL;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(cast_pad_kernel<bf16_t>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, lds, rows, cols,
                       (bf16_t*)dst, ldd, dcols);
  else if (dtype == CG_BF16X2)
    hipLaunchKernelGGL((cast_pad_kernel<bf16_t, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, lds, rows,
                       cols, (bf16_t*)dst, ldd, dcols);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(cast_pad_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, lds, rows, cols,
                       (float*)dst, ldd, dcols);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Device-resident codon batches (src/codonlm/data_loading.py PackedDataset :43-129 and
// dynamic_lm_collate_fn :380-393): token rows gathered from HBM by sample index, widened to
// int64 and (dynamic layout) shifted into x = seq[:-1], y = seq[1:] with a PAD tail.
// Out-of-range sample indices produce PAD rows instead of faulting.
// ===========================================================================
template <typename T_>
__global__ __launch_bounds__(256) void gather_windows_kernel(const T_* __restrict__ X, long long ldx, long long nrows,
                                                             const int64_t* __restrict__ rows, int B, int T,
                                                             int64_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * T) return;
  const int b = (int)(i / T), t = (int)(i - (long long)b * T);
  const int64_t r = rows[b];
  out[i] = (r >= 0 && r < nrows) ? (int64_t)X[r * ldx + t] : 0;
}
extern "C" int cg_gather_windows(int elem_bytes, const void* X, long long ldx, long long nrows, const int64_t* rows,
                                 int B, int T, int64_t* out, void* stream) {
  if (B < 0 || T < 0 || ldx < T || nrows < 0) return CG_EINVAL;
  const long long total = (long long)B * T;
  if (total == 0) return CG_OK;
  if (!X || !rows || !out) return CG_EINVAL;
  const dim3 g((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(gather_windows_kernel<uint8_t>, g, dim3(256), 0, s, (const uint8_t*)X, ldx, nrows, rows, B, T, out); break;
    case 2: hipLaunchKernelGGL(gather_windows_kernel<int16_t>, g, dim3(256), 0, s, (const int16_t*)X, ldx, nrows, rows, B, T, out); break;
    case 4: hipLaunchKernelGGL(gather_windows_kernel<int32_t>, g, dim3(256), 0, s, (const int32_t*)X, ldx, nrows, rows, B, T, out); break;
    case 8: hipLaunchKernelGGL(gather_windows_kernel<int64_t>, g, dim3(256), 0, s, (const int64_t*)X, ldx, nrows, rows, B, T, out); break;
    default: return CG_EUNSUPPORTED;
  }
  CG_LAUNCH_CHECK();
  return CG_OK;
}
template <typename T_>
__global__ __launch_bounds__(256) void gather_sequences_kernel(const T_* __restrict__ flat,
                                                               const int64_t* __restrict__ starts,
                                                               const int64_t* __restrict__ lens, long long nseq,
                                                               const int64_t* __restrict__ rows, int B, int Tout,
                                                               int64_t* __restrict__ x, int64_t* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * Tout) return;
  const int b = (int)(i / Tout), t = (int)(i - (long long)b * Tout);
  const int64_t r = rows[b];
  int64_t xv = 0, yv = 0;
  if (r >= 0 && r < nseq && t + 1 < lens[r]) {
    const T_* s = flat + starts[r];
    xv = (int64_t)s[t];
    yv = (int64_t)s[t + 1];
  }
  x[i] = xv;
  y[i] = yv;
}
extern "C" int cg_gather_sequences(int elem_bytes, const void* flat, const int64_t* starts, const int64_t* lens,
                                   long long nseq, const int64_t* rows, int B, int Tout, int64_t* x, int64_t* y,
                                   void* stream) {
  if (B < 0 || Tout < 0 || nseq < 0) return CG_EINVAL;
  const long long total = (long long)B * Tout;
  if (total == 0) return CG_OK;
  if (!flat || !starts || !lens || !rows || !x || !y) return CG_EINVAL;
  const dim3 g((unsigned)((total + 255) / 256));
  hipStream_t s = (hipStream_t)stream;
  switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(gather_sequences_kernel<uint8_t>, g, dim3(256), 0, s, (const uint8_t*)flat, starts, lens, nseq, rows, B, Tout, x, y); break;
    case 2: hipLaunchKernelGGL(gather_sequences_kernel<int16_t>, g, dim3(256), 0, s, (const int16_t*)flat, starts, lens, nseq, rows, B, Tout, x, y); break;
    case 4: hipLaunchKernelGGL(gather_sequences_kernel<int32_t>, g, dim3(256), 0, s, (const int32_t*)flat, starts, lens, nseq, rows, B, Tout, x, y); break;
    case 8: hipLaunchKernelGGL(gather_sequences_kernel<int64_t>, g, dim3(256), 0, s, (const int64_t*)flat, starts, lens, nseq, rows, B, Tout, x, y); break;
    default: return CG_EUNSUPPORTED;
  }
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Sequence pooling of hidden states (scripts/extract_embeddings.py _pool_state :94-114):
// mode 0 mean over non-PAD positions, 1 mean over content-token positions (id bitmask),
// 2 state at position (#non-PAD - 1).  One thread per (sequence, feature); the token ids of a
// row are read once per wave from L1/L2, the states coalesced along the feature axis.
// ===========================================================================
template <typename T_>
__global__ __launch_bounds__(256) void pool_hidden_kernel(const T_* __restrict__ h, long long ldh,
                                                          const int64_t* __restrict__ idx, int T, int d, int pad,
                                                          int mode, cg_id_mask cm, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= d) return;
  const int64_t* row = idx + (long long)b * T;
  const T_* hb = h + (long long)b * T * ldh + c;
  if (mode == 2) {
    int n = 0;
    for (int t = 0; t < T; ++t) n += row[t] != pad;
    const int pos = n > 0 ? n - 1 : 0;
    out[(long long)b * d + c] = ld_act<T_>(hb + (long long)pos * ldh);
    return;
  }
  float s = 0.f, cnt = 0.f;
  for (int t = 0; t < T; ++t) {
    const int64_t v = row[t];
    if (mode == 0 ? v != pad : cg_mask_has(cm, v)) {
      s += ld_act<T_>(hb + (long long)t * ldh);
      cnt += 1.f;
    }
  }
  out[(long long)b * d + c] = s / fmaxf(cnt, 1.f);
}
extern "C" int cg_pool_hidden(int dtype, const void* h, long long ldh, const int64_t* idx, int B, int T, int d,
                              int pad_id, int mode, const uint32_t* content_mask, float* out, void* stream) {
  if (B < 0 || T < 0 || d < 0 || ldh < d || mode < 0 || mode > 2) return CG_EINVAL;
  if ((long long)B * d == 0) return CG_OK;
  if (!h || !idx || !out || (mode == 1 && !content_mask)) return CG_EINVAL;
  cg_id_mask cm = {};
  cg_mask_fill(cm, content_mask);  // NULL (modes 0 and 2 never read it): the empty set
  const dim3 g(cg_cdiv(d, 256), B);
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(pool_hidden_kernel<bf16_t>, g, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h, ldh, idx, T,
                       d, pad_id, mode, cm, out);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(pool_hidden_kernel<float>, g, dim3(256), 0, (hipStream_t)stream, (const float*)h, ldh, idx, T, d,
                       pad_id, mode, cm, out);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Auxiliary objectives' labels (src/codonlm/training/objectives.py): integer work, one
// thread per (b, t), ids passed by value.
// ===========================================================================
struct IdSet {
  int n;
  int id[8];
};
__device__ __forceinline__ bool in_set(const IdSet& s, int64_t v) {
  bool r = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) r |= (i < s.n) && (v == (int64_t)s.id[i]);
  return r;
}
static bool make_set(const int* ids, int n, IdSet& s) {
  if (n < 0 || n > 8 || (n > 0 && !ids)) return false;
  s.n = n;
  for (int i = 0; i < 8; ++i) s.id[i] = i < n ? ids[i] : 0;
  return true;
}
// offset_target_mask (objectives.py:6-23): target y[t+k-1] is valid when it exists, is not PAD
// and no boundary id occurs in y[t .. t+k-2]; invalid targets become PAD (ignored by the CE)
__global__ __launch_bounds__(256) void offset_targets_kernel(const int64_t* __restrict__ y, int B, int T, int k,
                                                             IdSet bnd, int64_t* __restrict__ out,
                                                             int* __restrict__ nvalid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int v = 0;
  if (i < (long long)B * T) {
    const long long b = i / T;
    const int t = (int)(i - b * T);
    const int64_t* row = y + b * T;
    int64_t tgt = 0;
    if (t + k - 1 < T) {
      tgt = row[t + k - 1];
      bool ok = tgt != 0;
      for (int s = 0; s < k - 1 && ok; ++s) ok = !in_set(bnd, row[t + s]);
      if (!ok) tgt = 0;
    }
    out[i] = tgt;
    v = tgt != 0;
  }
  if (nvalid) {  // uniform branch: every lane reaches the ballot
    const unsigned long long bal = __ballot(v);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(nvalid, (int)__popcll(bal));
  }
}
extern "C" int cg_offset_targets(const int64_t* y, int B, int T, int offset, const int* boundary_ids, int n_boundary,
                                 int64_t* out, int* n_valid, void* stream) {
  IdSet bnd;
  if (B < 0 || T < 0 || offset < 1 || !make_set(boundary_ids, n_boundary, bnd)) return CG_EINVAL;
  const long long total = (long long)B * T;
  if (total == 0) return CG_OK;
  if (!y || !out) return CG_EINVAL;
  hipLaunchKernelGGL(offset_targets_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y,
                     B, T, offset, bnd, out, n_valid);
  CG_LAUNCH_CHECK();
  return CG_OK;
}
// termination_distance_bucket_labels (objectives.py:63-91): distance to the next stop id at or
// after t, bucketed as #(edges < distance); no later stop -> n_edges; PAD -> ignore_index.
// One workgroup per row: each thread owns a contiguous chunk, a suffix-min over the chunks'
// first stop positions gives every chunk its next stop, then a reverse sweep inside the chunk.
__global__ __launch_bounds__(256) void termination_labels_kernel(const int64_t* __restrict__ y, int T, IdSet stops,
                                                                 IdSet edges, int ignore, int64_t* __restrict__ lab) {
  __shared__ int sfx[257];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const int64_t* row = y + b * T;
  int64_t* out = lab + b * T;
  const int per = (T + 255) / 256;
  const int t0 = min(T, tid * per), t1 = min(T, t0 + per);
  int first = T;
  for (int t = t0; t < t1; ++t)
    if (in_set(stops, row[t])) {
      first = t;
      break;
    }
  sfx[tid] = first;
  if (tid == 0) sfx[256] = T;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive suffix minimum
    const int v = tid + o < 256 ? sfx[tid + o] : T;
    __syncthreads();
    sfx[tid] = min(sfx[tid], v);
    __syncthreads();
  }
  int nxt = sfx[tid + 1];
  for (int t = t1 - 1; t >= t0; --t) {
    const int64_t v = row[t];
    if (in_set(stops, v)) nxt = t;
    int64_t o;
    if (v == 0) {
      o = ignore;
    } else if (nxt == T) {
      o = edges.n;
    } else {
      const int dist = nxt - t;
      int c = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) c += (e < edges.n) && (dist > edges.id[e]);
      o = c;
    }
    out[t] = o;
  }
}
extern "C" int cg_termination_labels(const int64_t* y, int B, int T, const int* stop_ids, int n_stop, const int* edges,
                                     int n_edges, int ignore_index, int64_t* labels, void* stream) {
  IdSet st, ed;
  if (B < 0 || T < 0 || n_stop < 1 || !make_set(stop_ids, n_stop, st) || !make_set(edges, n_edges, ed))
    return CG_EINVAL;
  for (int e = 1; e < n_edges; ++e)
    if (edges[e] < edges[e - 1]) return CG_EINVAL;
  const long long total = (long long)B * T;
  if (total == 0) return CG_OK;
  if (!y || !labels) return CG_EINVAL;
  hipLaunchKernelGGL(termination_labels_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, y, T, st, ed,
                     ignore_index, labels);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// Batched 2-byte transpose (bf16 weight matrices -> K-contiguous operands for the
// backward dX products, so they run on the LDS-DMA tile).  64x64 tiles through LDS,
// 16-B global accesses on both sides.
// ===========================================================================
__global__ __launch_bounds__(256) void transpose16_kernel(cg_transpose_batch tb) {
  __shared__ uint16_t tile[64][64 + 8];
  const cg_transpose_item& it = tb.items[blockIdx.y];
  const int tc = (it.cols + 63) >> 6, tr = (it.rows + 63) >> 6;
  const int tid = threadIdx.x;
  for (int t = blockIdx.x; t < tc * tr; t += gridDim.x) {
    const int r0 = (t / tc) * 64, c0 = (t % tc) * 64;
    const uint16_t* src = (const uint16_t*)it.src;
    uint16_t* dst = (uint16_t*)it.dst;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i, r = e >> 3, c = (e & 7) * 8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r0 + r < it.rows && c0 + c < it.cols) v = *(const uint4*)(src + (long long)(r0 + r) * it.lds + c0 + c);
      const uint16_t* pv = (const uint16_t*)&v;
#pragma unroll
      for (int j = 0; j < 8; ++j) tile[r][c + j] = pv[j];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i, c = e >> 3, r = (e & 7) * 8;  // dst row = source column
      if (c0 + c < it.cols && r0 + r < it.rows) {
        uint16_t w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = tile[r + j][c];
        *(uint4*)(dst + (long long)(c0 + c) * it.ldd + r0 + r) = *(const uint4*)w;
      }
    }
    __syncthreads();
  }
}

extern "C" int cg_transpose16_batch(const cg_transpose_batch* tb, void* stream) {
  if (!tb || tb->n < 0 || tb->n > CG_TRANSPOSE_MAX) return CG_EINVAL;
  if (tb->n == 0) return CG_OK;
  int maxt = 0;
  for (int i = 0; i < tb->n; ++i) {
    const cg_transpose_item& it = tb->items[i];
    if (it.rows < 0 || it.cols < 0 || !it.src || !it.dst) return CG_EINVAL;
    if ((it.rows & 7) || (it.cols & 7) || (it.lds & 7) || (it.ldd & 7)) return CG_EUNSUPPORTED;
    if (((uintptr_t)it.src & 15) || ((uintptr_t)it.dst & 15)) return CG_EUNSUPPORTED;
    maxt = std::max(maxt, cg_cdiv(it.rows, 64) * cg_cdiv(it.cols, 64));
  }
  hipLaunchKernelGGL(transpose16_kernel, dim3(std::min(maxt, 1024), tb->n), dim3(256), 0, (hipStream_t)stream, *tb);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// diagnostic CU occupier (cg_diag_occupy): each workgroup takes a whole CU (all of its LDS) and
// sleeps until the deadline on the 100 MHz real-time counter; every wave reaches the exit.
// ===========================================================================
__global__ __launch_bounds__(1024) void diag_occupy_kernel(long long ticks) {
  extern __shared__ char hold[];
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) hold[0] = 0;
  while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

extern "C" int cg_diag_occupy(int n_cus, int usec, void* stream) {
  if (n_cus <= 0 || usec <= 0) return CG_OK;
  if (usec > 10 * 1000 * 1000) return CG_EINVAL;  // bounded: at most 10 s
  cg_func_lds((const void*)diag_occupy_kernel, 160 * 1024);
  hipLaunchKernelGGL(diag_occupy_kernel, dim3(n_cus), dim3(1024), 160 * 1024, (hipStream_t)stream,
                     (long long)usec * 100);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

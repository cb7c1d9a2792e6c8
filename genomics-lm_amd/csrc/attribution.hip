// Input attribution (contract: include/codonlm_hip.h, cg_attr_seed / cg_attr_reduce): the seed of
// an input-gradient-only backward and the per-token reductions of the gradient it ends with.  Both
// are streaming kernels: a wave owns a row, no shared memory, no atomics.
#include <math.h>
#include "common.h"

namespace {
constexpr int AT_WAVES = 4;    // rows per workgroup pass
constexpr int AT_BLK = 4096;   // grid cap; rows beyond 4 * AT_BLK are grid-strided

int attr_blocks(long long rows) { return cg_grid_cap((rows + AT_WAVES - 1) / AT_WAVES, AT_BLK); }

// d[r][c] = w (delta_{c,y} - softmax(z_r)_c) (LOGPROB) or w delta_{c,y} (LOGIT), in the dlogits
// element layouts of cg_cross_entropy (common.h st_grad: fp32 or split bf16); a row with y
// outside [0, V) or w == 0 is all zero; columns [V, half) are zero in every row.  The softmax is
// evaluated in fp64 from the fp32 logits and rounded once: rest = sum_{c != y} exp(z_c - max) is a
// sum of non-negative terms, so d_y = w rest / (rest + e_y) keeps its relative accuracy however
// close p_y is to 1 (1 - p_y formed from p_y would cancel).
template <typename TD, bool SPLIT>
__global__ __launch_bounds__(64 * AT_WAVES) void attr_seed_kernel(const float* __restrict__ logits, long long ldl,
                                                                   const int64_t* __restrict__ y,
                                                                   const float* __restrict__ w, long long rows, int V,
                                                                   int mode, TD* __restrict__ d, long long ldd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long half = SPLIT ? ldd / 2 : ldd;
  for (long long row = (long long)blockIdx.x * AT_WAVES + wave; row < rows; row += (long long)gridDim.x * AT_WAVES) {
    TD* dr = d + row * ldd;
    const long long t = y[row];
    const float wr = w ? w[row] : 1.0f;
    if (t < 0 || t >= V || wr == 0.0f) {
      for (long long c = lane; c < half; c += 64) st_grad<TD, SPLIT>(dr, c, half, 0.f);
      continue;
    }
    if (mode == CG_ATTR_LOGIT) {
      for (long long c = lane; c < half; c += 64) st_grad<TD, SPLIT>(dr, c, half, c == t ? wr : 0.f);
      continue;
    }
    const float* __restrict__ z = logits + row * ldl;
    float mloc = -INFINITY;
    for (int c = lane; c < V; c += 64) mloc = fmaxf(mloc, z[c]);
    const double m = (double)wave_max(mloc);
    double rest = 0.0;
    for (int c = lane; c < V; c += 64)
      if (c != t) rest += exp((double)z[c] - m);
    rest = wave_sum(rest);
    const double scale = (double)wr / (rest + exp((double)z[t] - m));
    for (long long c = lane; c < half; c += 64) {
      float g = 0.f;
      if (c < V) g = (float)(c == t ? scale * rest : -scale * exp((double)z[c] - m));
      st_grad<TD, SPLIT>(dr, c, half, g);
    }
  }
}

// four consecutive elements of a row starting at k0 (a multiple of 4): one 16-byte load where the
// whole row takes them (VEC), else element loads with zeros past d.  Both give the lane the same
// four values, so the two paths sum in the same order.
template <bool VEC>
__device__ __forceinline__ void ld4(const float* __restrict__ p, int k0, int d, float* v) {
  if constexpr (VEC) {
    ld_vec<4>(p + k0, v);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = k0 + u < d ? p[k0 + u] : 0.f;
  }
}

// lane l takes elements 4 (l + 64 j) .. + 3 for j = 0, 1, ... in order (one FMA chain per output),
// then the fixed butterfly: a row's three values depend on that row's operands alone
template <bool VEC>
__global__ __launch_bounds__(64 * AT_WAVES) void attr_reduce_kernel(const float* __restrict__ g, long long ldg,
                                                                     const int64_t* __restrict__ idx,
                                                                     const float* __restrict__ tok, long long lde,
                                                                     int V, const float* __restrict__ x0,
                                                                     long long ldx, long long rows, int d,
                                                                     float* __restrict__ gxt, float* __restrict__ gxi,
                                                                     float* __restrict__ gnorm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long row = (long long)blockIdx.x * AT_WAVES + wave; row < rows; row += (long long)gridDim.x * AT_WAVES) {
    const float* __restrict__ gr = g + row * ldg;
    const long long t = idx[row];
    const float* __restrict__ er = (gxt && t >= 0 && t < V) ? tok + t * lde : nullptr;
    const float* __restrict__ xr = gxi ? x0 + row * ldx : nullptr;
    float at = 0.f, ai = 0.f, an = 0.f;
    for (int k0 = 4 * lane; k0 < d; k0 += 256) {
      float gv[4], ov[4];
      ld4<VEC>(gr, k0, d, gv);
      if (er) {
        ld4<VEC>(er, k0, d, ov);
#pragma unroll
        for (int u = 0; u < 4; ++u) at = fmaf(gv[u], ov[u], at);
      }
      if (xr) {
        ld4<VEC>(xr, k0, d, ov);
#pragma unroll
        for (int u = 0; u < 4; ++u) ai = fmaf(gv[u], ov[u], ai);
      }
      if (gnorm) {
#pragma unroll
        for (int u = 0; u < 4; ++u) an = fmaf(gv[u], gv[u], an);
      }
    }
    if (gxt) {
      at = wave_sum(at);
      if (lane == 0) gxt[row] = at;
    }
    if (gxi) {
      ai = wave_sum(ai);
      if (lane == 0) gxi[row] = ai;
    }
    if (gnorm) {
      an = wave_sum(an);
      if (lane == 0) gnorm[row] = sqrtf(an);
    }
  }
}

}  // namespace

extern "C" int cg_attr_seed(const float* logits, long long ldl, const int64_t* y, const float* w, int rows, int V,
                            int mode, int d_dtype, void* d, long long ldd, void* stream) {
  if (rows < 0 || V <= 0) return CG_EINVAL;
  if (mode != CG_ATTR_LOGPROB && mode != CG_ATTR_LOGIT) return CG_EINVAL;
  if (d_dtype != CG_F32 && d_dtype != CG_BF16X2) return CG_EUNSUPPORTED;
  if (rows == 0) return CG_OK;
  if (!y || !d || (mode == CG_ATTR_LOGPROB && (!logits || ldl < V))) return CG_EINVAL;
  if (d_dtype == CG_BF16X2 ? ((ldd & 1) || ldd / 2 < V) : ldd < V) return CG_EINVAL;
  const dim3 grid(attr_blocks(rows)), block(64 * AT_WAVES);
  hipStream_t s = (hipStream_t)stream;
  if (d_dtype == CG_BF16X2)
    hipLaunchKernelGGL((attr_seed_kernel<bf16_t, true>), grid, block, 0, s, logits, ldl, y, w, (long long)rows, V,
                       mode, (bf16_t*)d, ldd);
  else
    hipLaunchKernelGGL((attr_seed_kernel<float, false>), grid, block, 0, s, logits, ldl, y, w, (long long)rows, V,
                       mode, (float*)d, ldd);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_attr_reduce(const float* g, long long ldg, const int64_t* idx, const float* tok_emb,
                              long long ld_e, int V, const float* x0, long long ldx, int rows, int d, float* gxt,
                              float* gxi, float* gnorm, void* stream) {
  if (rows < 0 || d <= 0) return CG_EINVAL;
  if (rows == 0) return CG_OK;
  if (!g || !idx || ldg < d) return CG_EINVAL;
  if (gxt && (!tok_emb || ld_e < d || V <= 0)) return CG_EINVAL;
  if (gxi && (!x0 || ldx < d)) return CG_EINVAL;
  if (!gxt && !gxi && !gnorm) return CG_OK;
  const bool vec = d % 4 == 0 && cg_rows16(g, ldg, 4) && (!gxt || cg_rows16(tok_emb, ld_e, 4)) && (!gxi || cg_rows16(x0, ldx, 4));
  const dim3 grid(attr_blocks(rows)), block(64 * AT_WAVES);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(attr_reduce_kernel<true>, grid, block, 0, s, g, ldg, idx, tok_emb, ld_e, V, x0, ldx,
                       (long long)rows, d, gxt, gxi, gnorm);
  else
    hipLaunchKernelGGL(attr_reduce_kernel<false>, grid, block, 0, s, g, ldg, idx, tok_emb, ld_e, V, x0, ldx,
                       (long long)rows, d, gxt, gxi, gnorm);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// Batched on-device scoring: one fused pass over fp32 logits rows (contract: include/codonlm_hip.h,
// cg_score_rows).  A wave owns a row, lane l holds columns l, l + 64, ... in registers (one
// chunked read); every row quantity is a wave reduction evaluated in fp64 from the fp32 logits
// and rounded once.  The accumulators follow cg_cross_entropy: per-workgroup partials, then one
// single-workgroup launch that adds them in a fixed order -- no floating-point atomics.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {
constexpr int SC_V = 1024;      // widest vocabulary (16 chunks of 64 columns per lane)
constexpr int SC_WAVES = 4;     // rows per workgroup pass
constexpr int SC_BLK = 4096;    // grid cap; rows beyond 4 * SC_BLK are grid-strided

struct ScoreArgs {
  const float* logits; long long ldl;
  const int64_t* targets;
  int rows, V, ignore;
  double eps;
  float* lse; float* logp; float* entropy; int32_t* argmax; int32_t* rank;
  const int32_t* sel; int n_sel; float* delta; long long ld_delta;
  double* row_logp;  // workspace: fp64 logp of every row (0 on invalid rows), for the sequence sums
  double* part;      // workspace: [gridDim.x][4] accumulator partials, or NULL
};

// NCH = 64-column chunks a lane holds (V <= 64 * NCH)
template <int NCH>
__global__ __launch_bounds__(64 * SC_WAVES) void score_rows_kernel(ScoreArgs A) {
  __shared__ double wpart[SC_WAVES][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = A.V;
  const bool want_ent = A.entropy != nullptr;
  const bool want_smooth = A.part != nullptr && A.eps != 0.0;
  double a_nll = 0.0, a_obj = 0.0, a_n = 0.0, a_hit = 0.0;
  for (long long row = (long long)blockIdx.x * SC_WAVES + wave; row < A.rows;
       row += (long long)gridDim.x * SC_WAVES) {
    const float* __restrict__ zr = A.logits + row * A.ldl;
    float z[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = lane + 64 * k;
      z[k] = c < V ? zr[c] : -INFINITY;
    }
    // maximum and its lowest index (the lane's chunks ascend, so > keeps the lane's first)
    float mloc = z[0];
    int iloc = lane;
#pragma unroll
    for (int k = 1; k < NCH; ++k)
      if (z[k] > mloc) { mloc = z[k]; iloc = lane + 64 * k; }
    const float mx = wave_max(mloc);
    const int amax = wave_min(mloc == mx ? iloc : INT_MAX);
    // s1 = sum over c != argmax of exp(z - max) (the argmax term is exactly 1) and, for the
    // entropy, sum exp(z - max) (max - z): fp64 sums of non-negative terms, so log1p(s1) = lse - max
    // and everything built from it keep full relative accuracy however peaked the row is
    const double m = (double)mx;
    double s1 = 0.0, sez = 0.0, ssm = 0.0;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = lane + 64 * k;
      if (c < V && c != amax) {
        const double dz = m - (double)z[k];
        const double e = exp(-dz);
        s1 += e;
        if (e > 0.0) sez += e * dz;  // p == 0 (z = -inf) adds 0, never 0 * inf
      }
    }
    s1 = wave_sum(s1);
    if (want_ent) sez = wave_sum(sez);
    const double lgs = log1p(s1);
    const double lse = m + lgs;
    if (want_smooth) {
#pragma unroll
      for (int k = 0; k < NCH; ++k)
        if (lane + 64 * k < V) ssm += lse - (double)z[k];
      ssm = wave_sum(ssm);
    }
    // the target
    long long y = -1;
    bool valid = false;
    if (A.targets) {
      y = A.targets[row];
      valid = y != A.ignore && y >= 0 && y < V;
    }
    double lp = 0.0;
    int rk = -1;
    if (valid) {
      const float zy = zr[y];
      lp = ((double)zy - m) - lgs;
      if (A.rank) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
          const int c = lane + 64 * k;
          if (c < V && (z[k] > zy || (z[k] == zy && c < y))) ++cnt;
        }
        rk = wave_sum(cnt);
      }
      const double nll = -lp;
      a_nll += nll;
      a_obj += want_smooth ? (1.0 - A.eps) * nll + (A.eps / (double)V) * ssm : nll;
      a_n += 1.0;
      if (amax == y) a_hit += 1.0;
    }
    if (lane == 0) {
      if (A.lse) A.lse[row] = (float)lse;
      if (A.logp) A.logp[row] = (float)lp;
      // lse - sum p z = (lse - max) + sum e (max - z) / sum e
      if (want_ent) A.entropy[row] = (float)(lgs + sez / (1.0 + s1));
      if (A.argmax) A.argmax[row] = amax;
      if (A.rank) A.rank[row] = rk;
      if (A.row_logp) A.row_logp[row] = lp;
    }
    if (A.delta) {
      // (z_s - lse) - (z_y - lse) = z_s - z_y on a valid row: the lse cancels before any rounding
      const double base = valid ? (double)zr[y] : lse;
      for (int j = lane; j < A.n_sel; j += 64) {
        const int s = A.sel[j];
        float dv = -INFINITY;
        if (s >= 0 && s < V) dv = (float)((double)zr[s] - base);
        A.delta[row * A.ld_delta + j] = dv;
      }
    }
  }
  if (A.part) {
    if (lane == 0) {
      wpart[wave][0] = a_nll; wpart[wave][1] = a_obj; wpart[wave][2] = a_n; wpart[wave][3] = a_hit;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      const int q = threadIdx.x;
      A.part[(long long)blockIdx.x * 4 + q] = ((wpart[0][q] + wpart[1][q]) + wpart[2][q]) + wpart[3][q];
    }
  }
}

// acc[q] += sum of the per-workgroup partials: thread t takes partials t, t + 1024, ... in
// order, then a fixed tree
__global__ __launch_bounds__(1024) void score_final_kernel(const double* __restrict__ part, int nblk,
                                                            double* __restrict__ acc) {
  __shared__ double red[1024];
  for (int q = 0; q < 4; ++q) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 1024) s += part[(long long)b * 4 + q];
    block_sum_1024(s, red);
    if (threadIdx.x == 0) acc[q] += red[0];
    __syncthreads();
  }
}

// one wave per sequence: lane l adds rows t = l, l + 64, ... of the sequence in order, then the
// fixed butterfly.  An invalid row holds exactly 0, so a sequence's sum does not depend on how far
// it is padded or on its neighbours.
__global__ __launch_bounds__(64) void score_seq_kernel(const double* __restrict__ row_logp,
                                                        const int64_t* __restrict__ targets, int T, int V,
                                                        int ignore, double* __restrict__ seq_logp,
                                                        int32_t* __restrict__ seq_count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  int n = 0;
  for (int t = lane; t < T; t += 64) {
    const long long r = (long long)b * T + t;
    s += row_logp[r];
    if (targets) {
      const long long y = targets[r];
      n += (y != ignore && y >= 0 && y < V) ? 1 : 0;
    }
  }
  s = wave_sum(s);
  n = wave_sum(n);
  if (lane == 0) {
    if (seq_logp) seq_logp[b] = s;
    if (seq_count) seq_count[b] = n;
  }
}

int score_blocks(int rows) { return cg_grid_cap(cg_cdiv(rows, SC_WAVES), SC_BLK); }
// [4 * blocks] fp64 partials, then one fp64 per row
size_t score_part_bytes(int rows) { return (size_t)score_blocks(rows) * 4 * sizeof(double); }
}  // namespace

extern "C" size_t cg_score_workspace(int rows) {
  if (rows < 0) rows = 0;
  return score_part_bytes(rows) + (size_t)rows * sizeof(double);
}

extern "C" int cg_score_rows(const cg_score_desc* d, void* stream) {
  if (!d || d->rows < 0 || d->V <= 0) return CG_EINVAL;
  if (d->V > SC_V) return CG_EUNSUPPORTED;
  if (d->rows == 0) return CG_OK;
  if (!d->logits || d->ldl < d->V) return CG_EINVAL;
  if (d->delta && (!d->sel || d->n_sel <= 0 || d->ld_delta < d->n_sel)) return CG_EINVAL;
  const bool want_seq = d->seq_logp || d->seq_count;
  if (want_seq && (d->T <= 0 || d->rows % d->T)) return CG_EINVAL;
  if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->ws_bytes < cg_score_workspace(d->rows)) return CG_EINVAL;
  if (d->acc && ((uintptr_t)d->acc & 7)) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = score_blocks(d->rows);
  ScoreArgs A;
  A.logits = d->logits; A.ldl = d->ldl;
  A.targets = d->targets;
  A.rows = d->rows; A.V = d->V; A.ignore = d->ignore_index;
  A.eps = (double)d->smoothing;
  A.lse = d->lse; A.logp = d->logp; A.entropy = d->entropy; A.argmax = d->argmax; A.rank = d->rank;
  A.sel = d->sel; A.n_sel = d->n_sel; A.delta = d->delta; A.ld_delta = d->ld_delta;
  A.part = d->acc ? (double*)d->workspace : nullptr;
  A.row_logp = want_seq ? (double*)((char*)d->workspace + score_part_bytes(d->rows)) : nullptr;
  const dim3 g(nblk), b(64 * SC_WAVES);
  if (d->V <= 128)
    hipLaunchKernelGGL(score_rows_kernel<2>, g, b, 0, s, A);
  else if (d->V <= 256)
    hipLaunchKernelGGL(score_rows_kernel<4>, g, b, 0, s, A);
  else if (d->V <= 512)
    hipLaunchKernelGGL(score_rows_kernel<8>, g, b, 0, s, A);
  else
    hipLaunchKernelGGL(score_rows_kernel<16>, g, b, 0, s, A);
  CG_LAUNCH_CHECK();
  if (d->acc) {
    hipLaunchKernelGGL(score_final_kernel, dim3(1), dim3(1024), 0, s, (const double*)A.part, nblk, d->acc);
    CG_LAUNCH_CHECK();
  }
  if (want_seq) {
    hipLaunchKernelGGL(score_seq_kernel, dim3(d->rows / d->T), dim3(64), 0, s, (const double*)A.row_logp,
                       d->targets, d->T, d->V, d->ignore_index, d->seq_logp, d->seq_count);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

// Context diagnostic: segment-aware n-gram baselines and the sliced loss / calibration pass
// (contracts: include/codonlm_hip.h, cg_ngram_count / cg_ngram_totals / cg_ngram_nll / cg_diag_rows).
// Integer tables use integer atomics (order-independent).  Every fp64 sum follows cg_score_rows: a
// fixed order inside the wave and the workgroup, per-workgroup partials in the workspace, then one
// single-workgroup launch that adds them in block order -- no floating-point atomics.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {
constexpr int NG_V = CG_NGRAM_MAX_V;
constexpr int NG_BLK = 1024;        // grid cap of the counting and the baseline-nll kernels
constexpr int NG_WAVES = 4;         // rows per workgroup pass of the baseline-nll kernel
constexpr int DG_BLK = 2048;        // grid cap of the diagnostic pass (rows beyond it are grid-strided)
constexpr int DG_CHUNK = 256;       // positions of a row one scan step covers (= the workgroup)
constexpr int DG_CAL = 2 * CG_DIAG_SLICES;             // first calibration accumulator
constexpr int DG_BRIER = DG_CAL + 3 * CG_DIAG_MAX_BINS;  // the two Brier accumulators
constexpr int DG_NACC = DG_BRIER + 2;

__device__ __forceinline__ bool in_vocab(long long t, int V) { return t >= 0 && t < V; }

// ------------------------------------------------------------------ counting
// grid-stride over the flat positions; the bigram table of the workgroup lives in LDS as 32-bit
// counts (a workgroup sees fewer than 2^32 positions: the entry point bounds n), the unigram counts
// are its column sums
__global__ __launch_bounds__(256) void ngram_count_kernel(const int64_t* __restrict__ x, const int64_t* __restrict__ y,
                                                          long long n, int T, int V, int pad, cg_id_mask reset,
                                                          unsigned long long* __restrict__ uni,
                                                          unsigned long long* __restrict__ bi,
                                                          unsigned long long* __restrict__ tri,
                                                          unsigned long long* __restrict__ n_bad) {
  extern __shared__ uint32_t cnt[];  // [V][V]
  const int VV = V * V;
  for (int i = threadIdx.x; i < VV; i += 256) cnt[i] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * 256;
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  int t = (int)(i % T);
  const int tstep = (int)(stride % T);
  unsigned int bad = 0;
  for (; i < n; i += stride) {
    const long long yy = y[i];
    if (yy != pad) {
      const long long p = x[i];
      if (in_vocab(yy, V) && in_vocab(p, V)) {
        long long p2 = pad;
        if (t != 0 && !cg_mask_has(reset, p)) p2 = x[i - 1];
        if (in_vocab(p2, V)) {
          atomicAdd(&cnt[(int)p * V + (int)yy], 1u);
          atomicAdd(&tri[((long long)p2 * V + p) * V + yy], 1ull);
        } else {
          ++bad;
        }
      } else {
        ++bad;
      }
    }
    t += tstep;
    if (t >= T) t -= T;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < VV; c += 256) {
    const uint32_t v = cnt[c];
    if (v) atomicAdd(&bi[c], (unsigned long long)v);
  }
  if (threadIdx.x < V) {
    unsigned long long s = 0;
    for (int p = 0; p < V; ++p) s += cnt[p * V + threadIdx.x];
    if (s) atomicAdd(&uni[threadIdx.x], s);
  }
  if (n_bad && bad) atomicAdd(n_bad, (unsigned long long)bad);
}

// one wave per table row: the sum of its counts over the targets 1 .. V-1
__global__ __launch_bounds__(256) void ngram_totals_kernel(const long long* __restrict__ uni,
                                                           const long long* __restrict__ bi,
                                                           const long long* __restrict__ tri, int V,
                                                           long long* __restrict__ uni_total,
                                                           long long* __restrict__ bi_total,
                                                           long long* __restrict__ tri_total) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int R = 1 + V + V * V;
  if (r >= R) return;
  const long long* src;
  long long* dst;
  if (r == 0) { src = uni; dst = uni_total; }
  else if (r <= V) { src = bi + (long long)(r - 1) * V; dst = bi_total + (r - 1); }
  else { src = tri + (long long)(r - 1 - V) * V; dst = tri_total + (r - 1 - V); }
  long long s = 0;
  for (int c = lane; c < V; c += 64)
    if (c >= 1) s += src[c];
  s = wave_sum(s);
  if (lane == 0) *dst = s;
}

struct NllArgs {
  const int64_t* x; const int64_t* y;
  int B, T, V, pad;
  cg_id_mask reset;
  double alpha;
  const long long* uni; const long long* bi; const long long* tri;
  const long long* uni_total; const long long* bi_total; const long long* tri_total;
  float* tok_tri; double* row_sums; int32_t* row_count;
  double* part;  // workspace: [gridDim.x][5], or NULL
};

// one wave per row: lane l takes positions l, l + 64, ... in order, then the fixed butterfly
__global__ __launch_bounds__(64 * NG_WAVES) void ngram_nll_kernel(NllArgs A) {
  __shared__ double wpart[NG_WAVES][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = A.V, T = A.T;
  const double den0 = A.alpha * (double)(V - 1);
  const double lg_uniform = log((double)(V - 1));
  const double tu = (double)A.uni_total[0];
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = blockIdx.x * NG_WAVES + wave; b < A.B; b += gridDim.x * NG_WAVES) {
    const long long base = (long long)b * T;
    double s_uni = 0.0, s_bi = 0.0, s_tri = 0.0;
    int n = 0;
    for (int t = lane; t < T; t += 64) {
      const long long yy = A.y[base + t];
      float out = 0.f;
      if (yy != A.pad) {
        const long long p = A.x[base + t];
        if (in_vocab(yy, V) && in_vocab(p, V)) {
          long long p2 = A.pad;
          if (t != 0 && !cg_mask_has(A.reset, p)) p2 = A.x[base + t - 1];
          if (in_vocab(p2, V)) {
            const double cu = (double)A.uni[yy];
            const double cb = (double)A.bi[p * V + yy], tb = (double)A.bi_total[p];
            const long long ctx = p2 * V + p;
            double ct = cb, tt = tb;
            const long long tt_i = A.tri_total[ctx];
            if (tt_i != 0) { ct = (double)A.tri[ctx * V + yy]; tt = (double)tt_i; }
            const double l_tri = -log((ct + A.alpha) / (tt + den0));
            s_uni += -log((cu + A.alpha) / (tu + den0));
            s_bi += -log((cb + A.alpha) / (tb + den0));
            s_tri += l_tri;
            ++n;
            out = (float)l_tri;
          }
        }
      }
      if (A.tok_tri) A.tok_tri[base + t] = out;
    }
    s_uni = wave_sum(s_uni); s_bi = wave_sum(s_bi); s_tri = wave_sum(s_tri);
    n = wave_sum(n);
    const double s_flat = (double)n * lg_uniform;
    if (lane == 0) {
      if (A.row_sums) {
        double* r = A.row_sums + (long long)b * 4;
        r[0] = s_flat; r[1] = s_uni; r[2] = s_bi; r[3] = s_tri;
      }
      if (A.row_count) A.row_count[b] = n;
    }
    acc[0] += s_flat; acc[1] += s_uni; acc[2] += s_bi; acc[3] += s_tri; acc[4] += (double)n;
  }
  if (A.part) {
    if (lane == 0)
      for (int q = 0; q < 5; ++q) wpart[wave][q] = acc[q];
    __syncthreads();
    if (threadIdx.x < 5) {
      const int q = threadIdx.x;
      A.part[(long long)blockIdx.x * 5 + q] = ((wpart[0][q] + wpart[1][q]) + wpart[2][q]) + wpart[3][q];
    }
  }
}

// out[q] += the partials of accumulator q in block order, one thread per accumulator
__global__ __launch_bounds__(128) void ngram_final_kernel(const double* __restrict__ part, int nblk,
                                                          double* __restrict__ acc) {
  const int q = threadIdx.x;
  if (q >= 5) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(long long)b * 5 + q];
  acc[q] += s;
}

// ------------------------------------------------------------------ the diagnostic pass
struct DiagArgs {
  const float* logits; long long ldl;
  const int64_t* x; const int64_t* y;
  int B, T, V, pad, sep;
  const uint8_t* row_flag; const uint8_t* tok_class;
  const float* edges; int n_bins;
  float* nll; int32_t* segpos; float* conf;
  double* row_nll; int32_t* row_count;
  double* part;  // workspace: [gridDim.x][DG_NACC], or NULL
};

__device__ __forceinline__ int pos_slice(int sp) {
  return sp == 0 ? CG_DIAG_POS_0 : sp < 4 ? CG_DIAG_POS_1_3 : sp < 16 ? CG_DIAG_POS_4_15
       : sp < 64 ? CG_DIAG_POS_16_63 : CG_DIAG_POS_64_PLUS;
}

// One workgroup of four waves per row.  A row is taken in chunks of 256 positions: (1) a thread per
// position scans the segment counter from wave ballots and a carry, (2) a wave per position (j = 4 k +
// wave) evaluates the logits row, lane l holding columns l and l + 64, and lane 0 adds the position
// to the wave's own accumulators in LDS, (3) the per-token outputs leave coalesced and wave 0 adds
// the chunk to the row sum (lane = t % 64, t ascending).
__global__ __launch_bounds__(DG_CHUNK) void diag_rows_kernel(DiagArgs A) {
  __shared__ double wacc[4][DG_NACC];
  __shared__ double dn[DG_CHUNK];
  __shared__ float cnll[DG_CHUNK], cconf[DG_CHUNK], sedge[CG_DIAG_MAX_BINS + 1];
  __shared__ int ssp[DG_CHUNK], sy[DG_CHUNK], ssep[DG_CHUNK];
  __shared__ int wreset[4], wtail[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = A.V, T = A.T;
  const unsigned long long lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);
  for (int q = tid; q < 4 * DG_NACC; q += DG_CHUNK) (&wacc[0][0])[q] = 0.0;
  if (A.edges && tid <= A.n_bins) sedge[tid] = A.edges[tid];
  __syncthreads();
  for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
    const long long base = (long long)b * T;
    const int flag_slice = (A.row_flag && A.row_flag[b]) ? CG_DIAG_FLAG_SET : CG_DIAG_FLAG_CLEAR;
    int carry = 0;  // the segment counter entering the chunk
    double rs = 0.0;
    int rc = 0;
    for (int c0 = 0; c0 < T; c0 += DG_CHUNK) {
      // (1) the segment counter of the chunk's positions
      const int t = c0 + tid;
      long long yy = A.pad, xx = -1;
      if (t < T) { yy = A.y[base + t]; xx = A.x[base + t]; }
      const bool valid = yy != A.pad && in_vocab(yy, V);
      const bool rst = valid && xx == A.sep;
      const unsigned long long vb = __ballot(valid), rb = __ballot(rst);
      const int before = __popcll(vb & lt);
      if (lane == 0) {
        // the counter after the wave's last position, from its last reset or the wave's start
        int tail = __popcll(vb);
        if (rb) tail -= __popcll(vb & ((1ull << (63 - __clzll(rb))) - 1ull));
        wreset[wave] = rb != 0;
        wtail[wave] = tail;
      }
      __syncthreads();
      int wcarry = carry;
      for (int w = 0; w < 4; ++w) {
        if (w == wave) wcarry = carry;
        carry = wreset[w] ? wtail[w] : carry + wtail[w];
      }
      int sp;
      const unsigned long long rme = rb & le;
      if (rme) sp = before - __popcll(vb & ((1ull << (63 - __clzll(rme))) - 1ull));
      else sp = wcarry + before;
      ssp[tid] = valid ? sp : -1;
      sy[tid] = valid ? (int)yy : 0;
      ssep[tid] = rst;
      __syncthreads();
      // (2) a wave per position
      for (int j = wave; j < DG_CHUNK; j += 4) {
        const int spj = __builtin_amdgcn_readfirstlane(ssp[j]);
        if (spj < 0) {
          if (lane == 0) { cnll[j] = 0.f; cconf[j] = 0.f; dn[j] = 0.0; }
          continue;
        }
        const int yj = __builtin_amdgcn_readfirstlane(sy[j]);
        const float* __restrict__ zr = A.logits + (base + c0 + j) * A.ldl;
        const float z0 = lane < V ? zr[lane] : -INFINITY;
        const float z1 = lane + 64 < V ? zr[lane + 64] : -INFINITY;
        // the maximum and its lowest index
        float mloc = z0;
        int iloc = lane;
        if (z1 > mloc) { mloc = z1; iloc = lane + 64; }
        const float mx = wave_max(mloc);
        const int amax = wave_min(mloc == mx ? iloc : INT_MAX);
        // s1 = sum over c != argmax of exp(z - max) (that term is exactly 1), s2 of its square
        const double m = (double)mx;
        double s1 = 0.0, s2 = 0.0;
        if (lane < V && lane != amax) { const double e = exp((double)z0 - m); s1 += e; s2 += e * e; }
        if (lane + 64 < V && lane + 64 != amax) { const double e = exp((double)z1 - m); s1 += e; s2 += e * e; }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const double lgs = log1p(s1);            // lse - max
        const double dzy = (double)zr[yj] - m;   // <= 0
        const double nll = lgs - dzy;
        const double conf = 1.0 / (1.0 + s1);    // exp(max - lse)
        const double py = yj == amax ? conf : exp(dzy) * conf;
        const double brier = (1.0 + s2) * conf * conf - 2.0 * py + 1.0;
        const float conf32 = (float)conf;
        int bin = -1;
        if (A.edges) {
          const bool hit = lane < A.n_bins && conf32 > sedge[lane] && conf32 <= sedge[lane + 1];
          const unsigned long long hb = __ballot(hit);
          if (hb) bin = __ffsll((long long)hb) - 1;
        }
        if (lane == 0) {
          double* a = wacc[wave];
          a[2 * CG_DIAG_ALL] += nll; a[2 * CG_DIAG_ALL + 1] += 1.0;
          if (ssep[j]) { a[2 * CG_DIAG_AFTER_SEP] += nll; a[2 * CG_DIAG_AFTER_SEP + 1] += 1.0; }
          a[2 * flag_slice] += nll; a[2 * flag_slice + 1] += 1.0;
          const int ps = pos_slice(spj);
          a[2 * ps] += nll; a[2 * ps + 1] += 1.0;
          if (A.tok_class) {
            const int k = A.tok_class[yj];
            if (k < 4) { a[2 * (CG_DIAG_CLS_SPECIAL_SLICE + k)] += nll; a[2 * (CG_DIAG_CLS_SPECIAL_SLICE + k) + 1] += 1.0; }
          }
          if (bin >= 0) {
            a[DG_CAL + 3 * bin] += 1.0;
            a[DG_CAL + 3 * bin + 1] += (double)conf32;
            a[DG_CAL + 3 * bin + 2] += yj == amax ? 1.0 : 0.0;
          }
          a[DG_BRIER] += brier; a[DG_BRIER + 1] += 1.0;
          cnll[j] = (float)nll; cconf[j] = conf32; dn[j] = nll;
        }
      }
      __syncthreads();
      // (3) the chunk's outputs
      if (t < T) {
        if (A.nll) A.nll[base + t] = cnll[tid];
        if (A.conf) A.conf[base + t] = cconf[tid];
        if (A.segpos) A.segpos[base + t] = ssp[tid];
      }
      if (wave == 0) {
#pragma unroll
        for (int q = 0; q < DG_CHUNK / 64; ++q) {
          rs += dn[lane + 64 * q];
          rc += ssp[lane + 64 * q] >= 0 ? 1 : 0;
        }
      }
      __syncthreads();
    }
    if (wave == 0 && (A.row_nll || A.row_count)) {
      rs = wave_sum(rs);
      rc = wave_sum(rc);
      if (lane == 0) {
        if (A.row_nll) A.row_nll[b] = rs;
        if (A.row_count) A.row_count[b] = rc;
      }
    }
  }
  if (A.part) {
    __syncthreads();
    if (tid < DG_NACC)
      A.part[(long long)blockIdx.x * DG_NACC + tid] = ((wacc[0][tid] + wacc[1][tid]) + wacc[2][tid]) + wacc[3][tid];
  }
}

__global__ __launch_bounds__(DG_NACC) void diag_final_kernel(const double* __restrict__ part, int nblk, int n_bins,
                                                             double* __restrict__ slices, double* __restrict__ calib,
                                                             double* __restrict__ brier_acc) {
  const int q = threadIdx.x;
  double* dst = nullptr;
  if (q < DG_CAL) dst = slices ? slices + q : nullptr;
  else if (q < DG_BRIER) dst = (calib && q - DG_CAL < 3 * n_bins) ? calib + (q - DG_CAL) : nullptr;
  else if (q < DG_NACC) dst = brier_acc ? brier_acc + (q - DG_BRIER) : nullptr;
  if (!dst) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(long long)b * DG_NACC + q];
  *dst += s;
}

int nll_blocks(int B) { return cg_grid_cap(cg_cdiv(B, NG_WAVES), NG_BLK); }
int diag_blocks(int B) { return cg_grid_cap(B, DG_BLK); }
}  // namespace

extern "C" int cg_ngram_count(const int64_t* x, const int64_t* y, int B, int T, int V, int pad_id,
                              const uint32_t* reset_mask, long long* uni, long long* bi, long long* tri,
                              long long* n_bad, void* stream) {
  if (B < 0 || T < 0 || V <= 0) return CG_EINVAL;
  if (V > NG_V) return CG_EUNSUPPORTED;
  if (pad_id < 0 || pad_id >= V) return CG_EINVAL;
  if (B == 0 || T == 0) return CG_OK;
  cg_id_mask m;
  if (!x || !y || !uni || !bi || !tri || !cg_mask_fill(m, reset_mask)) return CG_EINVAL;
  const long long n = (long long)B * T;
  if (n > (1ll << 40)) return CG_EUNSUPPORTED;
  const int nblk = cg_grid_cap((n + 256 * 8 - 1) / (256 * 8), NG_BLK);
  const int lds = V * V * (int)sizeof(uint32_t);
  cg_func_lds((const void*)ngram_count_kernel, lds);
  hipLaunchKernelGGL(ngram_count_kernel, dim3(nblk), dim3(256), lds, (hipStream_t)stream, x, y, n, T, V, pad_id, m,
                     (unsigned long long*)uni, (unsigned long long*)bi, (unsigned long long*)tri,
                     (unsigned long long*)n_bad);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_ngram_totals(const long long* uni, const long long* bi, const long long* tri, int V,
                               long long* uni_total, long long* bi_total, long long* tri_total, void* stream) {
  if (V <= 0) return CG_EINVAL;
  if (V > NG_V) return CG_EUNSUPPORTED;
  if (!uni || !bi || !tri || !uni_total || !bi_total || !tri_total) return CG_EINVAL;
  const int R = 1 + V + V * V;
  hipLaunchKernelGGL(ngram_totals_kernel, dim3(cg_cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, uni, bi, tri, V,
                     uni_total, bi_total, tri_total);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" size_t cg_ngram_nll_workspace(int B) {
  return (size_t)nll_blocks(B < 0 ? 0 : B) * 5 * sizeof(double);
}

extern "C" int cg_ngram_nll(const cg_ngram_nll_desc* d, void* stream) {
  if (!d || d->B < 0 || d->T < 0 || d->V <= 0) return CG_EINVAL;
  if (d->V > NG_V) return CG_EUNSUPPORTED;
  if (d->pad_id < 0 || d->pad_id >= d->V || !(d->alpha > 0.0) || !isfinite(d->alpha)) return CG_EINVAL;
  if (d->B == 0 || d->T == 0) return CG_OK;
  NllArgs A;
  if (!d->x || !d->y || !cg_mask_fill(A.reset, d->reset_mask)) return CG_EINVAL;
  if (!d->uni || !d->bi || !d->tri || !d->uni_total || !d->bi_total || !d->tri_total) return CG_EINVAL;
  if (d->acc && (!d->workspace || ((uintptr_t)d->workspace & 7) || ((uintptr_t)d->acc & 7) ||
                 d->ws_bytes < cg_ngram_nll_workspace(d->B)))
    return CG_EINVAL;
  if (d->row_sums && ((uintptr_t)d->row_sums & 7)) return CG_EINVAL;
  A.x = d->x; A.y = d->y; A.B = d->B; A.T = d->T; A.V = d->V; A.pad = d->pad_id; A.alpha = d->alpha;
  A.uni = d->uni; A.bi = d->bi; A.tri = d->tri;
  A.uni_total = d->uni_total; A.bi_total = d->bi_total; A.tri_total = d->tri_total;
  A.tok_tri = d->tok_tri; A.row_sums = d->row_sums; A.row_count = d->row_count;
  A.part = d->acc ? (double*)d->workspace : nullptr;
  const int nblk = nll_blocks(d->B);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ngram_nll_kernel, dim3(nblk), dim3(64 * NG_WAVES), 0, s, A);
  CG_LAUNCH_CHECK();
  if (d->acc) {
    hipLaunchKernelGGL(ngram_final_kernel, dim3(1), dim3(128), 0, s, (const double*)A.part, nblk, d->acc);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

extern "C" size_t cg_diag_workspace(int B) {
  return (size_t)diag_blocks(B < 0 ? 0 : B) * DG_NACC * sizeof(double);
}

extern "C" int cg_diag_rows(const cg_diag_desc* d, void* stream) {
  if (!d || d->B < 0 || d->T < 0 || d->V <= 0) return CG_EINVAL;
  if (d->V > NG_V) return CG_EUNSUPPORTED;
  if (d->pad_id < 0 || d->pad_id >= d->V) return CG_EINVAL;
  if (d->edges ? (d->n_bins < 1 || d->n_bins > CG_DIAG_MAX_BINS) : d->calib != nullptr) return CG_EINVAL;
  if (d->B == 0 || d->T == 0) return CG_OK;
  if (!d->logits || d->ldl < d->V || !d->x || !d->y) return CG_EINVAL;
  const bool want_acc = d->slices || d->calib || d->brier_acc;
  if (want_acc && (!d->workspace || ((uintptr_t)d->workspace & 7) || d->ws_bytes < cg_diag_workspace(d->B)))
    return CG_EINVAL;
  if (((uintptr_t)d->slices | (uintptr_t)d->calib | (uintptr_t)d->brier_acc | (uintptr_t)d->row_nll) & 7)
    return CG_EINVAL;
  DiagArgs A;
  A.logits = d->logits; A.ldl = d->ldl; A.x = d->x; A.y = d->y;
  A.B = d->B; A.T = d->T; A.V = d->V; A.pad = d->pad_id; A.sep = d->sep_id;
  A.row_flag = d->row_flag; A.tok_class = d->tok_class;
  A.edges = d->edges; A.n_bins = d->edges ? d->n_bins : 0;
  A.nll = d->nll; A.segpos = d->segpos; A.conf = d->conf;
  A.row_nll = d->row_nll; A.row_count = d->row_count;
  A.part = want_acc ? (double*)d->workspace : nullptr;
  const int nblk = diag_blocks(d->B);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(diag_rows_kernel, dim3(nblk), dim3(DG_CHUNK), 0, s, A);
  CG_LAUNCH_CHECK();
  if (want_acc) {
    hipLaunchKernelGGL(diag_final_kernel, dim3(1), dim3(DG_NACC), 0, s, (const double*)A.part, nblk, A.n_bins,
                       d->slices, d->calib, d->brier_acc);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

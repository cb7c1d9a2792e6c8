// Motif mining (contract: include/codonlm_hip.h, cg_window_keep / cg_window_pool / cg_kmeans_step):
// sliding-window pooling of hidden states in place, and one deterministic step of Lloyd's k-means.
// No floating-point atomics: every sum has one owner and a fixed order.
#include <math.h>
#include <type_traits>
#include "common.h"

namespace {
inline int win_count(int T, int window, int stride) { return T >= window ? (T - window) / stride + 1 : 0; }

// one thread per window: any token of it in the mask clears the flag
__global__ __launch_bounds__(256) void window_keep_kernel(const int64_t* __restrict__ idx, long long nw_total,
                                                          int nwin, int T, int window, int stride, cg_id_mask em,
                                                          int32_t* __restrict__ keep) {
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= nw_total) return;
  const long long b = w / nwin;
  const int j = (int)(w - b * nwin);
  const int64_t* row = idx + b * T + (long long)j * stride;
  int ok = 1;
  for (int t = 0; t < window; ++t)
    if (cg_mask_has(em, row[t])) ok = 0;
  keep[w] = ok;
}

// one thread per (window, column): the window's rows are added in ascending t, coalesced along the
// feature axis; overlapping windows re-read their rows from L2
template <typename T_>
__global__ __launch_bounds__(256) void window_pool_kernel(const T_* __restrict__ h, long long ldh, int nwin, int T,
                                                          int d, int window, int stride,
                                                          const int32_t* __restrict__ dst_row,
                                                          float* __restrict__ out, long long ldo,
                                                          long long out_rows) {
  const long long w = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= d) return;
  const long long r = dst_row[w];
  if (r < 0 || r >= out_rows) return;
  const long long b = w / nwin;
  const int j = (int)(w - b * nwin);
  const T_* p = h + (b * T + (long long)j * stride) * ldh + c;
  float s = 0.f;
  for (int t = 0; t < window; ++t) s += ld_act<T_>(p + (long long)t * ldh);
  out[r * ldo + c] = s / (float)window;
}

// ---------------------------------------------------------------------------
// k-means step.
//  1. kmeans_cnorm_kernel: |c|^2 of every centre (one wave per centre), +inf for the pad centres
//     of the last 32-centre tile.
//  2. kmeans_assign_kernel<NT>: a workgroup of 4 waves takes 128 points, a wave 32 of them against
//     all NT * 32 centres: x.c on v_mfma_f32_32x32x2_f32 (an exact fp32 fma chain), NT accumulator
//     tiles per wave, the operands staged through LDS 32 columns at a time so that x is read from
//     HBM once.  Epilogue: score |c|^2 - 2 x.c, argmin over (score, index) -- per lane over its NT
//     centres in ascending order, then a butterfly over the 32 lanes of a half-wave -- the winner's
//     distance recomputed directly, and the workgroup's fp64 share of the inertia.
//  3. kmeans_stats_kernel: a workgroup owns a chunk of CG_KMEANS_CHUNK rows and 64 columns; each of
//     its waves walks its share of the chunk's rows in order, thread = column, adding into an LDS
//     slab [k][64] fp32 of which no other thread touches that word; the waves' slabs are added in
//     wave order and go to the workspace as one partial.
//  4. kmeans_final_kernel: the partials added in chunk order in fp64 (one thread per element).
// ---------------------------------------------------------------------------
constexpr int KM_ROWS = 128;  // points per assign workgroup
constexpr int KM_DK = 32;     // columns per LDS stage
constexpr int KM_LD = 36;     // row stride of a staged tile in floats (16-byte aligned rows)
constexpr int KM_COLS = 64;   // columns per statistics workgroup

__global__ __launch_bounds__(256) void kmeans_cnorm_kernel(const float* __restrict__ cen, long long ldc, int k, int d,
                                                           int kpad, float* __restrict__ cn) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= kpad) return;
  if (c >= k) {
    if (lane == 0) cn[c] = INFINITY;
    return;
  }
  const float* __restrict__ r = cen + (long long)c * ldc;
  float s = 0.f;
  for (int j = lane; j < d; j += 64) s = fmaf(r[j], r[j], s);
  s = wave_sum(s);
  if (lane == 0) cn[c] = s;
}

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, long long ldx, long long n,
                                                            int d, const float* __restrict__ cen, long long ldc,
                                                            int k, const float* __restrict__ cn,
                                                            int32_t* __restrict__ labels, float* __restrict__ dist2,
                                                            double* __restrict__ ipart) {
  __shared__ __attribute__((aligned(16))) float xs[KM_ROWS * KM_LD];
  __shared__ __attribute__((aligned(16))) float cs[NT * 32 * KM_LD];
  __shared__ float cns[NT * 32];
  __shared__ int lab[KM_ROWS];
  __shared__ float dd[KM_ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, l31 = lane & 31;
  const long long r0 = (long long)blockIdx.x * KM_ROWS;
  for (int c = tid; c < NT * 32; c += 256) cns[c] = cn[c];
  v16f acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  // staging through registers, so that the loads of the next stage are in flight under this stage's
  // MFMAs.  VEC (d % 4 == 0, 16-byte aligned rows): a thread moves 16-byte pieces, 32 rows of 8 pieces
  // per pass; otherwise single elements, 8 rows of 32 columns per pass.  Both fill the same image.
  using ST = typename std::conditional<VEC, float4, float>::type;
  constexpr int RS = VEC ? 32 : 8, NX = KM_ROWS / RS, NC = NT * 32 / RS;
  const int scol = VEC ? 4 * (tid & 7) : (tid & 31), srow = VEC ? (tid >> 3) : (tid >> 5);
  ST sx[NX], sc[NC];
  auto fetch = [&](int k0) __attribute__((always_inline)) {
    const bool cok = k0 + scol < d;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const long long gr = r0 + srow + RS * i;
      sx[i] = (cok && gr < n) ? *(const ST*)(x + gr * ldx + k0 + scol) : ST{};
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int row = srow + RS * i;
      sc[i] = (cok && row < k) ? *(const ST*)(cen + (long long)row * ldc + k0 + scol) : ST{};
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < d; k0 += KM_DK) {
#pragma unroll
    for (int i = 0; i < NX; ++i) *(ST*)(xs + (srow + RS * i) * KM_LD + scol) = sx[i];
#pragma unroll
    for (int i = 0; i < NC; ++i) *(ST*)(cs + (srow + RS * i) * KM_LD + scol) = sc[i];
    __syncthreads();
    if (k0 + KM_DK < d) fetch(k0 + KM_DK);
    // half-wave hl takes columns 16 hl + j at MFMA step j: both operands in the same order
    float4 a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = *(const float4*)(xs + (wave * 32 + l31) * KM_LD + 16 * hl + 4 * q);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 b = *(const float4*)(cs + (t * 32 + l31) * KM_LD + 16 * hl + 4 * q);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b.y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b.z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b.w, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // accumulator element i of a lane: point (i & 3) + 8 (i >> 2) + 4 hl of the wave's 32, centre 32 t + l31
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float best = INFINITY;
    int bi = 0x7FFFFFFF;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float s = fmaf(-2.f, acc[t][i], cns[t * 32 + l31]);
      if (s < best) {
        best = s;
        bi = t * 32 + l31;
      }
    }
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const float os = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (os < best || (os == best && oi < bi)) {
        best = os;
        bi = oi;
      }
    }
    if (l31 == 0) lab[wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * hl] = bi < k ? bi : 0;
  }
  __syncthreads();
  // the winner's distance, four rows in flight: lane l adds columns l, l + 64, ... of each row in
  // order (rows past n read row n - 1 and are dropped), then the fixed butterfly
  for (int rr = 0; rr < 32; rr += 4) {
    const float* xr[4];
    const float* cr[4];
    int c[4];
    float s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long gr = r0 + wave * 32 + rr + u;
      c[u] = lab[wave * 32 + rr + u];
      xr[u] = x + (gr < n ? gr : n - 1) * ldx;
      cr[u] = cen + (long long)c[u] * ldc;
      s[u] = 0.f;
    }
    for (int j = lane; j < d; j += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float df = xr[u][j] - cr[u][j];
        s[u] = fmaf(df, df, s[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = wave * 32 + rr + u;
      const long long gr = r0 + row;
      const float t = gr < n ? wave_sum(s[u]) : 0.f;
      if (lane == 0) {
        dd[row] = t;
        if (gr < n) {
          labels[gr] = c[u];
          if (dist2) dist2[gr] = t;
        }
      }
    }
  }
  __syncthreads();
  if (wave == 0) {
    const double v = wave_sum((double)dd[lane] + (double)dd[lane + 64]);
    if (lane == 0) ipart[blockIdx.x] = v;
  }
}

// 16 rows of one column and their labels (lane u & 15 holds row u's): issued a group ahead of their use
struct KmGroup {
  float v[16];
  int lb;
};
__device__ __forceinline__ void km_load_group(KmGroup& g, const float* __restrict__ x, long long ldx,
                                              const int32_t* __restrict__ labels, long long base, long long r1,
                                              int col, bool live, int lane) {
  g.lb = base + (lane & 15) < r1 ? labels[base + (lane & 15)] : -1;
#pragma unroll
  for (int u = 0; u < 16; ++u) g.v[u] = (live && base + u < r1) ? x[(base + u) * ldx + col] : 0.f;
}
__device__ __forceinline__ void km_add_group(const KmGroup& g, float* slab, int* cnt, int k, int lane, bool counting) {
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int lb = __builtin_amdgcn_readlane(g.lb, u);  // uniform: rows past the end carry -1
    if ((unsigned)lb < (unsigned)k) {
      slab[lb * KM_COLS + lane] += g.v[u];
      if (counting) cnt[lb] += 1;
    }
  }
}

// `sub` waves per workgroup: wave w walks rows [w, w + 1) * CHUNK / sub of the chunk in order into its
// own slab; the slabs are then added in wave order.  sub depends on k alone (km_sub).
__global__ __launch_bounds__(1024) void kmeans_stats_kernel(const float* __restrict__ x, long long ldx, long long n,
                                                            int d, int k, int sub,
                                                            const int32_t* __restrict__ labels,
                                                            float* __restrict__ part, int32_t* __restrict__ cpart) {
  extern __shared__ float slabs[];  // [sub][k][KM_COLS], then int cnt[sub][k]
  int* cnts = (int*)(slabs + (size_t)sub * k * KM_COLS);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* slab = slabs + (size_t)wave * k * KM_COLS;
  int* cnt = cnts + wave * k;
  const long long chunk = blockIdx.x;
  const int col = blockIdx.y * KM_COLS + lane;
  const bool live = col < d, counting = blockIdx.y == 0 && lane == 0;
  for (int c = 0; c < k; ++c) slab[c * KM_COLS + lane] = 0.f;
  for (int c = lane; c < k; c += 64) cnt[c] = 0;
  __syncthreads();
  const int per = CG_KMEANS_CHUNK / sub;
  const long long r0 = chunk * CG_KMEANS_CHUNK + (long long)wave * per;
  const long long r1 = r0 + per < n ? r0 + per : n;
  KmGroup ga, gb;
  km_load_group(ga, x, ldx, labels, r0, r1, col, live, lane);
  for (long long base = r0; base < r1; base += 32) {
    km_load_group(gb, x, ldx, labels, base + 16, r1, col, live, lane);
    km_add_group(ga, slab, cnt, k, lane, counting);
    km_load_group(ga, x, ldx, labels, base + 32, r1, col, live, lane);
    km_add_group(gb, slab, cnt, k, lane, counting);
  }
  __syncthreads();
  for (int c = wave; c < k; c += sub) {
    float s = slabs[c * KM_COLS + lane];
    for (int w = 1; w < sub; ++w) s += slabs[((size_t)w * k + c) * KM_COLS + lane];
    if (live) part[(chunk * k + c) * d + col] = s;
  }
  if (blockIdx.y == 0)
    for (int c = threadIdx.x; c < k; c += 64 * sub) {
      int s = 0;
      for (int w = 0; w < sub; ++w) s += cnts[w * k + c];
      cpart[chunk * k + c] = s;
    }
}

// element e < k d: sums[e]; e in [k d, k d + k): counts
__global__ __launch_bounds__(256) void kmeans_final_kernel(const float* __restrict__ part,
                                                           const int32_t* __restrict__ cpart, long long nchunk,
                                                           int k, int d, double* __restrict__ sums,
                                                           long long* __restrict__ counts) {
  const long long kd = (long long)k * d;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < kd) {
    double s = 0.0;
    for (long long c = 0; c < nchunk; ++c) s += (double)part[c * kd + e];
    sums[e] = s;
  } else if (e < kd + k) {
    const int cl = (int)(e - kd);
    long long s = 0;
    for (long long c = 0; c < nchunk; ++c) s += cpart[c * k + cl];
    counts[cl] = s;
  }
}

// thread t adds partials t, t + 256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void kmeans_inertia_kernel(const double* __restrict__ ipart, long long nb,
                                                             double* __restrict__ inertia) {
  __shared__ double red[256];
  double s = 0.0;
  for (long long i = threadIdx.x; i < nb; i += 256) s += ipart[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *inertia = red[0];
}

// waves per statistics workgroup: the power of two (at most 16) whose slabs fit 64 KiB of LDS
inline int km_sub(int k) {
  int sub = 16;
  while (sub > 1 && sub * k * (KM_COLS * 4 + 4) > 65536) sub >>= 1;
  return sub;
}
struct KmLayout {
  size_t cn, ipart, cpart, part, total;
  long long nblk, nchunk;
};
inline KmLayout km_layout(long long n, int d, int k) {
  KmLayout L;
  L.nblk = (n + KM_ROWS - 1) / KM_ROWS;
  L.nchunk = (n + CG_KMEANS_CHUNK - 1) / CG_KMEANS_CHUNK;
  L.cn = 0;
  L.ipart = cg_rup(256 * sizeof(float), 16);
  L.cpart = L.ipart + cg_rup((size_t)L.nblk * sizeof(double), 16);
  L.part = L.cpart + cg_rup((size_t)L.nchunk * k * sizeof(int32_t), 16);
  L.total = L.part + cg_rup((size_t)L.nchunk * k * d * sizeof(float), 16);
  return L;
}
}  // namespace

extern "C" int cg_window_keep(const int64_t* idx, int B, int T, int window, int stride, const uint32_t* exclude_mask,
                              int32_t* keep, void* stream) {
  if (B < 0 || T < 0 || window < 1 || stride < 1) return CG_EINVAL;
  const int nwin = win_count(T, window, stride);
  if (B == 0 || nwin == 0) return CG_OK;
  cg_id_mask em;
  if (!idx || !keep || !cg_mask_fill(em, exclude_mask)) return CG_EINVAL;
  const long long total = (long long)B * nwin;
  hipLaunchKernelGGL(window_keep_kernel, dim3(cg_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, idx, total,
                     nwin, T, window, stride, em, keep);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_window_pool(int dtype, const void* h, long long ldh, int B, int T, int d, int window, int stride,
                              const int32_t* dst_row, float* out, long long ldo, long long out_rows, void* stream) {
  if (B < 0 || T < 0 || d < 0 || out_rows < 0 || window < 1 || stride < 1 || ldh < d || ldo < d) return CG_EINVAL;
  if (dtype != CG_F32 && dtype != CG_BF16) return CG_EUNSUPPORTED;
  const int nwin = win_count(T, window, stride);
  if (B == 0 || d == 0 || nwin == 0) return CG_OK;
  if (!h || !dst_row || !out) return CG_EINVAL;
  const long long total = (long long)B * nwin;
  if (total > 0x7FFFFFFFLL) return CG_EUNSUPPORTED;
  const dim3 grid((unsigned)total, cg_cdiv(d, 256));
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(window_pool_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)h, ldh, nwin,
                       T, d, window, stride, dst_row, out, ldo, out_rows);
  else
    hipLaunchKernelGGL(window_pool_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)h, ldh, nwin,
                       T, d, window, stride, dst_row, out, ldo, out_rows);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" size_t cg_kmeans_workspace(long long n, int d, int k) {
  if (n <= 0 || k < 1 || k > 256 || d < 1 || d > 1024) return 0;
  return km_layout(n, d, k).total;
}

extern "C" int cg_kmeans_step(const cg_kmeans_desc* p, void* stream) {
  if (!p) return CG_EINVAL;
  if (p->k < 1 || p->k > 256 || p->d < 1 || p->d > 1024) return CG_EUNSUPPORTED;
  if (p->n < 0) return CG_EINVAL;
  if (p->n == 0) return CG_OK;
  if (!p->x || !p->centers || !p->labels || !p->workspace) return CG_EINVAL;
  if (p->ldx < p->d || p->ldc < p->d || (p->sums && !p->counts)) return CG_EINVAL;
  const KmLayout L = km_layout(p->n, p->d, p->k);
  if (p->ws_bytes < L.total || ((uintptr_t)p->workspace & 15)) return CG_EINVAL;
  if (L.nblk > 0x7FFFFFFFLL) return CG_EUNSUPPORTED;
  char* ws = (char*)p->workspace;
  float* cn = (float*)(ws + L.cn);
  double* ipart = (double*)(ws + L.ipart);
  int32_t* cpart = (int32_t*)(ws + L.cpart);
  float* part = (float*)(ws + L.part);
  hipStream_t s = (hipStream_t)stream;
  const int nt = p->k <= 32 ? 1 : p->k <= 64 ? 2 : p->k <= 128 ? 4 : 8;
  hipLaunchKernelGGL(kmeans_cnorm_kernel, dim3(nt * 8), dim3(256), 0, s, p->centers, p->ldc, p->k, p->d, nt * 32, cn);
  CG_LAUNCH_CHECK();
  const dim3 grid((unsigned)L.nblk), block(256);
  // 16-byte staging where every row of both operands takes it; the ranking products are the same
  // fma chains either way (the staged image is the same)
  const bool vec = p->d % 4 == 0 && p->ldx % 4 == 0 && p->ldc % 4 == 0 && !((uintptr_t)p->x & 15) &&
                   !((uintptr_t)p->centers & 15);
#define KM_ASSIGN(NT)                                                                                            \
  if (vec)                                                                                                       \
    hipLaunchKernelGGL((kmeans_assign_kernel<NT, true>), grid, block, 0, s, p->x, p->ldx, p->n, p->d, p->centers, \
                       p->ldc, p->k, cn, p->labels, p->dist2, ipart);                                            \
  else                                                                                                           \
    hipLaunchKernelGGL((kmeans_assign_kernel<NT, false>), grid, block, 0, s, p->x, p->ldx, p->n, p->d, p->centers, \
                       p->ldc, p->k, cn, p->labels, p->dist2, ipart)
  switch (nt) {
    case 1: KM_ASSIGN(1); break;
    case 2: KM_ASSIGN(2); break;
    case 4: KM_ASSIGN(4); break;
    default: KM_ASSIGN(8); break;
  }
#undef KM_ASSIGN
  CG_LAUNCH_CHECK();
  if (p->sums) {  // counts come with the sums (checked above)
    const int sub = km_sub(p->k);
    const int lds = sub * (p->k * KM_COLS * (int)sizeof(float) + p->k * (int)sizeof(int));
    cg_func_lds((const void*)kmeans_stats_kernel, lds);
    hipLaunchKernelGGL(kmeans_stats_kernel, dim3((unsigned)L.nchunk, cg_cdiv(p->d, KM_COLS)), dim3(KM_COLS * sub), lds,
                       s, p->x, p->ldx, p->n, p->d, p->k, sub, p->labels, part, cpart);
    CG_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_final_kernel, dim3(cg_cdiv((long long)p->k * p->d + p->k, 256)), dim3(256), 0, s, part,
                       cpart, L.nchunk, p->k, p->d, p->sums, p->counts);
    CG_LAUNCH_CHECK();
  }
  if (p->inertia) {
    hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(1), dim3(256), 0, s, ipart, L.nblk, p->inertia);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

// Structural regression probes (contract: include/codonlm_hip.h, cg_shape_targets / cg_gram_accum):
// per-codon DNAshape targets straight from token ids, and the grouped augmented Gram matrix of
// hidden states and targets in fp64 on v_mfma_f64_16x16x4_f64.
// No floating-point atomics: every sum has one owner and a fixed order.
#include <type_traits>
#include "common.h"

namespace {
typedef double v4d __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// cg_shape_targets
// ---------------------------------------------------------------------------
struct CodonTab {
  int8_t c[256];  // ids 0..255: 6 bits = three 2-bit nucleotides (first in the high bits), -1 = no codon
};

enum { NT_A = 0, NT_C = 1, NT_G = 2, NT_T = 3 };
constexpr uint32_t di(int a, int b) { return 1u << (a * 4 + b); }
constexpr uint32_t tetra(int a, int b, int c, int e) { return (uint32_t)(a << 6 | b << 4 | c << 2 | e); }

// the 14 values of one nucleotide from its window's facts: two (bit x*4 + y: the dinucleotide xy occurs)
// and four flags for the tetranucleotides the rules name.  First matching rule wins.
__device__ __forceinline__ void shape_rules(uint32_t two, bool aaaa, bool gggg, bool cccc, bool ggcc, double* v) {
  const bool aa = two & di(NT_A, NT_A), tt = two & di(NT_T, NT_T), gc = two & di(NT_G, NT_C),
             cg = two & di(NT_C, NT_G), at = two & di(NT_A, NT_T), ta = two & di(NT_T, NT_A);
  v[0] = aaaa ? 3.5 : (gggg || cccc) ? 5.8 : 4.5;      // MGW
  v[1] = (gc || cg) ? 5.0 : (aa || tt) ? 0.0 : 2.5;    // Roll
  v[2] = aaaa ? -10.0 : ggcc ? -2.0 : -5.0;            // EP
  v[3] = gc ? -11.0 : at ? -18.0 : -14.0;              // ProT
  v[4] = cg ? 36.0 : ta ? 32.0 : 34.0;                 // HelT
  v[5] = aaaa ? -0.8 : (gc || cg) ? 0.2 : -0.3;        // Slide
  v[6] = cg ? 3.2 : aa ? 3.4 : 3.3;                    // Rise
  v[7] = (aa || tt) ? 0.0 : gc ? 0.2 : -0.1;           // Shift
  v[8] = aa ? 0.0 : cg ? 0.5 : -0.2;                   // Tilt
  v[9] = gc ? -12.0 : at ? 0.0 : -6.0;                 // Buckle
  v[10] = at ? 2.0 : gc ? 0.5 : 1.0;                   // Opening
  v[11] = gc ? 0.0 : 0.1;                              // Shear
  v[12] = aa ? 0.1 : -0.1;                             // Stagger
  v[13] = cg ? -0.1 : 0.0;                             // Stretch
}

// one thread per token: its own three nucleotides, the last two of the previous codon of its run
// and the first two of the next -- seven slots, nt[2..4] its own
__global__ __launch_bounds__(256) void shape_targets_kernel(const int64_t* __restrict__ idx, long long total, int T,
                                                            CodonTab tab, float* __restrict__ y, long long ldy,
                                                            int32_t* __restrict__ valid) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= total) return;
  const int t = (int)(r % T);
  auto code = [&](long long rr) -> int {
    const int64_t v = idx[rr];
    return (v >= 0 && v < 256) ? (int)tab.c[v] : -1;
  };
  const int c = code(r);
  if (c < 0) {
    valid[r] = 0;
    return;
  }
  const int p = t > 0 ? code(r - 1) : -1;
  const int q = t + 1 < T ? code(r + 1) : -1;
  int nt[7];
  nt[0] = (p >> 2) & 3;
  nt[1] = p & 3;
  nt[2] = (c >> 4) & 3;
  nt[3] = (c >> 2) & 3;
  nt[4] = c & 3;
  nt[5] = (q >> 4) & 3;
  nt[6] = (q >> 2) & 3;
  const int lo = p < 0 ? 2 : 0, hi = q < 0 ? 5 : 7;  // the slots that exist: [lo, hi)
  double val[3][14];
#pragma unroll
  for (int i = 0; i < 3; ++i) {  // nucleotide i sits in slot 2 + i; its window is slots [i, i + 5) that exist
    const int a = i > lo ? i : lo, b = i + 5 < hi ? i + 5 : hi;
    uint32_t two = 0;
    bool aaaa = false, gggg = false, cccc = false, ggcc = false;
#pragma unroll
    for (int s = 0; s < 6; ++s)
      if (s >= a && s + 2 <= b) two |= 1u << (nt[s] * 4 + nt[s + 1]);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s >= a && s + 4 <= b) {
        const uint32_t w = (uint32_t)(nt[s] << 6 | nt[s + 1] << 4 | nt[s + 2] << 2 | nt[s + 3]);
        aaaa |= w == tetra(NT_A, NT_A, NT_A, NT_A);
        gggg |= w == tetra(NT_G, NT_G, NT_G, NT_G);
        cccc |= w == tetra(NT_C, NT_C, NT_C, NT_C);
        ggcc |= w == tetra(NT_G, NT_G, NT_C, NT_C);
      }
    shape_rules(two, aaaa, gggg, cccc, ggcc, val[i]);
  }
  float* out = y + r * ldy;
#pragma unroll
  for (int k = 0; k < 14; ++k) out[k] = (float)(((val[0][k] + val[1][k]) + val[2][k]) / 3.0);
  valid[r] = 1;
}

// ---------------------------------------------------------------------------
// cg_gram_accum.
//  1. gram_count_kernel: workgroup g counts the rows of group g (integers).
//  2. gram_perm_kernel: workgroup g writes the indices of its rows, ascending, at perm[off[g] ...),
//     off[g] = the counts of the groups before it: a stable sort of the member rows by group.  Rows
//     of no group are in no list, so nothing of them is ever read.
//  3. gram_tile_kernel: workgroup (pair, slice, g) owns the 64 x 64 block (I, J), I <= J, of group g's
//     Gram over slice `slice` of the group's list.  GR_KC rows at a time are gathered through the
//     list into LDS as fp32 (a wave reads 64 consecutive columns of a row; exact for fp32 and bf16
//     inputs) and widened to fp64 as MFMA operands; the next chunk's loads are in flight under this
//     chunk's MFMAs, the row indices a chunk further ahead.  4 waves in 2 x 2, a wave 32 x 32 = 2 x 2 accumulators of
//     v_mfma_f64_16x16x4_f64; both operands are fragments of the same staged chunk (Z^T Z).  The
//     block goes to the workspace as one partial.
//  4. gram_final_kernel: one thread per (g, i, j): the slices' partials of element (min, max) added
//     in slice order, then added to or written over gram -- (i, j) and (j, i) read the same words.
// ---------------------------------------------------------------------------
constexpr int GR_BLK = 64;   // block edge
#ifndef CG_GRAM_KC
#define CG_GRAM_KC 16  // 16 and 32 time alike for fp32 hidden states, 16 is faster for bf16
#endif
constexpr int GR_KC = CG_GRAM_KC;  // rows per LDS stage (a multiple of 4)
constexpr int GR_LD = 144;   // row stride of a stage in floats: 128 + 16, the four k rows of an MFMA
                             // operand start 64 bytes apart modulo 256
constexpr int GR_MAX_G = 4096;
constexpr int GR_MAX_P = 8192;
constexpr long long GR_MAX_ROWS = 1LL << 30;

__global__ __launch_bounds__(1024) void gram_count_kernel(const int32_t* __restrict__ grp, long long rows,
                                                          int32_t* __restrict__ cnt) {
  __shared__ int wc[16];
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int n = 0;
  for (long long r = threadIdx.x; r < rows; r += 1024) n += grp[r] == g;
  n = wave_sum(n);
  if (lane == 0) wc[wave] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < 16; ++w) s += wc[w];
    cnt[g] = s;
  }
}

__global__ __launch_bounds__(1024) void gram_perm_kernel(const int32_t* __restrict__ grp, long long rows,
                                                         const int32_t* __restrict__ cnt, int32_t* __restrict__ off,
                                                         int32_t* __restrict__ perm) {
  __shared__ int wc[16];
  __shared__ int base_s;
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    int b = 0;
    for (int i = 0; i < g; ++i) b += cnt[i];
    base_s = b;
    off[g] = b;
  }
  __syncthreads();
  int run = base_s;  // where the next member row of this group goes (uniform)
  for (long long r0 = 0; r0 < rows; r0 += 1024) {
    const long long r = r0 + threadIdx.x;
    const bool in = r < rows && grp[r] == g;
    const unsigned long long bal = __ballot(in);
    if (lane == 0) wc[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; ++w) {
      const int c = wc[w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (in) perm[run + before + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)r;
    run += all;
    __syncthreads();
  }
}

// rows of the slice: the group's list cut into `S` runs of equal length, a multiple of GR_KC
// (int: rows <= GR_MAX_ROWS = 2^30 leaves room for the rounding and for positions a few stages past the end)
__device__ __forceinline__ void gram_slice(int n, int S, int s, int& a, int& b) {
  const int per = ((n + S - 1) / S + GR_KC - 1) / GR_KC * GR_KC;
  a = s * per < n ? s * per : n;
  b = a + per < n ? a + per : n;
}

template <typename T_>
__global__ __launch_bounds__(256) void gram_tile_kernel(const T_* __restrict__ h, long long ldh, int d,
                                                        const float* __restrict__ y, long long ldy, int m,
                                                        const int32_t* __restrict__ cnt,
                                                        const int32_t* __restrict__ off,
                                                        const int32_t* __restrict__ perm, int nb, int S,
                                                        double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float zs[GR_KC * GR_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // block pair (I, J), I <= J, from the linear index (row-major over the upper triangle)
  int I = 0, rem = blockIdx.x;
  while (rem >= nb - I) {
    rem -= nb - I;
    ++I;
  }
  const int J = I + rem;
  const int s = blockIdx.y, g = blockIdx.z;
  int ra, rb;
  gram_slice(cnt[g], S, s, ra, rb);
  const int32_t* __restrict__ list = perm + off[g];
  // staging: thread -> column sc of the 128 staged (64 of I, then 64 of J), rows sr, sr + 2, ...; the
  // values stay fp32 (what the inputs hold) and are widened as MFMA operands.  Row indices are
  // fetched two chunks ahead, values one chunk ahead.
  const int sc = tid & 127, sr = tid >> 7;
  const int gc = (sc < GR_BLK ? I * GR_BLK + sc : J * GR_BLK + sc - GR_BLK);  // column of z
  const int P = d + m + 1;
  int ri[GR_KC / 2];
  float st[GR_KC / 2];
  auto fetch_rows = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < GR_KC / 2; ++i) {
      const int pos = k0 + sr + 2 * i;
      ri[i] = pos < rb ? list[pos] : -1;
    }
  };
  auto fetch = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < GR_KC / 2; ++i) {
      const long long r = ri[i];
      float v = 0.f;
      if (r >= 0 && gc < P) {
        if (gc < d)
          v = ld_act<T_>(h + r * ldh + gc);
        else if (gc < d + m)
          v = y[r * ldy + (gc - d)];
        else
          v = 1.f;
      }
      st[i] = v;
    }
  };
  v4d acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[a][b][e] = 0.0;
  const int wi = wave >> 1, wj = wave & 1, l15 = lane & 15, kq = lane >> 4;
  fetch_rows(ra);
  fetch();
  fetch_rows(ra + GR_KC);
  for (int k0 = ra; k0 < rb; k0 += GR_KC) {
#pragma unroll
    for (int i = 0; i < GR_KC / 2; ++i) zs[(sr + 2 * i) * GR_LD + sc] = st[i];
    __syncthreads();
    fetch();
    fetch_rows(k0 + 2 * GR_KC);
#pragma unroll
    for (int kk = 0; kk < GR_KC / 4; ++kk) {
      // lane: A[i = l15][k = kq] = z[k][i], B[k = kq][j = l15] = z[k][j]
      const float* row = zs + (kk * 4 + kq) * GR_LD;
      const double a0 = (double)row[wi * 32 + l15], a1 = (double)row[wi * 32 + 16 + l15];
      const double b0 = (double)row[GR_BLK + wj * 32 + l15], b1 = (double)row[GR_BLK + wj * 32 + 16 + l15];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 reg
  double* out = part + (((size_t)g * S + s) * gridDim.x + blockIdx.x) * (GR_BLK * GR_BLK);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        out[(wi * 32 + a * 16 + kq + 4 * e) * GR_BLK + wj * 32 + b * 16 + l15] = acc[a][b][e];
}

__global__ __launch_bounds__(256) void gram_final_kernel(const double* __restrict__ part, int P, int nb, int S,
                                                         int npair, long long total, int accumulate,
                                                         double* __restrict__ gram, long long ldg) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % P);
  const long long gi = e / P;
  const int i = (int)(gi % P);
  const long long g = gi / P;
  const int a = i < j ? i : j, b = i < j ? j : i;
  const int I = a / GR_BLK, J = b / GR_BLK;
  const int pair = I * nb - I * (I - 1) / 2 + (J - I);
  const double* p = part + ((size_t)g * S * npair + pair) * (GR_BLK * GR_BLK) + (a % GR_BLK) * GR_BLK + b % GR_BLK;
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += p[(size_t)s * npair * (GR_BLK * GR_BLK)];
  double* o = gram + (g * P + i) * ldg + j;
  *o = accumulate ? *o + sum : sum;
}

struct GramLayout {
  size_t cnt, off, perm, part, total;
  int nb, npair, S;
};
// slices per group: enough workgroups for the machine, no slice below 64 rows of an even split;
// fixed by (rows, P, G)
inline GramLayout gram_layout(long long rows, int P, int G) {
  GramLayout L;
  L.nb = (P + GR_BLK - 1) / GR_BLK;
  L.npair = L.nb * (L.nb + 1) / 2;
  long long S = (1024 + (long long)G * L.npair - 1) / ((long long)G * L.npair);
  const long long cap = rows / ((long long)G * 64);
  if (S > cap) S = cap;
  if (S > 16) S = 16;
  if (S < 1) S = 1;
  L.S = (int)S;
  L.cnt = 0;
  L.off = cg_rup((size_t)G * sizeof(int32_t), 256);
  L.perm = L.off + cg_rup((size_t)G * sizeof(int32_t), 256);
  L.part = L.perm + cg_rup((size_t)rows * sizeof(int32_t), 256);
  L.total = L.part + (size_t)G * L.S * L.npair * GR_BLK * GR_BLK * sizeof(double);
  return L;
}
inline bool gram_sizes_ok(long long rows, int d, int m, int G) {
  return rows >= 0 && rows <= GR_MAX_ROWS && d >= 0 && m >= 0 && G >= 1;
}
inline bool gram_sizes_supported(int d, int m, int G) { return (long long)d + m + 1 <= GR_MAX_P && G <= GR_MAX_G; }
}  // namespace

extern "C" int cg_shape_targets(const int64_t* idx, int B, int T, const int32_t* codon_of, int V, float* y,
                                long long ldy, int32_t* valid, void* stream) {
  if (B < 0 || T < 0 || V < 0 || V > 256 || ldy < CG_SHAPE_TARGETS) return CG_EINVAL;
  if (B == 0 || T == 0) return CG_OK;
  if (!idx || !y || !valid || (V > 0 && !codon_of)) return CG_EINVAL;
  CodonTab tab;
  for (int i = 0; i < 256; ++i) {
    tab.c[i] = -1;
    if (i < V && codon_of[i] >= 0) {
      if (codon_of[i] > 63) return CG_EINVAL;
      tab.c[i] = (int8_t)codon_of[i];
    }
  }
  const long long total = (long long)B * T;
  if (total > 0x7FFFFFFFLL * 256) return CG_EUNSUPPORTED;
  hipLaunchKernelGGL(shape_targets_kernel, dim3(cg_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, idx, total, T,
                     tab, y, ldy, valid);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" size_t cg_gram_workspace(long long rows, int d, int m, int G) {
  if (!gram_sizes_ok(rows, d, m, G) || !gram_sizes_supported(d, m, G)) return 0;
  return gram_layout(rows, d + m + 1, G).total;
}

extern "C" int cg_gram_accum(int dtype, const void* h, long long ldh, int d, const float* y, long long ldy, int m,
                             const int32_t* grp, long long rows, int G, int accumulate, double* gram, long long ldg,
                             void* workspace, size_t ws_bytes, void* stream) {
  if (!gram_sizes_ok(rows, d, m, G) || ldh < d || ldy < m || (accumulate != 0 && accumulate != 1)) return CG_EINVAL;
  const int P = d + m + 1;
  if (ldg < P) return CG_EINVAL;
  if (dtype != CG_F32 && dtype != CG_BF16) return CG_EUNSUPPORTED;
  if (!gram_sizes_supported(d, m, G)) return CG_EUNSUPPORTED;
  if (rows == 0 && accumulate) return CG_OK;
  if (!gram) return CG_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long total = (long long)G * P * P;
  if (total > 0x7FFFFFFFLL * 256) return CG_EUNSUPPORTED;
  if (rows == 0) {  // overwrite with the empty sums
    hipLaunchKernelGGL(gram_final_kernel, dim3(cg_cdiv(total, 256)), dim3(256), 0, s, (const double*)nullptr, P, 1, 0,
                       1, total, 0, gram, ldg);
    CG_LAUNCH_CHECK();
    return CG_OK;
  }
  if ((d > 0 && !h) || (m > 0 && !y) || !grp || !workspace || ((uintptr_t)workspace & 255)) return CG_EINVAL;
  const GramLayout L = gram_layout(rows, P, G);
  if (ws_bytes < L.total) return CG_EINVAL;
  char* ws = (char*)workspace;
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  int32_t* off = (int32_t*)(ws + L.off);
  int32_t* perm = (int32_t*)(ws + L.perm);
  double* part = (double*)(ws + L.part);
  hipLaunchKernelGGL(gram_count_kernel, dim3(G), dim3(1024), 0, s, grp, rows, cnt);
  CG_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_perm_kernel, dim3(G), dim3(1024), 0, s, grp, rows, cnt, off, perm);
  CG_LAUNCH_CHECK();
  const dim3 grid(L.npair, L.S, G);
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(gram_tile_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)h, ldh, d, y, ldy, m, cnt, off,
                       perm, L.nb, L.S, part);
  else
    hipLaunchKernelGGL(gram_tile_kernel<float>, grid, dim3(256), 0, s, (const float*)h, ldh, d, y, ldy, m, cnt, off,
                       perm, L.nb, L.S, part);
  CG_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_final_kernel, dim3(cg_cdiv(total, 256)), dim3(256), 0, s, part, P, L.nb, L.S, L.npair, total,
                     accumulate, gram, ldg);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

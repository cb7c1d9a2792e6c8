// Multi-offset priors of a decode step (contract: include/codonlm_hip.h, cg_offset_prior_add):
//   logits[b] += weight[i] * head(W2_i gelu(W1_i hist[b][pos[b]+1-k_i] + b1_i) + b2_i)
// in three launches whatever the number of heads:
//   stage 1  u1[i][b] = gelu(W1_i x + b1_i), x gathered from the ln_f history by the kernel itself
//   stage 2  u2[i][b] = W2_i u1[i][b] + b2_i
//   stage 3  logits[b][v] += sum_i weight[i] * (head[v] . u2[i][b]), heads in the caller's order
//
// One kernel body serves the three.  A workgroup owns TN output columns of one head (stage 3: of
// the shared head matrix, for every offset head in turn) and a tile of 64 rows of the batch.  Its
// slice of the weight goes into LDS once, as fp32.  A lane is a ROW of the batch: it reads its own
// input row (stage 1: straight from the history row pos + 1 - k of its sequence) into registers,
// 32 elements at a time (the next chunk's loads in flight under this one's FMAs), and
// every weight element it multiplies by is an LDS broadcast read, so there is no cross-lane
// reduction at all.  The four waves split the d-long dot product into four
// contiguous k ranges; each lane runs one ascending FMA chain per (row, column) over its range,
// and the four partial sums meet in LDS and are added as ((p0 + p1) + p2) + p3.  That order is the
// same for every row whatever the batch or the other rows are: a row's result does not depend on B.
// A (row, head) pair that is inactive (row outside [0, Tmax), zero weight, or pos + 1 - k < 0) is
// skipped in all three stages by the same predicate: nothing of it is read or written.  Loads
// are kept free of per-load branches (the compiler waits for every outstanding load where such a
// branch joins): what a load must not fetch is replaced by an in-bounds address and zeros.
#include <type_traits>
#include "common.h"
#include "offset_prior.h"

namespace {
constexpr int OP_LDS_MAX = 160 * 1024;

// the history row the pair (row at position p, head i) reads, or -1
__device__ __forceinline__ int pair_src(const cg_offprior_args& a, int p, int i) {
  if (p < 0 || p >= a.Tmax || a.weight[i] == 0.f || a.offset[i] < 1) return -1;
  const int src = p + 1 - a.offset[i];
  return src >= 0 ? src : -1;
}

// kw: the k range of one wave (a multiple of 8), kwp: kw rounded up to XK; vec: every input row
// starts on a 16-byte boundary.  XK: the input elements a lane holds per step; a step is one
// (head, XK-chunk) pair, and the loads of step s + 1 are issued before the FMAs of step s.
template <typename T_, int STAGE, int TN, int XK>
__global__ __launch_bounds__(256) void offset_prior_kernel(cg_offprior_args a, int kw, int kwp, int vec) {
  constexpr int EPL = 16 / sizeof(T_);  // 16 bytes of a row as floats
  constexpr int NO = TN * 64 / 256;  // outputs a thread finishes
  extern __shared__ __attribute__((aligned(16))) float op_smem[];
  float* Ws = op_smem;                   // [TN][4 waves][kwp], zero beyond the N columns and the d elements
  float* red = op_smem + TN * 4 * kwp;   // [4 waves][TN][64 rows]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int d = a.d, B = a.B;
  const int N = STAGE == 3 ? a.V : d;
  const int n0 = blockIdx.x * TN;
  const int b0 = blockIdx.z * 64, b = b0 + lane;
  const int i_lo = STAGE == 3 ? 0 : (int)blockIdx.y, n_i = STAGE == 3 ? a.n : 1;

  // positions are read once: this lane's row, and the rows whose outputs this thread finishes
  // ((row, column) = (o / TN, o % TN), o = tid + 256 t); -1 = no such row
  const int p_lane = b < B ? a.pos[b] : -1;
  int p_out[NO];
#pragma unroll
  for (int t = 0; t < NO; ++t) {
    const int row = b0 + (tid + 256 * t) / TN;
    p_out[t] = row < B ? a.pos[row] : -1;
  }
  // nothing to do for this workgroup's rows: leave before the weight slice is fetched
  int any_pair = 0;
  for (int i = i_lo; i < i_lo + n_i; ++i) any_pair |= pair_src(a, p_lane, i) >= 0;
  if (!__syncthreads_or(any_pair)) return;

  const int k0 = wave * kw, kend = min(d, k0 + kw);
  const int nchunk = kwp / XK, nstep = n_i * nchunk;
  // this lane's row of head i, elements k0 + kc .. + XK, as floats (zeros: inactive pair, past kend)
  auto load_x = [&](int step, float (&xr)[XK]) {
    const int i = i_lo + step / nchunk, kc = (step % nchunk) * XK;
    const int src = pair_src(a, p_lane, i);
    const T_* x = nullptr;
    if (src >= 0)
      x = STAGE == 1 ? (const T_*)a.hist + ((long long)b * a.Tmax + src) * d
                     : (const T_*)(STAGE == 2 ? a.u1 : a.u2) + ((long long)i * B + b) * d;
    if (vec) {
      // one branch around all of the step's loads (a branch per load would make each wait for the
      // one before it).  kend is a multiple of EPL here, so a 16-byte group is inside the wave's
      // range or outside it, the same for every lane: a group outside reads element 0 of the row
      // instead and is replaced by zeros
#pragma unroll
      for (int j = 0; j < XK; ++j) xr[j] = 0.f;
      if (x) {
#pragma unroll
        for (int j = 0; j < XK; j += EPL) {
          const int k = k0 + kc + j;
          const bool in = k + EPL <= kend;
          float v[EPL];
          ld_vec<EPL>(x + (in ? k : 0), v);
#pragma unroll
          for (int e = 0; e < EPL; ++e) xr[j + e] = in ? v[e] : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < XK; ++j) xr[j] = (x && k0 + kc + j < kend) ? ld_act<T_>(x + k0 + kc + j) : 0.f;
    }
  };
  float xa[XK], xb[XK];
  load_x(0, xa);  // (in flight while the weight slice is staged)

  const T_* w = (const T_*)(STAGE == 1 ? a.w1[i_lo] : STAGE == 2 ? a.w2[i_lo] : a.head);
  if (vec) {
    // 16 bytes per load, every load of a thread issued before the first LDS write; a 16-byte group
    // lies inside one wave's k range (kw is a multiple of 8)
    for (int e = tid; e < TN * 4 * kwp / 4; e += 256) ((float4*)Ws)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    constexpr int QMAX = 4;  // groups per thread and pass
    const int gpr = d / EPL, ngroup = TN * gpr;
    for (int q0 = 0; q0 < ngroup; q0 += 256 * QMAX) {
      float v[QMAX][EPL];
#pragma unroll
      for (int u = 0; u < QMAX; ++u) {  // (no branch: a group past the slice reads the slice's first instead)
        const int q = q0 + tid + 256 * u;
        const bool in = q < ngroup && n0 + q / gpr < N;
        ld_vec<EPL>(w + (in ? (long long)(n0 + q / gpr) * d + (q % gpr) * EPL : (long long)n0 * d), v[u]);
      }
#pragma unroll
      for (int u = 0; u < QMAX; ++u) {
        const int q = q0 + tid + 256 * u;
        if (q < ngroup && n0 + q / gpr < N) {
          const int c = q / gpr, k = (q % gpr) * EPL, wv = k / kw;
          float* dst = Ws + (c * 4 + wv) * kwp + (k - wv * kw);
#pragma unroll
          for (int e = 0; e < EPL; ++e) dst[e] = v[u][e];
        }
      }
    }
  } else {
    for (int row = wave; row < TN * 4; row += 4) {  // row = (column c, k range wv) of the slice
      const int c = row >> 2, wv = row & 3;
      for (int j = lane; j < kwp; j += 64) {
        const int k = wv * kw + j;
        Ws[row * kwp + j] = (n0 + c < N && j < kw && k < d) ? ld_act<T_>(w + (long long)(n0 + c) * d + k) : 0.f;
      }
    }
  }
  float out_acc[NO];
  bool out_hit[NO];
#pragma unroll
  for (int t = 0; t < NO; ++t) {
    const int o = tid + 256 * t, row = b0 + o / TN, col = n0 + o % TN;
    out_hit[t] = false;
    out_acc[t] = (STAGE == 3 && row < B && col < N) ? a.logits[(long long)row * a.ldl + col] : 0.f;
  }
  float acc[TN];
  __syncthreads();  // the weight slice

  auto compute = [&](int step, const float (&xr)[XK]) {
    const int i = i_lo + step / nchunk, kc = (step % nchunk) * XK;
    if (kc == 0) {
#pragma unroll
      for (int c = 0; c < TN; ++c) acc[c] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < XK; j += 4) {
#pragma unroll
      for (int c = 0; c < TN; ++c) {
        const float4 wv = *(const float4*)(Ws + (c * 4 + wave) * kwp + kc + j);  // one address: a broadcast
        acc[c] = fmaf(xr[j], wv.x, acc[c]);
        acc[c] = fmaf(xr[j + 1], wv.y, acc[c]);
        acc[c] = fmaf(xr[j + 2], wv.z, acc[c]);
        acc[c] = fmaf(xr[j + 3], wv.w, acc[c]);
      }
    }
    if (kc + XK < kwp) return;
    // the head's four partial sums meet: ((p0 + p1) + p2) + p3
    if (step >= nchunk) __syncthreads();  // the previous head's readers of `red`
#pragma unroll
    for (int c = 0; c < TN; ++c) red[(wave * TN + c) * 64 + lane] = acc[c];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      const int o = tid + 256 * t, r = o / TN, c = o % TN;
      const int row = b0 + r, col = n0 + c;
      if (col < N && pair_src(a, p_out[t], i) >= 0) {
        const float s = ((red[(0 * TN + c) * 64 + r] + red[(1 * TN + c) * 64 + r]) + red[(2 * TN + c) * 64 + r]) +
                        red[(3 * TN + c) * 64 + r];
        if constexpr (STAGE == 3) {
          out_acc[t] = fmaf(a.weight[i], s, out_acc[t]);
          out_hit[t] = true;
        } else {
          float v = s + (STAGE == 1 ? a.b1[i] : a.b2[i])[col];
          if constexpr (STAGE == 1) v = std::is_same<T_, bf16_t>::value ? gelu_fast(v) : gelu_f(v);
          st_act<T_>((T_*)(STAGE == 1 ? a.u1 : a.u2) + ((long long)i * B + row) * d + col, v);
        }
      }
    }
  };
  for (int step = 0; step < nstep; step += 2) {  // (nstep and step are uniform: the barriers are too)
    if (step + 1 < nstep) load_x(step + 1, xb);
    compute(step, xa);
    if (step + 1 >= nstep) break;
    if (step + 2 < nstep) load_x(step + 2, xa);
    compute(step + 1, xb);
  }
  if constexpr (STAGE == 3) {
#pragma unroll
    for (int t = 0; t < NO; ++t) {
      const int o = tid + 256 * t;
      if (out_hit[t]) a.logits[(long long)(b0 + o / TN) * a.ldl + n0 + o % TN] = out_acc[t];
    }
  }
}

template <typename T_, int STAGE, int TN, int XK>
int launch_stage_xk(const cg_offprior_args& a, int kw, hipStream_t s) {
  constexpr int EPL = 16 / sizeof(T_);  // 16 bytes of a row as floats
  const int N = STAGE == 3 ? a.V : a.d;
  const int kwp = (kw + XK - 1) / XK * XK;
  const size_t lds = ((size_t)TN * 4 * kwp + 4 * TN * 64) * sizeof(float);
  if (lds > (size_t)OP_LDS_MAX) return CG_EUNSUPPORTED;
  // 16-byte loads: every input row and every weight row on a 16-byte boundary
  uintptr_t ptrs = (uintptr_t)(STAGE == 1 ? a.hist : STAGE == 2 ? a.u1 : a.u2) | (uintptr_t)a.head;
  for (int i = 0; i < a.n; ++i) ptrs |= (uintptr_t)a.w1[i] | (uintptr_t)a.w2[i];
  const int vec = a.d % EPL == 0 && ptrs % 16 == 0;
  const dim3 g(cg_cdiv(N, TN), STAGE == 3 ? 1 : a.n, cg_cdiv(a.B, 64));
  cg_func_lds((const void*)offset_prior_kernel<T_, STAGE, TN, XK>, (int)lds);
  hipLaunchKernelGGL((offset_prior_kernel<T_, STAGE, TN, XK>), g, dim3(256), lds, s, a, kw, kwp, vec);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

template <typename T_, int STAGE, int TN>
int launch_stage(const cg_offprior_args& a, hipStream_t s) {
  // (64 elements per step were tried: two such buffers leave the compiler short of registers, and it
  // then waits for every load before it issues the next)
  return launch_stage_xk<T_, STAGE, TN, 32>(a, (cg_cdiv(a.d, 4) + 7) / 8 * 8, s);
}

template <typename T_>
int launch_all(const cg_offprior_args& a, hipStream_t s) {
  int r = launch_stage<T_, 1, 8>(a, s);
  if (r == CG_OK) r = launch_stage<T_, 2, 8>(a, s);
  if (r == CG_OK) r = launch_stage<T_, 3, 4>(a, s);
  return r;
}
}  // namespace

extern "C" int cg_offset_prior_stages(const cg_offprior_args* a, void* stream) {
  if (!a || a->n < 1 || a->n > 8 || a->B <= 0 || a->d <= 0 || a->V <= 0 || a->Tmax <= 0 || a->ldl < a->V)
    return CG_EINVAL;
  if (!a->hist || !a->pos || !a->u1 || !a->u2 || !a->logits || !a->head) return CG_EINVAL;
  for (int i = 0; i < a->n; ++i)
    if (!a->w1[i] || !a->w2[i] || !a->b1[i] || !a->b2[i]) return CG_EINVAL;
  if (a->dtype == CG_BF16) return launch_all<bf16_t>(*a, (hipStream_t)stream);
  if (a->dtype == CG_F32) return launch_all<float>(*a, (hipStream_t)stream);
  return CG_EUNSUPPORTED;
}

// Fused termination-head loss (contract: include/codonlm_hip.h, cg_term_ce_fwd / cg_term_ce_bwd):
// the class-weighted, ignore_index cross-entropy of a small linear head over the labelled rows only.
// No floating-point atomics: every sum has one owner and a fixed order.
//
// Rows are taken in chunks of 64, one wave per chunk, lane = row for the labels: a ballot of the
// labelled lanes gives the rows the wave then visits in ascending order.  A row without a label
// costs its label read and nothing else.
//  1. term_fwd_kernel: per labelled row the C logits (lanes over the columns, 16-byte loads with an
//     element tail, one fma chain per lane and class, the fixed wave butterfly), log-sum-exp, the
//     row's probabilities to the workspace, the chunk's (sum w nll, sum w) as fp64 partials.
//  2. term_loss_kernel: the partials added in chunk order -> loss, sums, and the header the backward reads.
//  3. term_bwd_kernel: a wave owns (chunk, 256 columns), a lane 4 adjacent columns: g of the chunk's
//     rows goes through LDS, the rows are visited in order, dW partials stay in registers, dx is written
//     per row.  db partials by the chunk's first column slab.
//  4. term_reduce_kernel: the chunks' dW / db partials added in chunk order in fp64.
#include <math.h>
#include "common.h"

namespace {
constexpr int TC_ROWS = 64;    // rows per chunk = lanes per wave
constexpr int TC_COLS = 256;   // columns per backward wave (4 per lane)
constexpr int TC_MAXC = 16;

// the lane's label: y in [0, C) and its class weight, or y = -1 (ignore_index, out of range, past the end)
__device__ __forceinline__ int lane_label(const int64_t* __restrict__ labels, long long r, long long rows, int C,
                                          long long ignore, const float* __restrict__ class_w, float& wy) {
  wy = 0.f;
  if (r >= rows) return -1;
  const int64_t lb = labels[r];
  if (lb == ignore || lb < 0 || lb >= C) return -1;
  wy = class_w ? class_w[lb] : 1.f;
  return (int)lb;
}

template <typename T, int CP, bool VEC>
__global__ __launch_bounds__(256) void term_fwd_kernel(const T* __restrict__ x, long long ldx, long long rows, int d,
                                                       int C, const float* __restrict__ W, long long ldw,
                                                       const float* __restrict__ bias,
                                                       const int64_t* __restrict__ labels, long long ignore,
                                                       const float* __restrict__ class_w, float* __restrict__ prob,
                                                       double* __restrict__ lpart) {
  const int lane = threadIdx.x & 63;
  const long long chunk = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long base = chunk * TC_ROWS;
  if (base >= rows) return;
  float wy;
  const int y = lane_label(labels, base + lane, rows, C, ignore, class_w, wy);
  unsigned long long todo = __ballot(y >= 0);
  const int d4 = VEC ? (d & ~3) : 0;
  float my = 0.f;
  while (todo) {
    const int u = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const long long r = base + u;
    const int yu = __shfl(y, u);
    const T* __restrict__ xr = x + r * ldx;
    float acc[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[c] = 0.f;
    for (int j = 4 * lane; j < d4; j += 256) {
      float xv[4];
      ld_vec<4>(xr + j, xv);
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) {
          const float4 wv = *(const float4*)(W + c * ldw + j);
          acc[c] = fmaf(xv[0], wv.x, acc[c]);
          acc[c] = fmaf(xv[1], wv.y, acc[c]);
          acc[c] = fmaf(xv[2], wv.z, acc[c]);
          acc[c] = fmaf(xv[3], wv.w, acc[c]);
        }
    }
    for (int j = d4 + lane; j < d; j += 64) {
      const float xs = ld_act<T>(xr + j);
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) acc[c] = fmaf(xs, W[c * ldw + j], acc[c]);
    }
    float mx = -INFINITY, ly = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) {
        acc[c] = wave_sum(acc[c]) + bias[c];
        mx = fmaxf(mx, acc[c]);
        if (c == yu) ly = acc[c];
      }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) se += expf(acc[c] - mx);
    const float lse = mx + logf(se);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) prob[r * C + c] = expf(acc[c] - lse);
    }
    if (lane == u) my = wy * (lse - ly);
  }
  const double num = wave_sum((double)my);
  const double den = wave_sum((double)wy);
  if (lane == 0) {
    lpart[2 * chunk] = num;
    lpart[2 * chunk + 1] = den;
  }
}

// thread t adds partials t, t + 256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void term_loss_kernel(const double* __restrict__ lpart, long long nchunk,
                                                        double* __restrict__ hdr, float* __restrict__ loss,
                                                        float* __restrict__ sums) {
  __shared__ double red[2][256];
  double n = 0.0, dn = 0.0;
  for (long long i = threadIdx.x; i < nchunk; i += 256) {
    n += lpart[2 * i];
    dn += lpart[2 * i + 1];
  }
  red[0][threadIdx.x] = n;
  red[1][threadIdx.x] = dn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    hdr[0] = red[0][0];
    hdr[1] = red[1][0];
    if (loss) *loss = (float)(red[0][0] / red[1][0]);  // no labelled row: 0 / 0 = NaN
    if (sums) {
      sums[0] = (float)red[0][0];
      sums[1] = (float)red[1][0];
    }
  }
}

template <typename T, int CP, bool VEC>
__global__ __launch_bounds__(64) void term_bwd_kernel(const T* __restrict__ x, long long ldx, long long rows, int d,
                                                      int C, const float* __restrict__ W, long long ldw,
                                                      const int64_t* __restrict__ labels, long long ignore,
                                                      const float* __restrict__ class_w, float scale,
                                                      const float* __restrict__ scale_dev,
                                                      const double* __restrict__ hdr, const float* __restrict__ prob,
                                                      float* __restrict__ dwpart, float* __restrict__ dbpart,
                                                      float* __restrict__ dx, long long lddx, int acc_dx) {
  __shared__ float gs[TC_ROWS][CP];
  const int lane = threadIdx.x;
  const long long chunk = blockIdx.x;
  const long long base = chunk * TC_ROWS;
  const int col0 = (blockIdx.y * 64 + lane) * 4;
  float wy;
  const int y = lane_label(labels, base + lane, rows, C, ignore, class_w, wy);
  {
    const float s = scale * (scale_dev ? *scale_dev : 1.f);
    const float coef = y >= 0 ? s * wy / (float)hdr[1] : 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      gs[lane][c] = (y >= 0 && c < C) ? coef * (prob[(base + lane) * C + c] - (c == y ? 1.f : 0.f)) : 0.f;
  }
  __syncthreads();
  const unsigned long long lab = __ballot(y >= 0);
  if (dbpart && blockIdx.y == 0 && lane < C) {
    float s = 0.f;
    for (int u = 0; u < TC_ROWS; ++u) s += gs[u][lane];  // unlabelled rows hold 0
    dbpart[chunk * TC_MAXC + lane] = s;
  }
  if (col0 >= d) return;
  const bool full = VEC && col0 + 3 < d;  // the lane's four columns as one 16-byte piece
  float wr[CP][4], acc[CP][4];
#pragma unroll
  for (int c = 0; c < CP; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc[c][k] = 0.f;
      wr[c][k] = (dx && c < C && col0 + k < d) ? W[c * ldw + col0 + k] : 0.f;
    }
  auto load_x = [&](int u, float* v) __attribute__((always_inline)) {
    const T* __restrict__ p = x + (base + u) * ldx + col0;
    if (full) {
      ld_vec<4>(p, v);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = col0 + k < d ? ld_act<T>(p + k) : 0.f;
    }
  };
  // rows to visit: the labelled ones, and with a dx that is overwritten every row of the chunk
  const long long left = rows - base;
  const unsigned long long all = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
  unsigned long long todo = (dx && !acc_dx) ? all : lab;
  // the next labelled row's x is in flight under this row's arithmetic
  float xn[4] = {0.f, 0.f, 0.f, 0.f};
  if (lab) load_x(__ffsll((long long)lab) - 1, xn);
  while (todo) {
    const int u = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    float* __restrict__ dr = dx ? dx + (base + u) * lddx + col0 : nullptr;
    float dv[4] = {0.f, 0.f, 0.f, 0.f};
    const bool is_lab = (lab >> u) & 1ull;
    if (is_lab) {
      float xv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xv[k] = xn[k];
      const unsigned long long later = lab & ~((2ull << u) - 1ull);
      if (later) load_x(__ffsll((long long)later) - 1, xn);
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) {
          const float g = gs[u][c];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            acc[c][k] = fmaf(g, xv[k], acc[c][k]);
            dv[k] = fmaf(g, wr[c][k], dv[k]);
          }
        }
    } else if (acc_dx) {
      continue;
    }
    if (dr) {
      if (full) {
        float4 o = make_float4(dv[0], dv[1], dv[2], dv[3]);
        if (acc_dx) {
          const float4 t = *(const float4*)dr;
          o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
        }
        *(float4*)dr = o;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (col0 + k < d) dr[k] = acc_dx ? dr[k] + dv[k] : dv[k];
      }
    }
  }
  if (dwpart) {
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) {
        float* __restrict__ o = dwpart + (chunk * C + c) * d + col0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (col0 + k < d) o[k] = acc[c][k];
      }
  }
}

// element e < C d: dW[c][j]; e in [C d, C d + C): db
__global__ __launch_bounds__(256) void term_reduce_kernel(const float* __restrict__ dwpart,
                                                          const float* __restrict__ dbpart, long long nchunk, int C,
                                                          int d, float* __restrict__ dW, long long lddw, int acc_dW,
                                                          float* __restrict__ db, int acc_db) {
  const long long cd = (long long)C * d;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < cd) {
    if (!dW) return;
    double s = 0.0;
#pragma unroll 8
    for (long long c = 0; c < nchunk; ++c) s += (double)dwpart[c * cd + e];
    float* o = dW + (e / d) * lddw + e % d;
    *o = acc_dW ? *o + (float)s : (float)s;
  } else if (e < cd + C) {
    if (!db) return;
    const int cl = (int)(e - cd);
    double s = 0.0;
#pragma unroll 8
    for (long long c = 0; c < nchunk; ++c) s += (double)dbpart[c * TC_MAXC + cl];
    db[cl] = acc_db ? db[cl] + (float)s : (float)s;
  }
}

struct TcLayout {
  size_t hdr, lpart, prob, dbpart, dwpart, total;
  long long nchunk;
};
inline TcLayout tc_layout(long long rows, int d, int C) {
  TcLayout L;
  L.nchunk = (rows + TC_ROWS - 1) / TC_ROWS;
  L.hdr = 0;
  L.lpart = 16;
  L.prob = L.lpart + cg_rup((size_t)L.nchunk * 2 * sizeof(double), 16);
  L.dbpart = L.prob + cg_rup((size_t)rows * C * sizeof(float), 16);
  L.dwpart = L.dbpart + cg_rup((size_t)L.nchunk * TC_MAXC * sizeof(float), 16);
  L.total = L.dwpart + cg_rup((size_t)L.nchunk * C * d * sizeof(float), 16);
  return L;
}

int tc_check(const cg_term_ce_desc* p) {
  if (!p) return CG_EINVAL;
  if (p->C > TC_MAXC) return CG_EUNSUPPORTED;
  if (p->x_dtype != CG_F32 && p->x_dtype != CG_BF16) return CG_EUNSUPPORTED;
  if (p->C < 1 || p->d < 1 || p->rows < 0 || p->ldx < p->d || p->ldw < p->d) return CG_EINVAL;
  if (p->rows == 0) return CG_OK;
  if (!p->x || !p->W || !p->bias || !p->labels || !p->workspace) return CG_EINVAL;
  if (((uintptr_t)p->workspace & 15) || p->ws_bytes < tc_layout(p->rows, p->d, p->C).total) return CG_EINVAL;
  if ((p->rows + TC_ROWS - 1) / TC_ROWS > 0x7FFFFFFFLL) return CG_EUNSUPPORTED;
  return CG_OK;
}
// 16-byte pieces of x and W rows (8-byte for bf16 x)
bool tc_vec(const cg_term_ce_desc* p) {
  const uintptr_t xa = p->x_dtype == CG_BF16 ? 7 : 15;
  return p->ldx % 4 == 0 && p->ldw % 4 == 0 && !((uintptr_t)p->x & xa) && !((uintptr_t)p->W & 15);
}
inline int tc_cp(int C) { return C <= 1 ? 1 : C <= 2 ? 2 : C <= 4 ? 4 : C <= 8 ? 8 : 16; }
}  // namespace

extern "C" size_t cg_term_ce_workspace(long long rows, int d, int C) {
  if (rows <= 0 || d < 1 || C < 1 || C > TC_MAXC) return 0;
  return tc_layout(rows, d, C).total;
}

#define TC_DISPATCH(LAUNCH)                                          \
  do {                                                               \
    const bool bf = p->x_dtype == CG_BF16;                           \
    switch (tc_cp(p->C) * 4 + (bf ? 2 : 0) + (vec ? 1 : 0)) {        \
      case 4: LAUNCH(float, 1, false); break;                        \
      case 5: LAUNCH(float, 1, true); break;                         \
      case 6: LAUNCH(bf16_t, 1, false); break;                       \
      case 7: LAUNCH(bf16_t, 1, true); break;                        \
      case 8: LAUNCH(float, 2, false); break;                        \
      case 9: LAUNCH(float, 2, true); break;                         \
      case 10: LAUNCH(bf16_t, 2, false); break;                      \
      case 11: LAUNCH(bf16_t, 2, true); break;                       \
      case 16: LAUNCH(float, 4, false); break;                       \
      case 17: LAUNCH(float, 4, true); break;                        \
      case 18: LAUNCH(bf16_t, 4, false); break;                      \
      case 19: LAUNCH(bf16_t, 4, true); break;                       \
      case 32: LAUNCH(float, 8, false); break;                       \
      case 33: LAUNCH(float, 8, true); break;                        \
      case 34: LAUNCH(bf16_t, 8, false); break;                      \
      case 35: LAUNCH(bf16_t, 8, true); break;                       \
      case 64: LAUNCH(float, 16, false); break;                      \
      case 65: LAUNCH(float, 16, true); break;                       \
      case 66: LAUNCH(bf16_t, 16, false); break;                     \
      default: LAUNCH(bf16_t, 16, true); break;                      \
    }                                                                \
  } while (0)

extern "C" int cg_term_ce_fwd(const cg_term_ce_desc* p, void* stream) {
  const int rc = tc_check(p);
  if (rc != CG_OK || p->rows == 0) return rc;
  const TcLayout L = tc_layout(p->rows, p->d, p->C);
  char* ws = (char*)p->workspace;
  double* hdr = (double*)(ws + L.hdr);
  double* lpart = (double*)(ws + L.lpart);
  float* prob = (float*)(ws + L.prob);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = tc_vec(p);
  const dim3 grid((unsigned)cg_cdiv(L.nchunk, 4)), block(256);
#define TC_FWD(T_, CP_, V_)                                                                                       \
  hipLaunchKernelGGL((term_fwd_kernel<T_, CP_, V_>), grid, block, 0, s, (const T_*)p->x, p->ldx, p->rows, p->d, \
                     p->C, p->W, p->ldw, p->bias, p->labels, (long long)p->ignore_index, p->class_w, prob, lpart)
  TC_DISPATCH(TC_FWD);
#undef TC_FWD
  CG_LAUNCH_CHECK();
  hipLaunchKernelGGL(term_loss_kernel, dim3(1), dim3(256), 0, s, lpart, L.nchunk, hdr, p->loss, p->sums);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_term_ce_bwd(const cg_term_ce_desc* p, void* stream) {
  const int rc = tc_check(p);
  if (rc != CG_OK) return rc;
  if ((p->dW && p->lddw < p->d) || (p->dx && p->lddx < p->d)) return CG_EINVAL;
  if (p->rows == 0 || (!p->dW && !p->db && !p->dx)) return CG_OK;
  const TcLayout L = tc_layout(p->rows, p->d, p->C);
  char* ws = (char*)p->workspace;
  const double* hdr = (const double*)(ws + L.hdr);
  const float* prob = (const float*)(ws + L.prob);
  float* dbpart = p->db ? (float*)(ws + L.dbpart) : nullptr;
  float* dwpart = p->dW ? (float*)(ws + L.dwpart) : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = tc_vec(p) && (!p->dx || (p->lddx % 4 == 0 && !((uintptr_t)p->dx & 15)));
  const dim3 grid((unsigned)L.nchunk, cg_cdiv(p->d, TC_COLS)), block(64);
#define TC_BWD(T_, CP_, V_)                                                                                       \
  hipLaunchKernelGGL((term_bwd_kernel<T_, CP_, V_>), grid, block, 0, s, (const T_*)p->x, p->ldx, p->rows, p->d, \
                     p->C, p->W, p->ldw, p->labels, (long long)p->ignore_index, p->class_w, p->scale,           \
                     p->scale_dev, hdr, prob, dwpart, dbpart, p->dx, p->lddx, p->acc_dx)
  TC_DISPATCH(TC_BWD);
#undef TC_BWD
  CG_LAUNCH_CHECK();
  if (p->dW || p->db) {
    hipLaunchKernelGGL(term_reduce_kernel, dim3(cg_cdiv((long long)p->C * p->d + p->C, 256)), dim3(256), 0, s, dwpart,
                       dbpart, L.nchunk, p->C, p->d, p->dW, p->lddw, p->acc_dW, p->db, p->acc_db);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

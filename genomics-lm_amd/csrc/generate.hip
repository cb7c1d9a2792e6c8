// Batched on-device generation: the per-row ("ragged") pieces of a KV-cached decode step, whose
// positions come from a device int32 pos[B], and the fused sampler / stop-rule step.
//
// A row with pos[b] < 0 or pos[b] >= Tmax is inactive everywhere in this file: it reads no cache
// row, writes nothing to the cache and leaves its outputs untouched.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {
__device__ __forceinline__ bool row_active(const int32_t* __restrict__ pos, int b, int Tmax, int& p) {
  p = pos[b];
  return p >= 0 && p < Tmax;
}

// sum over the lpr (2 / 4 / 8 / 16, a power of two) adjacent lanes of a key row, all in DPP (the
// steps of wave_reduce that stay inside a 16-lane row); every lane of the group gets the total
__device__ __forceinline__ float group_sum(float v, int lpr) {
  if (lpr >= 2) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));
  if (lpr >= 4) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));
  if (lpr >= 8) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, false));
  if (lpr >= 16) v += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, false));
  return v;
}

constexpr int DR_WAVES = 4;  // waves per workgroup
constexpr int DR_GC = 4;     // query heads of the group served per pass over the keys
}  // namespace

// ===========================================================================
// Ragged single-token attention over a KV cache.  One workgroup per (kv head, sequence): every
// K / V row is loaded once per pass and serves up to DR_GC query heads of the kv head's group.
// A row's hd elements lie over lpr adjacent lanes, 16 bytes per lane (lpr = hd / EPL rounded up
// to a power of two; the pad lanes of hd = 48 carry zeros), so a wave covers 64 / lpr keys per
// step.  Each lane group runs its own online softmax (running max, sum and its 16-byte slice of
// the output) over the keys it meets; the groups of a wave merge by lane exchange and the waves
// through LDS.  No score buffer: any Tmax.
// ===========================================================================
template <typename T_>
__global__ __launch_bounds__(64 * DR_WAVES) void attn_decode_ragged_kernel(
    const T_* __restrict__ q, long long ldq, const T_* __restrict__ cache, long long ldc, int Tmax,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ seg, int window, int H, int KV, int hd, int lpr,
    float scale, T_* __restrict__ y, long long ldy) {
  constexpr int EPL = 16 / sizeof(T_);  // 16 bytes of a row per lane: 8 bf16 or 4 fp32 elements
  __shared__ float sm[DR_WAVES][DR_GC], sl[DR_WAVES][DR_GC];
  __shared__ float sacc[DR_WAVES][DR_GC][64];
  const int kvh = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int p;
  if (!row_active(pos, b, Tmax, p)) return;
  const int wave = tid >> 6, lane = tid & 63;
  const int G = H / KV;
  int lo = seg ? seg[b] : 0;
  if (window > 0) lo = max(lo, p - window + 1);
  lo = min(max(lo, 0), p);
  const int rpw = 64 / lpr;           // key rows per wave per step
  const int r = lane / lpr, c = lane - r * lpr;
  const bool col_ok = c * EPL < hd;   // false on the pad lanes (hd / EPL not a power of two)
  const T_* kb = cache + (long long)b * Tmax * ldc + (long long)kvh * hd + c * EPL;
  const T_* vb = kb + (long long)KV * hd;

  for (int g0 = 0; g0 < G; g0 += DR_GC) {
    const int ng = min(DR_GC, G - g0);
    float qv[DR_GC][EPL], acc[DR_GC][EPL], mx[DR_GC], ls[DR_GC];
#pragma unroll
    for (int g = 0; g < DR_GC; ++g) {
      mx[g] = -INFINITY;
      ls[g] = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) { qv[g][e] = 0.f; acc[g][e] = 0.f; }
      if (g < ng && col_ok) {
        ld_vec<EPL>(q + (long long)b * ldq + (long long)(kvh * G + g0 + g) * hd + c * EPL, qv[g]);
#pragma unroll
        for (int e = 0; e < EPL; ++e) qv[g][e] *= scale;
      }
    }
    // the wave's keys: lo + wave * rpw + r, stepping by the workgroup's DR_WAVES * rpw rows; the
    // trip count is uniform over the wave (the DPP sums run with every lane enabled)
    for (int base = lo + wave * rpw; base <= p; base += DR_WAVES * rpw) {
      const int j = base + r;
      const bool valid = j <= p;
      float kx[EPL], vx[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) { kx[e] = 0.f; vx[e] = 0.f; }
      if (valid && col_ok) {
        ld_vec<EPL>(kb + (long long)j * ldc, kx);
        ld_vec<EPL>(vb + (long long)j * ldc, vx);
      }
#pragma unroll
      for (int g = 0; g < DR_GC; ++g) {
        if (g < ng) {
          float s = 0.f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) s = fmaf(qv[g][e], kx[e], s);
          s = group_sum(s, lpr);
          if (valid) {
            const float mn = fmaxf(mx[g], s);
            const float alpha = __expf(mx[g] - mn);  // 0 on the group's first key (mx = -inf)
            const float pe = __expf(s - mn);
            ls[g] = fmaf(ls[g], alpha, pe);
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[g][e] = fmaf(acc[g][e], alpha, pe * vx[e]);
            mx[g] = mn;
          }
        }
      }
    }
    // merge the wave's lane groups: butterfly over the row index bits of the lane id
#pragma unroll
    for (int g = 0; g < DR_GC; ++g) {
      if (g < ng) {
        for (int o = lpr; o < 64; o <<= 1) {
          const float mo = __shfl_xor(mx[g], o), lo_ = __shfl_xor(ls[g], o);
          const float mn = fmaxf(mx[g], mo);
          const float a = mx[g] == -INFINITY ? 0.f : __expf(mx[g] - mn);
          const float bb = mo == -INFINITY ? 0.f : __expf(mo - mn);
          ls[g] = ls[g] * a + lo_ * bb;
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[g][e] = acc[g][e] * a + __shfl_xor(acc[g][e], o) * bb;
          mx[g] = mn;
        }
        if (r == 0 && col_ok) {
          if (c == 0) { sm[wave][g] = mx[g]; sl[wave][g] = ls[g]; }
#pragma unroll
          for (int e = 0; e < EPL; ++e) sacc[wave][g][c * EPL + e] = acc[g][e];
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < ng * hd; i += 64 * DR_WAVES) {
      const int g = i / hd, e = i - g * hd;
      float mn = -INFINITY;
#pragma unroll
      for (int w = 0; w < DR_WAVES; ++w) mn = fmaxf(mn, sm[w][g]);
      float l = 0.f, o = 0.f;
#pragma unroll
      for (int w = 0; w < DR_WAVES; ++w) {
        const float a = sm[w][g] == -INFINITY ? 0.f : __expf(sm[w][g] - mn);
        l = fmaf(sl[w][g], a, l);
        o = fmaf(sacc[w][g][e], a, o);
      }
      st_act<T_>(y + (long long)b * ldy + (long long)(kvh * G + g0 + g) * hd + e, o / l);
    }
    __syncthreads();
  }
}

extern "C" int cg_attn_decode_ragged(int dtype, const void* q, long long ldq, const void* cache, long long ldc,
                                     int Tmax, const int32_t* pos, const int32_t* segstate, int window, int B, int H,
                                     int KV, int hd, void* y, long long ldy, void* stream) {
  if (B <= 0 || H <= 0 || KV <= 0 || H % KV || hd <= 0 || Tmax <= 0) return CG_EINVAL;
  if (!q || !cache || !y || !pos || ldc < 2LL * KV * hd || ldq < (long long)H * hd || ldy < (long long)H * hd)
    return CG_EINVAL;
  if (dtype != CG_BF16 && dtype != CG_F32) return CG_EUNSUPPORTED;
  const int es = dtype == CG_BF16 ? 2 : 4, epl = 16 / es;
  if (hd > 64 || hd % epl) return CG_EUNSUPPORTED;
  // 16-byte loads: every row start and every head column block on a 16-byte boundary
  if (((uintptr_t)q | (uintptr_t)cache) % 16 || (ldq * es) % 16 || (ldc * es) % 16) return CG_EUNSUPPORTED;
  int lpr = 1;
  while (lpr * epl < hd) lpr <<= 1;
  const float scale = 1.0f / sqrtf((float)hd);
  const dim3 g(KV, B);
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(attn_decode_ragged_kernel<bf16_t>, g, dim3(64 * DR_WAVES), 0, (hipStream_t)stream,
                       (const bf16_t*)q, ldq, (const bf16_t*)cache, ldc, Tmax, pos, segstate, window, H, KV, hd, lpr,
                       scale, (bf16_t*)y, ldy);
  else
    hipLaunchKernelGGL(attn_decode_ragged_kernel<float>, g, dim3(64 * DR_WAVES), 0, (hipStream_t)stream,
                       (const float*)q, ldq, (const float*)cache, ldc, Tmax, pos, segstate, window, H, KV, hd, lpr,
                       scale, (float*)y, ldy);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// The per-row steps around it
// ===========================================================================
// x[b] = tok_emb[tok[b]] + pos_emb[pos[b]]
__global__ __launch_bounds__(256) void embed_fwd_pos_kernel(const int64_t* __restrict__ tok, const float* __restrict__ te,
                                                            const float* __restrict__ pe,
                                                            const int32_t* __restrict__ pos, float* __restrict__ x,
                                                            int d, int V, int Tmax) {
  const int b = blockIdx.x;
  int p;
  if (!row_active(pos, b, Tmax, p)) return;
  const long long t = tok[b];
  if (t < 0 || t >= V) return;
  for (int c = threadIdx.x; c < d; c += 256) {
    float v = te[t * d + c];
    if (pe) v += pe[(long long)p * d + c];
    x[(long long)b * d + c] = v;
  }
}
extern "C" int cg_embed_fwd_pos(const int64_t* tok, const float* tok_emb, const float* pos_emb, const int32_t* pos,
                                float* x, int B, int d, int V, int Tmax, void* stream) {
  if (!tok || !tok_emb || !pos || !x || B <= 0 || d <= 0 || V <= 0 || Tmax <= 0) return CG_EINVAL;
  hipLaunchKernelGGL(embed_fwd_pos_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tok, tok_emb, pos_emb, pos, x,
                     d, V, Tmax);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// rotate-half RoPE of the q and k heads of row b with the table row of pos[b]
template <typename T_>
__global__ __launch_bounds__(256) void rope_pos_kernel(T_* __restrict__ qkv, long long ld,
                                                       const int32_t* __restrict__ pos, int nh, int hd,
                                                       const float* __restrict__ cosb, const float* __restrict__ sinb,
                                                       int Tmax) {
  const int b = blockIdx.x, half = hd >> 1;
  int p;
  if (!row_active(pos, b, Tmax, p)) return;
  for (int i = threadIdx.x; i < nh * half; i += 256) {
    const int h = i / half, k = i - h * half;
    T_* base = qkv + (long long)b * ld + (long long)h * hd;
    const float cs = cosb[(long long)p * half + k], sn = sinb[(long long)p * half + k];
    const float x1 = ld_act<T_>(base + k), x2 = ld_act<T_>(base + k + half);
    st_act<T_>(base + k, x1 * cs - x2 * sn);
    st_act<T_>(base + k + half, x2 * cs + x1 * sn);
  }
}
extern "C" int cg_rope_pos(int dtype, void* qkv, long long ldqkv, const int32_t* pos, int B, int H, int KV, int hd,
                           const float* cos_tab, const float* sin_tab, int Tmax, void* stream) {
  if (!qkv || !pos || !cos_tab || !sin_tab || B <= 0 || Tmax <= 0) return CG_EINVAL;
  if (hd & 1) return CG_EUNSUPPORTED;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(rope_pos_kernel<bf16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (bf16_t*)qkv, ldqkv, pos,
                       H + KV, hd, cos_tab, sin_tab, Tmax);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(rope_pos_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (float*)qkv, ldqkv, pos,
                       H + KV, hd, cos_tab, sin_tab, Tmax);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// cache[b][pos[b]][0..n) = src[b][0..n)  (the [k|v] columns of the step's qkv row)
template <typename T_>
__global__ __launch_bounds__(256) void kv_append_kernel(const T_* __restrict__ src, long long lds,
                                                        T_* __restrict__ cache, long long ldc, int Tmax,
                                                        const int32_t* __restrict__ pos, int n) {
  const int b = blockIdx.x;
  int p;
  if (!row_active(pos, b, Tmax, p)) return;
  const T_* s = src + (long long)b * lds;
  T_* dst = cache + ((long long)b * Tmax + p) * ldc;
  for (int c = threadIdx.x; c < n; c += 256) dst[c] = s[c];
}
extern "C" int cg_kv_append(int dtype, const void* src, long long lds, void* cache, long long ldc, int Tmax,
                            const int32_t* pos, int B, int n, void* stream) {
  if (!src || !cache || !pos || B <= 0 || n <= 0 || ldc < n || lds < n || Tmax <= 0) return CG_EINVAL;
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(kv_append_kernel<bf16_t>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, lds,
                       (bf16_t*)cache, ldc, Tmax, pos, n);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(kv_append_kernel<float>, dim3(B), dim3(256), 0, (hipStream_t)stream, (const float*)src, lds,
                       (float*)cache, ldc, Tmax, pos, n);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// the prefill's cache fill of one layer: cache[b][t][0..n) = src[b*T + t][0..n) for t < len[b]
template <typename T_>
__global__ __launch_bounds__(256) void kv_scatter_kernel(const T_* __restrict__ src, long long lds, int T,
                                                         T_* __restrict__ cache, long long ldc, int Tmax,
                                                         const int32_t* __restrict__ len, int n) {
  const int b = blockIdx.y;
  const int nb = min(min(len[b], T), Tmax);
  for (int t = blockIdx.x; t < nb; t += gridDim.x) {
    const T_* s = src + ((long long)b * T + t) * lds;
    T_* dst = cache + ((long long)b * Tmax + t) * ldc;
    for (int c = threadIdx.x; c < n; c += 256) dst[c] = s[c];
  }
}
extern "C" int cg_kv_scatter(int dtype, const void* src, long long lds, int T, void* cache, long long ldc, int Tmax,
                             const int32_t* len, int B, int n, void* stream) {
  if (!src || !cache || !len || B <= 0 || T <= 0 || n <= 0 || ldc < n || lds < n || Tmax <= 0) return CG_EINVAL;
  const dim3 g(T < 1024 ? T : 1024, B);
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(kv_scatter_kernel<bf16_t>, g, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, lds, T,
                       (bf16_t*)cache, ldc, Tmax, len, n);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(kv_scatter_kernel<float>, g, dim3(256), 0, (hipStream_t)stream, (const float*)src, lds, T,
                       (float*)cache, ldc, Tmax, len, n);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

__global__ void segstate_step_ragged_kernel(const int64_t* __restrict__ tok, const int32_t* __restrict__ pos, int B,
                                            int sep, int Tmax, int32_t* __restrict__ seg) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  int p;
  if (b < B && row_active(pos, b, Tmax, p) && tok[b] == sep) seg[b] = p;
}
extern "C" int cg_segstate_step_ragged(const int64_t* tok, const int32_t* pos, int B, int sep_id, int Tmax,
                                       int32_t* segstate, void* stream) {
  if (B <= 0 || sep_id < 0) return CG_OK;
  if (!tok || !pos || !segstate) return CG_EINVAL;
  hipLaunchKernelGGL(segstate_step_ragged_kernel, dim3(cg_cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, tok, pos, B,
                     sep_id, Tmax, segstate);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// dst[b][0..n) = src[row(b)][0..n) for the rows picked by `sel`: row(b) = b*T + sel[b]-1 (T > 0, the
// prefill's last prompt row, sel = len) or b where sel[b] is an active position (T == 0, the
// decode step's outputs).  seg_src / seg_dst (optional, T > 0): the same gather of one int32.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, long long lds,
                                                          const int32_t* __restrict__ sel, int T, int Tmax,
                                                          float* __restrict__ dst, long long ldd, int n,
                                                          const int32_t* __restrict__ seg_src,
                                                          int32_t* __restrict__ seg_dst) {
  const int b = blockIdx.x;
  long long row;
  if (T > 0) {
    const int l = min(max(sel[b], 1), T);
    row = (long long)b * T + l - 1;
    if (seg_dst && threadIdx.x == 0) seg_dst[b] = seg_src ? seg_src[row] : 0;
  } else {
    int p;
    if (!row_active(sel, b, Tmax, p)) return;
    row = b;
  }
  for (int c = threadIdx.x; c < n; c += 256) dst[(long long)b * ldd + c] = src[row * lds + c];
}
extern "C" int cg_gather_rows(const float* src, long long lds, const int32_t* sel, int T, int Tmax, float* dst,
                              long long ldd, int n, const int32_t* seg_src, int32_t* seg_dst, int B, void* stream) {
  if (!src || !sel || !dst || B <= 0 || n <= 0 || lds < n || ldd < n) return CG_EINVAL;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, src, lds, sel, T, Tmax, dst, ldd,
                     n, seg_src, seg_dst);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// out[b][c] = xf[b] . w[c] + bias[c] on the active rows: the termination head of a decode step
// (nc classes, one wave per (row, class); fp32 master weights in either mode)
template <typename T_>
__global__ __launch_bounds__(64) void row_head_kernel(const T_* __restrict__ xf, long long ldx,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      const int32_t* __restrict__ pos, int Tmax, int d,
                                                      float* __restrict__ out, long long ldo) {
  const int c = blockIdx.x, b = blockIdx.y;
  int p;
  if (!row_active(pos, b, Tmax, p)) return;
  float s = 0.f;
  for (int k = threadIdx.x; k < d; k += 64) s = fmaf(ld_act<T_>(xf + (long long)b * ldx + k), w[(long long)c * d + k], s);
  s = wave_sum(s);
  if (threadIdx.x == 0) out[(long long)b * ldo + c] = s + (bias ? bias[c] : 0.f);
}
extern "C" int cg_row_head(int dtype, const void* xf, long long ldx, const float* w, const float* bias,
                           const int32_t* pos, int Tmax, int B, int d, int nc, float* out, long long ldo,
                           void* stream) {
  if (!xf || !w || !pos || !out || B <= 0 || d <= 0 || nc <= 0 || ldo < nc) return CG_EINVAL;
  const dim3 g(nc, B);
  if (dtype == CG_BF16)
    hipLaunchKernelGGL(row_head_kernel<bf16_t>, g, dim3(64), 0, (hipStream_t)stream, (const bf16_t*)xf, ldx, w, bias,
                       pos, Tmax, d, out, ldo);
  else if (dtype == CG_F32)
    hipLaunchKernelGGL(row_head_kernel<float>, g, dim3(64), 0, (hipStream_t)stream, (const float*)xf, ldx, w, bias,
                       pos, Tmax, d, out, ldo);
  else
    return CG_EUNSUPPORTED;
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// ===========================================================================
// The fused sampler and stop-rule step (contract: include/codonlm_hip.h, cg_sample_step and
// cg_sample_step_plan).  One workgroup per sequence, thread t owns tokens 4t .. 4t+3.  Weights,
// the top-k rank count and the cumulative sums are fp64, so the drawn token is a function of the
// fp32 logits that a double-precision restatement reproduces.
//
// PLAN = true is cg_sample_step_plan: the step's allowed set comes from the sequence's plan (four
// adjacent bytes of the set row per thread, one block-wide OR for the empty-set fallback), the
// raw logits' logsumexp rides on two more block reductions when a log-probability is wanted, and
// thread 0 alone adds to the sequence's logp row.  PLAN = false compiles to cg_sample_step as it
// was: every plan branch is an `if constexpr`.
// ===========================================================================
constexpr int SMP_V = 1024;
template <bool PLAN>
__device__ __forceinline__ void sample_step_body(const cg_sample_params& P, const cg_sample_plan& PL,
                                                 const float* __restrict__ logits, long long ldl,
                                                 const float* __restrict__ term, long long ld_term,
                                                 cg_gen_state* __restrict__ state, int64_t* __restrict__ next_tok,
                                                 int64_t* __restrict__ out_ids, long long ld_out,
                                                 int32_t* __restrict__ n_active) {
  __shared__ double w[SMP_V];
  __shared__ double red[256];
  __shared__ int s_bias, s_pick, s_last;
  const int b = blockIdx.x, tid = threadIdx.x, V = P.V;
  cg_gen_state st = state[b];
  if (st.flags & CG_GEN_DONE) return;
  // the step's set: uniform over the workgroup (b and n_tokens are)
  const uint8_t* set_row = nullptr;
  int plen = 0;
  if constexpr (PLAN) {
    plen = PL.plan_len ? PL.plan_len[b] : 0;
    const int j = st.n_tokens;
    if (PL.n_sets > 0 && j >= 0 && j < plen && j < PL.ld_plan) {
      const int s = PL.plan[(long long)b * PL.ld_plan + j];
      if (s >= 0 && s < PL.n_sets) set_row = PL.sets + (long long)s * PL.ld_sets;
    }
  }
  // 1. termination bias
  if (tid == 0) {
    int apply = 0;
    const long long edge = (long long)P.target_codons - P.bias_window;
    if (term && P.stop_bias > 0.f && P.n_term_classes > 0 && st.n_codons >= (edge > 0 ? edge : 0)) {
      int cls = 0;
      float best = term[(long long)b * ld_term];
      for (int c = 1; c < P.n_term_classes; ++c) {
        const float v = term[(long long)b * ld_term + c];
        if (v > best) { best = v; cls = c; }
      }
      st.last_term_class = cls;
      if (cls <= P.trigger_class_max) { apply = 1; st.bias_steps++; }
    }
    s_bias = apply;
    s_pick = INT_MAX;
    s_last = -1;
  }
  bool in_set[4] = {false, false, false, false};
  bool use_set = false;
  if constexpr (PLAN) {
    int any = 0;
    if (set_row) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = 4 * tid + k;
        in_set[k] = v < V && set_row[v] != 0;
        any |= in_set[k] ? 1 : 0;
      }
    }
    use_set = __syncthreads_or(any) != 0;  // (also the barrier that publishes s_bias)
  } else {
    __syncthreads();
  }
  const double bias = s_bias ? (double)P.stop_bias : 0.0;
  // 2./3. mask and weights
  double lv[4];
  bool ok[4];
  double mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = 4 * tid + k;
    if constexpr (PLAN)
      ok[k] = use_set ? in_set[k] : (v < V && (!P.allowed || P.allowed[v]));
    else
      ok[k] = v < V && (!P.allowed || P.allowed[v]);
    lv[k] = 0.0;
    if (ok[k]) {
      lv[k] = (double)logits[(long long)b * ldl + v] + ((P.tok_class[v] & CG_TOK_STOP) ? bias : 0.0);
      mx = fmax(mx, lv[k]);
    }
  }
  red[tid] = mx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  mx = red[0];
  __syncthreads();
  // logsumexp of the V raw logits (no bias, no mask, no temperature): thread 0 keeps it
  double lse = 0.0;
  if constexpr (PLAN) {
    if (PL.logp || PL.tok_logp) {
      double raw[4], rmx = -INFINITY;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = 4 * tid + k;
        raw[k] = v < V ? (double)logits[(long long)b * ldl + v] : -INFINITY;
        rmx = fmax(rmx, raw[k]);
      }
      red[tid] = rmx;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
      }
      rmx = red[0];
      __syncthreads();
      double rs = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * tid + k < V) rs += exp(raw[k] - rmx);
      red[tid] = rs;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
      }
      lse = rmx + log(red[0]);
      __syncthreads();
    }
  }
  const double temp = fmax(1e-6, (double)P.temperature);
  double wv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wv[k] = ok[k] ? exp((lv[k] - mx) / temp) : 0.0;
    w[4 * tid + k] = wv[k];
  }
  __syncthreads();
  // 4. top-k by rank count (ties to the lower index)
  const int kk = P.topk > 0 ? min(P.topk, V) : V;
  if (kk < V) {
    int rank[4] = {0, 0, 0, 0};
    for (int u = 0; u < V; ++u) {
      const double wu = w[u];
#pragma unroll
      for (int k = 0; k < 4; ++k) rank[k] += (wu > wv[k] || (wu == wv[k] && u < 4 * tid + k)) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (rank[k] >= kk) wv[k] = 0.0;
  }
  // 5. draw: first index whose inclusive cumulative weight exceeds u * total
  const double tsum = ((wv[0] + wv[1]) + wv[2]) + wv[3];
  red[tid] = tsum;
  __syncthreads();
  double before = 0.0, total = 0.0;
  for (int t = 0; t < 256; ++t) {
    if (t == tid) before = total;
    total += red[t];
  }
  const uint32_t h = cg_fmix32(cg_row_hash(P.seed, st.stream) + (uint32_t)st.n_tokens * 0x9E3779B1u);
  const double target = (double)(h >> 8) * (1.0 / 16777216.0) * total;
  double cum = before;
  int pick = INT_MAX, last = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cum += wv[k];
    if (wv[k] > 0.0) {
      last = 4 * tid + k;
      if (cum > target && pick == INT_MAX) pick = 4 * tid + k;
    }
  }
  if (pick != INT_MAX) atomicMin(&s_pick, pick);
  if (last >= 0) atomicMax(&s_last, last);
  __syncthreads();
  if (tid != 0) return;
  int tok = s_pick != INT_MAX ? s_pick : s_last;
  if (tok < 0) tok = 0;  // nothing allowed: outside the contract
  // 6. record
  next_tok[b] = tok;
  if (out_ids && st.n_tokens < ld_out) out_ids[(long long)b * ld_out + st.n_tokens] = tok;
  if constexpr (PLAN) {
    if (PL.logp || PL.tok_logp) {
      // a drawn token was kept by the top-k cut, so w[tok] is its weight under `total`
      const double lp_model = (double)logits[(long long)b * ldl + tok] - lse;
      if (PL.logp) {
        PL.logp[2LL * b] += lp_model;
        PL.logp[2LL * b + 1] += log(w[tok] / total);
      }
      if (PL.tok_logp && st.n_tokens >= 0 && st.n_tokens < PL.ld_tok_logp)
        PL.tok_logp[(long long)b * PL.ld_tok_logp + st.n_tokens] = (float)lp_model;
    }
  }
  st.n_tokens++;
  const int cls = P.tok_class[tok];
  if (cls & CG_TOK_CODON) st.n_codons++;
  // 7. stop rules, the first that fires ends the sequence
  const bool at_target = st.n_codons >= P.target_codons;
  int f = st.flags;
  if ((cls & CG_TOK_STOP) && P.stop_on_bio_stop) {
    if (!at_target) {
      f |= CG_GEN_EARLY_STOP;
      if (!P.require_terminal_stop) f |= CG_GEN_TERMINAL_STOP | CG_GEN_DONE;
    } else {
      f |= CG_GEN_TERMINAL_STOP | CG_GEN_DONE;
    }
  }
  if (!(f & CG_GEN_DONE) && (cls & CG_TOK_EOS) && P.stop_on_eos && (at_target || !P.require_terminal_stop))
    f |= CG_GEN_EOS | CG_GEN_DONE;
  if (!(f & CG_GEN_DONE) && at_target && !P.require_terminal_stop) f |= CG_GEN_TARGET | CG_GEN_DONE;
  if (!(f & CG_GEN_DONE) && (st.n_codons >= P.max_codons || st.n_tokens >= P.max_tokens))
    f |= CG_GEN_CAP | CG_GEN_DONE;
  if constexpr (PLAN) {
    if (!(f & CG_GEN_DONE) && PL.end_with_plan && plen > 0 && st.n_tokens >= plen)
      f |= CG_GEN_PLAN_END | CG_GEN_DONE;
  }
  // 8. advance
  if (!(f & CG_GEN_DONE)) {
    st.pos = st.pos0 + st.n_tokens - 1;
    if (st.pos >= P.Tmax) f |= CG_GEN_CONTEXT_FULL | CG_GEN_DONE;
  }
  if (f & CG_GEN_DONE) st.pos = -1;
  st.flags = f;
  state[b] = st;
  // 9. active count
  if (n_active && !(f & CG_GEN_DONE)) atomicAdd(n_active, 1);
}

__global__ __launch_bounds__(256) void sample_step_kernel(cg_sample_params P, const float* __restrict__ logits,
                                                          long long ldl, const float* __restrict__ term,
                                                          long long ld_term, cg_gen_state* __restrict__ state,
                                                          int64_t* __restrict__ next_tok, int64_t* __restrict__ out_ids,
                                                          long long ld_out, int32_t* __restrict__ n_active) {
  sample_step_body<false>(P, cg_sample_plan{}, logits, ldl, term, ld_term, state, next_tok, out_ids, ld_out, n_active);
}

__global__ __launch_bounds__(256) void sample_step_plan_kernel(cg_sample_params P, cg_sample_plan PL,
                                                               const float* __restrict__ logits, long long ldl,
                                                               const float* __restrict__ term, long long ld_term,
                                                               cg_gen_state* __restrict__ state,
                                                               int64_t* __restrict__ next_tok,
                                                               int64_t* __restrict__ out_ids, long long ld_out,
                                                               int32_t* __restrict__ n_active) {
  sample_step_body<true>(P, PL, logits, ldl, term, ld_term, state, next_tok, out_ids, ld_out, n_active);
}

extern "C" int cg_sample_step(const cg_sample_params* p, const float* logits, long long ldl, const float* term_logits,
                              long long ld_term, cg_gen_state* state, int64_t* next_tok, int64_t* out_ids,
                              long long ld_out, int32_t* n_active, int B, void* stream) {
  if (!p || !logits || !state || !next_tok || !p->tok_class || B <= 0 || p->V <= 0 || ldl < p->V) return CG_EINVAL;
  if (term_logits && ld_term < p->n_term_classes) return CG_EINVAL;
  if (p->V > SMP_V) return CG_EUNSUPPORTED;
  if (n_active && hipMemsetAsync(n_active, 0, 4, (hipStream_t)stream) != hipSuccess) return CG_ELAUNCH;
  hipLaunchKernelGGL(sample_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, *p, logits, ldl, term_logits,
                     ld_term, state, next_tok, out_ids, ld_out, n_active);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_sample_step_plan(const cg_sample_params* p, const cg_sample_plan* plan, const float* logits,
                                   long long ldl, const float* term_logits, long long ld_term, cg_gen_state* state,
                                   int64_t* next_tok, int64_t* out_ids, long long ld_out, int32_t* n_active, int B,
                                   void* stream) {
  if (!p || !plan || !logits || !state || !next_tok || !p->tok_class || B <= 0 || p->V <= 0 || ldl < p->V)
    return CG_EINVAL;
  if (term_logits && ld_term < p->n_term_classes) return CG_EINVAL;
  if (plan->n_sets < 0) return CG_EINVAL;
  if (plan->n_sets > 0 &&
      (!plan->sets || !plan->plan || !plan->plan_len || plan->ld_sets < p->V || plan->ld_plan < 0))
    return CG_EINVAL;
  if (p->V > SMP_V) return CG_EUNSUPPORTED;
  if (n_active && hipMemsetAsync(n_active, 0, 4, (hipStream_t)stream) != hipSuccess) return CG_ELAUNCH;
  hipLaunchKernelGGL(sample_step_plan_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, *p, *plan, logits, ldl,
                     term_logits, ld_term, state, next_tok, out_ids, ld_out, n_active);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

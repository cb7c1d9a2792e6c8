// Per-head attention statistics without a T x T tensor (included by attention.hip after
// attention_mfma.h; contract: include/codonlm_hip.h, cg_attn_stats).
//
// The op is self-normalised: pass A over a query row's key tiles takes the row maximum and the
// normaliser Z in fp32, pass B forms p = exp(s - lse) again from the same QK^T product and adds it
// into every statistic, so P is fp32 in every sum and nothing depends on the forward's saved LSE.
//   * attn_stats_mfma : bf16, hd % 8 == 0.  The forward's machinery: 4 waves x 32 queries, Q
//     fragments in registers, K tiles through the LDS-DMA double buffer, QK^T on
//     v_mfma_f32_32x32x16_bf16 (lane l&31 = query, lanes l / l^32 share a query's 64 keys).
//   * attn_stats_vec  : fp32, and bf16 head dims the MFMA tiles do not cover.  One query per
//     thread, 128 queries per workgroup, K tile as fp32 in LDS.
// Both write the same workspace: per (b, h, 128-query tile) the fp64 sums of the kept rows'
// statistics and the column sums of P (`received`); attn_stats_finish_* add the tiles in ascending
// order.  No atomics: every output is a function of the inputs and the shapes only.
#pragma once

namespace as {
constexpr int NS = CG_AS_NSTAT;
constexpr int QT = 128;  // queries per workgroup
constexpr int STP = NS + 1;  // per-query staging row in LDS: the statistics and the kept flag

// partial sums of one query over the keys a lane (or thread) has seen
struct Acc {
  float ent, cls[4], dist[5], md, mx, first;
};
__device__ __forceinline__ Acc acc_zero() {
  Acc a;
  a.ent = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) a.cls[c] = 0.f;
#pragma unroll
  for (int c = 0; c < 5; ++c) a.dist[c] = 0.f;
  a.md = 0.f;
  a.mx = 0.f;
  a.first = 0.f;
  return a;
}
// everything but the class masses: p of a visible key at distance d = q - k >= 0, lnp = s - lse
__device__ __forceinline__ void acc_add(Acc& a, float p, float lnp, int d, bool first, bool far) {
  a.ent += p > 0.f ? p * lnp : 0.f;
  if (far) {
    a.dist[4] += p;
  } else {
    a.dist[0] += d == 0 ? p : 0.f;
    a.dist[1] += (unsigned)(d - 1) < 3u ? p : 0.f;
    a.dist[2] += (unsigned)(d - 4) < 12u ? p : 0.f;
    a.dist[3] += (unsigned)(d - 16) < 48u ? p : 0.f;
    a.dist[4] += d >= 64 ? p : 0.f;
  }
  a.md = fmaf(p, (float)d, a.md);
  a.mx = fmaxf(a.mx, p);
  a.first += first ? p : 0.f;
}
// the CG_AS_* row of one query from its summed partials; nv = visible keys
__device__ __forceinline__ void acc_stats(const Acc& a, int nv, float* st) {
  const float ent = -a.ent;
  st[CG_AS_ENTROPY] = ent;
  st[CG_AS_NORM_ENTROPY] = nv > 1 ? ent / logf((float)nv) : 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) st[CG_AS_MASS_SPECIAL + c] = a.cls[c];
#pragma unroll
  for (int c = 0; c < 5; ++c) st[CG_AS_DIST_0 + c] = a.dist[c];
  st[CG_AS_MEAN_DIST] = a.md;
  st[CG_AS_MAX_PROB] = a.mx;
  st[CG_AS_FIRST] = a.first;
}

__device__ __forceinline__ bool row_kept(const int64_t* idx, int pad_id, const uint8_t* row_keep, long long r) {
  return (!idx || idx[r] != (int64_t)pad_id) && (!row_keep || row_keep[r] != 0);
}
// class of key `key` of batch row b (255 = joins no class)
__device__ __forceinline__ int key_class(const int64_t* idx, const uint8_t* tok_class, int V, long long rowbase,
                                         int key, int T) {
  if (!tok_class || key >= T) return 255;
  const int64_t tok = idx[rowbase + key];
  return tok >= 0 && tok < (int64_t)V ? (int)tok_class[tok] : 255;
}

// Workgroup epilogue: the 128 staged rows (zeros where not kept or past T) are summed in query
// order in fp64 by one thread per statistic; thread NS counts the kept rows.
__device__ __forceinline__ void tile_sums(const float* stage, double* hpart, double* cnt, long long wg, long long bq,
                                          bool first_head, int tid) {
  if (tid <= NS) {
    double s = 0.0;
    for (int q = 0; q < QT; ++q) s += (double)stage[q * STP + tid];
    if (tid < NS) hpart[wg * NS + tid] = s;
    else if (first_head) cnt[bq] = s;
  }
}
}  // namespace as

// ---------------------------------------------------------------------------
// bf16 MFMA kernel.  grid (B*H, q-tiles), 256 threads.  smem: two K images | colsum / staging
// ---------------------------------------------------------------------------
template <int NKS>
__global__ __launch_bounds__(256) void attn_stats_mfma(const bf16_t* __restrict__ qkv, long long ld,
                                                       const int32_t* __restrict__ seg, int T, int H, int KV, int hd,
                                                       int window, float scale, const int64_t* __restrict__ idx,
                                                       int pad_id, const uint8_t* __restrict__ tok_class, int V,
                                                       const uint8_t* __restrict__ row_keep, float* __restrict__ rows,
                                                       int32_t* __restrict__ nvis, float* __restrict__ rpart,
                                                       double* __restrict__ hpart, double* __restrict__ cnt) {
  using namespace fa;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)(smem + 2 * IMG);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5;
  const int bh = blockIdx.x, b = bh / H, hh = bh % H, kvh = hh / (H / KV);
  const int nqt = gridDim.y;
  const int qtile = nqt - 1 - blockIdx.y;
  const int q0 = qtile * as::QT, q0w = q0 + wave * 32;
  const int myq = q0w + (lane & 31);
  const bool qok = myq < T;
  const long long rowbase = (long long)b * T;
  const bf16_t* qrow = qkv + (rowbase + (qok ? myq : 0)) * ld + (long long)hh * hd;
  v8bf qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = frag_global(qrow, qok, ks, hd, lane);
  const int lo = qok ? lo_of(seg, rowbase, myq, T, window) : 0x7fffffff;
  const int kmin = lo_of(seg, rowbase, q0, T, window);
  const int kmax = min(T - 1, q0 + as::QT - 1);
  const int w_lo_min = lo_of(seg, rowbase, q0w, T, window);
  const int w_qmax = min(T - 1, q0w + 31);
  const bool kept = qok && as::row_kept(idx, pad_id, row_keep, rowbase + myq);
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  const TileDma kd = tile_dma_src(qkv + rowbase * ld, ld, T, hd, wave_u, lane);
  const uint32_t kcol = (uint32_t)((H + kvh) * hd * 2);
  const uint32_t tstride = (uint32_t)(KT * ld * 2);
  const RowOff ro = row_offsets(lane);
  const int t0 = kmin / KT, t1 = kmax / KT;
  const long long wg = (long long)bh * nqt + qtile;

  // the column sums of the key tiles this workgroup never visits are zero
  if (rpart)
    for (int k = tid; k < T; k += 256)
      if (k < t0 * KT || k >= (t1 + 1) * KT) rpart[wg * T + k] = 0.f;

  // scores of tile k0 as x = s * scale, -inf where the lane's query does not see the key
  auto scores = [&](const char* Ki, int k0, v16f& s0, v16f& s1) __attribute__((always_inline)) {
    s0 = zero16();
    s1 = zero16();
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row_o(Ki, ro, 0, ks), qf[ks], s0, 0, 0, 0);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks)
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_row_o(Ki, ro, 32, ks), qf[ks], s1, 0, 0, 0);
    // the forward's wait after an MFMA chain before its accumulator is read (attention_mfma.h):
    // without it the row maxima can come from a stale accumulator and vary run to run
    asm volatile("s_nop 15\n\ts_nop 2" : "+v"(s0), "+v"(s1));
    const int kq = myq - k0, kl = lo - k0;  // visible iff kl <= key index <= kq
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = acc_row(r, lane);
      s0[r] = (j > kq || j < kl) ? -INFINITY : s0[r] * scale;
      s1[r] = (j + 32 > kq || j + 32 < kl) ? -INFINITY : s1[r] * scale;
    }
  };
  // one sweep of the K tiles t0..t1 through the double buffer; fn(Ki, k0, seen) once per tile, by
  // every wave (seen: some query of the wave sees a key of the tile)
  auto sweep = [&](auto&& fn) __attribute__((always_inline)) {
    tile_dma(lds0, kd, t0 * tstride + kcol, wave_u);
    dma_drain();
    __syncthreads();
    int cur = 0;
    for (int t = t0; t <= t1; ++t, cur ^= 1) {
      // the other buffer was last read before the previous barrier
      if (t < t1) tile_dma(lds0 + (cur ^ 1) * IMG, kd, (t + 1) * tstride + kcol, wave_u);
      const int k0 = t * KT;
      fn(smem + cur * IMG, k0, k0 <= w_qmax && k0 + KT - 1 >= w_lo_min);
      dma_drain();
      __syncthreads();
    }
  };

  // ---- pass A: row maximum and normaliser of the lane's half of the keys, then of the row
  float m = -INFINITY, l = 0.f;
  sweep([&](const char* Ki, int k0, bool seen) __attribute__((always_inline)) {
    if (!seen) return;
    v16f s0, s1;
    scores(Ki, k0, s0, s1);
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) mt = fmaxf(mt, fmaxf(s0[r], s1[r]));
    if (mt > -INFINITY) {
      const float mn = fmaxf(m, mt);
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += expf(s0[r] - mn) + expf(s1[r] - mn);
      l = l * expf(m - mn) + a;
      m = mn;
    }
  });
  float lse = 0.f;
  {
    const float mo = __shfl_xor(m, 32, 64), lo2 = __shfl_xor(l, 32, 64);
    const float m0 = hl ? mo : m, l0 = hl ? lo2 : l, m1 = hl ? m : mo, l1 = hl ? l : lo2;
    const float M = fmaxf(m0, m1);
    if (qok) lse = M + logf(l0 * expf(m0 - M) + l1 * expf(m1 - M));  // a query sees itself: M is finite
  }

  // ---- pass B: p and every sum
  as::Acc a = as::acc_zero();
  sweep([&](const char* Ki, int k0, bool seen) __attribute__((always_inline)) {
    v16f s0 = zero16(), s1 = zero16();
    if (seen) {
      scores(Ki, k0, s0, s1);
      // a tile wholly 64 or more keys below the wave's queries is DIST_64_PLUS as a whole
      const bool far = k0 + KT - 1 + 64 <= q0w;
      uint32_t cw[4][2];
      if (tok_class) {  // the tile's key classes as four 64-bit masks, this lane half's bits at 0..27
        const int c = as::key_class(idx, tok_class, V, rowbase, k0 + lane, T);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned long long mk = __ballot(c == k) >> (4 * hl);
          cw[k][0] = (uint32_t)mk;
          cw[k][1] = (uint32_t)(mk >> 32);
        }
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = kb ? s1[r] : s0[r];
          const int key = k0 + 32 * kb + acc_row(r, lane);
          const float p = x > -INFINITY ? expf(x - lse) : 0.f;
          as::acc_add(a, p, x - lse, myq - key, key == lo, far);
          if (tok_class) {
            const int bit = (r & 3) + 8 * (r >> 2);
#pragma unroll
            for (int k = 0; k < 4; ++k) a.cls[k] += (cw[k][kb] >> bit) & 1u ? p : 0.f;
          }
          if (kb) s1[r] = p;
          else s0[r] = p;
        }
      }
    }
    if (rpart) {
      const float v = colsum_wg(s0, s1, 1.0f, kept, red, wave, lane, tid);
      if (tid < KT && k0 + tid < T) rpart[wg * T + k0 + tid] = v;
    }
  });

  // ---- the row: both halves of the keys, then out
  float st[as::NS];
  {
    as::Acc o;
    o.ent = a.ent + __shfl_xor(a.ent, 32, 64);
#pragma unroll
    for (int c = 0; c < 4; ++c) o.cls[c] = a.cls[c] + __shfl_xor(a.cls[c], 32, 64);
#pragma unroll
    for (int c = 0; c < 5; ++c) o.dist[c] = a.dist[c] + __shfl_xor(a.dist[c], 32, 64);
    o.md = a.md + __shfl_xor(a.md, 32, 64);
    o.mx = fmaxf(a.mx, __shfl_xor(a.mx, 32, 64));
    o.first = a.first + __shfl_xor(a.first, 32, 64);
    as::acc_stats(o, qok ? myq - lo + 1 : 1, st);
  }
  float* stage = red;  // colsum_wg ended with a barrier
  if (hl == 0) {
    float* sr = stage + (myq - q0) * as::STP;
#pragma unroll
    for (int i = 0; i < as::NS; ++i) sr[i] = kept ? st[i] : 0.f;
    sr[as::NS] = kept ? 1.f : 0.f;
    if (qok) {
      if (rows) {
        float* rr = rows + ((long long)bh * T + myq) * as::NS;
#pragma unroll
        for (int i = 0; i < as::NS; ++i) rr[i] = kept ? st[i] : 0.f;
      }
      if (nvis && hh == 0) nvis[rowbase + myq] = myq - lo + 1;
    }
  }
  __syncthreads();
  as::tile_sums(stage, hpart, cnt, wg, (long long)b * nqt + qtile, hh == 0, tid);
}

// ---------------------------------------------------------------------------
// vector kernel.  grid (B*H, q-tiles), 128 threads, one query each
// ---------------------------------------------------------------------------
template <typename T_>
__global__ __launch_bounds__(128) void attn_stats_vec(const T_* __restrict__ qkv, long long ld,
                                                      const int32_t* __restrict__ seg, int T, int H, int KV, int hd,
                                                      int window, float scale, const int64_t* __restrict__ idx,
                                                      int pad_id, const uint8_t* __restrict__ tok_class, int V,
                                                      const uint8_t* __restrict__ row_keep, float* __restrict__ rows,
                                                      int32_t* __restrict__ nvis, float* __restrict__ rpart,
                                                      double* __restrict__ hpart, double* __restrict__ cnt) {
  constexpr int KT = 64, PS = KT + 1;
  __shared__ __attribute__((aligned(16))) float Ks[KT][AV_HD];
  __shared__ float Pt[as::QT * PS];  // the tile's kept P ([query][key], padded); then the staged rows
  __shared__ int cls[KT];
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, b = bh / H, hh = bh % H, kvh = hh / (H / KV);
  const int nqt = gridDim.y;
  const int qtile = nqt - 1 - blockIdx.y;
  const int q0 = qtile * as::QT, myq = q0 + tid;
  const bool qok = myq < T;
  const long long rowbase = (long long)b * T;
  float qv[AV_HD];
#pragma unroll
  for (int d = 0; d < AV_HD; ++d)
    qv[d] = (qok && d < hd) ? ld_act<T_>(qkv + (rowbase + myq) * ld + (long long)hh * hd + d) : 0.f;
  const int lo = qok ? fa::lo_of(seg, rowbase, myq, T, window) : 0x7fffffff;
  const int kmin = fa::lo_of(seg, rowbase, q0, T, window);
  const int kmax = min(T - 1, q0 + as::QT - 1);
  const bool kept = qok && as::row_kept(idx, pad_id, row_keep, rowbase + myq);
  const int t0 = kmin / KT, t1 = kmax / KT;
  const long long wg = (long long)bh * nqt + qtile;
  const long long koff = (long long)(H + kvh) * hd;

  if (rpart)
    for (int k = tid; k < T; k += 128)
      if (k < t0 * KT || k >= (t1 + 1) * KT) rpart[wg * T + k] = 0.f;

  auto load_tile = [&](int k0, bool with_cls) __attribute__((always_inline)) {
    __syncthreads();
    for (int e = tid; e < KT * AV_HD; e += 128) {
      const int j = e / AV_HD, d = e % AV_HD;
      Ks[j][d] = (k0 + j < T && d < hd) ? ld_act<T_>(qkv + (rowbase + k0 + j) * ld + koff + d) : 0.f;
    }
    if (with_cls && tid < KT) cls[tid] = as::key_class(idx, tok_class, V, rowbase, k0 + tid, T);
    __syncthreads();
  };
  auto score = [&](int j) __attribute__((always_inline)) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < AV_HD; d += 4) {
      const float4 k4 = *(const float4*)&Ks[j][d];
      acc = fmaf(qv[d], k4.x, acc);
      acc = fmaf(qv[d + 1], k4.y, acc);
      acc = fmaf(qv[d + 2], k4.z, acc);
      acc = fmaf(qv[d + 3], k4.w, acc);
    }
    return acc * scale;
  };

  float m = -INFINITY, l = 0.f;
  for (int t = t0; t <= t1; ++t) {
    const int k0 = t * KT;
    load_tile(k0, false);
#pragma unroll 1
    for (int j = 0; j < KT; ++j) {
      const int key = k0 + j;
      if (key > myq || key < lo) continue;
      const float x = score(j);
      if (x > m) {
        l = l * expf(m - x) + 1.f;
        m = x;
      } else {
        l += expf(x - m);
      }
    }
  }
  const float lse = qok ? m + logf(l) : 0.f;

  as::Acc a = as::acc_zero();
  for (int t = t0; t <= t1; ++t) {
    const int k0 = t * KT;
    load_tile(k0, true);
#pragma unroll 1
    for (int j = 0; j < KT; ++j) {
      const int key = k0 + j;
      float p = 0.f;
      if (key <= myq && key >= lo) {
        const float x = score(j);
        p = expf(x - lse);
        as::acc_add(a, p, x - lse, myq - key, key == lo, false);
        const int c = cls[j];
        if (c < 4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) a.cls[k] += c == k ? p : 0.f;
        }
      }
      if (rpart) Pt[tid * PS + j] = kept ? p : 0.f;
    }
    if (rpart) {
      __syncthreads();
      if (tid < KT && k0 + tid < T) {
        float v = 0.f;
        for (int q = 0; q < as::QT; ++q) v += Pt[q * PS + tid];
        rpart[wg * T + k0 + tid] = v;
      }
    }
  }
  __syncthreads();
  float st[as::NS];
  as::acc_stats(a, qok ? myq - lo + 1 : 1, st);
  float* sr = Pt + tid * as::STP;
#pragma unroll
  for (int i = 0; i < as::NS; ++i) sr[i] = kept ? st[i] : 0.f;
  sr[as::NS] = kept ? 1.f : 0.f;
  if (qok) {
    if (rows) {
      float* rr = rows + ((long long)bh * T + myq) * as::NS;
#pragma unroll
      for (int i = 0; i < as::NS; ++i) rr[i] = kept ? st[i] : 0.f;
    }
    if (nvis && hh == 0) nvis[rowbase + myq] = myq - lo + 1;
  }
  __syncthreads();
  as::tile_sums(Pt, hpart, cnt, wg, (long long)b * nqt + qtile, hh == 0, tid);
}

// received[b][h][k] = the q-tiles' column sums added in ascending tile order
__global__ __launch_bounds__(256) void attn_stats_finish_recv(const float* __restrict__ rpart,
                                                              float* __restrict__ received, int T, int nqt) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= T) return;
  const long long bh = blockIdx.y;
  float v = 0.f;
  for (int qt = 0; qt < nqt; ++qt) v += rpart[(bh * nqt + qt) * T + k];
  received[bh * T + k] = v;
}
// head_acc[h][s] += the (b, q-tile) sums in ascending (b, tile) order; n_rows += the kept count
__global__ __launch_bounds__(256) void attn_stats_finish_heads(const double* __restrict__ hpart,
                                                               const double* __restrict__ cnt,
                                                               double* __restrict__ head_acc,
                                                               double* __restrict__ n_rows, int B, int H, int nqt) {
  for (int e = threadIdx.x; e <= H * as::NS; e += 256) {
    double s = 0.0;
    if (e < H * as::NS) {
      if (!head_acc) continue;
      const int h = e / as::NS, i = e % as::NS;
      for (int b = 0; b < B; ++b)
        for (int qt = 0; qt < nqt; ++qt) s += hpart[(((long long)b * H + h) * nqt + qt) * as::NS + i];
      head_acc[e] += s;
    } else if (n_rows) {
      for (long long i = 0; i < (long long)B * nqt; ++i) s += cnt[i];
      n_rows[0] += s;
    }
  }
}

static inline size_t attn_stats_ws_doubles(int B, int T, int H) {
  const size_t nqt = (size_t)cg_cdiv(T, as::QT);
  return (size_t)B * H * nqt * as::NS + (size_t)B * nqt;
}

extern "C" size_t cg_attn_stats_workspace(int B, int T, int H) {
  if (B <= 0 || T <= 0 || H <= 0) return 0;
  return attn_stats_ws_doubles(B, T, H) * sizeof(double) +
         (size_t)B * H * cg_cdiv(T, as::QT) * (size_t)T * sizeof(float);
}

extern "C" int cg_attn_stats(const cg_attn_stats_desc* d, void* stream) {
  if (!d) return CG_EINVAL;
  if (d->B < 0 || d->T < 0 || d->H <= 0 || d->KV <= 0 || d->H % d->KV) return CG_EINVAL;
  if (d->tok_class && (!d->idx || d->V <= 0)) return CG_EINVAL;
  if (d->dtype != CG_BF16 && d->dtype != CG_F32) return CG_EUNSUPPORTED;
  if (d->hd <= 0 || d->hd > AV_HD) return CG_EUNSUPPORTED;
  if (d->B == 0 || d->T == 0) return CG_OK;
  if (!d->qkv || d->ldqkv < (long long)(d->H + 2 * d->KV) * d->hd) return CG_EINVAL;
  if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->ws_bytes < cg_attn_stats_workspace(d->B, d->T, d->H))
    return CG_EINVAL;
  const int B = d->B, T = d->T, H = d->H, nqt = cg_cdiv(T, as::QT);
  hipStream_t s = (hipStream_t)stream;
  double* hpart = (double*)d->workspace;
  double* cnt = hpart + (size_t)B * H * nqt * as::NS;
  float* rpart = d->received ? (float*)(cnt + (size_t)B * nqt) : nullptr;
  const float scale = 1.0f / sqrtf((float)d->hd);
  const dim3 g(B * H, nqt);
  const bool mfma = d->dtype == CG_BF16 && d->hd % 8 == 0 && d->ldqkv % 8 == 0 && ((uintptr_t)d->qkv & 15) == 0 &&
                    (long long)T * d->ldqkv * 2 < 0x7fffffffLL;
#define AS_ARGS(TY)                                                                                               \
  (const TY*)d->qkv, d->ldqkv, d->segstart, T, H, d->KV, d->hd, d->window, scale, d->idx, d->pad_id, d->tok_class, \
      d->V, d->row_keep, d->rows, d->nvis, rpart, hpart, cnt
  if (mfma) {
    const size_t sh = 2 * fa::IMG + fa::COLSUM_LDS;
    switch ((d->hd + 15) >> 4) {
      case 1: hipLaunchKernelGGL(attn_stats_mfma<1>, g, dim3(256), sh, s, AS_ARGS(bf16_t)); break;
      case 2: hipLaunchKernelGGL(attn_stats_mfma<2>, g, dim3(256), sh, s, AS_ARGS(bf16_t)); break;
      case 3: hipLaunchKernelGGL(attn_stats_mfma<3>, g, dim3(256), sh, s, AS_ARGS(bf16_t)); break;
      default: hipLaunchKernelGGL(attn_stats_mfma<4>, g, dim3(256), sh, s, AS_ARGS(bf16_t)); break;
    }
  } else if (d->dtype == CG_BF16) {
    hipLaunchKernelGGL(attn_stats_vec<bf16_t>, g, dim3(128), 0, s, AS_ARGS(bf16_t));
  } else {
    hipLaunchKernelGGL(attn_stats_vec<float>, g, dim3(128), 0, s, AS_ARGS(float));
  }
#undef AS_ARGS
  CG_LAUNCH_CHECK();
  if (d->received) {
    hipLaunchKernelGGL(attn_stats_finish_recv, dim3(cg_cdiv(T, 256), B * H), dim3(256), 0, s, rpart, d->received, T,
                       nqt);
    CG_LAUNCH_CHECK();
  }
  if (d->head_acc || d->n_rows) {
    hipLaunchKernelGGL(attn_stats_finish_heads, dim3(1), dim3(256), 0, s, hpart, cnt, d->head_acc, d->n_rows, B, H,
                       nqt);
    CG_LAUNCH_CHECK();
  }
  return CG_OK;
}

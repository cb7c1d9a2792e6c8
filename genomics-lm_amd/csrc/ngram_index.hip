// Memorization audit: an exact window-membership index over byte symbols
// (contracts: include/codonlm_hip.h, cg_ngram_index_build / cg_ngram_coverage).
// The table is open addressing over uint32 start positions: a slot is claimed once with an agent-scope
// 32-bit compare-and-swap and never changes afterwards, so a probe needs no other synchronisation.  Every
// output is an integer that does not depend on which duplicate won a slot.
#include "common.h"

namespace {
constexpr int NI_TILE = 256;                         // window starts per tile (= the workgroup)
constexpr int NI_HALO = CG_NGRAM_INDEX_MAX_N - 1;    // symbols past the tile its last window reads
constexpr int NI_WORDS = (NI_TILE + NI_HALO + 3 + 3) / 4;  // + up to 3 symbols in front of an unaligned tile
constexpr int NI_BND = (NI_TILE + NI_HALO + 31) / 32 + 1;  // boundary bits of a tile and its halo
constexpr int NI_BLK = 2048;                         // grid cap (tiles / queries beyond it are grid-strided)
constexpr int NI_QWORDS = CG_NGRAM_MAX_QUERY / 32;   // hit bits of one query
constexpr uint32_t NI_EMPTY = 0xFFFFFFFFu;

// src[a, b) (b - a <= NI_TILE + NI_HALO, b <= total) into the LDS tile as aligned 32-bit words (src is
// 4-byte aligned); returns the byte of the tile that holds symbol a.  The last word of the buffer is
// assembled from its bytes, so nothing past `total` is read.
__device__ __forceinline__ int stage_tile(const uint8_t* __restrict__ src, long long total, long long a, long long b,
                                          uint32_t* tile) {
  const long long a4 = a & ~3ll;
  const int words = (int)((b - a4 + 3) >> 2);
  for (int w = threadIdx.x; w < words; w += NI_TILE) {
    const long long p = a4 + 4ll * w;
    uint32_t v = 0;
    if (p + 4 <= total) {
      v = *(const uint32_t*)(src + p);
    } else {
      for (int k = 0; k < 4; ++k)
        if (p + k < total) v |= (uint32_t)src[p + k] << (8 * k);
    }
    tile[w] = v;
  }
  return (int)(a - a4);
}

// a function of the n symbols only: murmur3's 32-bit body over little-endian words, then its finaliser
__device__ __forceinline__ uint32_t window_hash(const uint8_t* w, int n) {
  uint32_t h = 0x9E3779B9u;
  int j = 0;
  for (; j < n; j += 4) {
    uint32_t k = w[j];
    if (j + 1 < n) k |= (uint32_t)w[j + 1] << 8;
    if (j + 2 < n) k |= (uint32_t)w[j + 2] << 16;
    if (j + 3 < n) k |= (uint32_t)w[j + 3] << 24;
    k *= 0xCC9E2D51u; k = (k << 15) | (k >> 17); k *= 0x1B873593u;
    h ^= k; h = (h << 13) | (h >> 19); h = h * 5u + 0xE6546B64u;
  }
  return cg_fmix32(h ^ (uint32_t)n);
}

// the window stored at position p of sym against the thread's own (in LDS); a position the buffer
// cannot hold (a table the caller did not fill as asked) compares unequal and is never read
__device__ __forceinline__ bool same_window(const uint8_t* __restrict__ sym, long long n_sym, uint32_t p,
                                            const uint8_t* w, int n) {
  if ((long long)p + n > n_sym) return false;
  const uint8_t* s = sym + p;
  for (int j = 0; j < n; ++j)
    if (s[j] != w[j]) return false;
  return true;
}

struct BuildArgs {
  const uint8_t* sym; long long n_sym;
  const int64_t* offsets;
  int seq_lo, seq_hi, n;
  uint32_t* table; unsigned long long capacity;
  unsigned long long* n_unique; unsigned long long* n_dropped;
};

// Tiles of 256 flat positions of [offsets[seq_lo], offsets[seq_hi]), grid-strided.  Per tile: the
// symbols and their halo go to LDS; the sequence starts (and the end of the range) that fall inside
// the tile or its halo become bits of an LDS mask, so a thread knows with two word reads whether its
// window would cross one; then hash, probe, claim.
__global__ __launch_bounds__(NI_TILE) void ngram_index_build_kernel(BuildArgs A) {
  __shared__ uint32_t tile[NI_WORDS];
  __shared__ uint32_t bnd[NI_BND];
  __shared__ unsigned int wsum[2][NI_TILE / 64];
  const int tid = threadIdx.x, n = A.n;
  long long lo = A.offsets[A.seq_lo], hi = A.offsets[A.seq_hi];
  lo = lo < 0 ? 0 : lo;
  hi = hi > A.n_sym ? A.n_sym : hi;
  const unsigned long long mask = A.capacity - 1;
  unsigned int claimed = 0, dropped = 0;
  const long long ntile = hi > lo ? (hi - lo + NI_TILE - 1) / NI_TILE : 0;
  for (long long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
    const long long t0 = lo + tl * NI_TILE;
    long long t1 = t0 + NI_TILE + NI_HALO;
    t1 = t1 > hi ? hi : t1;
    const int off = stage_tile(A.sym, A.n_sym, t0, t1, tile);
    for (int w = tid; w < NI_BND; w += NI_TILE) bnd[w] = 0;
    // s0 = the last sequence of the range that starts at or before t0 (the same search in every thread)
    int a = A.seq_lo, b = A.seq_hi;
    while (a < b) {
      const int m = a + (b - a + 1) / 2;
      if (A.offsets[m] <= t0) a = m; else b = m - 1;
    }
    __syncthreads();  // bnd is zero
    // offsets are non-decreasing: a thread stops at its first start past the halo
    for (long long s = (long long)a + 1 + tid; s <= A.seq_hi; s += NI_TILE) {
      const long long d = A.offsets[s] - t0;
      if (d >= NI_TILE + NI_HALO) break;
      if (d > 0) atomicOr(&bnd[d >> 5], 1u << (d & 31));
    }
    __syncthreads();
    const long long i = t0 + tid;
    bool live = i + n <= hi;
    if (live && n > 1) {
      // no sequence starts at i + 1 .. i + n - 1
      const int f = tid + 1;
      const unsigned long long two = (unsigned long long)bnd[f >> 5] | ((unsigned long long)bnd[(f >> 5) + 1] << 32);
      live = ((two >> (f & 31)) & ((1ull << (n - 1)) - 1ull)) == 0;
    }
    if (live) {
      const uint8_t* w = (const uint8_t*)tile + off + tid;
      unsigned long long slot = window_hash(w, n) & mask;
      bool done = false;
      for (unsigned long long probes = 0; probes < A.capacity; ++probes) {
        uint32_t cur = __hip_atomic_load(&A.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == NI_EMPTY) {
          uint32_t expected = NI_EMPTY;
          if (__hip_atomic_compare_exchange_strong(&A.table[slot], &expected, (uint32_t)i, __ATOMIC_RELAXED,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            ++claimed;
            done = true;
            break;
          }
          cur = expected;  // another window took the slot first
        }
        if (same_window(A.sym, A.n_sym, cur, w, n)) { done = true; break; }
        slot = (slot + 1) & mask;
      }
      if (!done) ++dropped;
    }
    __syncthreads();  // the tile and the mask are rewritten
  }
  claimed = (unsigned int)wave_sum((int)claimed);
  dropped = (unsigned int)wave_sum((int)dropped);
  if ((tid & 63) == 0) { wsum[0][tid >> 6] = claimed; wsum[1][tid >> 6] = dropped; }
  __syncthreads();
  if (tid < 2) {
    unsigned long long s = 0;
    for (int q = 0; q < NI_TILE / 64; ++q) s += wsum[tid][q];
    unsigned long long* dst = tid == 0 ? A.n_unique : A.n_dropped;
    if (dst && s) atomicAdd(dst, s);
  }
}

struct CoverArgs {
  const uint8_t* sym; long long n_sym;
  int n;
  const uint32_t* table; unsigned long long capacity;
  const uint8_t* qsym; long long n_qsym;
  const int64_t* qoffsets;
  int n_q, max_qlen;
  uint8_t* hit; int32_t* n_hit; int32_t* covered;
};

// One workgroup per query: (1) the window starts, a tile at a time, look their windows up and set a
// bit of the query's hit mask in LDS, (2) barrier, (3) position t is covered when a bit of
// [t - n + 1, t] is set; the two counts are reduced over the workgroup.
__global__ __launch_bounds__(NI_TILE) void ngram_coverage_kernel(CoverArgs A) {
  __shared__ uint32_t tile[NI_WORDS];
  __shared__ uint32_t bits[NI_QWORDS + 1];  // word 0 is a zero guard in front of the mask
  __shared__ int wsum[2][NI_TILE / 64];
  const int tid = threadIdx.x, n = A.n;
  const unsigned long long mask = A.capacity - 1;
  for (int q = blockIdx.x; q < A.n_q; q += gridDim.x) {
    long long q0 = A.qoffsets[q], q1 = A.qoffsets[q + 1];
    q0 = q0 < 0 ? 0 : q0;
    q1 = q1 > A.n_qsym ? A.n_qsym : q1;
    long long len64 = q1 - q0;
    len64 = len64 < 0 ? 0 : len64;
    const int len = len64 > A.max_qlen ? A.max_qlen : (int)len64;
    const int nstart = len >= n ? len - n + 1 : 0;
    for (int w = tid; w <= (len + 31) / 32; w += NI_TILE) bits[w] = 0;
    __syncthreads();
    for (int t0 = 0; t0 < nstart; t0 += NI_TILE) {
      int t1 = t0 + NI_TILE + NI_HALO;
      t1 = t1 > len ? len : t1;
      const int off = stage_tile(A.qsym, A.n_qsym, q0 + t0, q0 + t1, tile);
      __syncthreads();
      const int i = t0 + tid;
      if (i < nstart) {
        const uint8_t* w = (const uint8_t*)tile + off + tid;
        unsigned long long slot = window_hash(w, n) & mask;
        for (unsigned long long probes = 0; probes < A.capacity; ++probes) {
          const uint32_t cur = A.table[slot];
          if (cur == NI_EMPTY) break;
          if (same_window(A.sym, A.n_sym, cur, w, n)) {
            atomicOr(&bits[1 + (i >> 5)], 1u << (i & 31));
            break;
          }
          slot = (slot + 1) & mask;
        }
      }
      __syncthreads();  // the tile is rewritten
    }
    __syncthreads();
    int nh = 0, nc = 0;
    for (int t = tid; t < len; t += NI_TILE) {
      // bits t - 31 .. t of the mask in the high half of `two`; the guard word serves t < 32
      const int wd = 1 + (t >> 5);
      const unsigned long long two = ((unsigned long long)bits[wd] << 32) | bits[wd - 1];
      const uint32_t last32 = (uint32_t)(two >> ((t & 31) + 1));  // bit 31 = position t, bit 0 = t - 31
      const uint32_t h = last32 >> 31;
      nh += (int)h;
      nc += (last32 >> (32 - n)) != 0;
      if (A.hit) A.hit[q0 + t] = (uint8_t)h;
    }
    nh = wave_sum(nh);
    nc = wave_sum(nc);
    if ((tid & 63) == 0) { wsum[0][tid >> 6] = nh; wsum[1][tid >> 6] = nc; }
    __syncthreads();
    if (tid < 2) {
      int s = 0;
      for (int k = 0; k < NI_TILE / 64; ++k) s += wsum[tid][k];
      int32_t* dst = tid == 0 ? A.n_hit : A.covered;
      if (dst) dst[q] = s;
    }
    __syncthreads();  // bits and wsum are rewritten
  }
}

bool table_ok(const void* table, long long capacity) {
  return table && !((uintptr_t)table & 3) && capacity >= 2 && capacity <= (1ll << 32) &&
         (capacity & (capacity - 1)) == 0;
}
}  // namespace

extern "C" int cg_ngram_index_build(const cg_ngram_index_desc* d, void* stream) {
  if (!d || d->n < 1 || d->n_sym < 0 || d->n_seq < 0 || d->seq_lo < 0 || d->seq_hi < d->seq_lo || d->seq_hi > d->n_seq)
    return CG_EINVAL;
  if (d->n > CG_NGRAM_INDEX_MAX_N || d->n_sym > CG_NGRAM_INDEX_MAX_SYM) return CG_EUNSUPPORTED;
  if (d->seq_lo == d->seq_hi || d->n_sym < d->n) return CG_OK;
  if (!d->sym || ((uintptr_t)d->sym & 3) || !d->offsets || !table_ok(d->table, d->capacity)) return CG_EINVAL;
  if (((uintptr_t)d->n_unique | (uintptr_t)d->n_dropped) & 7) return CG_EINVAL;
  BuildArgs A;
  A.sym = d->sym; A.n_sym = d->n_sym; A.offsets = d->offsets;
  A.seq_lo = d->seq_lo; A.seq_hi = d->seq_hi; A.n = d->n;
  A.table = d->table; A.capacity = (unsigned long long)d->capacity;
  A.n_unique = (unsigned long long*)d->n_unique; A.n_dropped = (unsigned long long*)d->n_dropped;
  const int nblk = cg_grid_cap((d->n_sym + NI_TILE - 1) / NI_TILE, NI_BLK);
  hipLaunchKernelGGL(ngram_index_build_kernel, dim3(nblk), dim3(NI_TILE), 0, (hipStream_t)stream, A);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

extern "C" int cg_ngram_coverage(const cg_ngram_coverage_desc* d, void* stream) {
  if (!d || d->n < 1 || d->n_sym < 0 || d->n_qsym < 0 || d->n_q < 0 || d->max_qlen < 0) return CG_EINVAL;
  if (d->n > CG_NGRAM_INDEX_MAX_N || d->max_qlen > CG_NGRAM_MAX_QUERY || d->n_sym > CG_NGRAM_INDEX_MAX_SYM)
    return CG_EUNSUPPORTED;
  if (d->n_q == 0) return CG_OK;
  if (!d->qoffsets || !table_ok(d->table, d->capacity)) return CG_EINVAL;
  if ((d->n_sym > 0 && (!d->sym || ((uintptr_t)d->sym & 3))) || (d->n_qsym > 0 && (!d->qsym || ((uintptr_t)d->qsym & 3))))
    return CG_EINVAL;
  if (((uintptr_t)d->n_hit | (uintptr_t)d->covered) & 3) return CG_EINVAL;
  CoverArgs A;
  A.sym = d->sym; A.n_sym = d->n_sym; A.n = d->n;
  A.table = d->table; A.capacity = (unsigned long long)d->capacity;
  A.qsym = d->qsym; A.n_qsym = d->n_qsym; A.qoffsets = d->qoffsets;
  A.n_q = d->n_q; A.max_qlen = d->max_qlen;
  A.hit = d->hit; A.n_hit = d->n_hit; A.covered = d->covered;
  hipLaunchKernelGGL(ngram_coverage_kernel, dim3(cg_grid_cap(d->n_q, NI_BLK)), dim3(NI_TILE), 0, (hipStream_t)stream, A);
  CG_LAUNCH_CHECK();
  return CG_OK;
}

// Index arithmetic of the grouped dW kernel's LDS-DMA ring (gemm_dw.h), host-callable so that a
// stand-alone program can walk it under a host sanitizer (tools/dw_ring_check.cpp).
//
// The token range is counted in 64-token k-units whatever the ring's stage size: a work item
// (output tile x token slice) covers nt units, i.e. nt * (64 / BKT) ring stages, and the slices
// of a token split start at multiples of nt * 64 rows.  Stages are numbered by one global index
// g per workgroup that runs across tile seams; stage g lives in ring slot g % S.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DW_HD __host__ __device__ constexpr
#else
#define DW_HD constexpr
#endif

constexpr int DW_KUNIT = 64;

// k-units per token slice of a ksplit-way split (cg_gemm_dw_grouped sets Params::kc_steps from it)
DW_HD int dw_kc_steps(int K, int ksplit) {
  const int per = (K + ksplit - 1) / ksplit;
  return (per + DW_KUNIT - 1) / DW_KUNIT;
}
// k-units per work item (a ragged last unit -- and a last slice past K -- reads rows >= K out of
// range: zero fill)
DW_HD int dw_units(int K, int ksplit, int kc_steps) { return ksplit > 1 ? kc_steps : (K + DW_KUNIT - 1) / DW_KUNIT; }
// first token row that ring stage dt (0 .. nt * 64 / bkt - 1) of slice sl loads
DW_HD long long dw_stage_row0(int sl, int nt, int dt, int bkt) {
  return (long long)sl * nt * DW_KUNIT + (long long)dt * bkt;
}
// ring slot of global stage g
DW_HD int dw_slot(int g, int S) { return g % S; }
// the stage whose DMAs step g issues: it goes into the slot that stage g - 1 held, which every
// wave has finished with once it is past step g's barrier
DW_HD int dw_issue_stage(int g, int S) { return g + S - 1; }
// DMA wave-instructions that may stay outstanding when step g waits for the stage it needs:
//   64-token stages read stage g itself after the barrier: stages g+1 .. g+S-2 stay in flight
//   32-token stages read stage g+1 under stage g's MFMAs:  stages g+2 .. g+S-2 stay in flight
DW_HD int dw_wait_count(int S, int dps, bool read_ahead) { return (S - 2 - (read_ahead ? 1 : 0)) * dps; }

// byte offset (into the operand, relative to the stage's first token row and the tile's first
// column) that the lane whose DMA destination is stage-image byte `pos` must load: the image is
// 128-column sub-images of bkt k-rows x 256 B, 16-B chunks XOR-swizzled by bits 0-3 of the k-row
// (the bfg::mc_off image the fragment reads undo)
DW_HD unsigned dw_src_off(int pos, long long ld, int bkt) {
  const int sub_bytes = bkt * 256;
  const int sub = pos / sub_bytes, q = pos % sub_bytes;
  const int krow = q >> 8, phys = (q >> 4) & 15;
  const int ch = phys ^ (((krow & 3) << 2) | ((krow >> 2) & 3));
  return (unsigned)(((long long)krow * ld + 128 * sub + 8 * ch) * 2);
}

// Fragment reads of the 32-token ring.  Lane `lane` of a 16x16x32 fragment of columns rr0 .. rr0+15
// (rr0 a multiple of 16 below 128) reads, with two ds_read_b64_tr_b16 (hi = 0 / 1), the 8 bytes at
// k-row 8 (lane >> 4) + ((lane & 15) >> 2) + 4 hi, columns rr0 + 4 (lane & 3) .. + 3.  Their image
// offset mc_off(krow, rr0 / 8 + e) + 8 (lane & 1), e = (lane & 3) >> 1, splits into a lane constant
// and 2 * rr0 XORed into bits 5-7 (rr0 / 8 is even, so e never carries into it).  The image base
// (ring slot + sub-image, a multiple of 8 KiB on a 256-aligned LDS base) can be added before the XOR.
DW_HD unsigned dw_frag_lane_off(int lane, int hi) {
  const int krow = 8 * (lane >> 4) + ((lane & 15) >> 2) + 4 * hi;
  const int e = (lane & 3) >> 1;
  return (unsigned)(krow * 256 + 16 * (e ^ (((krow & 3) << 2) | ((krow >> 2) & 3))) + 8 * (lane & 1));
}
DW_HD unsigned dw_frag_addr(unsigned img, unsigned lane_off, int rr0) { return (img + lane_off) ^ (unsigned)(2 * rr0); }

// Host walk of the grouped dW kernel's ring arithmetic (csrc/gemm_dw_ring.h), meant to be built
// with a host sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I genomics-lm_amd/csrc tools/dw_ring_check.cpp -o dw_ring_check && ./dw_ring_check
// It replays, for token counts at the edges of a stage and of a token slice, what one workgroup
// does: which slot and which source rows every stage uses, when it is issued, waited for and
// read, and where its bytes lie in LDS -- on real arrays, so that an index out of range trips
// the sanitizer, and with explicit checks of the ring's invariants.  Exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_dw_ring.h"

static int fails = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      ++fails;                                 \
      std::printf("FAIL %s: ", #c);            \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
    }                                          \
  } while (0)

// slices x stages cover rows [0, K) exactly once, in order; rows >= K are the zero fill
static void walk_rows(int K, int ksplit, int bkt) {
  const int kc = ksplit > 1 ? dw_kc_steps(K, ksplit) : 0;
  const int nt = dw_units(K, ksplit, kc);
  const int spu = DW_KUNIT / bkt;
  std::vector<int> seen(K, 0);
  long long next = 0;
  for (int sl = 0; sl < ksplit; ++sl)
    for (int dt = 0; dt < nt * spu; ++dt) {
      const long long r0 = dw_stage_row0(sl, nt, dt, bkt);
      CHECK(r0 == next, "K %d ksplit %d bkt %d slice %d stage %d starts at %lld, expected %lld", K, ksplit, bkt, sl, dt, r0, next);
      next = r0 + bkt;
      for (long long r = r0; r < r0 + bkt; ++r)
        if (r < K) ++seen[r];
    }
  CHECK(next >= K, "K %d ksplit %d bkt %d: rows end at %lld", K, ksplit, bkt, next);
  for (int r = 0; r < K; ++r) CHECK(seen[r] == 1, "K %d ksplit %d bkt %d row %d loaded %d times", K, ksplit, bkt, r, seen[r]);
  // the slice boundaries do not depend on the stage size
  CHECK(dw_stage_row0(1, nt, 0, 32) == dw_stage_row0(1, nt, 0, 64), "slice boundary moved");
}

// one workgroup's ring over `stages` stages (its tiles back to back) on S slots
static void walk_ring(int stages, int S, int dps, bool read_ahead) {
  std::vector<int> slot(S, -1);       // stage resident in (or in flight to) each slot
  std::vector<int> issued_at;         // step during which stage s was issued (-1: prologue)
  std::vector<char> read(stages + S + 1, 0);
  int issued = 0, done_reading = -1;  // stages < issued are issued; every wave has read stages <= done_reading
  auto issue = [&](int s, int at) {
    const int sl = dw_slot(s, S);
    CHECK(slot[sl] <= done_reading, "stage %d overwrites slot %d holding unread stage %d", s, sl, slot[sl]);
    slot[sl] = s;
    issued_at.push_back(at);
    CHECK(s == issued, "stage %d issued out of order", s);
    ++issued;
  };
  auto landed = [&](int outstanding) { return issued - 1 - outstanding / dps; };  // newest stage surely landed
  for (int s = 0; s < S - 1; ++s) issue(s, -1);
  if (read_ahead) {  // the prologue's wait, barrier and read of stage 0
    CHECK(landed(dw_wait_count(S, dps, false)) >= 0, "stage 0 not landed");
    read[0] = 1;
  }
  for (int g = 0; g < stages; ++g) {
    const int need = read_ahead ? g + 1 : g;
    CHECK(landed(dw_wait_count(S, dps, read_ahead)) >= need, "step %d: stage %d may not have landed", g, need);
    CHECK(issued - 1 - need >= (read_ahead ? S - 3 : S - 2), "step %d: fewer stages in flight than planned", g);
    if (need < stages) CHECK(g - issued_at[need] >= (read_ahead && g > 0 ? 2 : 1) || issued_at[need] < 0, "step %d waits for stage %d issued in step %d", g, need, issued_at[need]);
    // past the barrier every wave has consumed stage g - 1
    done_reading = g - 1;
    CHECK(slot[dw_slot(need, S)] == need, "step %d reads slot %d which holds stage %d", g, dw_slot(need, S), slot[dw_slot(need, S)]);
    read[need] = 1;
    if (!read_ahead) CHECK(read[g], "step %d multiplies unread fragments", g);
    else CHECK(read[g], "step %d multiplies fragments of a stage never read", g);
    issue(dw_issue_stage(g, S), g);
  }
}

// the DMA image of a stage: every byte written once, and the fragment reads find their columns
static void walk_image(int bkt, int rows, int cols, int waves, long long ld) {
  const int bytes = rows * bkt * 2 + cols * bkt * 2;
  std::vector<int> lds(bytes, 0);
  const int a_bytes = rows * bkt * 2;
  for (int op = 0; op < 2; ++op) {
    const int ob = op ? cols * bkt * 2 : a_bytes, base = op ? a_bytes : 0;
    for (int w = 0; w < waves; ++w)
      for (int i = 0; i < ob / 1024 / waves; ++i)
        for (int lane = 0; lane < 64; ++lane) {
          const int pos = (w + waves * i) * 1024 + 16 * lane;
          const unsigned src = dw_src_off(pos, ld, bkt);
          const long long el = src / 2, krow = el / ld, col = el % ld;
          CHECK(krow < bkt && col + 8 <= (op ? cols : rows), "bkt %d pos %d loads row %lld col %lld", bkt, pos, krow, col);
          for (int b = 0; b < 16; ++b) ++lds[base + pos + b];
        }
  }
  for (int b = 0; b < bytes; ++b) CHECK(lds[b] == 1, "bkt %d LDS byte %d written %d times", bkt, b, lds[b]);
  if (bkt != 32) return;
  const int sub_bytes = bkt * 256;
  for (int sub = 0; sub < 2; ++sub)
    for (int rr0 = 0; rr0 < 128; rr0 += 16)
      for (int lane = 0; lane < 64; ++lane)
        for (int hi = 0; hi < 2; ++hi) {
          const unsigned img = 3u * 32768u + sub * sub_bytes;  // a ring slot + sub-image
          const unsigned a = dw_frag_addr(img, dw_frag_lane_off(lane, hi), rr0) - img;
          CHECK(a + 8 <= (unsigned)sub_bytes, "fragment read at %u leaves its sub-image", a);
          (void)lds[sub * sub_bytes + a + 7];
          const int krow = 8 * (lane >> 4) + ((lane & 15) >> 2) + 4 * hi, col = rr0 + 4 * (lane & 3);
          const unsigned src = dw_src_off((int)(a & ~15u), ld, bkt) + (a & 8u);
          CHECK(src == (unsigned)((krow * ld + col) * 2), "lane %d hi %d rr0 %d reads source byte %u, wants row %d col %d", lane, hi, rr0, src, krow, col);
        }
}

int main() {
  const int Ks[] = {1, 8, 31, 32, 33, 63, 64, 65, 96, 97, 129, 160, 161, 37, 100, 193, 1023, 2048, 32768};
  for (int K : Ks)
    for (int ksplit = 1; ksplit <= 8; ++ksplit)
      for (int bkt : {32, 64}) walk_rows(K, ksplit, bkt);
  for (int K : Ks) {
    const int units = dw_units(K, 1, 0);
    for (int tiles = 1; tiles <= 3; ++tiles) {
      walk_ring(tiles * units * 2, 5, 4, true);   // 256 x 256: 32-token stages, 5 slots, 4 DMAs per stage
      walk_ring(tiles * units * 2, 4, 4, true);   // (the 4-slot ring that was measured)
      walk_ring(tiles * units, 3, 6, false);      // 256 x 128
      walk_ring(tiles * units, 4, 8, false);      // 128 x 128
      walk_ring(tiles * units, 5, 8, false);
    }
  }
  for (long long ld : {256ll, 264ll, 2048ll}) {
    walk_image(32, 256, 256, 8, ld);
    walk_image(64, 256, 128, 8, ld);
    walk_image(64, 128, 128, 4, ld);
  }
  std::printf(fails ? "dw_ring_check: %d checks failed\n" : "dw_ring_check: ok\n", fails);
  return fails ? 1 : 0;
}

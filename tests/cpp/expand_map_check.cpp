// Host check of the expand kernel's block-to-thread mapping (spblas-reference_amd/csrc/expand_map.hpp): for both group
// widths (8 lanes per block: fp32, 4: fp64) it enumerates every range [b0, b1) with 0 <= b0 <= b1 <= 3 * L * 16 + 2, L =
// the blocks a wavefront takes per iteration, walks every thread through its iterations the way the kernel does, and asserts
//   - every block of the range is handled by exactly one group of lanes, exactly once, and no block outside it is;
//   - no table index outside [b0, b1) is ever read (the tables may end at b1);
//   - the table words a wavefront reads in one iteration are consecutive and lie in ONE aligned 128-byte line (32 words)
//     whenever b0 is a multiple of 32.
// Built with -fsanitize=address,undefined by tests/test_expand_mapping_cpu.py.  Prints "ok" and exits 0 on success.
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "expand_map.hpp"

using namespace spb;

static std::atomic<long long> fails{0};
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c) && fails++ < 20) {                \
      std::fprintf(stderr, "FAIL %s: ", #c);   \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
    }                                          \
  } while (0)

// the ranges whose b0 is part, part + parts, ... (the enumeration is spread over a few threads: 1.5 M ranges x 256 groups)
static long long check(int part, int parts) {
  long long ranges = 0;
  for (int lpb : {8, 4}) {
    const int groups = PB_EXP_THREADS / lpb;  // groups of lanes in the workgroup
    const int L = 2 * 64 / lpb;               // blocks of a wavefront per iteration
    const int BMAX = 3 * L * 16 + 2;
    // the lanes of a group agree on everything (checked once on a range every thread has work in)
    for (int tid = 0; tid < PB_EXP_THREADS; ++tid)
      for (int it = 0; it < 2; ++it) {
        const pb_exp_blocks m = pb_exp_map(tid, it, 5, BMAX, lpb), g = pb_exp_map(tid / lpb * lpb, it, 5, BMAX, lpb);
        CHECK(m.a == g.a && m.b == g.b && m.a_on == g.a_on && m.b_on == g.b_on, "lpb %d tid %d: lanes of a group disagree", lpb, tid);
      }
    std::vector<int> seen(BMAX + 1);
    for (int b0 = part; b0 <= BMAX; b0 += parts)
      for (int b1 = b0; b1 <= BMAX; ++b1, ++ranges) {
        for (int k = b0; k < b1; ++k)
          seen[k] = 0;
        auto touch = [&](int blk) {  // a group loads blksrc[blk], blkdst[blk] and the block's entries, stores its products
          CHECK(blk >= b0 && blk < b1, "lpb %d [%d,%d): table index %d", lpb, b0, b1, blk);
          if (blk >= b0 && blk < b1)
            ++seen[blk];
        };
        for (int g = 0; g < groups; ++g) {
          const int tid = g * lpb;
          for (int it = 0;; ++it) {  // the kernel's loop
            const pb_exp_blocks m = pb_exp_map(tid, it, b0, b1, lpb);
            CHECK(m.a_on || !m.b_on, "lpb %d [%d,%d) tid %d it %d: b without a", lpb, b0, b1, tid, it);
            if (!m.b_on) {
              if (m.a_on)
                touch(m.a);
              // the kernel stops here: nothing may be left for this thread
              const pb_exp_blocks nx = pb_exp_map(tid, it + 1, b0, b1, lpb);
              CHECK(!nx.a_on && !nx.b_on, "lpb %d [%d,%d) tid %d: work after iteration %d", lpb, b0, b1, tid, it);
              break;
            }
            touch(m.a);
            touch(m.b);
          }
        }
        for (int k = b0; k < b1; ++k)
          CHECK(seen[k] == 1, "lpb %d [%d,%d): block %d handled %d times", lpb, b0, b1, k, seen[k]);
        if (b0 % 32 == 0 && b1 > b0)  // the table words of a wavefront's iteration: consecutive, inside one aligned line
          for (int wave = 0; wave < PB_EXP_THREADS / 64; ++wave)
            for (int it = 0; pb_exp_map(wave * 64, it, b0, b1, lpb).a_on; ++it) {
              const pb_exp_blocks lo = pb_exp_map(wave * 64, it, b0, b1, lpb), hi = pb_exp_map(wave * 64 + 63, it, b0, b1, lpb);
              CHECK(hi.b - lo.a == L - 1 && hi.a - lo.a == 64 / lpb - 1 && lo.b - lo.a == 64 / lpb,
                    "lpb %d [%d,%d) wave %d it %d: words %d..%d not consecutive", lpb, b0, b1, wave, it, lo.a, hi.b);
              CHECK(lo.a / 32 == hi.b / 32 && lo.a % L == 0, "lpb %d [%d,%d) wave %d it %d: words %d..%d cross a 128-byte line", lpb,
                    b0, b1, wave, it, lo.a, hi.b);
            }
      }
  }
  return ranges;
}

int main() {
  const int parts = 8;
  long long done[parts] = {0};
  std::vector<std::thread> pool;
  for (int p = 0; p < parts; ++p)
    pool.emplace_back([&done, p] { done[p] = check(p, parts); });
  long long ranges = 0;
  for (int p = 0; p < parts; ++p) {
    pool[p].join();
    ranges += done[p];
  }
  if (fails) {
    std::fprintf(stderr, "%lld checks failed\n", fails.load());
    return 1;
  }
  std::printf("ok: %lld ranges\n", ranges);
  return 0;
}

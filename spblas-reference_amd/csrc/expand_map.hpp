// Which blocks of a range [b0, b1) of A' each thread of pb_expand_kernel (spmv_sliced.hip) handles.  Plain integer
// arithmetic, shared by the kernel and by a stand-alone host program (tests/cpp/expand_map_check.cpp) that enumerates it.
//
// lpb consecutive lanes own one block (8 for fp32, 4 for fp64), so one load instruction of a wavefront covers 64 / lpb
// consecutive blocks.  A thread keeps TWO blocks in flight per iteration, and the wavefront's two windows lie next to each
// other: in iteration `it` wavefront w covers the 2 * 64 / lpb blocks from b0 + it * 2 * PASS + w * 2 * 64 / lpb on, so the
// workgroup's 16 wavefronts read ONE contiguous piece of s_val, of s_col and of the two block tables per iteration, all of it
// requested while its neighbours are in flight.  (Until profiles/expand_read_attribution.md the second window lay PASS
// blocks behind the first: twice as many window edges, and every table line shared by four wavefronts at two different times.)
// The 4-byte table words of a wavefront's iteration are 2 * 64 / lpb consecutive words: one aligned 128-byte line (fp64) or an
// aligned half of one (fp32) whenever b0 is a multiple of 32.
#pragma once

#if defined(__HIPCC__)
#define PB_EXP_HD __host__ __device__ __forceinline__
#else
#define PB_EXP_HD inline
#endif

namespace spb {

constexpr int PB_EXP_THREADS = 1024;  // threads of an expand workgroup (PB_THREADS)

struct pb_exp_blocks {
  int a, b;         // the thread's two blocks of this iteration; they are also its indices into blksrc / blkdst
  bool a_on, b_on;  // ... and whether each lies in [b0, b1): nothing is loaded or stored for one that does not.
                    // b_on implies a_on, and a thread whose b_on is false has nothing in any later iteration
};

PB_EXP_HD pb_exp_blocks pb_exp_map(int tid, int it, int b0, int b1, int lpb) {
  const int pass = PB_EXP_THREADS / lpb;  // blocks one load instruction of the whole workgroup covers
  pb_exp_blocks m;
#ifdef PB_EXP_FAR_PASS  // A/B only (tools/build_variant.sh): the second window PASS blocks behind the first
  m.a = b0 + it * 2 * pass + tid / lpb;
  m.b = m.a + pass;
#else
  const int bpi = 64 / lpb;  // blocks one load instruction of a wavefront covers
  m.a = b0 + it * 2 * pass + (tid >> 6) * 2 * bpi + (tid & 63) / lpb;
  m.b = m.a + bpi;
#endif
  m.a_on = m.a < b1;
  m.b_on = m.b < b1;
  return m;
}

}  // namespace spb

#pragma once
// The level-set plan of the triangular solves (spblas_gfx950_sptrsv_create), shared by the vector solve (sptrsv.hip) and the
// solve with several right-hand sides (sptrsm.hip).  It holds structure only: both solves read it, neither changes it.
#include "common.hpp"

#include <vector>

struct spblas_gfx950_trsv_s {
  int64_t m = 0, nnz = 0;
  int uplo = 0, diag = 0;
  int32_t* order = nullptr;      // [m] rows sorted by level
  int32_t* level_ptr = nullptr;  // [n_levels + 1] device copy
  std::vector<int32_t> h_level_ptr;
  // launch groups: {first_level, last_level (exclusive), wide ? 1 : 0}
  struct group_t {
    int32_t l0, l1, wide;
  };
  std::vector<group_t> groups;
  int64_t max_width = 0;
  int lanes = 8;  // lanes per row in the solve kernels
  int narrow = 128;      // levels with fewer rows are "narrow": walked by one workgroup
  bool coop_ok = false;  // the solve is ONE cooperative launch (trsv_coop_kernel)
  int32_t* tickets = nullptr;         // device: status word and the grid barrier's counters / release lines
  // pinned, device-visible host word: a solve whose grid barrier ran into its poll bound sets it (system-scope store, only
  // on that path), the NEXT solve on this plan -- and spblas_gfx950_sptrsv_status -- reads it without touching the stream
  int* sticky = nullptr;
  spb::use_record use;  // the stream of the last solve / sweep / factorisation that read the plan: destroy frees behind it
};

namespace spb {

__device__ __forceinline__ bool trsv_strict(int c, int r, int upper) {
  return upper ? c > r : c < r;
}

// What every solve on a plan does before it launches anything (sptrsv.hip): refuses the plan's first solve on a capturing
// stream (the control words are sized and allocated here), reports a pending give-up of an earlier solve once, and zeroes
// the control words on the stream.  *bar_off = first int of the grid barrier inside pl->tickets; the status word is
// pl->tickets[groups + 1].
int trsv_begin_solve(spblas_gfx950_handle_t h, spblas_gfx950_trsv_s* pl, bool* capturing, size_t* bar_off);

} // namespace spb

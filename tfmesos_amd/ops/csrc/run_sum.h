// Hot runs of a run sum: the pieces shared by the fused sparse applies
// (sparse_apply.hip) and segment_sum_rows (coalesce.hip). Both sum, per
// destination, one contiguous run of a stable sort's permutation in position
// order; each keeps its own way of finding the run, of cutting a hot run
// into pieces (their pass-1 kernels decompose the work differently) and its
// own summation loop.
#pragma once

#include "tile.h"

// Hot runs. A run longer than CHUNK positions is cut into CHUNK-position
// pieces relative to the run start; separate waves sum the pieces into an
// fp32 scratch and the run's owner adds the partials in piece order. The
// piece k of a run starting at sorted position s owns scratch slot
// s / SLOT_DIV + k: runs are disjoint position ranges longer than
// CHUNK = 2 * SLOT_DIV, so a run's slots end before the next long run's
// begin (slots never collide) and n / SLOT_DIV + 1 slots always suffice.
constexpr int CHUNK = 512;     // positions one wave sums
constexpr int SLOT_DIV = 256;  // scratch slot of a long run = start/256 + k

// fp32 scratch rows a run sum over n positions needs (0: no run is long).
inline long run_scratch_rows(long n) {
  return n > CHUNK ? n / SLOT_DIV + 1 : 0;
}

// A position read from device memory, forced into [0, n].
DEVINL long clamp_pos(long p, long n) { return p < 0 ? 0 : (p > n ? n : p); }

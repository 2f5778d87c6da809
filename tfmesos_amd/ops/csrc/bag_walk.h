// The walk over one CSR bag shared by the pooled pulls (embedding_bag.hip:
// rows named by id; hash.hip: rows named by key, with an optional initial
// row for a key that has none), so both accumulate in the same order with
// the same expression and agree bit for bit on equal rows.
//
// One wave owns one (bag, 256-column tile): it takes the bag 64 positions at
// a time, one per lane, walks the contributing lanes in position order with
// a wave shuffle, keeps 4 row fetches in flight and accumulates in fp32
// registers. Fixed order, no atomics.
//
// The products c_i * row_i and the sums are SEPARATE fp32 operations (fp
// contraction is switched off in the walk): which of them a compiler fuses
// into an fma is otherwise its own choice per kernel and per element, and
// two kernels that must agree bit for bit cannot leave it open. It is also
// what the CPU reference computes (a product, then index_add_), so on the
// same rows the walk equals it bit for bit for combiner "sum".
//
// Src says what a position contributes (it may keep per-lane state):
//   long item(long p, bool& valid)   the lane's own position p in [s, e):
//       a handle of its row, and whether the position contributes;
//   void fetch(long id, int k, float (&v)[ACC])   all 64 lanes: the lane's
//       ACC elements (tile.h layout) of the row that lane k's item named;
//       id is that item's handle, the same in every lane.
#pragma once

#include "bag.h"
#include "tile.h"

// acc += sum over the contributing positions i of [s, e) of c_i * row_i.
// W: the bag's weight sum (bag_weight_sum) when mean, unused otherwise.
template <typename Src>
DEVINL void bag_walk(Src& src, const float* __restrict__ weights, long s,
                     long e, float W, bool mean, int lane,
                     float (&acc)[ACC]) {
#pragma clang fp contract(off)
  for (long p0 = s; p0 < e; p0 += WAVE) {
    const long p = p0 + lane;
    bool valid = false;
    long id = 0;
    if (p < e) id = src.item(p, valid);
    float cf = 0.f;
    if (valid) cf = bag_coef(weights ? weights[p] : 1.f, W, mean);
    else id = 0;
    // walk the valid lanes in position order, 4 row loads in flight
    unsigned long long m = __ballot(valid);
    while (__popcll(m) >= 4) {
      const int k0 = __ffsll(m) - 1; m &= m - 1;
      const int k1 = __ffsll(m) - 1; m &= m - 1;
      const int k2 = __ffsll(m) - 1; m &= m - 1;
      const int k3 = __ffsll(m) - 1; m &= m - 1;
      const long r0 = __shfl(id, k0), r1 = __shfl(id, k1);
      const long r2 = __shfl(id, k2), r3 = __shfl(id, k3);
      const float f0 = __shfl(cf, k0), f1 = __shfl(cf, k1);
      const float f2 = __shfl(cf, k2), f3 = __shfl(cf, k3);
      float v0[ACC], v1[ACC], v2[ACC], v3[ACC];
      src.fetch(r0, k0, v0);
      src.fetch(r1, k1, v1);
      src.fetch(r2, k2, v2);
      src.fetch(r3, k3, v3);
#pragma unroll
      for (int k = 0; k < ACC; ++k)
        acc[k] = (((acc[k] + f0 * v0[k]) + f1 * v1[k]) + f2 * v2[k]) +
                 f3 * v3[k];
    }
    while (m) {
      const int k0 = __ffsll(m) - 1; m &= m - 1;
      const long r = __shfl(id, k0);
      const float f = __shfl(cf, k0);
      float v[ACC];
      src.fetch(r, k0, v);
#pragma unroll
      for (int k = 0; k < ACC; ++k) acc[k] += f * v[k];
    }
  }
}

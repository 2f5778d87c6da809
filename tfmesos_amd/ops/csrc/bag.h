// CSR bag helpers shared by embedding_bag.hip (pooled pull) and
// sparse_apply.hip (pooled push), so both directions agree bit for bit on
// a bag's range, its weight sum W_b and every coefficient c_i.
#pragma once

#include "common.h"

// Positions [s, e) of bag b. offsets is a caller contract the GPU path
// does not validate (no device->host sync); clamping into [0, n] keeps a
// violating input from reading or writing out of bounds.
DEVINL void bag_range(const long* __restrict__ offsets, long b, long n,
                      long& s, long& e) {
  const long a = offsets[b], z = offsets[b + 1];
  s = a < 0 ? 0 : (a > n ? n : a);
  e = z < s ? s : (z > n ? n : z);
}

// W_b = sum of the weights of ALL positions of the bag (the bag length
// when unweighted). All 64 lanes call. Fixed order: lane l sums positions
// s+l, s+l+64, ... and an xor butterfly adds the lanes (a+b == b+a, so
// every lane ends with the same bits).
DEVINL float bag_weight_sum(const float* __restrict__ weights, long s, long e,
                            int lane) {
  if (weights == nullptr) return (float)(e - s);
  float w = 0.f;
  for (long p = s + lane; p < e; p += WAVE) w += weights[p];
#pragma unroll
  for (int m = WAVE / 2; m > 0; m >>= 1) w += __shfl_xor(w, m);
  return w;
}

// c_i: w_i for sum, w_i / W_b for mean, 0 when W_b == 0.
DEVINL float bag_coef(float w, float W, bool mean) {
  if (!mean) return w;
  return W == 0.f ? 0.f : w / W;
}

// FTRL-Proximal, one element: THE definition of the rule, shared by the
// dense apply (apply.hip) and the sparse apply (sparse_apply.hip).
//
// State per weight p: the accumulator a (sum of squared gradients only; it
// starts at 0 and acc0 = initial_accumulator_value is added on read, never
// stored) and the linear term c (starts at 0). lr_power is -0.5, l2 is the
// only regulariser (no weight decay, no l2 shrinkage).
//
// FTRL's weight is a pure function of (c, a). The tables here start from
// non-zero rows with zero state, so TF's rule would replace a row's initial
// value by about -lr*g/sqrt(acc0) on its first touch. A never-updated
// element (a == 0 and c == 0) therefore first gets the linear term that
// makes its current weight the FTRL solution: a zero gradient then leaves
// the weight where it is.
//
// All arithmetic is fp32 in the order written, not contracted into fused
// multiply-adds; sqrt and / are the correctly rounded ones; sign(0) = 0.
#pragma once

#include "common.h"

struct FtrlHp {
  float lr, l1, l2, acc0, gscale;
};

DEVINL float ftrl_sign(float x) {
  return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
}

// g: the (summed) gradient before grad_scale.
DEVINL void ftrl_elem(float& p, float& a, float& c, float g,
                      const FtrlHp& hp) {
#pragma clang fp contract(off)
  const float gv = g * hp.gscale;
  float lin = c;
  if (a == 0.f && lin == 0.f)   // never updated: seed the linear term
    lin = -(p * (__builtin_sqrtf(hp.acc0) / hp.lr + 2.f * hp.l2) +
            ftrl_sign(p) * hp.l1);
  const float n_new = a + gv * gv;
  const float s_old = __builtin_sqrtf(a + hp.acc0);
  const float s_new = __builtin_sqrtf(n_new + hp.acc0);
  const float sigma = (s_new - s_old) / hp.lr;
  const float z = lin + (gv - sigma * p);
  const float quad = s_new / hp.lr + 2.f * hp.l2;
  p = __builtin_fabsf(z) > hp.l1 ? (ftrl_sign(z) * hp.l1 - z) / quad : 0.f;
  a = n_new;
  c = z;
}

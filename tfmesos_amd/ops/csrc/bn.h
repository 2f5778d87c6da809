// Host-side interface of bn.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

// Which kernels one BN layer runs, decided once per call: the binding
// sizes `part` (Z * C * 2 floats) from it and the launchers follow it.
// rw_stats fixes the layout of part ([c][z] row-wise, [z][c] column-walk).
struct BnPlan {
  bool rw_stats;   // row-wise stats/finalize, else column-walk
  bool rw_apply;   // row-wise apply, else flat-walk (needs P*C < 2^31)
  int Z;           // stats slices
};
BnPlan bn_plan(long P, int C);
int bn_max_channels();

void launch_bn_fwd(const bf16_t* x, const bf16_t* g, const bf16_t* b,
                   bf16_t* y, long ldo, float* mean, float* invstd,
                   float* part, long P, int C, const BnPlan& plan, float eps,
                   bool relu, hipStream_t stream);
void launch_bn_bwd(const bf16_t* x, const bf16_t* dy, long ldy,
                   const bf16_t* g, const bf16_t* b, const float* mean,
                   const float* invstd, bf16_t* dx, bf16_t* dgamma,
                   bf16_t* dbeta, float* part, float* s1n, float* s2n,
                   long P, int C, const BnPlan& plan, bool relu,
                   hipStream_t stream);

// Grouped BN: n <= 8 branches [P, C_i] with C_i % 8 == 0,
// C_i <= bn_group_max_channels() and P*C_i < 2^31 (flat-walk applies).
// mean/invstd/dgamma/dbeta/s1n/s2n hold the branches' channels one after
// the other; part is bn_group_slices() * sum(C_i) * 2 floats.
struct BnGroup {
  int n;
  int C[8];
  const bf16_t* x[8];
  const bf16_t* g[8];
  const bf16_t* b[8];
  bf16_t* y[8];            // fwd: out base and row stride
  long yld[8];
  const bf16_t* dy[8];     // bwd: dy base and row stride, dense dx
  long dyld[8];
  bf16_t* dx[8];
};
int bn_group_max_channels();
int bn_group_slices(long P, const int* Cs, int n);
void launch_bn_group_fwd(const BnGroup& gr, float* mean, float* invstd,
                         float* part, long P, int Z, float eps, bool relu,
                         hipStream_t stream);
void launch_bn_group_bwd(const BnGroup& gr, const float* mean,
                         const float* invstd, bf16_t* dgamma, bf16_t* dbeta,
                         float* s1n, float* s2n, float* part, long P, int Z,
                         bool relu, hipStream_t stream);

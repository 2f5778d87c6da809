// Host-side interface of bn.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_bn_fwd(const bf16_t* x, const bf16_t* g, const bf16_t* b,
                   bf16_t* y, long ldo, float* mean, float* invstd,
                   float* part, long P, int C, int Z, float eps, bool relu,
                   hipStream_t stream);
void launch_bn_bwd(const bf16_t* x, const bf16_t* dy, long ldy,
                   const bf16_t* g, const bf16_t* b, const float* mean,
                   const float* invstd, bf16_t* dx, bf16_t* dgamma,
                   bf16_t* dbeta, float* part, float* s1n, float* s2n,
                   long P, int C, int Z, bool relu, hipStream_t stream);
int bn_stats_slices(long P, int C);
int bn_max_channels();
int bn_group_slices(long P, const int* Cs, int n);
void launch_bn_group_fwd(const bf16_t* const* xs, const bf16_t* const* gs,
                         const bf16_t* const* bs, const int* Cs, int n,
                         bf16_t* const* youts, const long* ylds,
                         float* mean, float* invstd,
                         float* part, long P, int Z, float eps, bool relu,
                         hipStream_t stream);
void launch_bn_group_bwd(const bf16_t* const* xs, const bf16_t* const* dys,
                         const long* dylds, const bf16_t* const* gs,
                         const bf16_t* const* bs, bf16_t* const* dxs,
                         const int* Cs, int n, const float* mean,
                         const float* invstd, bf16_t* dgamma, bf16_t* dbeta,
                         float* s1n, float* s2n, float* part, long P, int Z,
                         bool relu, hipStream_t stream);

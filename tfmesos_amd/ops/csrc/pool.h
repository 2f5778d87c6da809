// Host-side interface of pool.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_avg3x3(const bf16_t* X, bf16_t* Y, int N, int H, int W, int C,
                   hipStream_t stream);
void launch_maxpool3x3s2_fwd(const bf16_t* X, bf16_t* Y, long ldo,
                             unsigned char* idx,
                             int N, int H, int W, int C, int Ho, int Wo,
                             hipStream_t stream);
void launch_maxpool3x3s2_bwd(const bf16_t* dY, long ldy,
                             const unsigned char* idx,
                             bf16_t* dX, int N, int H, int W, int C, int Ho,
                             int Wo, hipStream_t stream);

// Host-side interface of elementwise.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_add_n(const bf16_t* const* srcs, int n, bf16_t* out, long total,
                  hipStream_t stream);
void launch_relu_bwd(const bf16_t* dy, const bf16_t* act, bf16_t* dx, long n,
                     hipStream_t stream);
void launch_colsum(const bf16_t* x, float* out, int M, int N,
                   hipStream_t stream);

// Host-side interface of embedding.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_gather_bf16(const bf16_t* table, const long* ids, bf16_t* out,
                        long n, int D, long V, hipStream_t stream);
void launch_gather_f32(const float* table, const long* ids, float* out,
                       long n, int D, long V, hipStream_t stream);
void launch_scatter_add_bf16(float* table, const long* ids,
                             const bf16_t* rows, long n, int D, long V,
                             hipStream_t stream);
void launch_scatter_add_f32(float* table, const long* ids, const float* rows,
                            long n, int D, long V, hipStream_t stream);

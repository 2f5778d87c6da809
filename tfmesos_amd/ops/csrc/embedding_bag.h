// Host-side interface of embedding_bag.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_embedding_bag(const void* table, bool t_bf16, const long* ids,
                          const long* offsets, const float* weights,
                          void* out, bool o_bf16, long B, long n, int D,
                          long V, bool mean, hipStream_t stream);

// Host-side interface of interaction.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kDotMaxF = 64;   // feature rows one wave's tiles cover

void launch_dot_interaction_fwd(const void* x, void* out, bool o_bf16, long B,
                                int F, int D, bool diag, bool keep,
                                hipStream_t stream);

void launch_dot_interaction_bwd(const void* x, const void* dout, bool g_bf16,
                                void* dx, long B, int F, int D, bool diag,
                                bool keep, hipStream_t stream);

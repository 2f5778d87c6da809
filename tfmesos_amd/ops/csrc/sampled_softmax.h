// Host-side interface of sampled_softmax.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kSampledMaxD = 256;   // row width one wave's A fragments cover

// splits of the candidate tiles in the forward: a function of (B, S) only
int sampled_softmax_nsplit(long B, long S);

void launch_sampled_softmax_fwd(const void* h, const void* w_true,
                                const void* w_samp, const float* true_adj,
                                const float* samp_adj, const long* labels,
                                const long* sampled, float* ws, float* lse,
                                float* loss, int B, int S, int D,
                                hipStream_t stream);

void launch_sampled_softmax_bwd(const void* h, const void* w_true,
                                const void* w_samp, const float* samp_adj,
                                const long* labels, const long* sampled,
                                const float* lse, const float* loss,
                                const float* g, void* dh, void* dw_true,
                                void* dw_samp, float* dtrue_adj,
                                float* dsamp_adj, int B, int S, int D,
                                hipStream_t stream);

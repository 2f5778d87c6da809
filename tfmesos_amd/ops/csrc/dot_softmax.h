// Host-side interface of dot_softmax.hip (shared with the binding TU); the
// definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kDotSoftmaxMaxD = 256;   // row width one wave's A fragments cover

// The splits of the streamed set a call runs with: the forward and the
// backward's role Q stream the V items, role W streams the B examples.
// splits == 0 is the default rule of mfma_stream.h (256 blocks' worth per
// role); anything else is clamped to the role's tile count and to 65535.
struct DotSoftmaxPlan { int fwd, bwd_q, bwd_w; };
DotSoftmaxPlan dot_softmax_plan(long B, long V, long splits);

void launch_dot_softmax_fwd(const void* q, const void* w, const float* bias,
                            const long* labels, float* ws, float* s_true,
                            float* lse, float* loss, int B, int V, int D,
                            int nsplit, hipStream_t stream);

void launch_dot_softmax_bwd(const void* q, const void* w, const float* bias,
                            const long* labels, const float* lse,
                            const float* loss, const float* g, float* part_q,
                            float* part_w, float* part_b, void* dq, void* dw,
                            float* dbias, int B, int V, int D, int nsplit_q,
                            int nsplit_w, hipStream_t stream);

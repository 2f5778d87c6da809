// Host-side interface of apply.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_sgd(float* p, const void* g, bool g_bf16, float* mbuf,
                bf16_t* pbf, long n, float lr, float momentum, float wd,
                float gscale, float negdecay, hipStream_t stream);
void launch_adam(float* p, const void* g, bool g_bf16, float* m, float* v,
                 bf16_t* pbf, long n, long step, float lr, float beta1,
                 float beta2, float eps, float wd, float gscale,
                 hipStream_t stream);
void launch_adagrad(float* p, const void* g, bool g_bf16, float* acc,
                    bf16_t* pbf, long n, float lr, float eps, float wd,
                    float gscale, hipStream_t stream);
// FTRL-Proximal (ftrl.h): acc = accumulator, lin = linear term, acc0 =
// initial_accumulator_value (added on read, never stored).
void launch_ftrl(float* p, const void* g, bool g_bf16, float* acc, float* lin,
                 bf16_t* pbf, long n, float lr, float l1, float l2,
                 float acc0, float gscale, hipStream_t stream);

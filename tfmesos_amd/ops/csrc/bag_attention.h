// Host-side interface of bag_attention.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kBagAttnMaxD = 128;   // head width one wave's A fragments cover

// upper bound of the 64-row tiles of B bags over n rows: shapes only
inline long bag_attention_max_tiles(long n, long B) { return (n + 63 * B) / 64; }

void launch_bag_attention_tiles(const long* offsets, const long* kv_offsets,
                                int* qpre, int* kpre, int n, int m, int B,
                                hipStream_t stream);

void launch_bag_attention_fwd(const void* q, const void* k, const void* v,
                              const long* offsets, const long* kv_offsets,
                              const int* qpre, const int* kpre, void* out,
                              float* lse, int n, int m, int B, int H, int D,
                              float scale, bool causal, hipStream_t stream);

void launch_bag_attention_bwd(const void* q, const void* k, const void* v,
                              const void* out, const void* dout,
                              const long* offsets, const long* kv_offsets,
                              const int* qpre, const int* kpre,
                              const float* lse, float* delta, void* dq,
                              void* dk, void* dv, int n, int m, int B, int H,
                              int D, float scale, bool causal,
                              hipStream_t stream);

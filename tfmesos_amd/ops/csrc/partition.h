// Host-side interface of partition.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

long shard_windows(long n);
void launch_shard_count(const long* ids, int* counts, long n, long V, int S,
                        bool div, hipStream_t stream);
void launch_shard_scatter(const long* ids, const long* incl, long* local,
                          long* perm, long* inv, long* starts, long n, long V,
                          int S, bool div, hipStream_t stream);
void launch_permute_rows(const void* rows, bool r_bf16, const long* perm,
                         void* out, bool o_bf16, long n_out, long n_rows,
                         int D, hipStream_t stream);
void launch_shard_bag_offsets(const long* perm, const long* starts,
                              const long* offsets, long* out, long n, long B,
                              int S, hipStream_t stream);
void launch_bag_coef(const long* offsets, const float* weights, float* coef,
                     long B, long n, bool mean, hipStream_t stream);

// Host-side interface of coalesce.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

long coalesce_windows(long n);
void launch_coalesce_count(const long* sorted, int* counts, long n,
                           hipStream_t stream);
void launch_coalesce_scatter(const long* sorted, const long* perm,
                             const long* incl, long* uniq, long* inverse,
                             long* seg, long* count, long n,
                             hipStream_t stream);
void launch_segment_sum_rows(const void* rows, bool r_bf16, const long* perm,
                             const long* seg, float* scratch, void* out,
                             bool o_bf16, long n, long num, int D,
                             hipStream_t stream);

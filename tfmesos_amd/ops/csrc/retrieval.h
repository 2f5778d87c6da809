// Host-side interface of retrieval.hip (shared with the binding TU); the
// definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kDotTopkMaxD = 256;   // row width one wave's A fragments cover
constexpr int kDotTopkMaxK = 64;    // one key a lane in the sorted half

// splits of the item tiles the launcher chooses: a function of (B, V) only
int dot_topk_nsplit(long B, long V);
// the splits a call runs with: splits == 0 is dot_topk_nsplit(B, V), anything
// else is clamped to [1, ceil(V/64)] and reduced so that no split is empty
int dot_topk_splits(long B, long V, long splits);

void launch_dot_topk(const void* q, const void* w, const float* bias,
                     long* ws, float* values, long* indices, int B, int V,
                     int D, int k, int nsplit, hipStream_t stream);

void launch_dot_rank(const void* q, const void* w, const float* bias,
                     const long* labels, long* true_key, long* ws, long* rank,
                     int B, int V, int D, int nsplit, hipStream_t stream);

// Host-side interface of norm.hip (shared with the binding TU); the
// definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

constexpr int kNormMaxD = 1024;        // two 16-byte chunks a lane, 64 lanes
constexpr int kNormMaxBlocks = 1024;   // backward blocks: four a CU

// How a call of n rows of width D is laid out: the lanes that share a row
// (8, 16, 32 or 64), the rows a 256-thread block holds (256 / lanes), and the
// blocks of the backward launch, each walking row groups b, b + blocks, ...
// blocks == 0 asks for the default rule, one block a row group up to
// kNormMaxBlocks; anything else is clamped to [1, min(groups, kNormMaxBlocks)].
// A function of (n, D, blocks) alone.
struct NormPlan { int lanes, rows, blocks; };
NormPlan norm_plan(long n, int D, long blocks);

// Parameters ([D], fp32 or bf16 by their *_bf16 flag) may be null; so may
// res / s_out (no residual), ds, part (no parameter gradients wanted).
struct NormFwdArgs {
  const void* x; const void* res;      // [n, D] bf16
  const void* w; const void* b;
  void* s_out; void* y;                // [n, D] bf16
  float* mean; float* rstd;            // [n]
  long n; int D;
  float eps;
  int w_bf16, b_bf16, rms;
};
void launch_norm_fwd(const NormFwdArgs& a, hipStream_t stream);

struct NormBwdArgs {
  const void* dy; const void* s; const void* ds;   // [n, D] bf16
  const float* mean; const float* rstd;            // [n]
  const void* w;
  void* dx;                            // [n, D] bf16
  float* part;                         // [blocks, 2, D] fp32 workspace
  void* dw; void* db;                  // [D], either may be null
  long n; int D;
  int w_bf16, dw_bf16, db_bf16, rms;
  int blocks;                          // norm_plan(n, D, ...).blocks
};
void launch_norm_bwd(const NormBwdArgs& a, hipStream_t stream);

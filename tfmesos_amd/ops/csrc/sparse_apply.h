// Host-side interface of sparse_apply.hip (shared with the binding TU).
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

enum SparseOpt {
  SPARSE_SGD = 0,
  SPARSE_SGD_MOM = 1,   // state1 = momentum buffer, beta1 = momentum
  SPARSE_ADAGRAD = 2,   // state1 = accumulator
  SPARSE_ADAM = 3,      // state1 = exp_avg, state2 = exp_avg_sq
  SPARSE_FTRL = 4,      // state1 = accumulator, state2 = linear (ftrl.h)
};

struct SparseHp {
  float lr, gscale, wd;
  float beta1, beta2, eps;
  float omb1, omb2;     // 1-beta1, 1-beta2, rounded once from double
  float bc1, bc2;       // Adam bias corrections (from step)
  float l1, l2, acc0;   // FTRL-Proximal (acc0: initial_accumulator_value)
};

// scratch: fp32 [run_scratch_rows(n), D] (run_sum.h), null when 0 rows.
void launch_sparse_apply(int opt, float* table, const long* sorted,
                         const long* perm, const void* grads, bool g_bf16,
                         float* scratch, float* s1, float* s2, bf16_t* shadow,
                         long n, int D, long V, const SparseHp& hp,
                         hipStream_t stream);

// Pooled (bag) push: grads is [B,D], one row per CSR bag; position i of
// the push contributes coef[i] * grads[bag_of[i]]. launch_bag_expand fills
// bag_of / coef (int / fp32 [n], zeroed by the caller) from the offsets.
void launch_bag_expand(const long* offsets, const float* weights, int* bag_of,
                       float* coef, long B, long n, bool mean,
                       hipStream_t stream);
void launch_sparse_apply_bag(int opt, float* table, const long* sorted,
                             const long* perm, const void* grads, bool g_bf16,
                             const int* bag_of, const float* coef,
                             float* scratch, float* s1, float* s2,
                             bf16_t* shadow, long n, int D, long V,
                             const SparseHp& hp, hipStream_t stream);

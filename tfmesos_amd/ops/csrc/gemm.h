// Host-side interface of gemm.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_gemm(const bf16_t* A, const bf16_t* B, const void* bias,
                 bool bias_bf16, void* C, bool out_f32, const bf16_t* aux,
                 void* colsum_out, float* ws, int* cnt, int kc, int nslice,
                 int M, int N, int K, int lda, int ldb, int ldc, bool ta,
                 bool tb, int act, int veca, int vecb, hipStream_t stream,
                 const SnapArgs* snap = nullptr, bool* snap_taken = nullptr);
void launch_gemm_fwd1(const bf16_t* A, const bf16_t* B, const void* bias,
                      bool bias_bf16, void* C, bool out_f32, int relu,
                      int kc, int nslice, int M, int N, int K, int lda,
                      int ldb, int ldc, int veca, int vecb, int variant,
                      const SnapArgs* snap, bool* snap_taken,
                      hipStream_t stream);
void launch_gemm_small(const bf16_t* A, const bf16_t* B, const void* bias,
                       bool bias_bf16, void* C, bool out_f32, int relu,
                       void* colsum_out, bool cs_f32, int M, int N, int K,
                       int lda, int ldb, int ldc, bool ta, int veca,
                       int vecb, const SmallSgdArgs* sga,
                       hipStream_t stream);
// launch_gemm's two split-K epilogue decisions, for the plan bindings:
// whether the last-arriver epilogue (TFA_GEMM_LA=1) replaces the stripe
// reduce launch, and whether that launch is the 1-element-per-thread one
bool gemm_last_arriver(int M, int N, bool colsum, int act);
bool gemm_reduce_small(long mn);
void launch_mlp_head_tail(const bf16_t* x, const HeadTailArgs* hta,
                          void* dw1, void* db1, bool grads_f32, int M,
                          int H, int B, const SmallSgdArgs* sga,
                          hipStream_t stream);
void launch_gemm_stripes_any(const bf16_t* A, const bf16_t* B, float* ws,
                             int kc, int nslice, int M, int N, int K,
                             int lda, int ldb, int ldc, bool ta, bool tb,
                             int veca, int vecb, hipStream_t stream);
void launch_splitk_reduce_sgd(const float* ws, int nslice, float* p,
                              bf16_t* shadow, long mn, float lr,
                              float gscale, float nd, hipStream_t stream);
void launch_gemm_stripes(const bf16_t* A, const bf16_t* B, float* ws,
                         int kc, int nslice, int M, int N, int K, int lda,
                         int ldb, int ldc, int veca, int vecb,
                         hipStream_t stream);

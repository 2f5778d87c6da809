// Host-side interface of conv.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

int conv_fwd_slices(int N, int K, int Ho, int Wo, int C, int R, int S);
int conv_bwdd_slices(int N, int H, int W, int C, int K, int R, int S);
void launch_conv_fwd(const bf16_t* X, const bf16_t* W, const float* bias,
                     bf16_t* Y, float* ws, int N, int C, int H, int Wd,
                     int K, int R, int S, int Ho, int Wo, int U, int V,
                     int P, int Q, bool relu, hipStream_t stream);
void launch_conv_bwd_data(const bf16_t* dY, long ldy, const bf16_t* Wt,
                          bf16_t* dX,
                          float* ws, int N, int C, int H, int Wd, int K,
                          int R, int S, int Ho, int Wo, int U, int V, int P,
                          int Q, hipStream_t stream);
int conv_bwdw_slices(int N, int C, int K, int R, int S, int Ho, int Wo);
void launch_conv_bwd_weight(const bf16_t* dY, long ldy, const bf16_t* X,
                            float* dW,
                            int N, int C, int H, int Wd, int K,
                            int R, int S, int Ho, int Wo, int U, int V,
                            int P, int Q, hipStream_t stream);

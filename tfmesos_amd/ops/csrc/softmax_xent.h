// Host-side interface of softmax_xent.hip (shared with the binding TU);
// the definitions there carry the argument contracts.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

void launch_softmax_xent_fused(const bf16_t* logits, const long* labels,
                               bf16_t* dlogits, float* loss, float scale,
                               int B, int C, hipStream_t stream);
void launch_softmax_xent_fwd(const bf16_t* logits, const long* labels,
                             bf16_t* probs, float* loss, int B, int C,
                             hipStream_t stream);
void launch_softmax_xent_bwd(const bf16_t* probs, const long* labels,
                             bf16_t* dlogits, float scale, int B, int C,
                             hipStream_t stream);
void launch_mlp_head_fused(const bf16_t* h, const bf16_t* w,
                           const bf16_t* bias, const long* labels,
                           bf16_t* dlogits, bf16_t* dh, float* loss,
                           void* dw2, void* db2, bool grads_f32,
                           float scale, int B, int H, int C,
                           hipStream_t stream);
void launch_mlp_fwd_head(const float* ws, int nslice, const bf16_t* b1,
                         const bf16_t* w, const bf16_t* bias,
                         const long* labels, bf16_t* dlogits, bf16_t* dh,
                         float* loss, void* dw2, void* db2, bool grads_f32,
                         float scale, int B, int H, int C,
                         hipStream_t stream);
void set_head_debug(void* ptr);

// Common device helpers for tfmesos_amd CDNA4 (gfx950) kernels.
// Target: MI355X only — wave64, MFMA, 160 KiB LDS/CU. No CUDA compat.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define DEVINL __device__ __forceinline__

typedef __hip_bfloat16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

DEVINL float bf2f(bf16_t v) { return __bfloat162float(v); }
DEVINL bf16_t f2bf(float v) { return __float2bfloat16(v); }

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// host-side descriptor for gemm_small's fused SGD tail (gemm.hip) —
// opaque pointers so the binding TU needs no device vector types
struct SmallSgdArgs {
  float* pmw; void* psw;      // W master fp32 / bf16 shadow [M,N]
  float* pmb; void* psb;      // bias master / shadow [N]
  const void* g2w;            // classifier W grad (bf16, from the head)
  float* pm2w; void* ps2w;
  const void* g2b;
  float* pm2b; void* ps2b;
  float lr;
  int n2w, n2b;
};

// optional side job of the one-launch forward GEMM and of the small
// split-K stripe reduce (gemm.hip): copy
// two small bf16 ranges into dst[0..n0) and dst[off1..off1+n1) — the
// mnist step snapshots the classifier shadow there, one launch ahead
// of the fused head+tail kernel that reads it
// rows > 0: s0 is a [rows, cols] classifier (rows <= 128, cols <= 16)
// and the job also lays out, zero-padded and whole on every call, the
// two operand images the fused kernel's waves would otherwise each build
// from it: the k-major [16][136] logits operand at dst[kSnapKmajOff..)
// and the [128][16] row image at dst[kSnapRowOff..).
struct SnapArgs {
  const void* s0; const void* s1;
  void* dst;
  int n0, n1, off1;
  int rows, cols;
};

// the mnist snapshot buffer, in bf16 elements
constexpr int kSnapB2Off = 2048;
constexpr int kSnapKmajOff = kSnapB2Off + 64;
constexpr int kSnapRowOff = kSnapKmajOff + 16 * 136;
constexpr int kSnapElems = kSnapRowOff + 128 * 16;

// host-side descriptor for the fused head+tail kernel (gemm.hip)
struct HeadTailArgs {
  const void* h;              // [B,H] bf16 relu output
  const void* w2;             // [H,C] bf16 (sgd mode: the live shadow)
  const void* b2;             // [C] bf16
  const long* labels;         // [B]
  float* loss;
  void* dw2; void* db2;       // grads mode outputs (grad dtype)
  unsigned* ticket;           // sgd mode: zeroed 16B-aligned device word,
                              // or null when w2/b2 are a snapshot
  float scale;
  int C;
};

#define HIP_CHECK(expr)                                                     \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      TORCH_CHECK(false, "HIP error: ", hipGetErrorString(_e), " at ",      \
                  __FILE__, ":", __LINE__);                                 \
    }                                                                       \
  } while (0)

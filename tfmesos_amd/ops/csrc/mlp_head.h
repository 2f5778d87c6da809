// Shared device phases of the mnist classifier head: the logits tile,
// the rowwise softmax/dlogits and the dh tile. Included by the
// single-launch head (softmax_xent.hip, mlp_head_mfma_kernel) and by
// the fused head+tail kernel (gemm.hip, mlp_head_tail_kernel), which
// recomputes them per wave — ONE definition, so the two paths cannot
// drift apart in arithmetic order (results are compared bit for bit).
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16v;

constexpr int HB = 128;        // padded B/H tile
constexpr int HP = 136;        // hs row stride (8-elem pad, 16B aligned)
constexpr int CP = 16;         // padded class dim
// fp32 logits staging: stride 17 (a 16-dword stride put every lane
// of a softmax row-read on 2 of 32 banks — 32-way conflicts)
constexpr int LSP = CP + 1;

// row (within the 32-row tile) of accumulator slot v in a 32x32 MFMA
// D fragment; the column is lane & 31
DEVINL int head_frag_row(int v, int lane) {
  return ((v >> 2) << 3) + ((lane >> 5) << 2) + (v & 3);
}

// logits tile [32 rows, 32 padded classes] = hs rows @ w, K = HB in
// eight MFMA steps. arow: this lane's hs row (lane & 31 of the tile);
// brow: this lane's w^T row (class lane & 31), or null for a class
// beyond the padded image — an all-zero B fragment.
DEVINL f32x16v head_logits_tile(const __bf16* arow, const __bf16* brow,
                                int lane) {
  f32x16v acc = {};
#pragma unroll
  for (int kh = 0; kh < HB / 16; ++kh) {
    const int k0 = kh * 16 + ((lane >> 5) << 3);
    bf16x8 a = *(const bf16x8*)&arow[k0];
    bf16x8 bv = {};
    if (brow != nullptr) bv = *(const bf16x8*)&brow[k0];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc, 0, 0, 0);
  }
  return acc;
}

// add the class bias and park the tile in the fp32 staging (rows
// row0.. of ls); bc is this lane's bias (0 beyond C)
DEVINL void head_store_logits(float* ls, const f32x16v& acc, int row0,
                              float bc, int lane) {
  const int col = lane & 31;
  if (col < CP) {
#pragma unroll
    for (int v = 0; v < 16; ++v)
      ls[(row0 + head_frag_row(v, lane)) * LSP + col] = acc[v] + bc;
  }
}

// rowwise softmax + dlogits over C <= 16 classes (scalar, one lane per
// row): emit(c, d) receives d = (p - onehot) * scale per class;
// returns -log p[label] (0 for a label outside [0, C)). lr is a row of
// the fp32 staging: all CP columns of it are written (zero logits
// beyond C), so the row is read whole, up front — one LDS wait, not one
// per class — and the loops are unrolled to CP behind c < C. The log is
// taken once, of the selected p[label], after the class loop: the same
// bits as a log inside it, at one transcendental per row instead of CP.
template <class F>
DEVINL float head_softmax_row(const float* lr, int C, int label,
                              float scale, F emit) {
  float l[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) l[c] = lr[c];
  float mx = -3.4e38f;
#pragma unroll
  for (int c = 0; c < CP; ++c)
    if (c < C) mx = fmaxf(mx, l[c]);
  float sum = 0.f;
  float e[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    e[c] = 0.f;
    if (c < C) {
      e[c] = __expf(l[c] - mx);
      sum += e[c];
    }
  }
  const float inv = 1.f / sum;
  float pl = 1.f;
  bool hit = false;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    if (c < C) {
      const float p = e[c] * inv;
      const float d = (p - (c == label ? 1.f : 0.f)) * scale;
      emit(c, d);
      if (c == label) {
        pl = p;
        hit = true;
      }
    }
  }
  return hit ? -__logf(fmaxf(pl, 1e-30f)) : 0.f;
}

// The two phases above without runtime generality, for the fused
// head+tail kernel alone (mlp_head_mfma_kernel keeps the forms above:
// it is the route the exact tests compare against). Same operations on
// the same values in the same order — the pad classes C..CP-1 take part
// as exact zeros instead of being predicated away.

// head_logits_tile with a B fragment for EVERY lane: brow is the lane's
// w^T row, or an all-zero row for the classes beyond the padded image.
// All 16 fragment reads are issued ahead of the first MFMA (the guarded
// form was eight LDS round trips in a row).
DEVINL f32x16v head_logits_tile_all(const __bf16* arow, const __bf16* brow,
                                    int lane) {
  bf16x8 a[HB / 16], bv[HB / 16];
#pragma unroll
  for (int kh = 0; kh < HB / 16; ++kh) {
    const int k0 = kh * 16 + ((lane >> 5) << 3);
    a[kh] = *(const bf16x8*)&arow[k0];
    bv[kh] = *(const bf16x8*)&brow[k0];
  }
  f32x16v acc = {};
#pragma unroll
  for (int kh = 0; kh < HB / 16; ++kh)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kh], bv[kh], acc, 0, 0, 0);
  return acc;
}

// The bias a pad class is staged with: its logit is 0 + bias (the
// classifier columns are zero there), cannot win the max and has
// exp(l - max) == +0 exactly, so sum, p and d come out as if the class
// had been skipped: sum + 0 is exact and p = d = +0 is what the zero
// fill stored.
DEVINL float head_pad_bias() { return -__builtin_inff(); }

// head_softmax_row over all CP slots of a row staged with
// head_pad_bias: no class predicate. d of the whole row goes out as two
// b128 stores to drow (the row's CP dlogits), then the label's element
// is patched by one b16 store behind them (same wave, in-order DS
// pipe). e[label] is recomputed from one more read of l[label] — the
// same exp of the same difference, the same bits. The parent's
// (p - onehot) * scale compiles to fma(e, inv, -onehot) then a multiply
// and p[label] to a plain multiply; both are spelled out here so that
// contraction cannot decide otherwise. With onehot == 0 the fma is the
// rounded product itself.
DEVINL float head_softmax_row_all(const float* lr, __bf16* drow, int C,
                                  int label, float scale) {
  float l[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) l[c] = lr[c];
  const bool hit = (unsigned)label < (unsigned)C;
  const int lab = hit ? label : 0;
  const float ll = lr[lab];
  float mx = -3.4e38f;
#pragma unroll
  for (int c = 0; c < CP; ++c) mx = fmaxf(mx, l[c]);
  float sum = 0.f;
  float e[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    e[c] = __expf(l[c] - mx);
    sum += e[c];
  }
  const float inv = 1.f / sum;
  bf16x8 lo, hi;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    lo[c] = (__bf16)((e[c] * inv) * scale);
    hi[c] = (__bf16)((e[8 + c] * inv) * scale);
  }
  *(bf16x8*)&drow[0] = lo;
  *(bf16x8*)&drow[8] = hi;
  const float el = __expf(ll - mx);
  if (hit) drow[lab] = (__bf16)(__builtin_fmaf(el, inv, -1.f) * scale);
  const float pl = el * inv;
  return hit ? -__logf(fmaxf(pl, 1e-30f)) : 0.f;
}

// dh tile [32 rows, 32 hidden cols] = dls rows @ w^T, K = CP (one
// MFMA). drow: this lane's dls row; wrow: this lane's wpad row (hidden
// column lane & 31 of the tile). Unmasked — the caller applies h > 0.
DEVINL f32x16v head_dh_tile(const __bf16* drow, const __bf16* wrow,
                            int lane) {
  bf16x8 a = *(const bf16x8*)&drow[(lane >> 5) << 3];
  bf16x8 bv = *(const bf16x8*)&wrow[(lane >> 5) << 3];
  f32x16v acc = {};
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc, 0, 0, 0);
}

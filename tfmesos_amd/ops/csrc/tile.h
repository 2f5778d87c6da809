// One wave's 256-column tile of a row, as fp32 registers: the load / store
// pair shared by embedding_bag.hip and coalesce.hip.
//   * VEC == 4 (D % 4 == 0, 16-byte aligned bases): lane l owns columns
//     4l..4l+3 of the tile (bf16x4 / f32x4 accesses);
//   * VEC == 1: lane l owns columns l, l+64, l+128, l+192 (a vector access
//     on an odd-D row would be misaligned).
// Columns at or beyond D load as 0 and are not stored.
#pragma once

#include "common.h"

constexpr int TILE = 256;   // columns per wave
constexpr int ACC = 4;      // accumulators per lane = TILE / WAVE

// The lane's ACC elements of one row's tile, as fp32.
template <typename T, int VEC>
DEVINL void ld_tile(const T* __restrict__ row, int c0, int lane, int D,
                    float (&v)[ACC]) {
  if constexpr (VEC == 4) {
    const int col = c0 + lane * 4;
    if (col < D) {
      if constexpr (sizeof(T) == 2) {
        const bf16x4 t = *(const bf16x4*)(const __bf16*)(row + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
      } else {
        const f32x4 t = *(const f32x4*)(row + col);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = t[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < ACC; ++e) {
      const int col = c0 + e * WAVE + lane;
      float x = 0.f;
      if (col < D) {
        if constexpr (sizeof(T) == 2) x = bf2f(*(const bf16_t*)(row + col));
        else x = *(const float*)(row + col);
      }
      v[e] = x;
    }
  }
}

template <typename O, int VEC>
DEVINL void st_tile(O* __restrict__ row, int c0, int lane, int D,
                    const float (&v)[ACC]) {
  if constexpr (VEC == 4) {
    const int col = c0 + lane * 4;
    if (col >= D) return;
    if constexpr (sizeof(O) == 2) {
      bf16x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = (__bf16)v[e];
      *(bf16x4*)(__bf16*)(row + col) = t;
    } else {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = v[e];
      *(f32x4*)(row + col) = t;
    }
  } else {
#pragma unroll
    for (int e = 0; e < ACC; ++e) {
      const int col = c0 + e * WAVE + lane;
      if (col < D) {
        if constexpr (sizeof(O) == 2) *(bf16_t*)(row + col) = f2bf(v[e]);
        else *(float*)(row + col) = v[e];
      }
    }
  }
}

// A wave's slice of a row as fp32 registers: the loads and stores shared by
// every kernel that walks embedding rows (embedding_bag, sparse_apply,
// partition, coalesce, hash).
//
// ld_vec / st_vec: a lane's VEC consecutive elements at a pointer, unchecked
// (bf16x4 / f32x4 when VEC == 4, one element when VEC == 1).
//
// ld_tile / st_tile / ld_row: one wave's 256-column tile of a row, ACC = 4
// elements per lane, checked against the row width D:
//   * VEC == 4 (D % 4 == 0, 16-byte aligned bases): lane l owns columns
//     4l..4l+3 of the tile;
//   * VEC == 1: lane l owns columns l, l+64, l+128, l+192 (a vector access
//     on an odd-D row would be misaligned).
// Columns at or beyond D load as 0 and are not stored.
#pragma once

#include <cstdint>

#include "common.h"

constexpr int TILE = 256;   // columns per wave
constexpr int ACC = 4;      // accumulators per lane = TILE / WAVE

// Host side: may rows of width D at these bases take the VEC == 4 path? It
// needs 16-byte aligned rows: D % 4 == 0 and 16-byte aligned bases (a view
// at a storage offset can break the latter). Null (unused) bases pass.
template <typename... P>
inline bool tile_vec4(int D, const P*... bases) {
  return D % 4 == 0 && (((uintptr_t)bases | ... | (uintptr_t)0) % 16) == 0;
}

template <typename T>
DEVINL float ld_elem(const T* __restrict__ p) {
  if constexpr (sizeof(T) == 2) return bf2f(*(const bf16_t*)p);
  else return *(const float*)p;
}

template <typename O>
DEVINL void st_elem(O* __restrict__ p, float x) {
  if constexpr (sizeof(O) == 2) *(bf16_t*)p = f2bf(x);
  else *(float*)p = x;
}

// The VEC elements at p (16-byte aligned when VEC == 4), as fp32.
template <typename T, int VEC>
DEVINL void ld_vec(const T* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if constexpr (sizeof(T) == 2) {
      const bf16x4 t = *(const bf16x4*)(const __bf16*)p;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (float)t[e];
    } else {
      const f32x4 t = *(const f32x4*)p;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = t[e];
    }
  } else {
    v[0] = ld_elem(p);
  }
}

template <typename O, int VEC>
DEVINL void st_vec(O* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if constexpr (sizeof(O) == 2) {
      bf16x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = (__bf16)v[e];
      *(bf16x4*)(__bf16*)p = t;
    } else {
      f32x4 t;
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = v[e];
      *(f32x4*)p = t;
    }
  } else {
    st_elem(p, v[0]);
  }
}

// The lane's ACC elements of one row's tile, as fp32.
template <typename T, int VEC>
DEVINL void ld_tile(const T* __restrict__ row, int c0, int lane, int D,
                    float (&v)[ACC]) {
  if constexpr (VEC == 4) {
    const int col = c0 + lane * 4;
    if (col < D) {
      ld_vec<T, 4>(row + col, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < ACC; ++e) {
      const int col = c0 + e * WAVE + lane;
      v[e] = col < D ? ld_elem(row + col) : 0.f;
    }
  }
}

// Row r's tile, or zeros for a row r < 0 (r is wave-uniform).
template <typename T, int VEC>
DEVINL void ld_row(const T* __restrict__ rows, long r, int c0, int lane,
                   int D, float (&v)[ACC]) {
  if (r >= 0) {
    ld_tile<T, VEC>(rows + r * D, c0, lane, D, v);
  } else {
#pragma unroll
    for (int e = 0; e < ACC; ++e) v[e] = 0.f;
  }
}

template <typename O, int VEC>
DEVINL void st_tile(O* __restrict__ row, int c0, int lane, int D,
                    const float (&v)[ACC]) {
  if constexpr (VEC == 4) {
    const int col = c0 + lane * 4;
    if (col < D) st_vec<O, 4>(row + col, v);
  } else {
#pragma unroll
    for (int e = 0; e < ACC; ++e) {
      const int col = c0 + e * WAVE + lane;
      if (col < D) st_elem(row + col, v[e]);
    }
  }
}

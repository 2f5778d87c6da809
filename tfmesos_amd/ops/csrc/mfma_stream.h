// Device helpers shared by the kernels that own 64 rows as MFMA A fragments
// and stream another row set through row-major LDS tiles
// (sampled_softmax.hip, bag_attention.hip, retrieval.hip): guarded 16-byte
// row pieces with a row stride, transpose reads of an LDS image, the
// wave-level LDS fence.
// Included after common.h, inside the including file's anonymous namespace
// and its no-packed-fp32-ops attribute region, so that the helpers carry the
// target features of the kernels they are inlined into.
#pragma once

// rows[row * rs + k .. +8), zero outside [0,nrows) x [0,D); rs = row stride
template <bool VEC>
DEVINL bf16x8 ld_piece(const __bf16* __restrict__ rows, int row, int nrows,
                       int k, int D, long rs) {
  bf16x8 z = {};
  if (VEC) {     // D % 8 == 0: a piece that starts inside the row ends inside
    const bool ok = row < nrows && k < D;
    const bf16x8 g = *(const bf16x8*)(rows + (ok ? (long)row * rs + k : 0));
    return ok ? g : z;
  }
  if (row < nrows) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) z[e] = rows[(long)row * rs + k + e];
  }
  return z;
}

template <bool VEC>
DEVINL void st_piece(__bf16* __restrict__ rows, int row, int k, int D, long rs,
                     bf16x8 v) {
  __bf16* dst = rows + (long)row * rs + k;
  if (VEC) {
    *(bf16x8*)dst = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) dst[e] = v[e];
  }
}

DEVINL bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

// MFMA B fragment out of a [row][d] image of stride XL: rows kfrag..kfrag+7
// at column cb + (lane & 15), two transpose-reads of four image rows each
// (lane mapping: gemm.hip, interaction.hip)
template <int XL>
DEVINL bf16x8 tr_frag(const __bf16* X, int kfrag, int cb, int lane) {
  const int a = (kfrag + ((lane & 15) >> 2)) * XL + cb + 4 * (lane & 3);
  const bf16x4 f0 = tr_read(&X[a]);
  const bf16x4 f1 = tr_read(&X[a + 4 * XL]);
  return __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// orders a wave's own LDS writes before its own LDS reads of other lanes'
// data (the P image, the epilogue's parked tile)
DEVINL void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the 16 lanes that share an accumulator row, fixed order
DEVINL float row_sum16(float v) {
#pragma unroll
  for (int x = 1; x < 16; x <<= 1) v += __shfl_xor(v, x);
  return v;
}

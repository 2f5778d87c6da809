// Pairwise feature interaction (DLRM's "dot" interaction, the Gram matrix
// under a factorization machine's second-order term), forward and backward.
//
//   x [B,F,D] bf16, Z[b] = x[b] x[b]^T in fp32, out[b] = (x[b,0,:] if keep)
//   followed by the lower triangle of Z[b] in row-major packed order
//   (p = i(i-1)/2 + j for j < i, or i(i+1)/2 + j for j <= i with diag);
//   dx[b] = (L + L^T) x[b] (+ dout[b,:D] on row 0 if keep), L unpacked from
//   dout[b]. F <= 64 (kDotMaxF), any D >= 1, any base alignment.
//
// Forward: one wave per example, WAVES waves per block, the grid strides
//   over B. Z is a Gram matrix, and the MFMA A fragment of x[b] and the B
//   fragment of x[b]^T are the SAME registers (lane l: 8 consecutive k of
//   row / column l % 32 or l % 16) — each lane loads 16 bytes of its
//   feature row per K step straight from global memory and issues
//   mfma(a, a, acc). No LDS and no transpose on the operand side.
//     F <= 16: 16x16x32; F <= 32: one 32x32x16 tile; F <= 64: the three
//     lower 32x32 tiles (the upper-right one is never computed).
//   Rows >= F and the K tail are zero-filled in registers. The wanted
//   triangle leaves the scattered accumulator layout through a wave-private
//   fp32 LDS image in packed order; the output row (kept row + triangle) is
//   then written front to back: scalar stores up to the first 16-byte
//   boundary of the row (rows are D + P wide, so row starts are aligned to
//   the element only), 16-byte stores from there, scalar stores for the rest.
//
// Backward: one wave per example. S = L + L^T is scattered into a bf16 LDS
//   image (pad rows/cols zeroed once — F is the same for every example), x[b]
//   is staged 64 columns at a time as [feature][d], and dx tile = S . x runs
//   on 16x16x32 MFMAs whose B fragments (8 features at one column d) come
//   back through ds_read_b64_tr_b16 (lane mapping: gemm.hip, conv.hip).
//   dout[b,:D] is added to row 0 in fp32, the tile is rounded once, parked
//   in the x image and leaves as 16-byte row-contiguous stores.
//   An fp32 dout is rounded to bf16 when S is built (the MFMA operand type).
//
// D % 8 == 0 with 16-byte-aligned x (and dx) takes b128 global accesses;
// anything else the element-wise guarded form of the same loads and stores.
// No atomics, fixed order => bit-reproducible; nothing is read back.
#include "interaction.h"

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are kept out of this
// file's kernels; everything here is scalar fp32 or MFMA.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int WAVES = 4;        // waves (= examples in flight) per block
constexpr int MAX_BLOCKS = 4096;
constexpr int KU = 4;           // forward K steps loaded ahead of their MFMAs

// packed index of the first pair of row i
DEVINL int tri_base(int i, int diag) {
  return diag ? i * (i + 1) / 2 : i * (i - 1) / 2;
}

// (i, j) of packed index p (p < 2080, exact in fp32; the two fix-ups
// cover a sqrt that lands one off at a row boundary)
DEVINL void tri_unpack(int p, int diag, int& i, int& j) {
  int r = (int)((1.f + sqrtf(8.f * (float)p + 1.f)) * 0.5f);
  if (r * (r - 1) / 2 > p) --r;
  if ((r + 1) * r / 2 <= p) ++r;
  j = p - r * (r - 1) / 2;
  i = diag ? r - 1 : r;
}

// x[row][k..k+8) of one example, zero outside [0,F) x [0,D)
template <bool VEC>
DEVINL bf16x8 ld_frag(const __bf16* __restrict__ xb, int row, int k, int F,
                      int D) {
  bf16x8 z = {};
  if (VEC) {     // D % 8 == 0: a piece that starts inside the row ends inside
    const bool ok = row < F && k < D;
    const bf16x8 g = *(const bf16x8*)(xb + (ok ? (long)row * D + k : 0));
    return ok ? g : z;
  }
  if (row < F) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) z[e] = xb[(long)row * D + k + e];
  }
  return z;
}

// row (within the 32-row tile) of accumulator slot v of a 32x32 MFMA D
// fragment; the column is lane & 31
DEVINL int frag_row32(int v, int lane) {
  return ((v >> 2) << 3) + ((lane >> 5) << 2) + (v & 3);
}

DEVINL void tri_put(float* tri, int i, int j, float v, int F, int diag) {
  if (i < F && (j < i || (diag && j == i))) tri[tri_base(i, diag) + j] = v;
}

DEVINL void tri_put32(float* tri, const f32x16& acc, int i0, int j0, int lane,
                      int F, int diag) {
#pragma unroll
  for (int v = 0; v < 16; ++v)
    tri_put(tri, i0 + frag_row32(v, lane), j0 + (lane & 31), acc[v], F, diag);
}

template <typename O> struct OutVec;
template <> struct OutVec<__bf16> { typedef bf16x8 type; };
template <> struct OutVec<float> { typedef f32x4 type; };

// MODE 0: F <= 16, 1: F <= 32, 2: F <= 64
template <int MODE, bool VEC, typename O>
__global__ __launch_bounds__(WAVES * WAVE) void dot_interaction_fwd_kernel(
    const __bf16* __restrict__ x, O* __restrict__ out, long B, int F, int D,
    int diag, int keep) {
  constexpr int PMAX = MODE == 0 ? 136 : MODE == 1 ? 528 : 2080;
  constexpr int VN = 16 / (int)sizeof(O);
  typedef typename OutVec<O>::type ovec;
  __shared__ float tri_s[WAVES][PMAX];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x >> 6;
  float* tri = tri_s[wave];
  const int P = tri_base(F, diag);
  const int D0 = keep ? D : 0;
  const int Wd = D0 + P;

  for (long b0 = (long)blockIdx.x * WAVES; b0 < B;
       b0 += (long)gridDim.x * WAVES) {
    const long b = b0 + wave;
    const bool live = b < B;      // wave-uniform
    const __bf16* xb = x + (live ? b : 0) * F * D;
    if (live) {
      if (MODE == 0) {
        const int row = lane & 15, ko = (lane >> 4) << 3;
        f32x4 acc = {};
        for (int k0 = 0; k0 < D; k0 += KU * 32) {
          bf16x8 a[KU];
#pragma unroll
          for (int u = 0; u < KU; ++u)
            a[u] = ld_frag<VEC>(xb, row, k0 + u * 32 + ko, F, D);
#pragma unroll
          for (int u = 0; u < KU; ++u)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u], a[u], acc, 0,
                                                          0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          tri_put(tri, (lane >> 4) * 4 + r, lane & 15, acc[r], F, diag);
      } else if (MODE == 1) {
        const int row = lane & 31, ko = (lane >> 5) << 3;
        f32x16 acc = {};
        for (int k0 = 0; k0 < D; k0 += KU * 16) {
          bf16x8 a[KU];
#pragma unroll
          for (int u = 0; u < KU; ++u)
            a[u] = ld_frag<VEC>(xb, row, k0 + u * 16 + ko, F, D);
#pragma unroll
          for (int u = 0; u < KU; ++u)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], a[u], acc, 0,
                                                          0, 0);
        }
        tri_put32(tri, acc, 0, 0, lane, F, diag);
      } else {
        const int row = lane & 31, ko = (lane >> 5) << 3;
        f32x16 acc00 = {}, acc10 = {}, acc11 = {};
        for (int k0 = 0; k0 < D; k0 += KU * 16) {
          bf16x8 a0[KU], a1[KU];
#pragma unroll
          for (int u = 0; u < KU; ++u) {
            a0[u] = ld_frag<VEC>(xb, row, k0 + u * 16 + ko, F, D);
            a1[u] = ld_frag<VEC>(xb, 32 + row, k0 + u * 16 + ko, F, D);
          }
#pragma unroll
          for (int u = 0; u < KU; ++u) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[u], a0[u],
                                                            acc00, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[u], a0[u],
                                                            acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[u], a1[u],
                                                            acc11, 0, 0, 0);
          }
        }
        tri_put32(tri, acc00, 0, 0, lane, F, diag);
        tri_put32(tri, acc10, 32, 0, lane, F, diag);
        tri_put32(tri, acc11, 32, 32, lane, F, diag);
      }
    }
    __syncthreads();
    if (live) {
      O* orow = out + b * Wd;
      // element e of the output row: the kept feature row, then the triangle
      auto val = [&](int e) -> O {
        return e < D0 ? (O)(float)xb[e] : (O)tri[e - D0];
      };
      int head = (int)(((16 - ((uintptr_t)orow & 15)) & 15) / sizeof(O));
      if (head > Wd) head = Wd;
      const int nvec = (Wd - head) / VN;
      const int tail = head + nvec * VN;
      for (int e = lane; e < head; e += WAVE) orow[e] = val(e);
      for (int v = lane; v < nvec; v += WAVE) {
        const int e0 = head + v * VN;
        ovec o;
#pragma unroll
        for (int u = 0; u < VN; ++u) o[u] = val(e0 + u);
        *(ovec*)(orow + e0) = o;
      }
      for (int e = tail + lane; e < Wd; e += WAVE) orow[e] = val(e);
    }
    __syncthreads();              // tri is rewritten by the next example
  }
}

// ------------------------------------------------------------------ backward

DEVINL bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

constexpr int DC = 64;          // columns of D per pass
constexpr int XL = DC + 8;      // x image row stride (16-byte aligned rows)

// MFMA B fragment out of the [feature][d] image: features kfrag..kfrag+7
// of column cb + (lane & 15), two transpose-reads of four image rows each
DEVINL bf16x8 tr_frag(const __bf16* X, int kfrag, int cb, int lane) {
  const int a = (kfrag + ((lane & 15) >> 2)) * XL + cb + 4 * (lane & 3);
  const bf16x4 f0 = tr_read(&X[a]);
  const bf16x4 f1 = tr_read(&X[a + 4 * XL]);
  return __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// KP: features padded to the MFMA K step (32 or 64); MT: 16-row tiles of
// dx (ceil(F / 16)); NW: waves per block (the KP = 64 images are 18 KiB a
// wave, two of them keep a block under a quarter of the CU's LDS)
template <int KP, int MT, int NW, bool VEC, typename G>
__global__ __launch_bounds__(NW * WAVE) void dot_interaction_bwd_kernel(
    const __bf16* __restrict__ x, const G* __restrict__ dout,
    __bf16* __restrict__ dx, long B, int F, int D, int diag, int keep) {
  constexpr int SL = KP + 8;    // S image row stride
  constexpr int MP = MT * 16;
  constexpr int PIECES = KP * (DC / 8) / WAVE;   // b128 pieces per lane
  __shared__ __align__(16) __bf16 S_s[NW][MP * SL];
  __shared__ __align__(16) __bf16 X_s[NW][KP * XL];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x >> 6;
  __bf16* S = S_s[wave];
  __bf16* X = X_s[wave];
  const int P = tri_base(F, diag);
  const int D0 = keep ? D : 0;
  const int Wd = D0 + P;

  // the pad rows and columns of S (and, without diag, its diagonal) are
  // never written again; every row of X is rewritten by each staging
  {
    const bf16x8 z = {};
    for (int q = lane * 8; q < MP * SL; q += WAVE * 8) *(bf16x8*)&S[q] = z;
  }
  __syncthreads();

  for (long b0 = (long)blockIdx.x * NW; b0 < B; b0 += (long)gridDim.x * NW) {
    const long b = b0 + wave;
    const bool live = b < B;      // wave-uniform
    const __bf16* xb = x + (live ? b : 0) * F * D;
    const G* gb = dout + (live ? b : 0) * Wd;
    __bf16* dxb = dx + (live ? b : 0) * F * D;
    if (live) {
      for (int p = lane; p < P; p += WAVE) {
        const float g = (float)gb[D0 + p];
        int i, j;
        tri_unpack(p, diag, i, j);
        if (i == j) {
          S[i * SL + i] = (__bf16)(2.f * g);
        } else {
          S[i * SL + j] = (__bf16)g;
          S[j * SL + i] = (__bf16)g;
        }
      }
    }
    for (int d0 = 0; d0 < D; d0 += DC) {
      if (live) {
        bf16x8 v[PIECES];
#pragma unroll
        for (int t = 0; t < PIECES; ++t) {
          const int q = lane + WAVE * t;
          v[t] = ld_frag<VEC>(xb, q >> 3, d0 + (q & 7) * 8, F, D);
        }
#pragma unroll
        for (int t = 0; t < PIECES; ++t) {
          const int q = lane + WAVE * t;
          *(bf16x8*)&X[(q >> 3) * XL + (q & 7) * 8] = v[t];
        }
      }
      __syncthreads();
      f32x4 acc[MT][DC / 16] = {};
      if (live) {
#pragma unroll
        for (int ks = 0; ks < KP / 32; ++ks) {
          const int kfrag = ks * 32 + ((lane >> 4) << 3);
          bf16x8 bf[DC / 16];
#pragma unroll
          for (int nt = 0; nt < DC / 16; ++nt)
            bf[nt] = tr_frag(X, kfrag, nt * 16, lane);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const bf16x8 a =
                *(const bf16x8*)&S[(mt * 16 + (lane & 15)) * SL + kfrag];
#pragma unroll
            for (int nt = 0; nt < DC / 16; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a, bf[nt], acc[mt][nt], 0, 0, 0);
          }
        }
        if (keep && lane < 16) {  // row 0 lives in slot 0 of lanes 0..15
#pragma unroll
          for (int nt = 0; nt < DC / 16; ++nt) {
            const int d = d0 + nt * 16 + lane;
            if (d < D) acc[0][nt][0] += (float)gb[d];
          }
        }
      }
      __syncthreads();            // every fragment read of X is done
      if (live) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < DC / 16; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = mt * 16 + (lane >> 4) * 4 + r;
              if (i < F)
                X[i * XL + nt * 16 + (lane & 15)] = (__bf16)acc[mt][nt][r];
            }
      }
      __syncthreads();
      if (live) {
        for (int q = lane; q < F * (DC / 8); q += WAVE) {
          const int row = q >> 3, c = (q & 7) * 8, d = d0 + c;
          if (d >= D) continue;
          const bf16x8 o = *(const bf16x8*)&X[row * XL + c];
          __bf16* dst = dxb + (long)row * D + d;
          if (VEC) {
            *(bf16x8*)dst = o;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (d + e < D) dst[e] = o[e];
          }
        }
      }
      __syncthreads();            // X is restaged by the next pass
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned grid_for(long B, int waves) {
  const long blocks = (B + waves - 1) / waves;
  return (unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
}

template <int MODE, typename O>
void launch_fwd_mode(const __bf16* x, O* out, long B, int F, int D, bool diag,
                     bool keep, hipStream_t stream) {
  const dim3 grid(grid_for(B, WAVES)), block(WAVES * WAVE);
  if ((D & 7) == 0 && aligned16(x))
    hipLaunchKernelGGL((dot_interaction_fwd_kernel<MODE, true, O>), grid,
                       block, 0, stream, x, out, B, F, D, (int)diag,
                       (int)keep);
  else
    hipLaunchKernelGGL((dot_interaction_fwd_kernel<MODE, false, O>), grid,
                       block, 0, stream, x, out, B, F, D, (int)diag,
                       (int)keep);
}

template <typename O>
void launch_fwd_typed(const __bf16* x, O* out, long B, int F, int D,
                      bool diag, bool keep, hipStream_t stream) {
  if (F <= 16) launch_fwd_mode<0>(x, out, B, F, D, diag, keep, stream);
  else if (F <= 32) launch_fwd_mode<1>(x, out, B, F, D, diag, keep, stream);
  else launch_fwd_mode<2>(x, out, B, F, D, diag, keep, stream);
}

template <int KP, int MT, typename G>
void launch_bwd_mode(const __bf16* x, const G* dout, __bf16* dx, long B,
                     int F, int D, bool diag, bool keep, hipStream_t stream) {
  constexpr int NW = KP == 64 ? 2 : 4;
  const dim3 grid(grid_for(B, NW)), block(NW * WAVE);
  if ((D & 7) == 0 && aligned16(x) && aligned16(dx))
    hipLaunchKernelGGL((dot_interaction_bwd_kernel<KP, MT, NW, true, G>),
                       grid, block, 0, stream, x, dout, dx, B, F, D,
                       (int)diag, (int)keep);
  else
    hipLaunchKernelGGL((dot_interaction_bwd_kernel<KP, MT, NW, false, G>),
                       grid, block, 0, stream, x, dout, dx, B, F, D,
                       (int)diag, (int)keep);
}

template <typename G>
void launch_bwd_typed(const __bf16* x, const G* dout, __bf16* dx, long B,
                      int F, int D, bool diag, bool keep,
                      hipStream_t stream) {
  if (F <= 16) launch_bwd_mode<32, 1>(x, dout, dx, B, F, D, diag, keep, stream);
  else if (F <= 32)
    launch_bwd_mode<32, 2>(x, dout, dx, B, F, D, diag, keep, stream);
  else if (F <= 48)
    launch_bwd_mode<64, 3>(x, dout, dx, B, F, D, diag, keep, stream);
  else launch_bwd_mode<64, 4>(x, dout, dx, B, F, D, diag, keep, stream);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// x [B,F,D] bf16 contiguous; out [B, (keep ? D : 0) + P] bf16 or fp32,
// contiguous. B > 0, 1 <= F <= kDotMaxF, D >= 1, P > 0.
void launch_dot_interaction_fwd(const void* x, void* out, bool o_bf16, long B,
                                int F, int D, bool diag, bool keep,
                                hipStream_t stream) {
  if (o_bf16)
    launch_fwd_typed((const __bf16*)x, (__bf16*)out, B, F, D, diag, keep,
                     stream);
  else
    launch_fwd_typed((const __bf16*)x, (float*)out, B, F, D, diag, keep,
                     stream);
}

// dout [B, (keep ? D : 0) + P] bf16 or fp32, contiguous; dx [B,F,D] bf16.
// Same bounds as the forward.
void launch_dot_interaction_bwd(const void* x, const void* dout, bool g_bf16,
                                void* dx, long B, int F, int D, bool diag,
                                bool keep, hipStream_t stream) {
  if (g_bf16)
    launch_bwd_typed((const __bf16*)x, (const __bf16*)dout, (__bf16*)dx, B, F,
                     D, diag, keep, stream);
  else
    launch_bwd_typed((const __bf16*)x, (const float*)dout, (__bf16*)dx, B, F,
                     D, diag, keep, stream);
}

// bf16 MFMA GEMM with fused epilogues (worker compute path).
//
// Replaces the reference workload's tf.matmul/xw_plus_b/relu placed on
// workers (examples/mnist/mnist_replica.py:140-143, matrix_factorization
// .py:30). CDNA4-native: v_mfma_f32_16x16x32_bf16 per-wave tiles, fp32
// accumulate, LDS-staged operand tiles, wave64 fragment layouts
// (A: lane l -> row l&15, k (l>>4)*8+j ; C/D: col l&15, row (l>>4)*4+r).
// All four op(A)/op(B) transpose combos are native (backward GEMMs
// dW = X^T dY and dX = dY W^T run without materialized transposes).
//
// Performance features (driven by profiles/r01_mnist_n1_kernel_stats.txt,
// where the un-split fwd GEMM ran 4 workgroups on a 256-CU chip):
//  * split-K: grid.z slices each store their fp32 partial tile into a
//    per-slice workspace stripe (plain stores, no atomics); a small
//    vectorized reduce kernel then sums the stripes in fixed slice order
//    and applies the bias/activation epilogue. Two launches, but the
//    reduce is coalesced cached f32x4 traffic and the kernel boundary is
//    the acquire fence — DETERMINISTIC and memory-model-clean (an
//    in-kernel last-arriver tail measured 3x slower: its uncached
//    per-element loads serialize).
//  * one-launch split-K for outputs up to 128x128 (gemm_fwd1_kernel):
//    the K slices of a tile are the waves of ONE workgroup and meet in
//    LDS — same sums in the same order as stripes + reduce, without
//    the workspace round trip and the second dispatch.
//  * vectorized LDS staging: b128 loads when the operand's leading dim
//    and base allow, b32 otherwise; both [X,K] and [K,X] storage orders
//    have contiguous global access patterns.
//  * fused epilogues: bias add, ReLU, ReLU-backward masking by a saved
//    activation (dX GEMM), and column-sum of op(B) (bias gradients ride
//    the dW GEMM; blockIdx.y==0 workgroups see every K tile of their
//    column strip in LDS anyway).
//
// Geometry: 64x64 block tile, 4 waves (2x2), 32x32 per wave, BK=32.
#include <cstdlib>

#include "common.h"
#include "gemm.h"
#include "mlp_head.h"

namespace {

constexpr int BM = 64, BN = 64, BK = 32;
// XOR-swizzled [64][32] tile for the 64x64 kernel's xk-staged
// operands (same scheme as conv.hip: stride exactly 32 elems, 8-elem
// chunk index XOR (r>>2)&3 — conflict-free for ds_read_b128's
// non-contiguous 16-lane groups AND the b128 staging writes; verified
// zero SQ_LDS_BANK_CONFLICT on the conv twins). gemm_small reuses
// the same helper for its wave-private 32x32 images.
constexpr int SWZ_ELEMS = BM * BK;

DEVINL __bf16* sptr(__bf16* S, int r, int c) {
  return S + r * BK + ((((c >> 3) ^ ((r >> 2) & 3)) << 3) | (c & 7));
}
DEVINL const __bf16* sptr(const __bf16* S, int r, int c) {
  return S + r * BK + ((((c >> 3) ^ ((r >> 2) & 3)) << 3) | (c & 7));
}

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// Stage a [X,K]-stored operand tile (row x contiguous in k) into S[x][k].
// Used for A when !TA and B when TB. 256 threads x 8 elems = 64x32 tile.
DEVINL void stage_xk(const __bf16* __restrict__ P, __bf16* S,
                     int x0, int k0, int X, int K, int ld, int t, int vec) {
  const int x = t >> 2;
  const int kk0 = (t & 3) * 8;
  const int gx = x0 + x;
  const int gk = k0 + kk0;
  const __bf16* src = P + (long)gx * ld + gk;
  if (gx < X && gk + 8 <= K) {
    if (vec == 8) {
      *(bf16x8*)sptr(S, x, kk0) = *(const bf16x8*)src;
    } else if (vec == 2) {
#pragma unroll
      for (int j = 0; j < 8; j += 2)
        *(bf16x2*)sptr(S, x, kk0 + j) = *(const bf16x2*)(src + j);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) *sptr(S, x, kk0 + j) = src[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      *sptr(S, x, kk0 + j) = (gx < X && gk + j < K) ? src[j] : (__bf16)0.f;
  }
}

// Stage a [K,X]-stored operand tile (row k contiguous in x) into the
// reduction-major transpose-read image S[k][x ^ 16*((k>>3)&1)].
// Used for A when TA and B when !TB. The earlier k-major form paid 8
// sub-dword LDS scatter writes per thread to transpose here; this one
// is a single b128 store, and the MFMA fragments come back via
// ds_read_b64_tr_b16 (semantics measured on-device, tools/trprobe.hip
// — see conv.hip's transpose-read section). The 16-column XOR per
// k-octet makes the two k-octets a 32-lane tr read touches land on
// disjoint bank octets (16x16x32 fragments read rows kfrag..kfrag+7,
// and rows r and r+8 alias banks at the 96-elem row stride).
constexpr int TR_L = 96;
constexpr int TR_ELEMS = BK * TR_L;

DEVINL bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

DEVINL int tr_xor(int k) { return 16 * ((k >> 3) & 1); }

DEVINL void stage_kx(const __bf16* __restrict__ P, __bf16* S,
                     int x0, int k0, int X, int K, int ld, int t, int vec) {
  const int k = t >> 3;          // 0..31 == BK
  const int xx0 = (t & 7) * 8;   // 0..56
  const int gk = k0 + k;
  const int gx = x0 + xx0;
  const __bf16* src = P + (long)gk * ld + gx;
  bf16x8 v = {};
  if (gk < K && gx + 8 <= X) {
    if (vec == 8) {
      v = *(const bf16x8*)src;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[j];
    }
  } else if (gk < K) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (gx + j < X) v[j] = src[j];
  }
  *(bf16x8*)&S[k * TR_L + (xx0 ^ tr_xor(k))] = v;
}

// MFMA fragment (8 reduction elems for column cb + (lane&15)) out of
// the stage_kx image via two transpose-reads.
DEVINL bf16x8 tr_frag(const __bf16* S, int kfrag, int cb, int lane) {
  const int a = (kfrag + ((lane & 15) >> 2)) * TR_L +
                ((cb + 4 * (lane & 3)) ^ tr_xor(kfrag));
  bf16x4 f0 = tr_read(&S[a]);
  bf16x4 f1 = tr_read(&S[a + 4 * TR_L]);
  return __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ACT: 0 none, 1 relu, 2 relu-bwd (mask by aux>0, the saved activation).
// SK: split-K over gridDim.z with last-arriver epilogue.
// CS: colsum_out[n] = sum_k op(B)[k][n] computed by blockIdx.y==0 WGs.
template <bool TA, bool TB, int ACT, bool BIAS, bool OUTF32, bool SK, bool CS>
__global__ __launch_bounds__(256)
void gemm_kernel(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                 const void* __restrict__ bias, bool bias_bf16,
                 void* __restrict__ Cout, const __bf16* __restrict__ aux,
                 void* __restrict__ colsum_out, float* __restrict__ ws,
                 int* __restrict__ cnt, int M, int N, int K, int lda, int ldb,
                 int ldc, int kc, int veca, int vecb, int rflags) {
  // double-buffered: stage tile i+1 while MFMA consumes tile i (one
  // barrier per K-iteration). The single-buffered version serialized
  // global-load latency -> barrier -> MFMA every iteration and ran
  // the deep backward shapes at ~1.1 us/iteration (11 TFLOP/s on the
  // NMF dW GEMM).
  // xk-staged operands: [x][k] XOR-swizzled tiles; kx-staged
  // (transposing) operands: reduction-major transpose-read image
  __shared__ __align__(16) __bf16 As[2][TA ? TR_ELEMS : SWZ_ELEMS];
  __shared__ __align__(16) __bf16 Bs[2][TB ? SWZ_ELEMS : TR_ELEMS];

  const int tm0 = blockIdx.y * BM;
  const int tn0 = blockIdx.x * BN;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = t >> 6;          // 0..3
  const int wr = wave >> 1, wc = wave & 1;

  const int ks = SK ? blockIdx.z * kc : 0;
  const int ke = SK ? min(ks + kc, K) : K;

  f32x4 acc[2][2] = {};
  float cs_acc = 0.f;

#define STAGE_AB(buf, kk0v)                                                 \
  do {                                                                      \
    if (TA) stage_kx(A, As[buf], tm0, kk0v, M, K, lda, t, veca);            \
    else    stage_xk(A, As[buf], tm0, kk0v, M, K, lda, t, veca);            \
    if (TB) stage_xk(B, Bs[buf], tn0, kk0v, N, K, ldb, t, vecb);            \
    else    stage_kx(B, Bs[buf], tn0, kk0v, N, K, ldb, t, vecb);            \
  } while (0)

  STAGE_AB(0, ks);
  __syncthreads();
  int cur = 0;
  for (int k0 = ks; k0 < ke; k0 += BK, cur ^= 1) {
    if (k0 + BK < ke) STAGE_AB(cur ^ 1, k0 + BK);

    if (CS && blockIdx.y == 0 && t < BN) {
#pragma unroll
      for (int kk = 0; kk < BK; ++kk)
        cs_acc += TB ? (float)*sptr(Bs[cur], t, kk)
                     : (float)Bs[cur][kk * TR_L + (t ^ tr_xor(kk))];
    }

    const int kfrag = (lane >> 4) * 8;
    bf16x8 bfrag[2];
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
      bfrag[fn] = TB
          ? *(const bf16x8*)sptr(Bs[cur],
                                 wc * 32 + fn * 16 + (lane & 15), kfrag)
          : tr_frag(Bs[cur], kfrag, wc * 32 + fn * 16, lane);
#pragma unroll
    for (int fm = 0; fm < 2; ++fm) {
      bf16x8 a = TA
          ? tr_frag(As[cur], kfrag, wr * 32 + fm * 16, lane)
          : *(const bf16x8*)sptr(As[cur],
                                 wr * 32 + fm * 16 + (lane & 15), kfrag);
#pragma unroll
      for (int fn = 0; fn < 2; ++fn)
        acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, bfrag[fn], acc[fm][fn], 0, 0, 0);
    }
    __syncthreads();
  }
#undef STAGE_AB

  if (CS && blockIdx.y == 0 && t < BN && tn0 + t < N) {
    if (SK)       // per-slice fp32 partial, summed by the reduce kernel
      ((float*)colsum_out)[(long)blockIdx.z * N + tn0 + t] = cs_acc;
    else if (OUTF32) ((float*)colsum_out)[tn0 + t] = cs_acc;
    else ((__bf16*)colsum_out)[tn0 + t] = (__bf16)cs_acc;
  }

  if (SK) {
    // store this slice's fp32 partial tile into its workspace stripe;
    // the follow-up reduce kernel sums stripes in fixed slice order —
    // or, when cnt != nullptr (small tile grids), the LAST-ARRIVING
    // slice block sums them here and applies the epilogue itself
    // (fixed z order, so still deterministic), saving the reduce
    // launch + its dependent-kernel boundary. rflags: bit0 relu,
    // bit1 fp32 out, bit2 bias.
    float* wslice = ws + (long)blockIdx.z * (long)M * ldc;
#pragma unroll
    for (int fm = 0; fm < 2; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) {
        const int col = tn0 + wc * 32 + fn * 16 + (lane & 15);
        if (col >= N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = tm0 + wr * 32 + fm * 16 + (lane >> 4) * 4 + r;
          if (row < M) wslice[(long)row * ldc + col] = acc[fm][fn][r];
        }
      }
    if (cnt != nullptr) {
      __threadfence();
      __shared__ int lastf;
      if (t == 0)
        lastf = (atomicAdd(&cnt[blockIdx.y * gridDim.x + blockIdx.x], 1) ==
                 (int)gridDim.z - 1) ? 1 : 0;
      __syncthreads();
      if (!lastf) return;
      __threadfence();   // acquire: don't serve stale L2 for the stripes
      if (t == 0) cnt[blockIdx.y * gridDim.x + blockIdx.x] = 0;
      const int ns = gridDim.z;
      // vectorized row-major sweep of the whole 64x64 tile: 4 f32x4
      // positions per thread, every stripe's loads independent — the
      // first cut walked the MFMA acc mapping with scalar loads and
      // the lone consumer block serialized ~144 cross-XCD round trips
      // (the one-WG-consumer trap, see mlp.py's FROMWS note)
      const int crow = t >> 2;             // 0..63 within tile
      const int ccol0 = (t & 3) * 16;      // 4 f32x4 groups per row
      // z2*M*ldc + row*ldc + col (col % 4 == 0) is 16-byte aligned for
      // every row and stripe only when ldc % 4 == 0 and the base is
      const bool vec4 = (ldc & 3) == 0 && ((uintptr_t)ws & 15) == 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int row = tm0 + crow;
        const int col = tn0 + ccol0 + u * 4;
        if (row >= M || col >= N) continue;
        const long idx = (long)row * ldc + col;
        f32x4 v = {};
        for (int z2 = 0; z2 < ns; ++z2) {
          const float* s2 = &ws[(long)z2 * M * ldc + idx];
          if (vec4 && col + 4 <= N) {
            v += *(const f32x4*)s2;
          } else {
            for (int j = 0; j < 4; ++j)
              if (col + j < N) v[j] += s2[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (col + j >= N) continue;
          float x = v[j];
          if (rflags & 4)
            x += bias_bf16 ? (float)((const __bf16*)bias)[col + j]
                           : ((const float*)bias)[col + j];
          if (rflags & 1) x = x > 0.f ? x : 0.f;
          if (rflags & 2) ((float*)Cout)[idx + j] = x;
          else ((__bf16*)Cout)[idx + j] = (__bf16)x;
        }
      }
    }
    return;
  }

  // epilogue: (last WG per tile when SK) bias + activation + store
  // (C/D map: col=l&15, row=(l>>4)*4+r)
#pragma unroll
  for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
      const int col = tn0 + wc * 32 + fn * 16 + (lane & 15);
      if (col >= N) continue;
      const float bv = !BIAS ? 0.f
          : (bias_bf16 ? (float)((const __bf16*)bias)[col]
                       : ((const float*)bias)[col]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = tm0 + wr * 32 + fm * 16 + (lane >> 4) * 4 + r;
        if (row >= M) continue;
        const long idx = (long)row * ldc + col;
        float v = acc[fm][fn][r];
        v += bv;
        if (ACT == 1) v = v > 0.f ? v : 0.f;
        if (ACT == 2) v = (float)aux[idx] > 0.f ? v : 0.f;
        if (ACT == 3) v -= (float)aux[idx];   // fused residual (NMF E)
        if (OUTF32)
          ((float*)Cout)[idx] = v;
        else
          ((__bf16*)Cout)[idx] = (__bf16)v;
      }
    }
  }
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// Range-checked loads: a raw buffer descriptor over a wave-uniform base
// and the byte extent of the tensor VIEW that was passed. A lane whose
// offset lies beyond the extent receives zeros from the hardware — no
// clamped address, no 64-bit add, no select after the load and no
// predicate kept alive across the loads. Offsets are 32-bit bytes; a
// predicate that is constant per lane is folded into the lane's base
// offset once (BUF_OOB: beyond every extent, with room to add to).
typedef __amdgpu_buffer_rsrc_t brsrc_t;
constexpr int BUF_OOB = 0x40000000;

DEVINL brsrc_t buf_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes,
                                           0x00020000);
}
DEVINL float buf_f32(brsrc_t r, int off) {
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

// split-K phase 2: out[i] = act(sum_z ws[z][i] + bias), f32x4-vectorized
// over the flattened [M,ldc] output (ldc == N, contiguous).
// 1-elem/thread variant for SMALL outputs (mnist fwd: mn = 10k gave
// only 10 WGs at 4 elems/thread — the reduce was WG-count
// latency-bound, not bandwidth-bound; 4x the blocks cut it ~2x)
// sj (optional, dst != null): the last, mostly idle block also copies
// two small bf16 ranges (see SnapArgs) — a side job for the NEXT launch
struct SnapJob {
  const __bf16* s0; const __bf16* s1;
  __bf16* dst;
  int n0, n1, off1;
  int rows, cols;   // > 0: s0 is [rows, cols], the images are laid out too
};

// The two operand images of a [rows, cols] classifier that
// mlp_head_tail_kernel's waves consume (see SnapArgs), as b128 chunks in
// wave-sized groups g < SNAP_NG: groups 0-3 are the 128 live k of the
// k-major [CP][HP] image (chunk = eight k of one class row), groups 4-7
// the [HB][CP] row image (chunk = half a row) and group 8 the k-major
// image's 16 pad chunks. Zero beyond rows and cols, so every chunk of
// both images is written on every snapshot and nothing of an earlier
// classifier survives. One block pays the (row, class) arithmetic here;
// every wave of the consumer then moves whole chunks.
// g is wave-uniform, so a wave runs one of the three forms. The loads
// are range-checked (buf_rsrc): a row >= rows is beyond the extent
// whatever the class, the class predicate is folded into the offset.
constexpr int SNAP_NG = 9;
static_assert(kSnapRowOff - kSnapKmajOff == CP * HP &&
              kSnapElems - kSnapRowOff == HB * CP && HP == HB + 8 &&
              HB * CP / 8 == 4 * WAVE, "snapshot layout");

struct SnapChunk {
  unsigned e[8];   // one element per register: packed only when stored,
};                 // so the loads can stay in flight meanwhile

DEVINL SnapChunk snap_chunk_load(const SnapJob& sj, int g, int lane) {
  const brsrc_t r = buf_rsrc(sj.s0, sj.rows * sj.cols * 2);
  const int q = (g & 3) * WAVE + lane;
  int off[8];
  if (g < 4) {          // class q >> 4, rows (q & 15) * 8 + j
    const int c = q >> 4;
    const int base =
        c < sj.cols ? ((q & 15) * 8 * sj.cols + c) * 2 : BUF_OOB;
#pragma unroll
    for (int j = 0; j < 8; ++j) off[j] = base + j * sj.cols * 2;
  } else {              // row q >> 1, classes (q & 1) * 8 + j
    const int c0 = (q & 1) * 8;
    const int base = ((q >> 1) * sj.cols + c0) * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      off[j] = (g < 8 && c0 + j < sj.cols) ? base + j * 2 : BUF_OOB;
  }
  SnapChunk ch;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    ch.e[j] = __builtin_amdgcn_raw_buffer_load_b16(r, off[j], 0, 0);
  return ch;
}

DEVINL void snap_chunk_store(const SnapJob& sj, int g, int lane,
                             const SnapChunk& ch) {
  // the empty asm pins the packing here: the compiler otherwise moves the
  // shifts up to the loads, and with them the wait for the loads
  unsigned e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    e[j] = ch.e[j];
    asm volatile("" : "+v"(e[j]));
  }
  u32x4 d;
#pragma unroll
  for (int j = 0; j < 4; ++j) d[j] = e[2 * j] | (e[2 * j + 1] << 16);
  const bf16x8 v = __builtin_bit_cast(bf16x8, d);
  const int q = (g & 3) * WAVE + lane;
  if (g < 4)
    *(bf16x8*)&sj.dst[kSnapKmajOff + (q >> 4) * HP + (q & 15) * 8] = v;
  else if (g < 8)
    *(bf16x8*)&sj.dst[kSnapRowOff + q * 8] = v;
  else if (lane < CP)
    *(bf16x8*)&sj.dst[kSnapKmajOff + lane * HP + HB] = v;
}

template <int ACT, bool BIAS, bool OUTF32>
__global__ __launch_bounds__(256)
void splitk_reduce_small_kernel(const float* __restrict__ ws,
                                const void* __restrict__ bias,
                                bool bias_bf16, void* __restrict__ Cout,
                                long mn, int ldc, int nslice, SnapJob sj) {
  if (sj.dst != nullptr && blockIdx.x == gridDim.x - 1) {
    for (int j = threadIdx.x; j < sj.n0; j += 256) sj.dst[j] = sj.s0[j];
    for (int j = threadIdx.x; j < sj.n1; j += 256)
      sj.dst[sj.off1 + j] = sj.s1[j];
    if (sj.rows > 0) {
      const int lane = threadIdx.x & 63;
      for (int g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
           g < SNAP_NG; g += 4)
        snap_chunk_store(sj, g, lane, snap_chunk_load(sj, g, lane));
    }
  }
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= mn) return;
  float v = 0.f;
  for (int z = 0; z < nslice; ++z) v += ws[(long)z * mn + i];
  if (BIAS) {
    const int col = (int)(i % ldc);
    v += bias_bf16 ? (float)((const __bf16*)bias)[col]
                   : ((const float*)bias)[col];
  }
  if (ACT == 1) v = v > 0.f ? v : 0.f;
  if (OUTF32) ((float*)Cout)[i] = v;
  else ((__bf16*)Cout)[i] = (__bf16)v;
}

// f32x4 stripe loads at ws + z*mn + i0 (i0 % 4 == 0) are 16-byte aligned
// for every slice z only when mn % 4 == 0 and the stripe base is: an odd
// mn puts every other stripe off the boundary, and gemm_sgd_pair hands
// its second half a base that is an arbitrary element offset into the
// shared workspace. Otherwise the same elements are loaded one by one,
// summed in the same order. With mn % 4 == 0 a thread's four elements
// are all inside mn, so the vector path needs no tail.
DEVINL bool stripes_vec4(const float* ws, long mn) {
  return (mn & 3) == 0 && ((uintptr_t)ws & 15) == 0;
}

template <int ACT, bool BIAS, bool OUTF32>
__global__ __launch_bounds__(256)
void splitk_reduce_kernel(const float* __restrict__ ws, const void* __restrict__ bias,
                          bool bias_bf16, void* __restrict__ Cout, long mn,
                          int ldc, int nslice,
                          const float* __restrict__ cs_part,
                          void* __restrict__ cs_out, bool cs_f32, int N) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= mn) return;
  if (cs_part != nullptr && i0 < N) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long n = i0 + j;
      if (n >= N) break;
      float s = 0.f;
      for (int z = 0; z < nslice; ++z) s += cs_part[(long)z * N + n];
      if (cs_f32) ((float*)cs_out)[n] = s;
      else ((__bf16*)cs_out)[n] = (__bf16)s;
    }
  }
  const bool vec4 = stripes_vec4(ws, mn);
  f32x4 v = {};
  for (int z = 0; z < nslice; ++z) {
    const float* s = ws + (long)z * mn + i0;
    if (vec4) {
      const f32x4 sv = *(const f32x4*)s;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += sv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < mn) v[j] += s[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = i0 + j;
    if (i >= mn) break;
    float x = v[j];
    if (BIAS) {
      const int col = (int)(i % ldc);
      x += bias_bf16 ? (float)((const __bf16*)bias)[col]
                     : ((const float*)bias)[col];
    }
    if (ACT == 1) x = x > 0.f ? x : 0.f;
    if (OUTF32) ((float*)Cout)[i] = x;
    else ((__bf16*)Cout)[i] = (__bf16)x;
  }
}

// ------------------------------------------------ one-launch split-K fwd
//
// C = act(A @ B + bias) for small outputs whose K has to be sliced (the
// mnist fwd 100x100x784): the K slices of one output tile are the WAVES
// of one workgroup instead of separate workgroups, and the fp32 partials
// meet in LDS instead of a global stripe workspace. One launch, one
// barrier, no workspace, no counters, no fences, no atomics. Wave z owns
// k in [z*kc, min((z+1)*kc, K)) with the kc / nslice the binding computes
// for the stripes path, chains the same 16x16x32 MFMAs over its k-steps
// in ascending order with gemm_kernel's operand placement, and the block
// then sums the partials z = 0..nslice-1 in that order before the
// bias/relu/cast — per element exactly gemm_kernel<SK> followed by the
// stripe reduce, so the two routes agree bit for bit.
//
// Loads: every global load of up to F1_KS k-steps (the whole slice at
// kc <= 96) is issued before the first wait, so a wave is one memory
// round trip deep. A fragments come straight from global (one b128 per
// lane when rows are 16B-aligned). B ([K,N], 8 k per lane) is loaded
// row-wise as dword-aligned b128 chunks and transposed through a
// wave-private k-major LDS image read back with ds_read_b64_tr_b16
// (the per-wave DS pipe is in order: no barrier), or loaded strided
// straight into the fragment when B rows are not dword-aligned. A B
// chunk that straddles N is read as the row's last whole chunk and
// shifted at commit time; unaligned operands take guarded element
// loads. Positions beyond M, N, K are zero-filled, never read.
//
// The wave's fp32 partial overlays its own (dead) B image; every LDS
// access in the kernel goes through __bf16 vector types, so the
// overlay involves no differently-typed views of the same bytes.
// sj: the W2/b2 snapshot side job (as in the small stripe reduce), done
// by the last (ragged) block; its loads are issued first and stored before
// the barrier, so the copy rides under the GEMM's own round trip.
typedef bf16x8 __attribute__((aligned(4))) bf16x8_a4;

constexpr int F1_KS = 3;   // k-steps in flight per wave
// shipped tile (launch_gemm_fwd1's variant code); measurements of all
// four are in docs/KERNELS.md
constexpr int kFwd1Tile = 0;

// elements P[off + j*stride] for j < nvalid, zeros beyond (never read):
// the guarded path of operands whose rows allow no vector access
DEVINL bf16x8 f1_load8(const __bf16* __restrict__ P, long off, long stride,
                       int nvalid) {
  bf16x8 v = {};
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j < nvalid) v[j] = P[off + j * stride];
  return v;
}

template <int TM, int TN>
struct Fwd1Geo {
  static constexpr int FM = TM / 16, FN = TN / 16;
  static constexpr int BP = TN + 8;          // B image row pitch, elems
  static constexpr int IMG_BYTES = BK * BP * 2;
  static constexpr int PART_BYTES = TM * TN * 4;
  static constexpr int WAVE_BYTES =
      IMG_BYTES > PART_BYTES ? IMG_BYTES : PART_BYTES;
};

// VA: A rows 16B-aligned and K % 8 == 0 (a k chunk is whole or absent).
// VB: B rows dword-aligned, N even and >= 8.
template <int TM, int TN, bool VA, bool VB>
__global__ __launch_bounds__(1024)
void gemm_fwd1_kernel(const __bf16* __restrict__ A,
                      const __bf16* __restrict__ B,
                      const void* __restrict__ bias, bool bias_bf16,
                      void* __restrict__ Cout, bool out_f32, int relu,
                      int M, int N, int K, int lda, int ldb, int ldc, int kc,
                      SnapJob sj) {
  using G = Fwd1Geo<TM, TN>;
  constexpr int FM = G::FM, FN = G::FN, BP = G::BP;
  extern __shared__ __align__(16) __bf16 f1_smem[];
  const int t = threadIdx.x;
  const int nth = blockDim.x;
  const int lane = t & 63;
  const int z = t >> 6;                 // K slice of this wave
  const int nslice = nth >> 6;
  const int m0 = blockIdx.y * TM;
  const int n0 = blockIdx.x * TN;
  const int ks = z * kc;
  const int ke = min(ks + kc, K);
  const int kfrag = (lane >> 4) * 8;
  __bf16* img = f1_smem + z * (G::WAVE_BYTES / 2);

  // snapshot side job: loads first, stores before the barrier
  const bool snapper = sj.dst != nullptr && blockIdx.x == gridDim.x - 1 &&
                       blockIdx.y == gridDim.y - 1;
  const int sn = sj.n0 + sj.n1;
  const bool imgs = sj.rows > 0;
  const int zu = __builtin_amdgcn_readfirstlane(z);   // provably uniform
  __bf16 sv[2] = {};
  SnapChunk sc = {};
  // unlikely: one block per launch — its code goes behind the kernel's
  // end instead of standing between every block's prologue and k loop
  if (__builtin_expect(snapper, 0)) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = t + u * nth;
      if (j < sn) sv[u] = j < sj.n0 ? sj.s0[j] : sj.s1[j - sj.n0];
    }
    // this wave's first group of image chunks
    if (imgs && zu < SNAP_NG) sc = snap_chunk_load(sj, zu, lane);
  }

  // this thread's first epilogue element (see the combine loop): its
  // bias is fetched now, not after the barrier
  float bv = 0.f;
  if (bias != nullptr && t < TM * TN) {
    const int col = n0 + ((t >> 8) % FN) * 16 + ((t >> 2) & 15);
    if (col < N)
      bv = bias_bf16 ? (float)((const __bf16*)bias)[col]
                     : ((const float*)bias)[col];
  }

  f32x4 acc[FM][FN] = {};
  for (int kb = ks; kb < ke; kb += F1_KS * BK) {
    bf16x8 ra[F1_KS][FM];
    bf16x8 rb[F1_KS][FN];
#pragma unroll
    for (int s = 0; s < F1_KS; ++s) {
      const int k0 = kb + s * BK;
#pragma unroll
      for (int fm = 0; fm < FM; ++fm) {
        ra[s][fm] = bf16x8{};
        const int row = m0 + fm * 16 + (lane & 15);
        const int gk = k0 + kfrag;
        if (k0 < ke && row < M && gk < K) {
          const long off = (long)row * lda + gk;
          if (VA) ra[s][fm] = *(const bf16x8*)(A + off);
          else ra[s][fm] = f1_load8(A, off, 1, K - gk);
        }
      }
#pragma unroll
      for (int u = 0; u < FN; ++u) {
        rb[s][u] = bf16x8{};
        if (VB) {
          // row-wise chunk u*64+lane of the [BK][TN] tile. A chunk that
          // straddles N is read as the row's LAST whole chunk (in
          // bounds, still dword-aligned) and shifted into place at
          // commit time — one unconditional b128 either way
          const int c = u * 64 + lane;
          const int gk = k0 + c / (TN / 8);
          const int gn = n0 + (c % (TN / 8)) * 8;
          if (k0 < ke && gk < K && gn < N)
            rb[s][u] =
                *(const bf16x8_a4*)(B + (long)gk * ldb + min(gn, N - 8));
        } else {
          // fragment u straight from global, one element per load
          const int col = n0 + u * 16 + (lane & 15);
          const int gk = k0 + kfrag;
          if (k0 < ke && col < N && gk < K)
            rb[s][u] = f1_load8(B, (long)gk * ldb + col, ldb, K - gk);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < F1_KS; ++s) {
      if (kb + s * BK >= ke) break;
      bf16x8 bf[FN];
      if (VB) {
#pragma unroll
        for (int u = 0; u < FN; ++u) {
          const int c = u * 64 + lane;
          const int gn = n0 + (c % (TN / 8)) * 8;
          // dwords the chunk was read early by (N even); live columns
          // move down, zeros come in above them
          const int sh = (gn - min(gn, N - 8)) >> 1;
          u32x4 d = __builtin_bit_cast(u32x4, rb[s][u]);
          if (sh & 1) d = u32x4{d[1], d[2], d[3], 0u};
          if (sh & 2) d = u32x4{d[2], d[3], 0u, 0u};
          *(bf16x8*)&img[(c / (TN / 8)) * BP + (c % (TN / 8)) * 8] =
              __builtin_bit_cast(bf16x8, d);
        }
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) {
          const int a = (kfrag + ((lane & 15) >> 2)) * BP + fn * 16 +
                        4 * (lane & 3);
          bf16x4 f0 = tr_read(&img[a]);
          bf16x4 f1 = tr_read(&img[a + 4 * BP]);
          bf[fn] = __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
        }
      } else {
#pragma unroll
        for (int fn = 0; fn < FN; ++fn) bf[fn] = rb[s][fn];
      }
#pragma unroll
      for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              ra[s][fm], bf[fn], acc[fm][fn], 0, 0, 0);
    }
  }

  // partial fragment f = fm*FN+fn of slice z: float (f*64 + lane)*4 + r
#pragma unroll
  for (int fm = 0; fm < FM; ++fm)
#pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      *(bf16x8*)&img[((fm * FN + fn) * 64 + lane) * 8] =
          __builtin_bit_cast(bf16x8, acc[fm][fn]);

  if (__builtin_expect(snapper, 0)) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = t + u * nth;
      if (j < sn) sj.dst[j < sj.n0 ? j : sj.off1 + (j - sj.n0)] = sv[u];
    }
    for (int j = t + 2 * nth; j < sn; j += nth)
      sj.dst[j < sj.n0 ? j : sj.off1 + (j - sj.n0)] =
          j < sj.n0 ? sj.s0[j] : sj.s1[j - sj.n0];
    if (imgs) {
      if (zu < SNAP_NG) snap_chunk_store(sj, zu, lane, sc);
      for (int g = zu + nslice; g < SNAP_NG; g += nslice)
        snap_chunk_store(sj, g, lane, snap_chunk_load(sj, g, lane));
    }
  }
  __syncthreads();

  for (int e = t; e < TM * TN; e += nth) {
    const int r = e & 3, pl = (e >> 2) & 63, f = e >> 8;
    const int col = n0 + (f % FN) * 16 + (pl & 15);
    const int row = m0 + (f / FN) * 16 + (pl >> 4) * 4 + r;
    if (row >= M || col >= N) continue;
    float v = 0.f;
    for (int z2 = 0; z2 < nslice; ++z2)
      v += __builtin_bit_cast(
          float, *(const bf16x2*)&f1_smem[z2 * (G::WAVE_BYTES / 2) + e * 2]);
    if (bias != nullptr)
      v += e == t ? bv
                  : (bias_bf16 ? (float)((const __bf16*)bias)[col]
                               : ((const float*)bias)[col]);
    if (relu) v = v > 0.f ? v : 0.f;
    const long idx = (long)row * ldc + col;
    if (out_f32) ((float*)Cout)[idx] = v;
    else ((__bf16*)Cout)[idx] = (__bf16)v;
  }
}

typedef __attribute__((ext_vector_type(16))) float f32x16;

// ---------------------------------------------------------- small-tile path
//
// One-kernel GEMM for tiny tile grids (the mnist fwd 100x100x784 and
// dW1 784x100x100): the two-phase split-K path paid TWO dispatch
// floors (~13 us for ~16 MFLOP). 32x32 output tile per block; the 4
// waves SPLIT K privately — each stages into its OWN LDS quarter, so
// the k-loop has NO barrier — then one barrier, a cross-wave
// accumulate by wave 0, and the fused epilogue (bias/relu, bf16/f32
// out). colsum (db1) is summed during B staging and reduced by
// blockIdx.x==0 only (it depends on K alone, so every m-tile block
// would compute the same value; single-writer keeps it deterministic,
// no atomics, overwrite semantics like the 64x64 path).
// TA: op(A) = A^T (A stored [K,M] — transposed scatter staging).
// B is always untransposed here ([K,N] memory).
//
// SmallSgd: optional fused optimizer tail (the mnist single-GPU fast
// path). When pmw != null the epilogue APPLIES this GEMM's output as
// an SGD gradient (master -= lr*g, refresh bf16 shadow) instead of
// storing it, the colsum applies the bias grad the same way, and one
// otherwise-idle wave of block (0,0) also applies the classifier
// grads (g2w/g2b, written by the head kernel that ran just before) —
// the step's separate flat-buffer sgd_kernel launch disappears.
// Valid only for plain SGD (no momentum/decay) with grad_scale 1
// (single worker); the distributed path keeps the PS apply.
struct SmallSgd {
  float* pmw;          // W master [M,N] fp32 (same layout as Cout)
  bf16_t* psw;         // W bf16 shadow
  float* pmb;          // bias master [N]
  bf16_t* psb;
  const bf16_t* g2w;   // classifier grads (from the head kernel)
  float* pm2w;
  bf16_t* ps2w;
  const bf16_t* g2b;
  float* pm2b;
  bf16_t* ps2b;
  float lr;
  int n2w, n2b;
};

// transpose-read fragment out of a k-major wave image (see tr_frag;
// same provider-lane scheme, 32-wide rows via sptr)
DEVINL bf16x8 trs_frag(const __bf16* S, int ko, int lane) {
  const int kq = ko + ((lane & 15) >> 2);
  const int c = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  bf16x4 f0 = tr_read(sptr(S, kq, c));
  bf16x4 f1 = tr_read(sptr(S, kq + 4, c));
  return __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// colsum partials of one wave: lane (kk, half) holds 16 columns of B
// row kk; xor-shuffle tree over the 32 rows, then lane kk==0 of each
// half parks its 16 sums in csw[32]
DEVINL void small_cs_reduce(const float* csp, float* csw, int lane) {
  float c2[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) c2[j] = csp[j];
#pragma unroll
  for (int off = 1; off < 32; off <<= 1)
#pragma unroll
    for (int j = 0; j < 16; ++j) c2[j] += __shfl_xor(c2[j], off, 64);
  if ((lane & 31) == 0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) csw[(lane >> 5) * 16 + j] = c2[j];
  }
}

// fused W1/b1 apply: ALL FOUR waves split the 16 output values
// (4 each, straight from the LDS partials) — the wave0-only form
// serialized the master-read/store latency on one wave per block
// and measured SLOWER than the separate wide sgd_kernel
//
// Two halves. small_sgd_fetch reads the masters this lane will update
// and is called at the TOP of the kernel: no master depends on anything
// the launch computes, each element is read and written by exactly one
// thread per launch, and stream order covers the previous step's store
// — so the read rides under the kernel's other loads instead of being a
// dependent round trip after the barrier (the one-function form
// compiled to load / wait / store per element, each load held behind
// the previous store because the pointers may alias). Lanes outside
// the tile read element 0 and drop the value: unconditional loads keep
// the compiler from fencing each one in a branch of its own.
// small_sgd_commit is what is left after the barrier: LDS reads,
// arithmetic and stores.
struct SmallSgdPre {
  float w[4];
  float b;
};

// Explicit s_waitcnt (gfx9 operand: vmcnt [3:0] and [15:14], expcnt
// [6:4], lgkmcnt [11:8]; all ones = no wait on that counter). The
// compiler's own wait insertion sees it and drops the waits it covers.
// Used where values fetched long ago are consumed across divergent
// store blocks: the compiler can only prove a small distance to such a
// load there and emits vmcnt(3), (2), (1), (0) between the stores —
// stores count on vmcnt too, so each block then waits for the stores
// before it to be acknowledged. One vmcnt(0) ahead of the first store,
// when nothing is in flight any more, costs nothing and removes them.
DEVINL void wait_vm0() { __builtin_amdgcn_s_waitcnt(0x0F70); }
DEVINL void wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

DEVINL int small_sgd_row(int m0, int w, int u, int lane) {
  const int v = w * 4 + u;
  return m0 + ((v >> 2) << 3) + ((lane >> 5) << 2) + (v & 3);
}

DEVINL void small_sgd_fetch(const SmallSgd& sg, SmallSgdPre& pre, bool cs,
                            int m0, int n0, int M, int N, int ldc, int w,
                            int lane) {
  const int n = n0 + (lane & 31);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int m = small_sgd_row(m0, w, u, lane);
    const long idx = (n < N && m < M) ? (long)m * ldc + n : 0;
    pre.w[u] = sg.pmw[idx];
  }
  pre.b = 0.f;
  if (cs && blockIdx.x == 0 && sg.pmb != nullptr) {
    const int nn = n0 + (lane & 31);
    pre.b = sg.pmb[nn < N ? nn : 0];
  }
}

// small_sgd_fetch for the fused head+tail kernel (ldc == N): the same
// elements, range-checked instead of clamped. Row m >= M lies beyond
// the extent together with every column n < N. In two parts, W1 and
// b1: the kernel's block roles each fetch what they apply.
DEVINL void small_sgd_fetch_buf_w(const SmallSgd& sg, SmallSgdPre& pre,
                                  int m0, int n0, int M, int N, int w,
                                  int lane) {
  const brsrc_t wr = buf_rsrc(sg.pmw, M * N * 4);
  const int n = n0 + (lane & 31);
  const int nb = n < N ? n * 4 : BUF_OOB;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    pre.w[u] = buf_f32(wr, nb + small_sgd_row(m0, w, u, lane) * N * 4);
}

DEVINL void small_sgd_fetch_buf_b(const SmallSgd& sg, SmallSgdPre& pre,
                                  int n0, int N, int lane) {
  if (sg.pmb != nullptr)
    pre.b = buf_f32(buf_rsrc(sg.pmb, N * 4), (n0 + (lane & 31)) * 4);
}

// small_sgd_commit's bias half on its own (wave 0, lanes 0..31)
DEVINL void small_sgd_commit_b(const SmallSgd& sg, const SmallSgdPre& pre,
                               const float (*csred)[32], int n0, int N,
                               int lane) {
  const int nn = n0 + lane;
  if (nn < N && sg.pmb != nullptr) {
    const float sv = csred[0][lane] + csred[1][lane] + csred[2][lane] +
                     csred[3][lane];
    const float pv = pre.b - sg.lr * sv;
    sg.pmb[nn] = pv;
    sg.psb[nn] = f2bf(pv);
  }
}

DEVINL void small_sgd_commit(const SmallSgd& sg, const SmallSgdPre& pre,
                             const float (*red)[64 * 16],
                             const float (*csred)[32], bool cs, int m0,
                             int n0, int M, int N, int ldc, int w, int lane) {
  const int n = n0 + (lane & 31);
  if (n < N) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = w * 4 + u;
      const int m = small_sgd_row(m0, w, u, lane);
      if (m >= M) continue;
      const float x = red[0][lane * 16 + v] + red[1][lane * 16 + v] +
                      red[2][lane * 16 + v] + red[3][lane * 16 + v];
      const long idx = (long)m * ldc + n;
      const float pv = pre.w[u] - sg.lr * x;
      sg.pmw[idx] = pv;
      sg.psw[idx] = f2bf(pv);
    }
  }
  if (cs && w == 0 && blockIdx.x == 0 && lane < 32)
    small_sgd_commit_b(sg, pre, csred, n0, N, lane);
}

// the colsum store of one N tile (wave 0, lanes 0..31)
DEVINL void small_store_cs(const float (*csred)[32], void* colsum_out,
                           bool cs_f32, int n0, int N, int lane) {
  const int nn = n0 + lane;
  if (nn < N) {
    const float sv = csred[0][lane] + csred[1][lane] + csred[2][lane] +
                     csred[3][lane];
    if (cs_f32) ((float*)colsum_out)[nn] = sv;
    else ((__bf16*)colsum_out)[nn] = (__bf16)sv;
  }
}

// plain store epilogue (wave 0): cross-wave sum, bias/relu, fp32 or
// bf16 out, and the colsum by blockIdx.x == 0
DEVINL void small_store(const float (*red)[64 * 16],
                        const float (*csred)[32], bool cs,
                        const void* bias, bool bias_bf16, void* Cout,
                        bool out_f32, int relu, void* colsum_out,
                        bool cs_f32, int m0, int n0, int M, int N, int ldc,
                        int lane) {
  f32x16 tot;
#pragma unroll
  for (int v = 0; v < 16; ++v)
    tot[v] = red[0][lane * 16 + v] + red[1][lane * 16 + v] +
             red[2][lane * 16 + v] + red[3][lane * 16 + v];
  const int n = n0 + (lane & 31);
  if (n < N) {
    float bvv = 0.f;
    if (bias != nullptr)
      bvv = bias_bf16 ? (float)((const __bf16*)bias)[n]
                      : ((const float*)bias)[n];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int m = m0 + ((v >> 2) << 3) + ((lane >> 5) << 2) + (v & 3);
      if (m >= M) continue;
      float x = tot[v] + bvv;
      if (relu) x = x > 0.f ? x : 0.f;
      if (out_f32) ((float*)Cout)[(long)m * ldc + n] = x;
      else ((__bf16*)Cout)[(long)m * ldc + n] = (__bf16)x;
    }
  }
  if (cs && blockIdx.x == 0 && lane < 32)
    small_store_cs(csred, colsum_out, cs_f32, n0, N, lane);
}

template <bool TA, bool CS>
__global__ __launch_bounds__(256)
void gemm_small_kernel(const __bf16* __restrict__ A,
                       const __bf16* __restrict__ B,
                       const void* __restrict__ bias, bool bias_bf16,
                       void* __restrict__ Cout, bool out_f32, int relu,
                       void* __restrict__ colsum_out, bool cs_f32,
                       int M, int N, int K, int lda, int ldb, int ldc,
                       int veca, int vecb, SmallSgd sg) {
  // wave-private 32x32 images, stride exactly 32 + the sptr chunk
  // swizzle: the transposing operands (A when TA, B always) store
  // K-MAJOR [k][col] — commit is two b128 stores (the transposed
  // scatter commit measured 3.5 extra LDS-conflict cycles per LDS
  // instruction here) — and fragments come back via ds_read_b64_tr_b16
  __shared__ __align__(16) __bf16 As[4][32 * BK];
  __shared__ __align__(16) __bf16 Bs[4][32 * BK];
  __shared__ float red[4][64 * 16];
  __shared__ float csred[4][32];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = t >> 6;
  const int m0 = blockIdx.x * 32;
  const int n0 = blockIdx.y * 32;
  const int kq = (((K + 3) / 4) + BK - 1) / BK * BK;  // per-wave K span
  const int ks = w * kq;
  const int ke = min(ks + kq, K);
  __bf16* Aw = As[w];
  __bf16* Bw = Bs[w];
  const int kk = lane & 31;
  const int half = lane >> 5;
  // bf16x8-aligned rows: pitch AND base (vec_level, as gemm_kernel) —
  // an operand that is a view into its storage has an aligned pitch
  // and a base that is not
  const bool av = veca == 8;
  const bool bv = vecb == 8;
  f32x4 acc[4] = {};
  float csp[16] = {};
  bf16x8 ra0, ra1, rb0, rb1;        // in-flight chunk (load -> commit)
  // APPLY: this lane's W1/b1 masters, in flight under the whole k-loop
  SmallSgdPre pre = {};
  if (sg.pmw != nullptr)
    small_sgd_fetch(sg, pre, CS, m0, n0, M, N, ldc, w, lane);

  // load: global reads into REGISTERS (vector when the row allows —
  // guarded scalar loads serialized the first cut at 2x the split-K
  // path); commit: LDS stores. Registers double-buffer the single LDS
  // image: the per-wave DS pipe is in-order, so this k-chunk's
  // fragment reads are serviced before the next chunk's commit writes.
  auto load_a = [&](int k0) {
    ra0 = bf16x8{};
    ra1 = bf16x8{};
    if (TA) {
      // A stored [K, M]: 16 consecutive m of one k
      const int gk = k0 + kk;
      const int gm = m0 + half * 16;
      if (gk < ke) {
        const __bf16* src = A + (long)gk * lda + gm;
        if (av && gm + 16 <= M && ((m0 & 7) == 0)) {
          ra0 = *(const bf16x8*)src;
          ra1 = *(const bf16x8*)(src + 8);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (gm + j < M) ra0[j] = src[j];
            if (gm + 8 + j < M) ra1[j] = src[8 + j];
          }
        }
      }
    } else {
      // A stored [M, K]: row m, 16 consecutive k
      const int gm = m0 + kk;
      const int gk0 = k0 + half * 16;
      if (gm < M) {
        const __bf16* src = A + (long)gm * lda + gk0;
        if (av && gk0 + 16 <= ke) {
          ra0 = *(const bf16x8*)src;
          ra1 = *(const bf16x8*)(src + 8);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (gk0 + j < ke) ra0[j] = src[j];
            if (gk0 + 8 + j < ke) ra1[j] = src[8 + j];
          }
        }
      }
    }
    // B stored [K, N]: 16 consecutive n of one k
    rb0 = bf16x8{};
    rb1 = bf16x8{};
    {
      const int gk = k0 + kk;
      const int gn = n0 + half * 16;
      if (gk < ke) {
        const __bf16* src = B + (long)gk * ldb + gn;
        if (bv && gn + 16 <= N && ((n0 & 7) == 0)) {
          rb0 = *(const bf16x8*)src;
          rb1 = *(const bf16x8*)(src + 8);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (gn + j < N) rb0[j] = src[j];
            if (gn + 8 + j < N) rb1[j] = src[8 + j];
          }
        }
      }
    }
  };
  auto commit = [&]() {
    // both layouts have row kk: TA-A/B rows are k (16 consecutive
    // cols of one k per register), non-TA A rows are m (16
    // consecutive k) — either way two b128 chunk-aligned stores
    *(bf16x8*)sptr(Aw, kk, half * 16) = ra0;
    *(bf16x8*)sptr(Aw, kk, half * 16 + 8) = ra1;
    *(bf16x8*)sptr(Bw, kk, half * 16) = rb0;
    *(bf16x8*)sptr(Bw, kk, half * 16 + 8) = rb1;
    if (CS) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        csp[j] += (float)rb0[j];
        csp[8 + j] += (float)rb1[j];
      }
    }
  };

  load_a(ks);
  commit();
  for (int k0 = ks; k0 < ke; k0 += BK) {
    const bool more = k0 + BK < ke;
    if (more) load_a(k0 + BK);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int ko = kh * 16 + ((lane >> 5) << 3);
      bf16x8 a = TA ? trs_frag(Aw, ko, lane)
                    : *(const bf16x8*)sptr(Aw, lane & 31, ko);
      bf16x8 b = trs_frag(Bw, ko, lane);
      *(f32x16*)acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          a, b, *(f32x16*)acc, 0, 0, 0);
    }
    if (more) commit();
  }

  // cross-wave reduce (the only barrier) + epilogue by wave 0
#pragma unroll
  for (int v = 0; v < 16; ++v) red[w][lane * 16 + v] = ((float*)acc)[v];
  if (CS && blockIdx.x == 0) small_cs_reduce(csp, csred[w], lane);
  __syncthreads();
  wait_vm0();   // the prefetched masters landed a k-loop ago
  if (sg.pm2w != nullptr && w == 1 && blockIdx.x == 0 && blockIdx.y == 0) {
    // classifier apply: ~1k elems on one idle wave; runs strictly
    // after the head kernel wrote g2w/g2b (stream order), and nothing
    // reads the classifier shadow until the next step's head.
    // Vectorized 4-deep with every load issued before any store — the
    // first cut (scalar strided loop) serialized ~16 global round
    // trips on this single wave and cost MORE than the sgd_kernel it
    // replaced. Buffers are 256-elem-aligned flat-store slices, so
    // the f32x4/bf16x4 accesses are aligned.
    // The first pass of the two scalar loops below (the n2w % 4 tail
    // and the bias) is loaded here as well, ahead of every store: a
    // load issued after a store to a pointer it may alias waits for it.
    const int nv = sg.n2w >> 2;
    // Lanes beyond a range read its element 0 and drop the value (a
    // load guarded per lane sits in a branch of its own, and the
    // compiler waited for the loads in flight inside each of them).
    f32x4 mv[4] = {};
    bf16x4 gv[4] = {};
    if (nv > 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = lane + u * 64;
        gv[u] = ((const bf16x4*)sg.g2w)[i < nv ? i : 0];
        mv[u] = ((const f32x4*)sg.pm2w)[i < nv ? i : 0];
      }
    }
    const int it = (nv << 2) + lane;
    const int itc = it < sg.n2w ? it : 0;
    const int ibc = lane < sg.n2b ? lane : 0;
    const float mt = sg.pm2w[itc];
    const bf16_t gt = sg.g2w[itc];
    const float mb = sg.pm2b[ibc];
    const bf16_t gb = sg.g2b[ibc];
    wait_vm0();   // the one round trip of this wave
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = lane + u * 64;
      if (i < nv) {
        f32x4 pv;
        bf16x4 sv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pv[j] = mv[u][j] - sg.lr * (float)gv[u][j];
          sv[j] = (__bf16)pv[j];
        }
        ((f32x4*)sg.pm2w)[i] = pv;
        ((bf16x4*)sg.ps2w)[i] = sv;
      }
    }
    for (int i = 256 + lane; i < nv; i += 64) {   // >64 KB W2 (not mnist)
      f32x4 pv;
      bf16x4 sv;
      const bf16x4 g = ((const bf16x4*)sg.g2w)[i];
      const f32x4 m = ((const f32x4*)sg.pm2w)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pv[j] = m[j] - sg.lr * (float)g[j];
        sv[j] = (__bf16)pv[j];
      }
      ((f32x4*)sg.pm2w)[i] = pv;
      ((bf16x4*)sg.ps2w)[i] = sv;
    }
    if (it < sg.n2w) {                                      // n2w % 4
      const float pv = mt - sg.lr * bf2f(gt);
      sg.pm2w[it] = pv;
      sg.ps2w[it] = f2bf(pv);
    }
    if (lane < sg.n2b) {
      const float pv = mb - sg.lr * bf2f(gb);
      sg.pm2b[lane] = pv;
      sg.ps2b[lane] = f2bf(pv);
    }
    for (int i = lane + 64; i < sg.n2b; i += 64) {          // > 64 classes
      const float pv = sg.pm2b[i] - sg.lr * bf2f(sg.g2b[i]);
      sg.pm2b[i] = pv;
      sg.ps2b[i] = f2bf(pv);
    }
  }
  if (sg.pmw != nullptr) {
    small_sgd_commit(sg, pre, red, csred, CS, m0, n0, M, N, ldc, w, lane);
    return;
  }
  if (w != 0) return;
  small_store(red, csred, CS, bias, bias_bf16, Cout, out_f32, relu,
              colsum_out, cs_f32, m0, n0, M, N, ldc, lane);
}

// ------------------------------------------------ fused head + tail
//
// mnist step, launches 3 and 4 in one: every block of the dW1 tail
// (grid ceil(M/32) x ceil(H/32)) RECOMPUTES the slice of the classifier
// head it consumes instead of waiting for a one-workgroup head kernel
// to write dh. Wave w of gemm_small_kernel<TA> at K = B <= 128 consumes
// exactly dh rows 32w..32w+31 of its 32-column N tile, and the head's
// wave ownership is the same rows, so each wave stages its 32 rows of
// h and the 2 KB classifier into wave-private LDS, runs the shared
// logits / softmax / dh phases (mlp_head.h) and writes the bf16 dh
// fragment straight into its k-major Bs image — no block barrier on
// the way, and dh, dlogits, dW2 and db2 never touch global memory.
// From there it IS gemm_small_kernel: two MFMAs per wave, the red
// barrier, and the W1/b1 apply (APPLY) or the dW1/db1 store.
//
// One block additionally produces dW2 = h^T dls, db2 and the loss from
// the full hs/dls images every block holds after the barrier (same
// MFMA order over rows and the same 16-partial db2 order as the head;
// the transposed fragments come from the row-major images via
// ds_read_b64_tr_b16). !APPLY: classifier blocks of their own store
// them (block roles, below). APPLY: every block read the live W2/b2
// shadow at its start, so they may only be overwritten once all blocks
// have read — an arrival ticket without any spinning picks the block
// that arrives last: after the barrier
// (all four waves' W2/b2 loads have landed in LDS) one lane draws an
// agent-scope fetch_add ticket, the block applies its own W1 tile
// while the ticket is in flight, and whoever drew nblocks-1 does the
// classifier work and stores 0 back (stream order makes the
// self-reset sufficient for the next launch and for graph replay).
// The ticket measured ~5 us (16.4 us vs 11.4 us for the grads mode
// that needs none): the classifier work is serialized behind the last
// arrival. So where the step's preceding launch can take a 2 KB
// snapshot of W2/b2 (the small stripe reduce, SnapJob), the kernel
// reads the snapshot instead (ticket == null) and fixed blocks, with
// no tile of their own, apply to the live shadow concurrently — no
// atomics at all. The ticket stays for shapes whose fwd GEMM takes no
// snapshot. (The one-launch forward, gemm_fwd1_kernel, takes it the
// same way.)
// Unlike the rejected split-K last-arriver epilogue, the ticket's last
// arriver reads NOTHING another block wrote in this launch — no stripe
// pull, no acquire of foreign data, no L1-staleness hazard; the ticket
// only orders other blocks' completed READS before its writes.
struct HeadTail {
  const __bf16* h;       // [B, H] relu output
  const __bf16* w2;      // [H, C] (APPLY: live shadow, or its snapshot)
  const bf16_t* b2;      // [C]
  const long* labels;    // [B]
  float* loss;
  void* dw2;             // !APPLY: [H, C] / [C] in the grad dtype
  void* db2;
  unsigned* ticket;      // APPLY: zeroed device word; null = snapshot
  float scale;
  int C;
};

// Block roles. Everything but the ticket instantiation runs on a grid
// two rows of blockIdx.x longer than the mt x nt dW1 tiles, and every
// block has exactly ONE role, decided from its index alone (scalar
// branches at the top of the kernel, one straight-line body per role):
//   HT_TILE  x <  mt       a dW1 tile: h, classifier, logits, softmax,
//                          dh, the two dW1 MFMAs, the W1 apply / dW1
//                          store. No colsum, no bias, no classifier work.
//   HT_DB1   x == mt       one per N tile: the same head into Bs, the
//                          db1 colsum, the b1 apply / db1 store. No x,
//                          no As, no dW1 MFMA, no red, no W1 master.
//   HT_CLS   x == mt + 1   y == 0: dW2; y == 1: db2 and the loss (one
//                          N tile: y == 0 does both; y >= 2 leaves at
//                          once). h, logits, softmax into dls / lsum —
//                          no x, wpd, dh, Bs, dW1.
//   HT_ALL   the ticket instantiation, on the mt x nt grid: whoever
//            arrives last must hold hs and dls, so every block is a
//            tile, blockIdx.x == 0 adds db1 and the last arrival adds
//            the classifier work.
// Before, the snapshot step's last M tile ran the classifier work
// behind its tile and the first M tile the colsum behind its own: the
// kernel lasts as long as its longest block. SNAP tile blocks read only
// the snapshot images, the HT_CLS blocks alone write live W2/b2 and the
// HT_DB1 blocks alone b1; nothing else in the launch reads them.
enum { HT_ALL = 0, HT_TILE = 1, HT_DB1 = 2, HT_CLS = 3 };

struct HeadTailSmem {
  alignas(16) __bf16 hs[HB * HP];       // [row][k], all waves
  alignas(16) __bf16 wtp[4][(CP + 1) * HP];   // per wave [c][k] + a zero row
  alignas(16) __bf16 wpd[4][32 * CP];   // per wave, N tile rows
  alignas(16) __bf16 dls[HB * CP];      // [row][c]
  float ls[HB * LSP];
  float lsum[HB];
  alignas(16) __bf16 As[4][32 * BK];
  alignas(16) __bf16 Bs[4][32 * BK];
  float red[4][64 * 16];
  float csred[4][32];
  float db2p[CP * 16];
  unsigned tick;
};

// SNAP (APPLY only): w2/b2 are the snapshot and the classifier blocks
// are fixed, known at entry — they fetch their W2/b2 masters with
// everything else. !SNAP: the ticket decides, so they are fetched after
// it. bx: the block's M tile (HT_ALL, HT_TILE); tiles: mt * nt.
template <bool APPLY, bool GF32, bool SNAP, int ROLE>
DEVINL void head_tail_body(HeadTailSmem& sm, const __bf16* __restrict__ X,
                           const HeadTail& ht, void* __restrict__ Cout,
                           void* __restrict__ colsum_out, int M, int N,
                           int K, const SmallSgd& sg, int tiles) {
  static_assert(ROLE != HT_ALL || (APPLY && !SNAP), "HT_ALL: ticket only");
  static_assert(ROLE == HT_ALL || !APPLY || SNAP, "roles need no ticket");
  constexpr bool TILE = ROLE == HT_ALL || ROLE == HT_TILE;  // x, As, dW1
  constexpr bool DH = ROLE != HT_CLS;                       // wpd, dh, Bs
  auto& hs = sm.hs;
  auto& wtp = sm.wtp;
  auto& wpd = sm.wpd;
  auto& dls = sm.dls;
  auto& ls = sm.ls;
  auto& lsum = sm.lsum;
  auto& As = sm.As;
  auto& Bs = sm.Bs;
  auto& red = sm.red;
  auto& csred = sm.csred;
  auto& db2p = sm.db2p;
  auto& tick = sm.tick;
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = t >> 6;
  const int m0 = blockIdx.x * 32;
  const int n0 = blockIdx.y * 32;
  const int C = ht.C;
  const int ks = w * 32;              // kq == 32 for every K <= 128
  const int ke = min(ks + 32, K);
  __bf16* Aw = As[w];
  __bf16* Bw = Bs[w];
  __bf16* wtw = wtp[w];
  __bf16* wpw = wpd[w];
  const int kk = lane & 31;
  const int half = lane >> 5;

  // 1. EVERY global load of the launch, back to back, so the kernel is
  // one memory round trip deep: the x chunk (gemm_small's load_a, A
  // half), this wave's 32 rows of h (b64 chunks, two rows per pass), the
  // classifier (one hidden row per lane), its bias, the labels and —
  // APPLY — the fp32 masters this lane updates after the barrier.
  // All of them are unconditional, range-checked buffer loads (see
  // buf_rsrc: a lane with nothing to read sits beyond the extent and
  // gets zeros) with every conversion AFTER the last load: a load
  // guarded by a lane condition gets a branch of its own, and the
  // compiler drains the loads in flight (s_waitcnt vmcnt(0)) inside
  // such branches — the guarded form of this prologue was three round
  // trips, not one. In x, h and the masters a row beyond the tensor is
  // beyond the extent whatever the column, so only the column
  // predicate, constant per lane, is folded into the offset. (The
  // !SNAP classifier gather keeps clamped addresses and selects.)
  const int gk = ks + kk;
  const int gm = m0 + half * 16;
  const bool xvec = (M & 7) == 0;       // rows of x are whole b128 chunks
  bf16x8 ra0 = {}, ra1 = {};
  // ragged rows: element loads, one whole register each (two bf16
  // sharing a register would make the second load wait for the first).
  // Assigned and read only where !xvec — no initializer: zeroing 16
  // registers on the vector path put counted waits there, for loads
  // the compiler must assume pending on them.
  unsigned xs[16];
  if (TILE) {
    const brsrc_t xr = buf_rsrc(X, K * M * 2);
    const int xrow = gk * M + gm;
    if (xvec) {
      // M % 8 == 0 and gm % 8 == 0: a chunk is whole or absent
      ra0 = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
          xr, gm < M ? xrow * 2 : BUF_OOB, 0, 0));
      ra1 = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
          xr, gm + 8 < M ? (xrow + 8) * 2 : BUF_OOB, 0, 0));
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        xs[j] = __builtin_amdgcn_raw_buffer_load_b16(
            xr, gm + j < M ? (xrow + j) * 2 : BUF_OOB, 0, 0);
    }
  }
  const int hc4 = kk * 4;               // this lane's h columns
  bf16x4 hv[16];
  {
    const brsrc_t hr = buf_rsrc(ht.h, K * N * 2);
    const int hb = (hc4 < N ? hc4 * 2 : BUF_OOB) + (ks + half) * N * 2;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      hv[i] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(
          hr, hb + 2 * i * N * 2, 0, 0));
  }
  // SNAP: the snapshot's producer laid both classifier images out,
  // zero-padded (SnapJob) — four b128 chunks of the k-major one per lane
  // (the 128 live k of each class row; the pad columns are never read)
  // and one chunk of this block's 32 rows of the row image
  __bf16 wv[2][CP];
  bf16x8 wkm[4], wrow;
  if (SNAP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + j * 64;
      wkm[j] = *(const bf16x8*)&ht.w2[kSnapKmajOff + (q >> 4) * HP +
                                      (q & 15) * 8];
    }
    if (DH) wrow = *(const bf16x8*)&ht.w2[kSnapRowOff + n0 * CP + lane * 8];
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int hr = lane + q * 64;
#pragma unroll
      for (int c = 0; c < CP; ++c)
        wv[q][c] = ht.w2[(hr < N && c < C) ? hr * C + c : 0];
    }
  }
  const unsigned braw =
      __builtin_amdgcn_raw_buffer_load_b16(buf_rsrc(ht.b2, C * 2), kk * 2, 0, 0);
  // the label's low dword is all (int)label keeps; a b64 load's unused
  // high register was reused at once, behind a vmcnt(0)
  const int label = (int)__builtin_amdgcn_raw_buffer_load_b32(
      buf_rsrc(ht.labels, K * 8), (ks + kk) * 8, 0, 0);
  // each role fetches the masters it applies, and no others
  SmallSgdPre pre = {};
  float pm2[16] = {};
  float pm2bv = 0.f;
  if (APPLY) {
    if (TILE) small_sgd_fetch_buf_w(sg, pre, m0, n0, M, N, w, lane);
    if (ROLE == HT_DB1 || (ROLE == HT_ALL && blockIdx.x == 0))
      small_sgd_fetch_buf_b(sg, pre, n0, N, lane);
    if (ROLE == HT_CLS) {
      const brsrc_t w2r = buf_rsrc(sg.pm2w, N * C * 4);
      const int cb = kk < C ? kk * 4 : BUF_OOB;
#pragma unroll
      for (int v = 0; v < 16; ++v)
        pm2[v] = buf_f32(w2r, cb + (ks + head_frag_row(v, lane)) * C * 4);
      pm2bv = buf_f32(buf_rsrc(sg.pm2b, C * 4), t * 4);
    }
  }

  // 2. conversions, then the LDS images (zeros beyond B, H and C, so
  // none of them needs a separate clear pass over live data)
  if (!SNAP) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (!(lane + q * 64 < N && c < C)) wv[q][c] = (__bf16)0.f;
  }
  // beyond C: the pad bias (the load returned 0 there)
  const float bc =
      kk < C ? __builtin_bit_cast(float, braw << 16) : head_pad_bias();
  if (TILE && !xvec) {
    u32x4 d0, d1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d0[j] = xs[2 * j] | (xs[2 * j + 1] << 16);
      d1[j] = xs[8 + 2 * j] | (xs[9 + 2 * j] << 16);
    }
    ra0 = __builtin_bit_cast(bf16x8, d0);
    ra1 = __builtin_bit_cast(bf16x8, d1);
  }

  if (!SNAP) {
    const bf16x8 z8 = {};
    for (int i = lane * 8; i < CP * HP; i += 64 * 8) *(bf16x8*)&wtw[i] = z8;
    if (DH) *(bf16x8*)&wpw[lane * 8] = z8;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    *(bf16x4*)&hs[(ks + 2 * i + half) * HP + hc4] = hv[i];
  // the zero row behind the CP class rows: the B fragment of the lanes
  // of classes 16..31 (its HB live k)
  if (lane < HB / 8) *(bf16x8*)&wtw[CP * HP + lane * 8] = bf16x8{};
  if (SNAP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = lane + j * 64;
      *(bf16x8*)&wtw[(q >> 4) * HP + (q & 15) * 8] = wkm[j];
    }
    if (DH) *(bf16x8*)&wpw[lane * 8] = wrow;
  } else {
    // wtw: column hr of the [c][k] image, all CP classes (wv is zero
    // beyond C and H — the same zeros the clear put there); wpw: the
    // lane's whole row of the N tile as two b128 stores
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int hr = lane + q * 64;
#pragma unroll
      for (int c = 0; c < CP; ++c) wtw[c * HP + hr] = wv[q][c];
      if (DH && hr >= n0 && hr < n0 + 32 && hr < N) {
        bf16x8 lo, hi;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          lo[c] = wv[q][c];
          hi[c] = wv[q][8 + c];
        }
        *(bf16x8*)&wpw[(hr - n0) * CP] = lo;
        *(bf16x8*)&wpw[(hr - n0) * CP + 8] = hi;
      }
    }
  }

  // 3. logits for rows ks..ks+31 (the wave's DS pipe is in order, so
  // the fragment reads see the stores above without a barrier)
  {
    const f32x16v acc = head_logits_tile_all(
        &hs[(ks + kk) * HP], &wtw[min(kk, CP) * HP], lane);
    head_store_logits(ls, acc, ks, bc, lane);
  }
  // 4. softmax + dlogits, one lane per row; rows >= B stay zero
  if (lane < 32) {
    const int row = ks + lane;
    float neglogp = 0.f;
    if (row < K) {
      neglogp = head_softmax_row_all(&ls[row * LSP], &dls[row * CP], C, label,
                                     ht.scale);
    } else {
      // their logits are the bias, not zero
      const bf16x8 z8 = {};
      *(bf16x8*)&dls[row * CP] = z8;
      *(bf16x8*)&dls[row * CP + 8] = z8;
    }
    lsum[row] = neglogp;
  }
  // 5. dh fragment -> relu mask -> bf16 -> the k-major Bs image, where
  // commit() would have put the loaded dh (zeros beyond B and H)
  // The 16 mask values do not depend on the MFMA: they are read ahead
  // of it, in one batch (read inside the loop, each one waited for the
  // Bs store before it, which might alias it — 16 LDS round trips)
  if (DH) {
    const int colh = n0 + kk;
    __bf16 hm[16];
#pragma unroll
    for (int v = 0; v < 16; ++v)
      hm[v] = hs[(ks + head_frag_row(v, lane)) * HP + colh];
    const f32x16v acc =
        head_dh_tile(&dls[(ks + kk) * CP], &wpw[kk * CP], lane);
    wait_lgkm0();   // hm, under the MFMA: no LDS wait inside the loop
    // h > 0 alone is the mask: beyond B and H the hs image holds the
    // zeros the buffer loads returned. Row rl = 8 * (v >> 2) + 4 * half
    // + (v & 3) of the image has swizzle term (rl >> 2) & 3 = (2 * (v >>
    // 2) + half) & 3, two values per lane: two bases plus constants
    // address the lane's 16 stores (sptr(Bw, rl, kk), spelled out)
    const int sw = (kk >> 3) ^ half;
    __bf16* const bq[2] = {Bw + half * 4 * BK + (sw << 3) + (kk & 7),
                           Bw + half * 4 * BK + ((sw ^ 2) << 3) + (kk & 7)};
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const float m = (float)hm[v] > 0.f ? acc[v] : 0.f;
      const bf16_t r = f2bf(m);
      bq[(v >> 2) & 1][((v >> 2) * 8 + (v & 3)) * BK] = *(const __bf16*)&r;
    }
  }
  if (TILE) {
    *(bf16x8*)sptr(Aw, kk, half * 16) = ra0;
    *(bf16x8*)sptr(Aw, kk, half * 16 + 8) = ra1;
  }
  // 6. db1 colsum from the bf16 dh values, same partials and tree as
  // gemm_small's commit()/small_cs_reduce (grads mode below 32 tiles
  // sums serially after the barrier instead, see there)
  if (ROLE == HT_DB1 ? (APPLY || tiles >= 32)
                     : (ROLE == HT_ALL && blockIdx.x == 0)) {
    const bf16x8 rb0 = *(const bf16x8*)sptr(Bw, kk, half * 16);
    const bf16x8 rb1 = *(const bf16x8*)sptr(Bw, kk, half * 16 + 8);
    float csp[16] = {};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      csp[j] += (float)rb0[j];
      csp[8 + j] += (float)rb1[j];
    }
    small_cs_reduce(csp, csred[w], lane);
  }
  // 7. dW1 partial of this wave's K span
  if (TILE) {
    f32x4 acc[4] = {};
    if (ks < ke) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        const int ko = kh * 16 + ((lane >> 5) << 3);
        bf16x8 a = trs_frag(Aw, ko, lane);
        bf16x8 b = trs_frag(Bw, ko, lane);
        *(f32x16*)acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            a, b, *(f32x16*)acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) red[w][lane * 16 + v] = ((float*)acc)[v];
  }
  __syncthreads();
  wait_vm0();   // the prefetched masters landed a whole head ago

  constexpr bool ticketed = ROLE == HT_ALL;   // ht.ticket != null
  if (ROLE == HT_ALL) {
    if (t == 0)
      tick = __hip_atomic_fetch_add(ht.ticket, 1u, __ATOMIC_ACQ_REL,
                                    __HIP_MEMORY_SCOPE_AGENT);
    small_sgd_commit(sg, pre, red, csred, true, m0, n0, M, N, N, w, lane);
    __syncthreads();
    if (tick != gridDim.x * gridDim.y - 1) return;
    // only now known: the W2/b2 masters, all 17 loads in one batch
    // (the stores above are to W1/b1, but may alias for all the
    // compiler knows — the batch waits for them once, not per load)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int hrow = ks + head_frag_row(v, lane);
      pm2[v] = sg.pm2w[(kk < C && hrow < N) ? hrow * C + kk : 0];
    }
    pm2bv = sg.pm2b[t < C ? t : 0];
    wait_vm0();
  } else if (ROLE == HT_TILE) {
    if (APPLY) {
      small_sgd_commit(sg, pre, red, csred, false, m0, n0, M, N, N, w, lane);
    } else if (tiles >= 32) {
      if (w == 0)
        small_store(red, csred, false, nullptr, false, Cout, GF32, 0,
                    nullptr, GF32, m0, n0, M, N, N, lane);
    } else {
      // below 32 tiles gemm_bias_act runs dW1 on gemm_kernel<tn,CS>,
      // not on gemm_small_kernel: K chained through ONE 16x16x32
      // accumulator per element and a serial colsum over k (the HT_DB1
      // blocks, below). Reproduce that order from the four waves'
      // k-major images (all complete after the barrier) so grads mode
      // equals the two-kernel path bit for bit at every tile count.
      // Wave w owns one 16x16 quarter.
      const int wr = w >> 1, wc = w & 1;
      const int kfrag = (lane >> 4) * 8;
      const int kr = kfrag + ((lane & 15) >> 2);
      const int cq = 4 * (lane & 3);
      f32x4 c4 = {};
      for (int q = 0; q * 32 < K; ++q) {
        bf16x4 a0 = tr_read(sptr(As[q], kr, wr * 16 + cq));
        bf16x4 a1 = tr_read(sptr(As[q], kr + 4, wr * 16 + cq));
        bf16x4 b0 = tr_read(sptr(Bs[q], kr, wc * 16 + cq));
        bf16x4 b1 = tr_read(sptr(Bs[q], kr + 4, wc * 16 + cq));
        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7),
            __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7), c4,
            0, 0, 0);
      }
      const int col = n0 + wc * 16 + (lane & 15);
      if (col < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wr * 16 + (lane >> 4) * 4 + r;
          if (row >= M) continue;
          float v = c4[r];
          v += 0.f;                      // gemm_kernel's bias-less add
          if (GF32) ((float*)Cout)[(long)row * N + col] = v;
          else ((__bf16*)Cout)[(long)row * N + col] = (__bf16)v;
        }
      }
    }
    return;
  } else if (ROLE == HT_DB1) {
    if (APPLY) {
      if (t < 32) small_sgd_commit_b(sg, pre, csred, n0, N, t);
    } else if (tiles >= 32) {
      if (t < 32) small_store_cs(csred, colsum_out, GF32, n0, N, t);
    } else if (t < 32 && n0 + t < N) {
      float cs = 0.f;
      for (int q = 0; q * 32 < K; ++q)
#pragma unroll
        for (int k2 = 0; k2 < 32; ++k2) cs += (float)*sptr(Bs[q], k2, t);
      if (GF32) ((float*)colsum_out)[n0 + t] = cs;
      else ((__bf16*)colsum_out)[n0 + t] = (__bf16)cs;
    }
    return;
  }
  // HT_CLS: with two N tiles or more, y == 0 forms dW2 and y == 1 db2
  // and the loss, side by side; both hold the same hs and dls
  const bool do_dw2 = ROLE == HT_ALL || gridDim.y < 2 || blockIdx.y == 0;
  const bool do_db2 = ROLE == HT_ALL || gridDim.y < 2 || blockIdx.y == 1;

  // 8. classifier grads by ONE block: dW2[H,C] = h^T @ dls, K = B over
  // the eight 16-row steps, wave w owns hidden rows 32w..32w+31
  if (do_dw2) {
    f32x16v acc2 = {};
    const int kr = (lane & 15) >> 2;
    const int ca = ks + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const int cb = 4 * (lane & 3);
    const bool bzero = ((lane >> 4) & 1) != 0;   // classes 16..31
#pragma unroll
    for (int kh = 0; kh < HB / 16; ++kh) {
      const int kq = kh * 16 + ((lane >> 5) << 3) + kr;
      bf16x4 a0 = tr_read(&hs[kq * HP + ca]);
      bf16x4 a1 = tr_read(&hs[(kq + 4) * HP + ca]);
      bf16x4 b0 = tr_read(&dls[kq * CP + cb]);
      bf16x4 b1 = tr_read(&dls[(kq + 4) * CP + cb]);
      bf16x8 a = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      bf16x8 bv = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
      if (bzero) bv = bf16x8{};
      acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc2, 0, 0, 0);
    }
    if (kk < C) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int hrow = ks + head_frag_row(v, lane);
        if (hrow < N) {
          const int idx = hrow * C + kk;
          if (APPLY) {
            // bf16-rounded like the grads the head used to store
            const float pv = pm2[v] - sg.lr * bf2f(f2bf(acc2[v]));
            sg.pm2w[idx] = pv;
            sg.ps2w[idx] = f2bf(pv);
          } else if (GF32) {
            ((float*)ht.dw2)[idx] = acc2[v];
          } else {
            ((bf16_t*)ht.dw2)[idx] = f2bf(acc2[v]);
          }
        }
      }
    }
  }
  if (!do_db2) return;
  // db2[c] = sum_b dls[b][c], 16 partial lanes per class as in the head
  if (t < C * 16) {
    const int c = t >> 4, part = t & 15;
    float s = 0.f;
    for (int b2 = part; b2 < K; b2 += 16) s += (float)dls[b2 * CP + c];
    db2p[t] = s;
  }
  __syncthreads();
  if (t < C) {
    float s = 0.f;
#pragma unroll
    for (int p2 = 0; p2 < 16; ++p2) s += db2p[t * 16 + p2];
    if (APPLY) {
      const float pv = pm2bv - sg.lr * bf2f(f2bf(s));
      sg.pm2b[t] = pv;
      sg.ps2b[t] = f2bf(pv);
    } else if (GF32) {
      ((float*)ht.db2)[t] = s;
    } else {
      ((bf16_t*)ht.db2)[t] = f2bf(s);
    }
  }
  // mean loss: the head's 256-slot LDS tree (slots >= 128 are zero
  // there) replayed on wave 0 — same pairs, same order
  if (w == 0) {
    float v = (lsum[lane] + 0.f) + (lsum[lane + 64] + 0.f);
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    if (lane == 0) *ht.loss = v / K;
  }
  if (ticketed && t == 0)
    __hip_atomic_store(ht.ticket, 0u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// One role per block, chosen by scalar compares of the block index
// (roles and grid: see HT_TILE above; launch_mlp_head_tail sizes it).
template <bool APPLY, bool GF32, bool SNAP>
__global__ __launch_bounds__(256)
void mlp_head_tail_kernel(const __bf16* __restrict__ X, HeadTail ht,
                          void* __restrict__ Cout,
                          void* __restrict__ colsum_out,
                          int M, int N, int K, SmallSgd sg) {
  __shared__ HeadTailSmem sm;
  if constexpr (APPLY && !SNAP) {
    head_tail_body<APPLY, GF32, SNAP, HT_ALL>(
        sm, X, ht, Cout, colsum_out, M, N, K, sg, gridDim.x * gridDim.y);
  } else {
    const int mt = gridDim.x - 2;
    const int tiles = mt * gridDim.y;
    if ((int)blockIdx.x < mt)
      head_tail_body<APPLY, GF32, SNAP, HT_TILE>(
          sm, X, ht, Cout, colsum_out, M, N, K, sg, tiles);
    else if ((int)blockIdx.x == mt)
      head_tail_body<APPLY, GF32, SNAP, HT_DB1>(
          sm, X, ht, Cout, colsum_out, M, N, K, sg, tiles);
    else if (blockIdx.y < 2)
      head_tail_body<APPLY, GF32, SNAP, HT_CLS>(
          sm, X, ht, Cout, colsum_out, M, N, K, sg, tiles);
  }
}

// split-K phase 2 fused with the SGD apply (the NMF factor update):
// instead of materializing the fp32 gradient and re-reading it in a
// separate apply kernel, the stripe sum feeds p -= lr*(gscale*g +
// nd*min(p,0)) and the bf16 shadow refresh directly.
__global__ __launch_bounds__(256)
void splitk_reduce_sgd_kernel(const float* __restrict__ ws, int nslice,
                              float* __restrict__ p,
                              __bf16* __restrict__ shadow, long mn,
                              float lr, float gscale, float nd) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= mn) return;
  const bool vec4 = stripes_vec4(ws, mn);
  f32x4 v = {};
  for (int z = 0; z < nslice; ++z) {
    const float* sp = ws + (long)z * mn + i0;
    if (vec4) {
      const f32x4 sv = *(const f32x4*)sp;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += sv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < mn) v[j] += sp[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = i0 + j;
    if (i >= mn) break;
    float pv = p[i];
    float g = gscale * v[j];
    if (nd != 0.f) g += nd * fminf(pv, 0.f);
    pv -= lr * g;
    p[i] = pv;
    if (shadow != nullptr) shadow[i] = (__bf16)pv;
  }
}

}  // namespace

// last-arriver epilogue: MEASURED DEAD END on the mnist fwd shape
// (4 tiles x 9 slices): the 4 consumer blocks pull the stripes
// cross-XCD through the release/acquire fences and the fwd GEMM
// went 8.2 -> 48 us scalar / ~20 us vectorized, vs 12.9 us for
// stripes + the wide reduce kernel. Same lesson as the FROMWS head:
// few-WG consumers must not read many-XCD-producer output. Kept
// behind TFA_GEMM_LA=1 for re-measurement; default off.
bool gemm_last_arriver(int M, int N, bool colsum, int act) {
  static int la_on = -1;
  if (la_on < 0) {
    const char* e = getenv("TFA_GEMM_LA");
    la_on = e ? atoi(e) : 0;
  }
  return la_on && !colsum && act <= 1 &&
         (long)ceil_div(N, BN) * ceil_div(M, BM) <= 64;
}

// stripe reduce of SMALL outputs: 1 elem/thread (see
// splitk_reduce_small_kernel), else 4
bool gemm_reduce_small(long mn) { return mn <= (1 << 16); }

void launch_gemm(const bf16_t* A, const bf16_t* B, const void* bias,
                 bool bias_bf16, void* C, bool out_f32, const bf16_t* aux,
                 void* colsum_out, float* ws, int* cnt, int kc, int nslice,
                 int M, int N, int K, int lda, int ldb, int ldc, bool ta,
                 bool tb, int act, int veca, int vecb, hipStream_t stream,
                 const SnapArgs* snap, bool* snap_taken) {
  // snap: side copy for the next launch, done only where the small
  // stripe reduce runs; *snap_taken tells the caller whether it was
  SnapJob sj = {};
  if (snap_taken) *snap_taken = false;
  const bool sk = nslice > 1;
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), sk ? nslice : 1);
  dim3 block(256);
  const bool has_bias = bias != nullptr;
  const bool cs = colsum_out != nullptr;
  const int rflags = (act == 1 ? 1 : 0) | (out_f32 ? 2 : 0) |
                     (has_bias ? 4 : 0);
  if (!gemm_last_arriver(M, N, cs, act)) cnt = nullptr;
#define LAUNCH(TAv, TBv, ACTv, BIASv, OUTv, SKv, CSv)                       \
  hipLaunchKernelGGL((gemm_kernel<TAv, TBv, ACTv, BIASv, OUTv, SKv, CSv>),  \
                     grid, block, 0, stream, (const __bf16*)A,              \
                     (const __bf16*)B, bias, bias_bf16, C,                  \
                     (const __bf16*)aux, colsum_out, ws, cnt, M, N, K, lda, \
                     ldb, ldc, kc, veca, vecb, rflags)
  // constraint combos (relu_bwd only nt/bf16, colsum only tn) are
  // validated by the bindings in ext.hip
  if (act == 2) {
    LAUNCH(false, true, 2, false, false, false, false);
    return;
  }
  if (act == 3) {   // out = A@B - aux (nn, bf16 out; binding-gated)
    LAUNCH(false, false, 3, false, false, false, false);
    return;
  }
  if (cs && !sk) {
    if (out_f32) LAUNCH(true, false, 0, false, true, false, true);
    else         LAUNCH(true, false, 0, false, false, false, true);
    return;
  }
  if (cs && sk) {
    // phase 1: tn with per-slice output AND colsum partials; phase 2
    // reduces both. cs_part lives at ws + mn*nslice (sized by binding)
    const long mn = (long)M * ldc;
    float* cs_part = ws + mn * nslice;
    void* user_cs = colsum_out;
    colsum_out = cs_part;    // phase 1 writes the partials
    LAUNCH(true, false, 0, false, false, true, true);
    colsum_out = user_cs;
    dim3 rgrid((unsigned)(((mn + 3) / 4 + 255) / 256)), rblock(256);
    if (out_f32)
      hipLaunchKernelGGL((splitk_reduce_kernel<0, false, true>), rgrid,
                         rblock, 0, stream, ws, nullptr, false, C, mn, ldc,
                         nslice, cs_part, colsum_out, out_f32, N);
    else
      hipLaunchKernelGGL((splitk_reduce_kernel<0, false, false>), rgrid,
                         rblock, 0, stream, ws, nullptr, false, C, mn, ldc,
                         nslice, cs_part, colsum_out, out_f32, N);
    return;
  }
  if (sk) {
    // phase 1: partials (epilogue template args unused in SK stores);
    // all four transpose combos (deep-K BACKWARD shapes with small
    // tile grids — e.g. NMF dW [1000,200,k=1000] — were 1 wave/SIMD
    // and LDS-latency-bound without slicing)
    if (ta) { if (tb) LAUNCH(true, true, 0, false, false, true, false);
              else    LAUNCH(true, false, 0, false, false, true, false); }
    else    { if (tb) LAUNCH(false, true, 0, false, false, true, false);
              else    LAUNCH(false, false, 0, false, false, true, false); }
    if (cnt != nullptr) return;   // last-arriver epilogue ran in-kernel
    // phase 2: fixed-order stripe reduce + fused epilogue (small
    // outputs: 1 elem/thread for 4x the workgroups)
    const long mn = (long)M * ldc;
    const bool small_r = gemm_reduce_small(mn);
    dim3 rgrid((unsigned)(small_r ? (mn + 255) / 256
                                  : ((mn + 3) / 4 + 255) / 256));
    dim3 rblock(256);
    if (small_r && snap != nullptr) {
      sj.s0 = (const __bf16*)snap->s0; sj.s1 = (const __bf16*)snap->s1;
      sj.dst = (__bf16*)snap->dst;
      sj.n0 = snap->n0; sj.n1 = snap->n1; sj.off1 = snap->off1;
      sj.rows = snap->rows; sj.cols = snap->cols;
      if (snap_taken) *snap_taken = true;
    }
#define RLAUNCH(ACTv, BIASv, OUTv)                                          \
    do { if (small_r)                                                       \
      hipLaunchKernelGGL((splitk_reduce_small_kernel<ACTv, BIASv, OUTv>),   \
                         rgrid, rblock, 0, stream, ws, bias, bias_bf16, C,  \
                         mn, ldc, nslice, sj);                              \
    else                                                                    \
      hipLaunchKernelGGL((splitk_reduce_kernel<ACTv, BIASv, OUTv>), rgrid,  \
                         rblock, 0, stream, ws, bias, bias_bf16, C, mn,     \
                         ldc, nslice, (const float*)nullptr,                \
                         (void*)nullptr, false, 0);                         \
    } while (0)
    if (act == 1) {
      if (has_bias) { if (out_f32) RLAUNCH(1, true, true);
                      else RLAUNCH(1, true, false); }
      else          { if (out_f32) RLAUNCH(1, false, true);
                      else RLAUNCH(1, false, false); }
    } else {
      if (has_bias) { if (out_f32) RLAUNCH(0, true, true);
                      else RLAUNCH(0, true, false); }
      else          { if (out_f32) RLAUNCH(0, false, true);
                      else RLAUNCH(0, false, false); }
    }
#undef RLAUNCH
    return;
  }
#define DISP_OUT(TAv, TBv, ACTv, BIASv)                                     \
  do { if (out_f32) LAUNCH(TAv, TBv, ACTv, BIASv, true, false, false);      \
       else LAUNCH(TAv, TBv, ACTv, BIASv, false, false, false); } while (0)
#define DISP_BIAS(TAv, TBv, ACTv)                                           \
  do { if (has_bias) DISP_OUT(TAv, TBv, ACTv, true);                        \
       else DISP_OUT(TAv, TBv, ACTv, false); } while (0)
#define DISP_ACT(TAv, TBv)                                                  \
  do { if (act == 1) DISP_BIAS(TAv, TBv, 1); else DISP_BIAS(TAv, TBv, 0); } while (0)
  if (ta) { if (tb) DISP_ACT(true, true); else DISP_ACT(true, false); }
  else    { if (tb) DISP_ACT(false, true); else DISP_ACT(false, false); }
#undef DISP_ACT
#undef DISP_BIAS
#undef DISP_OUT
#undef LAUNCH
}

// one-launch split-K forward (see gemm_fwd1_kernel). variant < 0: the
// shipped geometry; else bits 0-1 pick the tile (0 16x16, 1 16x32,
// 2 32x16, 3 32x32) and bit 2 forces the strided B load — kept for the
// microbenchmark. Shape limits are checked by the binding.
void launch_gemm_fwd1(const bf16_t* A, const bf16_t* B, const void* bias,
                      bool bias_bf16, void* C, bool out_f32, int relu,
                      int kc, int nslice, int M, int N, int K, int lda,
                      int ldb, int ldc, int veca, int vecb, int variant,
                      const SnapArgs* snap, bool* snap_taken,
                      hipStream_t stream) {
  SnapJob sj = {};
  if (snap != nullptr) {
    sj.s0 = (const __bf16*)snap->s0; sj.s1 = (const __bf16*)snap->s1;
    sj.dst = (__bf16*)snap->dst;
    sj.n0 = snap->n0; sj.n1 = snap->n1; sj.off1 = snap->off1;
    sj.rows = snap->rows; sj.cols = snap->cols;
  }
  if (snap_taken) *snap_taken = snap != nullptr;
  if (variant < 0) variant = kFwd1Tile;
  // A b128 per lane: 16B-aligned rows and no ragged k chunk; B dword-
  // aligned row chunks: even pitch and an even number of live columns
  const bool va = veca == 8 && K % 8 == 0;
  const bool vb = vecb >= 2 && N % 2 == 0 && N >= 8 && !(variant & 4);
  dim3 block(64 * nslice);
#define F1V(TMv, TNv, VAv, VBv)                                             \
  hipLaunchKernelGGL((gemm_fwd1_kernel<TMv, TNv, VAv, VBv>),                \
                     dim3(ceil_div(N, TNv), ceil_div(M, TMv)), block,       \
                     (nslice * (Fwd1Geo<TMv, TNv>::WAVE_BYTES)), stream,    \
                     (const __bf16*)A, (const __bf16*)B, bias, bias_bf16,   \
                     C, out_f32, relu, M, N, K, lda, ldb, ldc, kc, sj)
#define F1(TMv, TNv)                                                        \
  do { if (va) { if (vb) F1V(TMv, TNv, true, true);                         \
                 else F1V(TMv, TNv, true, false); }                         \
       else    { if (vb) F1V(TMv, TNv, false, true);                        \
                 else F1V(TMv, TNv, false, false); } } while (0)
  switch (variant & 3) {
    case 0: F1(16, 16); break;
    case 1: F1(16, 32); break;
    case 2: F1(32, 16); break;
    default: F1(32, 32); break;
  }
#undef F1
#undef F1V
}

// split-K phase 1 ONLY: store the fp32 partial stripes and return —
// the caller fuses the stripe reduction into a consumer kernel (the
// mnist fused head reduces them while staging h into LDS, so h never
// exists in global memory and the reduce launch disappears).

void launch_gemm_small(const bf16_t* A, const bf16_t* B, const void* bias,
                       bool bias_bf16, void* C, bool out_f32, int relu,
                       void* colsum_out, bool cs_f32, int M, int N, int K,
                       int lda, int ldb, int ldc, bool ta, int veca,
                       int vecb, const SmallSgdArgs* sga,
                       hipStream_t stream) {
  dim3 grid(ceil_div(M, 32), ceil_div(N, 32)), block(256);
  SmallSgd sg = {};
  if (sga) {
    sg.pmw = sga->pmw; sg.psw = (bf16_t*)sga->psw;
    sg.pmb = sga->pmb; sg.psb = (bf16_t*)sga->psb;
    sg.g2w = (const bf16_t*)sga->g2w;
    sg.pm2w = sga->pm2w; sg.ps2w = (bf16_t*)sga->ps2w;
    sg.g2b = (const bf16_t*)sga->g2b;
    sg.pm2b = sga->pm2b; sg.ps2b = (bf16_t*)sga->ps2b;
    sg.lr = sga->lr; sg.n2w = sga->n2w; sg.n2b = sga->n2b;
  }
  const bool cs = colsum_out != nullptr || sg.pmb != nullptr;
#define GS(TAv, CSv)                                                        \
  hipLaunchKernelGGL((gemm_small_kernel<TAv, CSv>), grid, block, 0,         \
                     stream, (const __bf16*)A, (const __bf16*)B, bias,      \
                     bias_bf16, C, out_f32, relu, colsum_out, cs_f32, M, N, \
                     K, lda, ldb, ldc, veca, vecb, sg)
  if (ta) { if (cs) GS(true, true); else GS(true, false); }
  else    { if (cs) GS(false, true); else GS(false, false); }
#undef GS
}

// fused head + tail (see mlp_head_tail_kernel). sga != null: APPLY
// (plain-SGD step, bf16-rounded classifier grads); else dW1/db1 and
// dW2/db2 are stored in the grad dtype. Shape limits are checked by
// the bindings.
void launch_mlp_head_tail(const bf16_t* x, const HeadTailArgs* hta,
                          void* dw1, void* db1, bool grads_f32, int M,
                          int H, int B, const SmallSgdArgs* sga,
                          hipStream_t stream) {
  // two more rows of blockIdx.x for the db1 and classifier roles; the
  // ticket instantiation runs on the tiles alone
  const bool roles = !(sga && hta->ticket != nullptr);
  dim3 grid(ceil_div(M, 32) + (roles ? 2 : 0), ceil_div(H, 32)), block(256);
  HeadTail ht;
  ht.h = (const __bf16*)hta->h;
  ht.w2 = (const __bf16*)hta->w2;
  ht.b2 = (const bf16_t*)hta->b2;
  ht.labels = hta->labels;
  ht.loss = hta->loss;
  ht.dw2 = hta->dw2;
  ht.db2 = hta->db2;
  ht.ticket = hta->ticket;
  ht.scale = hta->scale;
  ht.C = hta->C;
  SmallSgd sg = {};
  if (sga) {
    sg.pmw = sga->pmw; sg.psw = (bf16_t*)sga->psw;
    sg.pmb = sga->pmb; sg.psb = (bf16_t*)sga->psb;
    sg.pm2w = sga->pm2w; sg.ps2w = (bf16_t*)sga->ps2w;
    sg.pm2b = sga->pm2b; sg.ps2b = (bf16_t*)sga->ps2b;
    sg.lr = sga->lr; sg.n2w = sga->n2w; sg.n2b = sga->n2b;
    if (ht.ticket == nullptr)
      hipLaunchKernelGGL((mlp_head_tail_kernel<true, false, true>), grid,
                         block, 0, stream, (const __bf16*)x, ht, nullptr,
                         nullptr, M, H, B, sg);
    else
      hipLaunchKernelGGL((mlp_head_tail_kernel<true, false, false>), grid,
                         block, 0, stream, (const __bf16*)x, ht, nullptr,
                         nullptr, M, H, B, sg);
  } else if (grads_f32) {
    hipLaunchKernelGGL((mlp_head_tail_kernel<false, true, false>), grid,
                       block, 0, stream, (const __bf16*)x, ht, dw1, db1, M, H,
                       B, sg);
  } else {
    hipLaunchKernelGGL((mlp_head_tail_kernel<false, false, false>), grid,
                       block, 0, stream, (const __bf16*)x, ht, dw1, db1, M, H,
                       B, sg);
  }
}


// phase-1-only split-K stripes for ANY transpose combo (the fused
// GEMM->SGD path reduces them with splitk_reduce_sgd_kernel)
void launch_gemm_stripes_any(const bf16_t* A, const bf16_t* B, float* ws,
                             int kc, int nslice, int M, int N, int K,
                             int lda, int ldb, int ldc, bool ta, bool tb,
                             int veca, int vecb, hipStream_t stream) {
  const long Mtiles = ((long)M + BM - 1) / BM;
  dim3 grid((unsigned)ceil_div(N, BN), (unsigned)Mtiles, nslice);
  dim3 block(256);
#define SLAUNCH(TAv, TBv)                                                   \
  hipLaunchKernelGGL((gemm_kernel<TAv, TBv, 0, false, false, true, false>), \
                     grid, block, 0, stream, (const __bf16*)A,              \
                     (const __bf16*)B, nullptr, false, nullptr, nullptr,    \
                     nullptr, ws, nullptr, M, N, K, lda, ldb, ldc, kc, veca,\
                     vecb, 0)
  if (ta) { if (tb) SLAUNCH(true, true); else SLAUNCH(true, false); }
  else    { if (tb) SLAUNCH(false, true); else SLAUNCH(false, false); }
#undef SLAUNCH
}

void launch_splitk_reduce_sgd(const float* ws, int nslice, float* p,
                              bf16_t* shadow, long mn, float lr,
                              float gscale, float nd, hipStream_t stream) {
  dim3 rgrid((unsigned)(((mn + 3) / 4 + 255) / 256)), rblock(256);
  hipLaunchKernelGGL(splitk_reduce_sgd_kernel, rgrid, rblock, 0, stream,
                     ws, nslice, p, (__bf16*)shadow, mn, lr, gscale, nd);
}

void launch_gemm_stripes(const bf16_t* A, const bf16_t* B, float* ws,
                         int kc, int nslice, int M, int N, int K, int lda,
                         int ldb, int ldc, int veca, int vecb,
                         hipStream_t stream) {
  dim3 grid(ceil_div(N, BN), ceil_div(M, BM), nslice);
  dim3 block(256);
  hipLaunchKernelGGL((gemm_kernel<false, false, 0, false, false, true,
                                  false>),
                     grid, block, 0, stream, (const __bf16*)A,
                     (const __bf16*)B, nullptr, false, nullptr, nullptr,
                     nullptr, ws, nullptr, M, N, K, lda, ldb, ldc, kc,
                     veca, vecb, 0);
}

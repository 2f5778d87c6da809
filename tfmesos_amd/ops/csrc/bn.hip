// Fused train-mode batch-norm (+ReLU) for channels-last bf16 activations.
//
// The Inception blocks are conv -> BN -> relu; profiling the torch
// fallback (profiles/r01_inception_n1_kernel_stats.txt) showed the BN
// tensor-math soup (fp32 casts + separate mean/var/normalize/affine/relu
// kernels) at ~36% of the training step. The activation layout is the
// conv kernels' channels-last ([P, C] with P = N*H*W pixels, channels
// innermost), so every wave reads 64 consecutive channels — perfectly
// coalesced. Three kernels per direction:
//
//   fwd: stats-partial (no atomics -> per-slice partials)
//        -> finalize (mean/invstd) -> apply (normalize+affine+ReLU)
//   bwd: stats-partial (sum dy_eff, sum dy_eff*xhat; ReLU mask y>0
//        fused) -> finalize (dgamma/dbeta + normalized sums) -> apply
//        (dx in one pass)
//
// and three families of them, which differ in how threads walk [P, C]
// and in nothing else: column-walk / flat-walk (any C), row-wise
// (C % 8 == 0, constants in registers) and grouped (several branches in
// one launch). bn_plan() picks the family; the arithmetic of an element
// and every reduce is written once, in the rule section below.
#include "common.h"
#include "bn.h"

namespace {

constexpr int MAXC = 2048;   // LDS scale/shift staging bound (40 KB worst case)

// magic division for the flat-index -> channel decode of the flat-walk
// kernels (see conv.hip for the derivation); exact for x < 2^31, which
// the bindings check
struct FDiv {
  unsigned long long m;
  int s;
};
inline FDiv make_fd(int d) {
  FDiv f;
  int L = 0;
  while ((1LL << L) < d) ++L;
  f.s = 31 + L;
  f.m = ((1ULL << f.s) + d - 1) / d;
  return f;
}
DEVINL unsigned fd(unsigned x, FDiv f) {
  return (unsigned)(((unsigned long long)x * f.m) >> f.s);
}

DEVINL bf16x8 ld8(const __bf16* p) { return *(const bf16x8*)p; }
DEVINL void st8(__bf16* p, bf16x8 v) { *(bf16x8*)p = v; }

// ------------------------------------------------------------------ the rule
//
// One channel's constants, and the element math of both directions:
//   y  = bf16(x*sc + sh), relu applied before the rounding
//   dx = bf16(sc * (dy_eff - a - xhat*bb)),  xhat = (x - mu)*is
// dy_eff is dy, or 0 where the forward stored y <= 0. That mask is
// recomputed instead of reading the y stream (one fewer full activation
// read): bn_relu_dead calls the forward element itself, so it is
// bit-exact with what the forward produced.
struct BnCh {
  float sc, sh;   // g*invstd, b - mean*sc
  float mu, is;   // mean, invstd
  float a, bb;    // backward: sum(dy_eff)/count, sum(dy_eff*xhat)/count
};

// g/b/mean/invstd/s1n/s2n point at the branch's channel 0; s1n/s2n are
// read only if BWD (the backward applies)
template <bool BWD>
DEVINL BnCh bn_ch(const __bf16* g, const __bf16* b, const float* mean,
                  const float* invstd, const float* s1n, const float* s2n,
                  int c) {
  BnCh k;
  k.mu = mean[c];
  k.is = invstd[c];
  k.sc = (float)g[c] * k.is;
  k.sh = (float)b[c] - k.mu * k.sc;
  k.a = BWD ? s1n[c] : 0.f;
  k.bb = BWD ? s2n[c] : 0.f;
  return k;
}

template <bool RELU>
DEVINL __bf16 bn_fwd_elem(float x, const BnCh& k) {
  float f = x * k.sc + k.sh;
  if (RELU) f = f > 0.f ? f : 0.f;
  return (__bf16)f;
}

DEVINL bool bn_relu_dead(float x, const BnCh& k) {
  return (float)bn_fwd_elem<false>(x, k) <= 0.f;
}

template <bool RELU>
DEVINL float bn_dy_eff(float x, float dy, const BnCh& k) {
  return RELU && bn_relu_dead(x, k) ? 0.f : dy;
}

DEVINL float bn_xhat(float x, const BnCh& k) { return (x - k.mu) * k.is; }

template <bool RELU>
DEVINL __bf16 bn_dx_elem(float x, float dy, const BnCh& k) {
  const float d = bn_dy_eff<RELU>(x, dy, k);
  return (__bf16)(k.sc * (d - k.a - bn_xhat(x, k) * k.bb));
}

// bf16x8 forms: k[c0 + j] is channel j's constants — a BnCh[8] in
// registers (c0 = 0) or a BnChLds
template <bool RELU, class K>
DEVINL bf16x8 bn_fwd_x8(bf16x8 x, const K& k, int c0 = 0) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = bn_fwd_elem<RELU>((float)x[j], k[c0 + j]);
  return o;
}

template <bool RELU, class K>
DEVINL bf16x8 bn_dx_x8(bf16x8 x, bf16x8 dy, const K& k, int c0 = 0) {
  bf16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = bn_dx_elem<RELU>((float)x[j], (float)dy[j], k[c0 + j]);
  return o;
}

// per-channel constants of up to N channels staged in LDS by a 256-thread
// block (the flat-walk kernels), one array per constant: sc, then the
// four backward-only ones if BWD, then sh if SH (the backward needs it
// for the relu mask alone)
template <int N, bool BWD, bool SH>
struct BnChLds {
  static constexpr int kSh = BWD ? 5 : 1;
  float v[kSh + (SH ? 1 : 0)][N];

  DEVINL void stage(const __bf16* g, const __bf16* b, const float* mean,
                    const float* invstd, const float* s1n, const float* s2n,
                    int C) {
    for (int c = threadIdx.x; c < C; c += 256) {
      const BnCh k = bn_ch<BWD>(g, b, mean, invstd, s1n, s2n, c);
      v[0][c] = k.sc;
      if constexpr (BWD) {
        v[1][c] = k.mu;
        v[2][c] = k.is;
        v[3][c] = k.a;
        v[4][c] = k.bb;
      }
      if constexpr (SH) v[kSh][c] = k.sh;
    }
    __syncthreads();
  }
  DEVINL BnCh operator[](int c) const {
    BnCh k = {v[0][c], 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (SH) k.sh = v[kSh][c];
    if constexpr (BWD) {
      k.mu = v[1][c];
      k.is = v[2][c];
      k.a = v[3][c];
      k.bb = v[4][c];
    }
    return k;
  }
};

// ---- column-walk: block 256 = 64 channel lanes x 4 pixel rows, slice z of Z

// sum and sum of squares of channel c over this thread's rows; 4 rows
// in flight per thread: these are independent strided loads and the
// kernel is latency-bound without the explicit MLP
DEVINL void bn_col_stats(const __bf16* __restrict__ x, long P, int C, int c,
                         int z, int Z, float& sum, float& sq) {
  const long step = (long)Z * 4;
  long p = (long)z * 4 + (threadIdx.x >> 6);
  for (; p + 3 * step < P; p += 4 * step) {
    const float v0 = (float)x[p * C + c];
    const float v1 = (float)x[(p + step) * C + c];
    const float v2 = (float)x[(p + 2 * step) * C + c];
    const float v3 = (float)x[(p + 3 * step) * C + c];
    sum += v0 + v1 + v2 + v3;
    sq += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
  }
  for (; p < P; p += step) {
    const float v = (float)x[p * C + c];
    sum += v;
    sq += v * v;
  }
}

// sum dy_eff and sum dy_eff*xhat of channel c over rows p, p + step, ...
template <bool RELU>
DEVINL void bn_col_bwd_rows(const __bf16* __restrict__ x,
                            const __bf16* __restrict__ dy, long ldy,
                            const BnCh& k, long P, int C, int c, long step,
                            long p, float& s1, float& s2) {
  for (; p < P; p += step) {
    const float xv = (float)x[p * C + c];
    const float d = bn_dy_eff<RELU>(xv, (float)dy[p * ldy + c], k);
    s1 += d;
    s2 += d * bn_xhat(xv, k);
  }
}

// fold the block's 4 pixel rows through LDS; row 0 of a live channel
// writes the pair to part[slot] ([z][c] layout: slot = z*Ctot + c)
DEVINL void bn_col_fold(float s, float q, float* __restrict__ part,
                        long slot, bool live) {
  const int cl = threadIdx.x & 63;
  const int pr = threadIdx.x >> 6;
  __shared__ float ls[4][64], lq[4][64];
  ls[pr][cl] = s;
  lq[pr][cl] = q;
  __syncthreads();
  if (pr == 0 && live) {
    part[slot * 2] = ls[0][cl] + ls[1][cl] + ls[2][cl] + ls[3][cl];
    part[slot * 2 + 1] = lq[0][cl] + lq[1][cl] + lq[2][cl] + lq[3][cl];
  }
}

// ---- finalize: one block of NT threads per channel sums its Z partials

DEVINL float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// NT = 64: one wave per channel over the [z][c] partials of the
// column-walk stats (a single-workgroup loop over Z was latency-bound at
// ~28 us). NT = 256: the [c][z] partials of the row-wise stats, lanes
// stride z coalesced (Z can be 2048, so a whole block per channel keeps
// enough loads in flight). The sums are valid in thread 0.
template <int NT>
DEVINL void bn_sum_parts(const float* __restrict__ part, int c, int C, int Z,
                         float& s, float& q) {
  const int t = threadIdx.x;
  s = q = 0.f;
  for (int z = t; z < Z; z += NT) {
    const long slot = NT == 64 ? (long)z * C + c : (long)c * Z + z;
    s += part[slot * 2];
    q += part[slot * 2 + 1];
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if (NT > 64) {
    __shared__ float ls[4], lq[4];
    if ((t & 63) == 0) {
      ls[t >> 6] = s;
      lq[t >> 6] = q;
    }
    __syncthreads();
    if (t == 0) {
      s = ls[0] + ls[1] + ls[2] + ls[3];
      q = lq[0] + lq[1] + lq[2] + lq[3];
    }
  }
}

// ---- row-wise: thread = one 8-channel octet u x one row lane rl

struct RwIdx {
  int tpr;   // threads per row = C/8
  int rpb;   // rows per block
  int u, rl, c0;
};
__host__ __device__ inline int rw_rpb(int C) {
  return 256 / (C >> 3) < 1 ? 1 : 256 / (C >> 3);
}
DEVINL RwIdx rw_idx(int C) {
  RwIdx i;
  i.tpr = C >> 3;
  i.rpb = rw_rpb(C);
  i.u = (int)(threadIdx.x % i.tpr);
  i.rl = (int)(threadIdx.x / i.tpr);
  i.c0 = i.u * 8;
  return i;
}

template <bool BWD>
DEVINL void rw_load_ch(BnCh (&k)[8], const __bf16* g, const __bf16* b,
                       const float* mean, const float* invstd,
                       const float* s1n, const float* s2n, int c0) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
    k[j] = bn_ch<BWD>(g, b, mean, invstd, s1n, s2n, c0 + j);
}

// cross-row tree reduce of one 8-float array through red[256 * 8]
// (log2(rpb) rounds, all rows participating — a serial per-thread loop
// here left tpr of 256 lanes active and dominated the big-layer
// kernels). Row lane 0 ends with the block's sums in v; the caller puts
// a barrier before it reuses red.
// KNOWN DEFECT, kept as it was: when cur is odd, row `half` is both a
// source (for row 0) and a destination (of row cur-1) in the same
// round, and it stays in the next round's range, so rows are counted
// twice whenever rpb is no power of two (C/8 = 6, 12, 24, ...: mean and
// invstd come out wrong, e.g. C = 48 at 104 x 104). The fold should add
// row rl + (cur - half) for rl < half; that changes what the Inception
// model computes and is left to a change of its own.
DEVINL void bn_rw_reduce(float (&v)[8], float* red, const RwIdx& i) {
#pragma unroll
  for (int j = 0; j < 8; ++j) red[threadIdx.x * 8 + j] = v[j];
  __syncthreads();
  for (int cur = i.rpb; cur > 1;) {
    const int half = cur >> 1;
    if (i.rl < cur - half) {   // fold rows [half, cur) onto [0, cur-half)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        red[threadIdx.x * 8 + j] += red[((i.rl + half) * i.tpr + i.u) * 8 + j];
    }
    __syncthreads();
    cur -= half;
  }
  if (i.rl == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = red[i.u * 8 + j];
  }
}

// reduce both arrays and write slice z's channel-major partials
// ([c][z]{s, q}, so the finalize lanes read CONSECUTIVE z)
DEVINL void bn_rw_fold(float (&s)[8], float (&q)[8],
                       float* __restrict__ part, const RwIdx& i, int z,
                       int Z) {
  __shared__ float red[256 * 8];
  bn_rw_reduce(s, red, i);
  __syncthreads();
  bn_rw_reduce(q, red, i);
  if (i.rl == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      part[((long)(i.c0 + j) * Z + z) * 2] = s[j];
      part[((long)(i.c0 + j) * Z + z) * 2 + 1] = q[j];
    }
  }
}

// ---- grouped: per-branch pointers ride a kernel argument
//
// One launch per phase for ALL terminal BNs of an Inception block
// (A/C/E blocks end in 4-6 independent conv->BN branches writing one
// concat buffer): grid.y (or a channel-block table) selects the branch.
// BN is per-channel, so the grouped result is IDENTICAL to separate
// per-branch BNs — only the launch count changes (6 kernels per
// BRANCH chain -> 6 per BLOCK; the per-kernel execution floor at
// these layer sizes made launch count the dominant BN cost).
constexpr int BNG_MAX = 8;
constexpr int BNG_MAXC = 512;   // per-branch LDS staging bound

struct BNGroupArgs {
  const __bf16* x[BNG_MAX];    // per-branch pre-BN conv output [P, C_b]
  const __bf16* dy[BNG_MAX];   // bwd: per-branch dy base
  long dyld[BNG_MAX];          // bwd: per-branch dy row stride
  __bf16* dx[BNG_MAX];         // bwd: per-branch dx out [P, C_b]
  __bf16* y[BNG_MAX];          // fwd: per-branch out base
  long yld[BNG_MAX];           // fwd: per-branch out row stride
  const __bf16* g[BNG_MAX];
  const __bf16* b[BNG_MAX];
  int C[BNG_MAX];
  int coff[BNG_MAX];           // channel offset within the group
  int cb0[BNG_MAX];            // first 64-wide channel block index
  FDiv dC[BNG_MAX];            // magic divide by C (flat-walk decode)
  int n;
};

DEVINL int bng_branch(const BNGroupArgs& a, int cb) {
  int br = 0;
  for (int i = 1; i < BNG_MAX; ++i)
    if (i < a.n && cb >= a.cb0[i]) br = i;
  return br;
}

// ------------------------------------------------------------------ kernels

// grid (ceil(C/64), Z)
__global__ __launch_bounds__(256)
void bn_stats_kernel(const __bf16* __restrict__ x, float* __restrict__ part,
                     long P, int C, int Z) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int z = blockIdx.y;
  float sum = 0.f, sq = 0.f;
  if (c < C) bn_col_stats(x, P, C, c, z, Z, sum, sq);
  bn_col_fold(sum, sq, part, (long)z * C + c, c < C);
}

// grid (cbtot, Z); the grouped layers are the small-P blocks where the
// column-walk granularity wins — see bn_plan
__global__ __launch_bounds__(256)
void bng_stats_kernel(BNGroupArgs a, float* __restrict__ part,
                      long P, int Ctot, int Z) {
  const int br = bng_branch(a, blockIdx.x);
  const int C = a.C[br];
  const int c = (blockIdx.x - a.cb0[br]) * 64 + (threadIdx.x & 63);
  const int z = blockIdx.y;
  float sum = 0.f, sq = 0.f;
  if (c < C) bn_col_stats(a.x[br], P, C, c, z, Z, sum, sq);
  bn_col_fold(sum, sq, part, (long)z * Ctot + a.coff[br] + c, c < C);
}

// grid (C); RW selects the partial layout and the block size
template <bool RW>
__global__ __launch_bounds__(RW ? 256 : 64)
void bn_finalize_kernel(const float* __restrict__ part,
                        float* __restrict__ mean,
                        float* __restrict__ invstd,
                        int C, int Z, float inv_count, float eps) {
  const int c = blockIdx.x;
  float s, q;
  bn_sum_parts<RW ? 256 : 64>(part, c, C, Z, s, q);
  if (threadIdx.x == 0) {
    const float m = s * inv_count;
    float var = q * inv_count - m * m;
    if (var < 0.f) var = 0.f;
    mean[c] = m;
    invstd[c] = __frsqrt_rn(var + eps);
  }
}

template <bool RW>
__global__ __launch_bounds__(RW ? 256 : 64)
void bn_bwd_finalize_kernel(const float* __restrict__ part,
                            __bf16* __restrict__ dgamma,
                            __bf16* __restrict__ dbeta,
                            float* __restrict__ s1n,
                            float* __restrict__ s2n,
                            int C, int Z, float inv_count) {
  const int c = blockIdx.x;
  float s1, s2;
  bn_sum_parts<RW ? 256 : 64>(part, c, C, Z, s1, s2);
  if (threadIdx.x == 0) {
    dbeta[c] = (__bf16)s1;
    dgamma[c] = (__bf16)s2;
    s1n[c] = s1 * inv_count;
    s2n[c] = s2 * inv_count;
  }
}

// Flat walk for C % 8 != 0: 8 consecutive elements per thread, which may
// straddle a row end. STRIDED: y is a channel-narrow view of a wider
// channels-last tensor (leading dim ldo > C) — the Inception block
// writes each branch's BN output straight into its slice of the
// pre-allocated concat buffer, eliminating the aten cat copy per block.
template <bool RELU, bool STRIDED>
__global__ __launch_bounds__(256)
void bn_apply_kernel(const __bf16* __restrict__ x,
                     const float* __restrict__ mean,
                     const float* __restrict__ invstd,
                     const __bf16* __restrict__ g, const __bf16* __restrict__ b,
                     __bf16* __restrict__ y, long ldo, FDiv dC,
                     long P, int C) {
  __shared__ BnChLds<MAXC, false, true> k;
  k.stage(g, b, mean, invstd, nullptr, nullptr, C);
  const long total = P * C;
  const long stride = (long)gridDim.x * 256 * 8;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < total;
       i += stride) {
    long jrow = STRIDED ? (long)fd((unsigned)i, dC) : 0;
    int c = STRIDED ? (int)(i - jrow * C) : (int)(i % C);
    for (int j = 0; j < 8 && i + j < total; ++j) {
      const __bf16 o = bn_fwd_elem<RELU>((float)x[i + j], k[c]);
      if (STRIDED) y[jrow * ldo + c] = o;
      else y[i + j] = o;
      if (++c == C) { c = 0; ++jrow; }
    }
  }
}

// grid (ceil(C/64), Z). The 4-deep loop stays in the kernel body, in
// front of the shared plain loop: moved into a helper, the compiler
// pairs its four products into packed FMAs another way, which changes
// the low bits of s2 (the contraction of a sum of products is its
// choice). The grouped kernel below was measured with the plain loop
// alone.
template <bool RELU>
__global__ __launch_bounds__(256)
void bn_bwd_stats_kernel(const __bf16* __restrict__ x,
                         const __bf16* __restrict__ dy, long ldy,
                         const __bf16* __restrict__ g,
                         const __bf16* __restrict__ b,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         float* __restrict__ part, long P, int C, int Z) {
  const int cl = threadIdx.x & 63;
  const int pr = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int z = blockIdx.y;
  float s1 = 0.f, s2 = 0.f;
  if (c < C) {
    const BnCh k = bn_ch<false>(g, b, mean, invstd, nullptr, nullptr, c);
    const long step = (long)Z * 4;
    long p = (long)z * 4 + pr;
    for (; p + 3 * step < P; p += 4 * step) {
      const long i0 = p * C + c, i1 = i0 + step * C;
      const long i2 = i1 + step * C, i3 = i2 + step * C;
      const long j0 = p * ldy + c, j1 = j0 + step * ldy;
      const long j2 = j1 + step * ldy, j3 = j2 + step * ldy;
      const float x0 = (float)x[i0], x1 = (float)x[i1];
      const float x2 = (float)x[i2], x3 = (float)x[i3];
      const float d0 = bn_dy_eff<RELU>(x0, (float)dy[j0], k);
      const float d1 = bn_dy_eff<RELU>(x1, (float)dy[j1], k);
      const float d2 = bn_dy_eff<RELU>(x2, (float)dy[j2], k);
      const float d3 = bn_dy_eff<RELU>(x3, (float)dy[j3], k);
      s1 += d0 + d1 + d2 + d3;
      s2 += d0 * bn_xhat(x0, k) + d1 * bn_xhat(x1, k) +
            d2 * bn_xhat(x2, k) + d3 * bn_xhat(x3, k);
    }
    bn_col_bwd_rows<RELU>(x, dy, ldy, k, P, C, c, step, p, s1, s2);
  }
  bn_col_fold(s1, s2, part, (long)z * C + c, c < C);
}

// grid (cbtot, Z)
template <bool RELU>
__global__ __launch_bounds__(256)
void bng_bwd_stats_kernel(BNGroupArgs a,
                          const float* __restrict__ mean,
                          const float* __restrict__ invstd,
                          float* __restrict__ part, long P, int Ctot,
                          int Z) {
  const int br = bng_branch(a, blockIdx.x);
  const int C = a.C[br];
  const int coff = a.coff[br];
  const int c = (blockIdx.x - a.cb0[br]) * 64 + (threadIdx.x & 63);
  const int z = blockIdx.y;
  float s1 = 0.f, s2 = 0.f;
  if (c < C)
    bn_col_bwd_rows<RELU>(
        a.x[br], a.dy[br], a.dyld[br],
        bn_ch<false>(a.g[br], a.b[br], mean + coff, invstd + coff, nullptr,
                     nullptr, c),
        P, C, c, (long)Z * 4, (long)z * 4 + (threadIdx.x >> 6), s1, s2);
  bn_col_fold(s1, s2, part, (long)z * Ctot + coff + c, c < C);
}

template <bool RELU>
__global__ __launch_bounds__(256)
void bn_bwd_apply_kernel(const __bf16* __restrict__ x,
                         const __bf16* __restrict__ dy, long ldy, FDiv dC,
                         const __bf16* __restrict__ g,
                         const __bf16* __restrict__ b,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         const float* __restrict__ s1n,
                         const float* __restrict__ s2n,
                         __bf16* __restrict__ dx, long P, int C) {
  __shared__ BnChLds<MAXC, true, RELU> k;
  k.stage(g, b, mean, invstd, s1n, s2n, C);
  const long total = P * C;
  const long stride = (long)gridDim.x * 256 * 8;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < total;
       i += stride) {
    long jrow = fd((unsigned)i, dC);           // i / C (i < 2^31)
    int c = (int)(i - jrow * C);
    for (int j = 0; j < 8 && i + j < total; ++j) {
      dx[i + j] = bn_dx_elem<RELU>((float)x[i + j],
                                   (float)dy[jrow * ldy + c], k[c]);
      if (++c == C) { c = 0; ++jrow; }
    }
  }
}

// ------------------------------------------------------------ row-wise path
//
// For C % 8 == 0 (every Inception BN layer): thread t owns a FIXED
// 8-channel octet u = t % (C/8) and walks pixel rows. Per-channel
// constants live in REGISTERS (loaded once per thread), the hot loop
// is one b128 load (+1 store) per 8 elements with zero LDS traffic —
// the flat-walk kernels gathered 6 per-channel constants from
// LDS per element and the PMC showed bank-conflict counts 10x the LDS
// instruction count (profiles/r01_inception_pmc.txt), capping them at
// 1.7-3 TB/s on an 6.3 TB/s chip.

// grid (Z); block 256 = (C/8) channel octets x rpb rows
__global__ __launch_bounds__(256)
void bn_stats_rw_kernel(const __bf16* __restrict__ x,
                        float* __restrict__ part,
                        long P, int C, int Z) {
  const RwIdx i = rw_idx(C);
  const int c0 = i.c0;
  const int z = blockIdx.x;
  float sum[8] = {}, sq[8] = {};
  if (i.rl < i.rpb) {
    const long rstep = (long)Z * i.rpb;
    long r = (long)z * i.rpb + i.rl;
    // 4 rows of loads in flight: the single-load loop was
    // latency-bound (one dependent accumulate per HBM round trip)
    for (; r + 3 * rstep < P; r += 4 * rstep) {
      const bf16x8 v0 = ld8(&x[r * C + c0]);
      const bf16x8 v1 = ld8(&x[(r + rstep) * C + c0]);
      const bf16x8 v2 = ld8(&x[(r + 2 * rstep) * C + c0]);
      const bf16x8 v3 = ld8(&x[(r + 3 * rstep) * C + c0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f0 = (float)v0[j], f1 = (float)v1[j];
        const float f2 = (float)v2[j], f3 = (float)v3[j];
        sum[j] += (f0 + f1) + (f2 + f3);
        sq[j] += (f0 * f0 + f1 * f1) + (f2 * f2 + f3 * f3);
      }
    }
    for (; r < P; r += rstep) {
      const bf16x8 v = ld8(&x[r * C + c0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j];
        sum[j] += f;
        sq[j] += f * f;
      }
    }
  }
  bn_rw_fold(sum, sq, part, i, z, Z);
}

template <bool RELU>
__global__ __launch_bounds__(256)
void bn_apply_rw_kernel(const __bf16* __restrict__ x,
                        const float* __restrict__ mean,
                        const float* __restrict__ invstd,
                        const __bf16* __restrict__ g,
                        const __bf16* __restrict__ b,
                        __bf16* __restrict__ y, long ldo, long P, int C) {
  const RwIdx i = rw_idx(C);
  if (i.rl >= i.rpb) return;
  const int c0 = i.c0;
  BnCh k[8];
  rw_load_ch<false>(k, g, b, mean, invstd, nullptr, nullptr, c0);
  const long rstep = (long)gridDim.x * i.rpb;
  long r = (long)blockIdx.x * i.rpb + i.rl;
  for (; r + rstep < P; r += 2 * rstep) {   // 2 loads in flight
    const bf16x8 v0 = ld8(&x[r * C + c0]);
    const bf16x8 v1 = ld8(&x[(r + rstep) * C + c0]);
    st8(&y[r * ldo + c0], bn_fwd_x8<RELU>(v0, k));
    st8(&y[(r + rstep) * ldo + c0], bn_fwd_x8<RELU>(v1, k));
  }
  for (; r < P; r += rstep)
    st8(&y[r * ldo + c0], bn_fwd_x8<RELU>(ld8(&x[r * C + c0]), k));
}

template <bool RELU>
__global__ __launch_bounds__(256)
void bn_bwd_stats_rw_kernel(const __bf16* __restrict__ x,
                            const __bf16* __restrict__ dy, long ldy,
                            const __bf16* __restrict__ g,
                            const __bf16* __restrict__ b,
                            const float* __restrict__ mean,
                            const float* __restrict__ invstd,
                            float* __restrict__ part, long P, int C, int Z) {
  const RwIdx i = rw_idx(C);
  const int c0 = i.c0;
  const int z = blockIdx.x;
  float s1[8] = {}, s2[8] = {};
  if (i.rl < i.rpb) {
    BnCh k[8];
    rw_load_ch<false>(k, g, b, mean, invstd, nullptr, nullptr, c0);
    const long rstep = (long)Z * i.rpb;
    long r = (long)z * i.rpb + i.rl;
    // 2 rows x (x, dy) = 4 loads in flight (see bn_stats_rw_kernel)
    for (; r + rstep < P; r += 2 * rstep) {
      const bf16x8 xv0 = ld8(&x[r * C + c0]);
      const bf16x8 dv0 = ld8(&dy[r * ldy + c0]);
      const bf16x8 xv1 = ld8(&x[(r + rstep) * C + c0]);
      const bf16x8 dv1 = ld8(&dy[(r + rstep) * ldy + c0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x0 = (float)xv0[j], x1 = (float)xv1[j];
        const float d0 = bn_dy_eff<RELU>(x0, (float)dv0[j], k[j]);
        const float d1 = bn_dy_eff<RELU>(x1, (float)dv1[j], k[j]);
        s1[j] += d0 + d1;
        s2[j] += d0 * bn_xhat(x0, k[j]) + d1 * bn_xhat(x1, k[j]);
      }
    }
    for (; r < P; r += rstep) {
      const bf16x8 xv = ld8(&x[r * C + c0]);
      const bf16x8 dv = ld8(&dy[r * ldy + c0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xf = (float)xv[j];
        const float d = bn_dy_eff<RELU>(xf, (float)dv[j], k[j]);
        s1[j] += d;
        s2[j] += d * bn_xhat(xf, k[j]);
      }
    }
  }
  bn_rw_fold(s1, s2, part, i, z, Z);
}

template <bool RELU>
__global__ __launch_bounds__(256)
void bn_bwd_apply_rw_kernel(const __bf16* __restrict__ x,
                            const __bf16* __restrict__ dy, long ldy,
                            const __bf16* __restrict__ g,
                            const __bf16* __restrict__ b,
                            const float* __restrict__ mean,
                            const float* __restrict__ invstd,
                            const float* __restrict__ s1n,
                            const float* __restrict__ s2n,
                            __bf16* __restrict__ dx, long P, int C) {
  const RwIdx i = rw_idx(C);
  if (i.rl >= i.rpb) return;
  const int c0 = i.c0;
  BnCh k[8];
  rw_load_ch<true>(k, g, b, mean, invstd, s1n, s2n, c0);
  const long rstep = (long)gridDim.x * i.rpb;
  long r = (long)blockIdx.x * i.rpb + i.rl;
  for (; r + rstep < P; r += 2 * rstep) {   // 4 loads in flight
    const bf16x8 xv0 = ld8(&x[r * C + c0]);
    const bf16x8 dv0 = ld8(&dy[r * ldy + c0]);
    const bf16x8 xv1 = ld8(&x[(r + rstep) * C + c0]);
    const bf16x8 dv1 = ld8(&dy[(r + rstep) * ldy + c0]);
    st8(&dx[r * C + c0], bn_dx_x8<RELU>(xv0, dv0, k));
    st8(&dx[(r + rstep) * C + c0], bn_dx_x8<RELU>(xv1, dv1, k));
  }
  for (; r < P; r += rstep)
    st8(&dx[r * C + c0],
        bn_dx_x8<RELU>(ld8(&x[r * C + c0]), ld8(&dy[r * ldy + c0]), k));
}

// ------------------------------------------------------ grouped flat walks

// grid (ew blocks, n): per-branch flat walk, strided store into the
// branch's out view, per-channel constants staged in LDS
template <bool RELU>
__global__ __launch_bounds__(256)
void bng_apply_kernel(BNGroupArgs a, const float* __restrict__ mean,
                      const float* __restrict__ invstd, long P) {
  const int br = blockIdx.y;
  const __bf16* x = a.x[br];
  const int C = a.C[br];
  const int coff = a.coff[br];
  __bf16* y = a.y[br];
  const long ldo = a.yld[br];
  __shared__ BnChLds<BNG_MAXC, false, true> k;
  k.stage(a.g[br], a.b[br], mean + coff, invstd + coff, nullptr, nullptr, C);
  const long total = P * C;
  const long stride = (long)gridDim.x * 256 * 8;
  const FDiv dC = a.dC[br];
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < total;
       i += stride) {
    const long prow = fd((unsigned)i, dC);  // C%8==0: chunk stays in-row
    const int c0 = (int)(i - prow * C);
    st8(&y[prow * ldo + c0], bn_fwd_x8<RELU>(ld8(&x[i]), k, c0));
  }
}

template <bool RELU>
__global__ __launch_bounds__(256)
void bng_bwd_apply_kernel(BNGroupArgs a,
                          const float* __restrict__ mean,
                          const float* __restrict__ invstd,
                          const float* __restrict__ s1n,
                          const float* __restrict__ s2n, long P) {
  const int br = blockIdx.y;
  const __bf16* x = a.x[br];
  const __bf16* dy = a.dy[br];
  const long ldy = a.dyld[br];
  __bf16* dx = a.dx[br];
  const int C = a.C[br];
  const int coff = a.coff[br];
  __shared__ BnChLds<BNG_MAXC, true, RELU> k;
  k.stage(a.g[br], a.b[br], mean + coff, invstd + coff, s1n + coff,
          s2n + coff, C);
  const long total = P * C;
  const long stride = (long)gridDim.x * 256 * 8;
  const FDiv dC = a.dC[br];
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8; i < total;
       i += stride) {
    const long prow = fd((unsigned)i, dC);
    const int c0 = (int)(i - prow * C);
    st8(&dx[i], bn_dx_x8<RELU>(ld8(&x[i]), ld8(&dy[prow * ldy + c0]), k, c0));
  }
}

// ------------------------------------------------------------- host: plans

inline bool rowwise_ok(int C) { return (C & 7) == 0 && C <= MAXC; }

inline unsigned rw_grid(long P, int C) {
  const int rpb = rw_rpb(C);
  long wgs = (P + rpb - 1) / rpb;
  if (wgs > 4096) wgs = 4096;
  if (wgs < 1) wgs = 1;
  return (unsigned)wgs;
}

// Row-wise stats only where the 8-channels-per-thread granularity
// still yields enough BLOCKS to cover the chip (>=512 at 2 passes per
// thread): small-P layers have 8x more parallelism at the old
// one-channel-per-thread granularity and measured FASTER there (the
// first rowwise cut regressed mid-size layers 2x on exactly this).
inline bool rowwise_stats(long P, int C) {
  return rowwise_ok(C) && P / ((long)rw_rpb(C) * 2) >= 512;
}

// Column-walk slices over cb 64-wide channel blocks: target >=2048
// workgroups across the cb x Z grid, each slice covering >=8 pixel
// rounds of 4 rows. The cap matters: narrow layers (C=64 -> one channel
// column) need Z ~ 2048 to cover the 256-CU chip; the old 256 cap left
// them 1 workgroup/CU and the PMC wait counters dominated everything
// else in the stats kernels.
inline int col_slices(long P, long cb) {
  long want = (2048 + cb - 1) / cb;
  long per = P / (4 * 8);
  long z = want < per ? want : per;
  if (z < 1) z = 1;
  if (z > 2048) z = 2048;
  return (int)z;
}

// Row-wise slices: grid = Z blocks, each covering all C and rpb rows
// per pass; ~2 passes per thread (2 loads in flight), more via the
// 4-deep unroll when P allows
inline int rw_slices(long P, int C) {
  const int rpb = rw_rpb(C);
  long z = (P + 2L * rpb - 1) / (2L * rpb);
  if (z > 2048) z = 2048;
  if (z < 1) z = 1;
  return (int)z;
}

inline unsigned ew_grid(long total) {
  long wgs = (total / 8 + 255) / 256;
  if (wgs > 8192) wgs = 8192;
  if (wgs < 1) wgs = 1;
  return (unsigned)wgs;
}

// launch K<true> or K<false> by relu
#define LAUNCH_RELU(K, grid, block, ...)                                    \
  do {                                                                      \
    if (relu)                                                               \
      hipLaunchKernelGGL((K<true>), grid, block, 0, stream, __VA_ARGS__);   \
    else                                                                    \
      hipLaunchKernelGGL((K<false>), grid, block, 0, stream, __VA_ARGS__);  \
  } while (0)

}  // namespace

BnPlan bn_plan(long P, int C) {
  BnPlan p;
  p.rw_stats = rowwise_stats(P, C);
  p.rw_apply = rowwise_ok(C);
  p.Z = p.rw_stats ? rw_slices(P, C) : col_slices(P, (C + 63) / 64);
  return p;
}

int bn_max_channels() { return MAXC; }

void launch_bn_fwd(const bf16_t* x_, const bf16_t* g_, const bf16_t* b_,
                   bf16_t* y_, long ldo, float* mean, float* invstd,
                   float* part, long P, int C, const BnPlan& plan, float eps,
                   bool relu, hipStream_t stream) {
  const __bf16* x = (const __bf16*)x_;
  const __bf16* g = (const __bf16*)g_;
  const __bf16* b = (const __bf16*)b_;
  __bf16* y = (__bf16*)y_;
  const int Z = plan.Z;
  const float inv_count = 1.f / (float)P;
  if (plan.rw_stats) {
    hipLaunchKernelGGL(bn_stats_rw_kernel, dim3(Z), dim3(256), 0, stream, x,
                       part, P, C, Z);
    hipLaunchKernelGGL(bn_finalize_kernel<true>, dim3(C), dim3(256), 0,
                       stream, part, mean, invstd, C, Z, inv_count, eps);
  } else {
    hipLaunchKernelGGL(bn_stats_kernel, dim3(ceil_div(C, 64), Z), dim3(256),
                       0, stream, x, part, P, C, Z);
    hipLaunchKernelGGL(bn_finalize_kernel<false>, dim3(C), dim3(64), 0,
                       stream, part, mean, invstd, C, Z, inv_count, eps);
  }
  if (plan.rw_apply) {
    LAUNCH_RELU(bn_apply_rw_kernel, dim3(rw_grid(P, C)), dim3(256), x, mean,
                invstd, g, b, y, ldo, P, C);
    return;
  }
  const dim3 ag(ew_grid(P * (long)C)), ab(256);
  const FDiv dC = make_fd(C);
#define APPLY(RELUv, STRv)                                                  \
  hipLaunchKernelGGL((bn_apply_kernel<RELUv, STRv>), ag, ab, 0, stream, x,  \
                     mean, invstd, g, b, y, ldo, dC, P, C)
  if (ldo != C) { if (relu) APPLY(true, true); else APPLY(false, true); }
  else          { if (relu) APPLY(true, false); else APPLY(false, false); }
#undef APPLY
}

void launch_bn_bwd(const bf16_t* x_, const bf16_t* dy_, long ldy,
                   const bf16_t* g_, const bf16_t* b_, const float* mean,
                   const float* invstd, bf16_t* dx_, bf16_t* dgamma_,
                   bf16_t* dbeta_, float* part, float* s1n, float* s2n,
                   long P, int C, const BnPlan& plan, bool relu,
                   hipStream_t stream) {
  const __bf16* x = (const __bf16*)x_;
  const __bf16* dy = (const __bf16*)dy_;
  const __bf16* g = (const __bf16*)g_;
  const __bf16* b = (const __bf16*)b_;
  __bf16* dx = (__bf16*)dx_;
  __bf16* dgamma = (__bf16*)dgamma_;
  __bf16* dbeta = (__bf16*)dbeta_;
  const int Z = plan.Z;
  const float inv_count = 1.f / (float)P;
  if (plan.rw_stats) {
    LAUNCH_RELU(bn_bwd_stats_rw_kernel, dim3(Z), dim3(256), x, dy, ldy, g, b,
                mean, invstd, part, P, C, Z);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<true>, dim3(C), dim3(256), 0,
                       stream, part, dgamma, dbeta, s1n, s2n, C, Z,
                       inv_count);
  } else {
    LAUNCH_RELU(bn_bwd_stats_kernel, dim3(ceil_div(C, 64), Z), dim3(256), x,
                dy, ldy, g, b, mean, invstd, part, P, C, Z);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(C), dim3(64), 0,
                       stream, part, dgamma, dbeta, s1n, s2n, C, Z,
                       inv_count);
  }
  if (plan.rw_apply)
    LAUNCH_RELU(bn_bwd_apply_rw_kernel, dim3(rw_grid(P, C)), dim3(256), x,
                dy, ldy, g, b, mean, invstd, s1n, s2n, dx, P, C);
  else
    LAUNCH_RELU(bn_bwd_apply_kernel, dim3(ew_grid(P * (long)C)), dim3(256),
                x, dy, ldy, make_fd(C), g, b, mean, invstd, s1n, s2n, dx, P,
                C);
}

// -------------------------------------------------------- grouped launchers

int bn_group_max_channels() { return BNG_MAXC; }

int bn_group_slices(long P, const int* Cs, int n) {
  long cbtot = 0;
  for (int i = 0; i < n; ++i) cbtot += ceil_div(Cs[i], 64);
  return col_slices(P, cbtot);
}

namespace {

// the kernel argument of one grouped launch chain, and its grids
struct BNGroupLaunch {
  BNGroupArgs a;
  int cbtot, ctot;
  dim3 ew;   // flat-walk grid (blocks, n)
};

BNGroupLaunch group_launch(const BnGroup& gr, long P) {
  BNGroupLaunch l = {};
  BNGroupArgs& a = l.a;
  a.n = gr.n;
  int cmax = 0;
  for (int i = 0; i < gr.n; ++i) {
    a.x[i] = (const __bf16*)gr.x[i];
    a.g[i] = (const __bf16*)gr.g[i];
    a.b[i] = (const __bf16*)gr.b[i];
    a.dy[i] = (const __bf16*)gr.dy[i];
    a.dyld[i] = gr.dyld[i];
    a.dx[i] = (__bf16*)gr.dx[i];
    a.y[i] = (__bf16*)gr.y[i];
    a.yld[i] = gr.yld[i];
    a.C[i] = gr.C[i];
    a.coff[i] = l.ctot;
    a.cb0[i] = l.cbtot;
    a.dC[i] = make_fd(gr.C[i]);
    l.ctot += gr.C[i];
    l.cbtot += ceil_div(gr.C[i], 64);
    cmax = gr.C[i] > cmax ? gr.C[i] : cmax;
  }
  long wgs = ((P * cmax) / 8 + 255) / 256;
  if (wgs > 2048) wgs = 2048;
  if (wgs < 1) wgs = 1;
  l.ew = dim3((unsigned)wgs, gr.n);
  return l;
}

}  // namespace

void launch_bn_group_fwd(const BnGroup& gr, float* mean, float* invstd,
                         float* part, long P, int Z, float eps, bool relu,
                         hipStream_t stream) {
  const BNGroupLaunch l = group_launch(gr, P);
  hipLaunchKernelGGL(bng_stats_kernel, dim3(l.cbtot, Z), dim3(256), 0, stream,
                     l.a, part, P, l.ctot, Z);
  hipLaunchKernelGGL(bn_finalize_kernel<false>, dim3(l.ctot), dim3(64), 0,
                     stream, part, mean, invstd, l.ctot, Z, 1.f / (float)P,
                     eps);
  LAUNCH_RELU(bng_apply_kernel, l.ew, dim3(256), l.a, mean, invstd, P);
}

void launch_bn_group_bwd(const BnGroup& gr, const float* mean,
                         const float* invstd, bf16_t* dgamma, bf16_t* dbeta,
                         float* s1n, float* s2n, float* part, long P, int Z,
                         bool relu, hipStream_t stream) {
  const BNGroupLaunch l = group_launch(gr, P);
  LAUNCH_RELU(bng_bwd_stats_kernel, dim3(l.cbtot, Z), dim3(256), l.a, mean,
              invstd, part, P, l.ctot, Z);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<false>, dim3(l.ctot), dim3(64), 0,
                     stream, part, (__bf16*)dgamma, (__bf16*)dbeta, s1n, s2n,
                     l.ctot, Z, 1.f / (float)P);
  LAUNCH_RELU(bng_bwd_apply_kernel, l.ew, dim3(256), l.a, mean, invstd, s1n,
              s2n, P);
}

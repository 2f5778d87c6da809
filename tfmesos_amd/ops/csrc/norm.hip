// Fused residual-add + LayerNorm / RMSNorm over packed bf16 rows, forward and
// backward, for MI355X (gfx950).
//
//   s    = bf16(fp32(x) + fp32(residual))           (s = x without a residual)
//   mean = sum(s) / D                               (0 with rms)
//   var  = sum((s - mean)^2) / D, rstd = 1 / sqrt(var + eps)
//   y    = bf16(w (s - mean) rstd + b)
//   g    = dy w, xh = (s - mean) rstd
//   dx   = bf16(rstd (g - mean_D(g) - xh mean_D(g xh)) + ds)   (no mean_D(g)
//          with rms);  dw = sum_rows dy xh, db = sum_rows dy
//
// Lane map. A row is C = ceil(D / 8) chunks of 8 bf16 (16 bytes). LPR, the
// smallest of 8 / 16 / 32 / 64 that is >= C, lanes share a row; lane l of the
// group owns chunk l (and chunk l + 64 when 512 < D <= 1024, CPL == 2). A
// wave holds 64 / LPR rows, a 256-thread block RPB = 256 / LPR: thread t is
// lane t % LPR of row slot t / LPR. A row group is RPB consecutive rows;
// block b walks groups b, b + gridDim.x, ... The row stays in registers from
// its load to its store. Every sum over a row is the lane's own elements in
// column order, then an xor butterfly over the group's lanes (offsets 1, 2,
// ... LPR / 2): a fixed order, and every lane of the group holds the same
// bits after it. Columns at or beyond D load as zero, are masked out of the
// deviations, and are never stored; rows at or beyond n likewise.
//
// VEC: D % 8 == 0 and every [n, D] base 16-byte aligned: one b128 access a
// chunk. Otherwise the guarded element-wise form of the same map. The host
// picks. Parameters are [D], fp32 or bf16 at any alignment, read element-wise
// once a thread (they stay in registers across the walk).
//
// Forward: one pass: load x (and residual), round s and store it if there is
// a residual, two-pass statistics on the registers, store y, mean, rstd.
//
// Backward: norm_bwd_kernel stores dx and keeps the lane's dw / db terms in
// fp32 registers across its walk (a lane sees the same columns in every
// row). At the end the row slots of a wave fold by xor shuffles over the
// upper lane bits (offsets LPR ... 32), the four waves through LDS in wave
// order ((w0 + w1) + w2) + w3, and the block writes one fp32 partial row
// [2, D]. norm_finish_kernel stages 8 columns of all partials in LDS and one
// thread a column adds them in block order 0 .. blocks - 1 (one chain of
// adds, fed by b128 LDS reads), rounding once to the parameter's dtype. No
// atomics, nothing pre-zeroed: the bits are a function of (n, D, blocks).
// Without parameter gradients part is null and neither the partials nor the
// finishing kernel run.
//
// Arithmetic is written out: contraction is off in this file and every fused
// multiply-add is an explicit fmaf, so the vector and the guarded form of a
// kernel give the same bits.
#include "norm.h"

#include <cstdint>
#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kFinCols = 8;            // columns a finishing block sums
constexpr int kFinThreads = 1024;      // 128 partial rows staged at a time

DEVINL float ld_param(const void* p, int is_bf16, int i) {
  return is_bf16 ? bf2f(((const bf16_t*)p)[i]) : ((const float*)p)[i];
}

DEVINL void st_param(void* p, int is_bf16, int i, float v) {
  if (is_bf16) ((bf16_t*)p)[i] = f2bf(v);
  else ((float*)p)[i] = v;
}

// The nv (<= 8; VEC: 0 or 8) leading elements of the chunk at p as fp32,
// zeros for the rest and for a row that is not live.
template <bool VEC>
DEVINL void ld_chunk(const __bf16* __restrict__ p, int nv, bool live,
                     float (&v)[8]) {
  if constexpr (VEC) {
    bf16x8 t = {};
    if (live && nv) t = *(const bf16x8*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (live && e < nv) ? (float)p[e] : 0.f;
  }
}

template <bool VEC>
DEVINL void st_chunk(__bf16* __restrict__ p, int nv, bool live,
                     const float (&v)[8]) {
  if constexpr (VEC) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (__bf16)v[e];
    if (live && nv) *(bf16x8*)p = t;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (live && e < nv) p[e] = (__bf16)v[e];
  }
}

// Sum over the LPR lanes of a row: every lane ends with the same bits.
template <int LPR>
DEVINL float group_sum(float v) {
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// Sum over the 64 / LPR row slots of a wave, column by column.
template <int LPR>
DEVINL float slot_sum(float v) {
#pragma unroll
  for (int o = LPR; o < WAVE; o <<= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// The lane's chunks: first column and valid elements of each.
template <int LPR, int CPL>
struct Lane {
  int col[CPL], nv[CPL];
  DEVINL Lane(int D) {
    const int l = threadIdx.x % LPR;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      col[j] = (l + j * LPR) * 8;
      nv[j] = min(max(D - col[j], 0), 8);
    }
  }
};

template <int LPR, int CPL, bool VEC>
__global__ __launch_bounds__(kThreads) void norm_fwd_kernel(NormFwdArgs a) {
  constexpr int RPB = kThreads / LPR;
  const Lane<LPR, CPL> ln(a.D);
  const int slot = threadIdx.x / LPR;
  const __bf16* x = (const __bf16*)a.x;
  const __bf16* res = (const __bf16*)a.res;
  __bf16* s_out = (__bf16*)a.s_out;
  __bf16* y = (__bf16*)a.y;

  float w[CPL][8], b[CPL][8];
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = e < ln.nv[j];
      w[j][e] = !ok ? 0.f : a.w ? ld_param(a.w, a.w_bf16, ln.col[j] + e) : 1.f;
      b[j][e] = ok && a.b ? ld_param(a.b, a.b_bf16, ln.col[j] + e) : 0.f;
    }

  const float fD = (float)a.D;
  const long groups = (a.n + RPB - 1) / RPB;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long row = g * RPB + slot;
    const bool live = row < a.n;
    const long off = row * a.D;

    float v[CPL][8];
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      ld_chunk<VEC>(x + off + ln.col[j], ln.nv[j], live, v[j]);
    if (res) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        float r[8];
        ld_chunk<VEC>(res + off + ln.col[j], ln.nv[j], live, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = (float)(__bf16)(v[j][e] + r[e]);
        st_chunk<VEC>(s_out + off + ln.col[j], ln.nv[j], live, v[j]);
      }
    }

    float mean = 0.f;
    if (!a.rms) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < CPL; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) t += v[j][e];
      mean = group_sum<LPR>(t) / fD;
    }
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[j][e] = e < ln.nv[j] ? v[j][e] - mean : 0.f;
        q = fmaf(v[j][e], v[j][e], q);
      }
    const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / fD + a.eps);

#pragma unroll
    for (int j = 0; j < CPL; ++j) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[j][e] = fmaf(w[j][e], v[j][e] * rstd, b[j][e]);
      st_chunk<VEC>(y + off + ln.col[j], ln.nv[j], live, v[j]);
    }
    if (live && threadIdx.x % LPR == 0) {
      a.mean[row] = mean;
      a.rstd[row] = rstd;
    }
  }
}

template <int LPR, int CPL, bool VEC>
__global__ __launch_bounds__(kThreads) void norm_bwd_kernel(NormBwdArgs a) {
  constexpr int RPB = kThreads / LPR;
  constexpr int W = LPR * CPL * 8;     // columns the lane map covers
  const Lane<LPR, CPL> ln(a.D);
  const int slot = threadIdx.x / LPR;
  const __bf16* dy = (const __bf16*)a.dy;
  const __bf16* s = (const __bf16*)a.s;
  const __bf16* ds = (const __bf16*)a.ds;
  __bf16* dx = (__bf16*)a.dx;

  float w[CPL][8], dw[CPL][8], db[CPL][8];
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool ok = e < ln.nv[j];
      w[j][e] = !ok ? 0.f : a.w ? ld_param(a.w, a.w_bf16, ln.col[j] + e) : 1.f;
      dw[j][e] = 0.f;
      db[j][e] = 0.f;
    }

  const float fD = (float)a.D;
  const long groups = (a.n + RPB - 1) / RPB;
  for (long g = blockIdx.x; g < groups; g += gridDim.x) {
    const long row = g * RPB + slot;
    const bool live = row < a.n;
    const long off = row * a.D;
    const float mean = live ? a.mean[row] : 0.f;
    const float rstd = live ? a.rstd[row] : 0.f;

    float d[CPL][8], xh[CPL][8];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      ld_chunk<VEC>(dy + off + ln.col[j], ln.nv[j], live, d[j]);
      ld_chunk<VEC>(s + off + ln.col[j], ln.nv[j], live, xh[j]);
    }
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xh[j][e] = e < ln.nv[j] ? (xh[j][e] - mean) * rstd : 0.f;
        dw[j][e] = fmaf(d[j][e], xh[j][e], dw[j][e]);
        db[j][e] += d[j][e];
        d[j][e] *= w[j][e];            // g
        t1 += d[j][e];
        t2 = fmaf(d[j][e], xh[j][e], t2);
      }
    const float c1 = a.rms ? 0.f : group_sum<LPR>(t1) / fD;
    const float c2 = group_sum<LPR>(t2) / fD;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float up[8] = {};
      if (ds) ld_chunk<VEC>(ds + off + ln.col[j], ln.nv[j], live, up);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        d[j][e] = fmaf(rstd, fmaf(-xh[j][e], c2, d[j][e] - c1), up[e]);
      st_chunk<VEC>(dx + off + ln.col[j], ln.nv[j], live, d[j]);
    }
  }

  if (!a.part) return;                 // block-uniform
  __shared__ float red[kThreads / WAVE][2][W];
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float tw = slot_sum<LPR>(dw[j][e]), tb = slot_sum<LPR>(db[j][e]);
      if (threadIdx.x % WAVE < LPR) {
        red[wave][0][ln.col[j] + e] = tw;
        red[wave][1][ln.col[j] + e] = tb;
      }
    }
  __syncthreads();
  float* out = a.part + (long)blockIdx.x * 2 * a.D;
  for (int i = threadIdx.x; i < 2 * W; i += kThreads) {
    const int which = i / W, c = i % W;
    if (c < a.D)
      out[which * a.D + c] = ((red[0][which][c] + red[1][which][c]) +
                              red[2][which][c]) + red[3][which][c];
  }
}

// part [blocks, 2 * D]: column c < D of dw, D + c of db. Block k sums
// columns 8k .. 8k + 7: all threads stage them column-major in LDS (at most
// 8 loads a thread, issued together), then one thread a column reads its
// partials back four at a time (b128) and adds them in block order.
__global__ __launch_bounds__(kFinThreads) void norm_finish_kernel(
    const float* __restrict__ part, int blocks, int D, void* dw, int dw_bf16,
    void* db, int db_bf16) {
  __shared__ f32x4 stage[kFinCols][kNormMaxBlocks / 4 + 1];
  const int c = threadIdx.x % kFinCols;
  const int col = blockIdx.x * kFinCols + c;
  constexpr int kStep = kFinThreads / kFinCols;
  float v[kNormMaxBlocks / kStep];
#pragma unroll
  for (int i = 0; i < kNormMaxBlocks / kStep; ++i) {
    const int p = threadIdx.x / kFinCols + i * kStep;
    v[i] = col < 2 * D && p < blocks ? part[(long)p * 2 * D + col] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < kNormMaxBlocks / kStep; ++i) {
    const int p = threadIdx.x / kFinCols + i * kStep;
    if (p < blocks) stage[c][p / 4][p % 4] = v[i];
  }
  __syncthreads();
  if (threadIdx.x >= kFinCols || col >= 2 * D) return;
  float acc = 0.f;
#pragma unroll 8
  for (int q = 0; q < blocks / 4; ++q) {
    const f32x4 four = stage[c][q];
    acc = (((acc + four[0]) + four[1]) + four[2]) + four[3];
  }
  for (int p = blocks / 4 * 4; p < blocks; ++p) acc += stage[c][p / 4][p % 4];
  if (col < D) {
    if (dw) st_param(dw, dw_bf16, col, acc);
  } else if (db) {
    st_param(db, db_bf16, col - D, acc);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fn(lanes, chunks a lane, vec) as integral constants
template <typename F>
void dispatch(int lanes, int D, bool vec, F fn) {
  auto with_vec = [&](auto l, auto c) {
    if (vec) fn(l, c, std::true_type());
    else fn(l, c, std::false_type());
  };
  using std::integral_constant;
  if (lanes == 8) with_vec(integral_constant<int, 8>(), integral_constant<int, 1>());
  else if (lanes == 16) with_vec(integral_constant<int, 16>(), integral_constant<int, 1>());
  else if (lanes == 32) with_vec(integral_constant<int, 32>(), integral_constant<int, 1>());
  else if (D <= 512) with_vec(integral_constant<int, 64>(), integral_constant<int, 1>());
  else with_vec(integral_constant<int, 64>(), integral_constant<int, 2>());
}

}  // namespace

NormPlan norm_plan(long n, int D, long blocks) {
  const int chunks = (D + 7) / 8;
  const int lanes = chunks <= 8 ? 8 : chunks <= 16 ? 16 : chunks <= 32 ? 32 : 64;
  const int rows = kThreads / lanes;
  const long groups = (n + rows - 1) / rows;
  const long most = groups < kNormMaxBlocks ? (groups < 1 ? 1 : groups)
                                            : kNormMaxBlocks;
  if (blocks <= 0 || blocks > most) blocks = most;
  return {lanes, rows, (int)blocks};
}

// x, res, s_out, y: [n, D] bf16 contiguous at any base alignment, res and
// s_out both null or both set; w, b [D] or null; mean, rstd fp32 [n].
// 1 <= n < 2^31, 1 <= D <= kNormMaxD.
void launch_norm_fwd(const NormFwdArgs& a, hipStream_t stream) {
  const NormPlan p = norm_plan(a.n, a.D, 0);
  const long groups = (a.n + p.rows - 1) / p.rows;
  // the walk keeps w and b in registers; two blocks' worth a CU beyond that
  const dim3 grid((unsigned)(groups < 2 * kNormMaxBlocks ? groups
                                                         : 2 * kNormMaxBlocks));
  const bool vec = a.D % 8 == 0 && aligned16(a.x) && aligned16(a.res) &&
                   aligned16(a.s_out) && aligned16(a.y);
  dispatch(p.lanes, a.D, vec, [&](auto l, auto c, auto v) {
    hipLaunchKernelGGL(
        (norm_fwd_kernel<decltype(l)::value, decltype(c)::value,
                         decltype(v)::value>),
        grid, dim3(kThreads), 0, stream, a);
  });
}

// dy, s, ds (or null), dx: [n, D] bf16 as above; mean, rstd: the forward's.
// a.blocks = norm_plan(n, D, .).blocks. part fp32 [blocks, 2, D], or null
// when neither dw nor db is wanted; dw, db [D] in the dtype their flag names.
void launch_norm_bwd(const NormBwdArgs& a, hipStream_t stream) {
  const NormPlan p = norm_plan(a.n, a.D, a.blocks);
  const bool vec = a.D % 8 == 0 && aligned16(a.dy) && aligned16(a.s) &&
                   aligned16(a.ds) && aligned16(a.dx);
  dispatch(p.lanes, a.D, vec, [&](auto l, auto c, auto v) {
    hipLaunchKernelGGL(
        (norm_bwd_kernel<decltype(l)::value, decltype(c)::value,
                         decltype(v)::value>),
        dim3(p.blocks), dim3(kThreads), 0, stream, a);
  });
  if (a.part)
    hipLaunchKernelGGL(norm_finish_kernel,
                       dim3((2 * a.D + kFinCols - 1) / kFinCols),
                       dim3(kFinThreads), 0, stream, a.part, p.blocks, a.D, a.dw,
                       a.dw_bf16, a.db, a.db_bf16);
}

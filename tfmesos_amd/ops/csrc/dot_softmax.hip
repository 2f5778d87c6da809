// Softmax cross-entropy over a whole vocabulary without forming [B, V]
// (dot_softmax_loss), forward and backward.
//
//   q [B,D], w [V,D] bf16; bias [V] fp32 (null = 0, -inf masks an item out);
//   labels [B] int64 in [0, V), or -1 for an ignored example.
//   s[b,j] = q[b].w[j] + bias[j]: fp32 dot product, then the bias.
//   lse[b] = log sum_j exp s[b,j],  loss[b] = lse[b] - s[b,labels[b]]
//   (+0 where ignored). With g = dloss (0 where ignored):
//   p[b,j] = g[b] exp(s[b,j] - lse[b]), and P' is P with the label's entry
//   replaced by g[b] expm1(-loss[b]) (= p - g, without the cancellation):
//   dq = P' W, dw = P'^T Q, dbias = column sums of P'.
//
// One loop (pass_loop) serves the forward and both backward products, built
// from the pieces of mfma_stream.h. A block of 4 waves OWNS 64 rows of one
// set - wave w the rows 16w..16w+15, as MFMA A fragments in registers - and
// STREAMS its split of the other set through two row-major LDS buffers in
// tiles of 64 rows, the streamed rows' side values riding along: the global
// loads of tile i+1 are issued before the arithmetic of tile i and written
// to the other buffer after it, one block barrier per tile.
//
//   FWD     owns queries, streams its split of the items with their bias.
//           Every lane keeps a running (max, sum) for its 4 accumulator rows
//           over its own columns, NEG standing for "nothing yet"; the 16
//           lanes of a row merge once after the last tile (xor shuffles,
//           fixed order) and (max, sum) go to ws [2][nsplit][B]. The one
//           lane whose column is labels[b] stores that score to s_true [B]:
//           columns are disjoint across tiles and splits, so every element
//           has one writer over the whole grid, and the loss subtracts the
//           very number that entered the sum. dot_softmax_finish_kernel
//           merges the splits in split order and writes lse and loss.
//   ROLE_Q  owns queries (with -lse, g, the label, g expm1(-loss)), streams
//           its split of the items: P' in fp32 from the recomputed scores
//           (dot + bias) - lse, rounded to bf16 into a wave-private LDS image
//           (the A operand), dq += P' . W_tile with B fragments read back
//           from the same row-major tile through transpose reads.
//   ROLE_W  owns items (with their bias), streams its split of the examples
//           (with -lse, g, the label, g expm1(-loss)): the same tile is
//           P'^T, dw += P'^T . Q_tile, dbias = its fp32 row sums.
//   The backward is one launch: the first nQ * nsplit_q blocks take ROLE_Q,
//   the rest ROLE_W, split-major so that neighbours stream the same tiles.
//   A role with one split rounds its output tile once, parks it in the then
//   idle stream buffer and stores 16-byte row pieces. A role with more
//   writes fp32 partial tiles to part [nsplit][rows][D] (and dbias partials
//   to part_b [nsplit][V]); dot_softmax_reduce_kernel sums them in split
//   order, rounds once and stores row-contiguous.
//
// D % 8 == 0 with 16-byte-aligned bases takes b128 global accesses; anything
// else the element-wise guarded form. 1 <= D <= 256 (kDotSoftmaxMaxD), DP =
// 64 / 128 / 256 columns of registers; 1 <= V < 2^31: item indices are kept
// in unsigned or long, and the owned set is addressed from the block's own
// base pointer. No atomics, fixed order => bit-reproducible for a given
// (shape, splits); nothing is read back.
#include "dot_softmax.h"

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are kept out of this
// file's kernels; everything here is scalar fp32, integer or MFMA.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

#include "mfma_stream.h"

enum { FWD = 0, ROLE_Q = 1, ROLE_W = 2 };

struct Args {
  const __bf16* q; const __bf16* w;
  const float* bias;              // null = 0
  const long* labels;
  const float* lse; const float* loss; const float* g;     // backward
  float* ws;                      // forward: [2][nsplit][B] (max, sum)
  float* s_true;                  // forward: [B], the label's score
  float* part_q;                  // [nsplit_q][B][D] where nsplit_q > 1
  float* part_w;                  // [nsplit_w][V][D] where nsplit_w > 1
  float* part_b;                  // [nsplit_w][V] where nsplit_w > 1
  __bf16* dq; __bf16* dw; float* dbias;
  int B, V, D;
  int tiles_per_split;            // forward
  int nQ, nW;                     // backward: owned tiles of the two roles
  int nsplit_q, nsplit_w, tps_q, tps_w;
};

template <int DP, bool BWD> struct Smem {
  __bf16 T[2][TILE * (DP + 8)];   // streamed tiles, [row][d]
  float add[2][TILE];             // streamed items' bias / examples' -lse
};
template <int DP> struct Smem<DP, true> : Smem<DP, false> {
  __bf16 P[WAVES][16 * PL];       // P', wave-private [row][col]
  float mul[2][TILE];             // ROLE_W: streamed examples' g,
  float lq[2][TILE];              //   g expm1(-loss)
  int lab[2][TILE];               //   and label (-1: none)
};

// (m, s) <- merge of (m, s) and (m2, s2): s exp(m) + s2 exp(m2), max-factored
DEVINL void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = s * __expf(m - M) + s2 * __expf(m2 - M);
  m = M;
}

// The side values of example b: the label as a column key that no column
// equals where there is none, and in the backward g (0 where ignored) and
// g expm1(-loss).
template <bool BWD>
DEVINL void example_side(const Args& a, long b, bool ok, float& mul, float& lq,
                         unsigned& key) {
  const long lab = a.labels[ok ? b : 0];
  key = ok && lab >= 0 && lab < a.V ? (unsigned)lab : ~0u;
  if constexpr (BWD) {
    mul = ok && lab != -1 ? a.g[b] : 0.f;
    lq = ok ? mul * expm1f(-a.loss[b]) : 0.f;
  }
}

// One block's pass: owned tile `own_tile`, streamed tiles [t_begin, t_end).
template <int ROLE, int DP, bool VEC>
DEVINL void pass_loop(const Args& a, Smem<DP, ROLE != FWD>& sm, int own_tile,
                      int t_begin, int t_end, int split, int nsplit) {
  typedef Stream<DP> G;
  constexpr bool OWN_Q = ROLE != ROLE_W;    // the owned rows are queries
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int D = a.D;
  const __bf16* str = OWN_Q ? a.w : a.q;
  const long n_own = OWN_Q ? a.B : a.V;
  const long n_str = OWN_Q ? a.V : a.B;
  const long base = (long)own_tile * OWN;   // first owned row
  const int n_here = (int)min((long)OWN, n_own - base);
  const int lrow0 = wave * 16 + acc_row(lane, 0);   // first accumulator row

  bf16x8 af[G::KS];
  load_owned<DP, VEC>(af, (OWN_Q ? a.q : a.w) + base * D, wave * 16, n_here, D,
                      D, lane);

  // side values of this lane's 4 accumulator rows
  bool o_ok[4];
  float o_add[4], o_mul[4], o_lq[4];
  unsigned o_key[4];                // the column (OWN_Q) / row that is a label
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long row = base + lrow0 + r;
    o_ok[r] = lrow0 + r < n_here;
    o_add[r] = 0.f; o_mul[r] = 1.f; o_lq[r] = 0.f;
    if constexpr (OWN_Q) {
      example_side<ROLE != FWD>(a, row, o_ok[r], o_mul[r], o_lq[r], o_key[r]);
      if (ROLE == ROLE_Q) o_add[r] = o_ok[r] ? -a.lse[row] : 0.f;
    } else {
      o_key[r] = (unsigned)row;     // < 2^31 + 64
      o_add[r] = a.bias && o_ok[r] ? a.bias[row] : 0.f;
    }
  }

  // streamed tile t: global -> registers (fetch), registers -> LDS (stash)
  bf16x8 pre[G::PIECES];
  float pre_add = 0.f, pre_mul = 0.f, pre_lq = 0.f;
  unsigned pre_key = ~0u;
  auto fetch = [&](int t) {
    const long c0 = (long)t * TILE;
    tile_fetch<DP, VEC>(pre, str, D, D, tid, [&](int trow) {
      return c0 + trow < n_str ? c0 + trow : -1L;
    });
    if (tid < TILE) {
      const long j = c0 + tid;
      const bool ok = j < n_str;
      if constexpr (OWN_Q) {
        pre_add = a.bias && ok ? a.bias[j] : 0.f;
      } else {
        example_side<true>(a, j, ok, pre_mul, pre_lq, pre_key);
        pre_add = ok ? -a.lse[j] : 0.f;
      }
    }
  };
  auto stash = [&](int buf) {
    tile_stash<DP>(sm.T[buf], pre, tid);
    if (tid < TILE) {
      sm.add[buf][tid] = pre_add;
      if constexpr (ROLE == ROLE_W) {
        sm.mul[buf][tid] = pre_mul;
        sm.lq[buf][tid] = pre_lq;
        sm.lab[buf][tid] = (int)pre_key;
      }
    }
  };

  float run_m[4], run_s[4];         // FWD: running max / sum; else s = row sum
#pragma unroll
  for (int r = 0; r < 4; ++r) { run_m[r] = NEG; run_s[r] = 0.f; }
  f32x4 acc2[G::NT] = {};           // backward: 16 x DP output tile

  auto body = [&](int t, int buf) {
    f32x4 acc[ST] = {};
    score_tile<DP>(af, sm.T[buf], acc, D, lane);

    float s_add[ST], s_mul[ST], s_lq[ST];
    unsigned s_col[ST], s_key[ST];  // s_col < 2^31 + 64: no wrap
    bool s_ok[ST];
#pragma unroll
    for (int nt = 0; nt < ST; ++nt) {
      const int col = nt * 16 + frag_row(lane);
      s_add[nt] = sm.add[buf][col];
      s_col[nt] = (unsigned)t * TILE + col;
      s_ok[nt] = s_col[nt] < (unsigned)n_str;
      s_mul[nt] = 1.f; s_lq[nt] = 0.f; s_key[nt] = s_col[nt];
      if constexpr (ROLE == ROLE_W) {
        s_mul[nt] = sm.mul[buf][col];
        s_lq[nt] = sm.lq[buf][col];
        s_key[nt] = (unsigned)sm.lab[buf][col];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (ROLE == FWD) {
        float sc[ST];
        float mx = run_m[r];
#pragma unroll
        for (int nt = 0; nt < ST; ++nt) {
          sc[nt] = acc[nt][r] + s_add[nt];
          if (s_ok[nt]) mx = fmaxf(mx, sc[nt]);
          if (o_ok[r] && s_col[nt] == o_key[r])     // one writer per example
            a.s_true[base + lrow0 + r] = sc[nt];
        }
        float s = run_s[r] * __expf(run_m[r] - mx);
#pragma unroll
        for (int nt = 0; nt < ST; ++nt)
          if (s_ok[nt]) s += __expf(sc[nt] - mx);
        run_m[r] = mx;
        run_s[r] = s;
      } else {
        __bf16* P = sm.P[wave];
#pragma unroll
        for (int nt = 0; nt < ST; ++nt) {
          // (dot + bias) - lse in both roles
          const float sc = OWN_Q ? (acc[nt][r] + s_add[nt]) + o_add[r]
                                 : (acc[nt][r] + o_add[r]) + s_add[nt];
          float p = (o_mul[r] * s_mul[nt]) * __expf(sc);
          if (s_key[nt] == o_key[r]) p = OWN_Q ? o_lq[r] : s_lq[nt];
          p = o_ok[r] && s_ok[nt] ? p : 0.f;
          run_s[r] += p;
          P[acc_row(lane, r) * PL + nt * 16 + frag_row(lane)] = (__bf16)p;
        }
      }
    }
    if constexpr (ROLE != FWD)
      image_times_tile<DP>(sm.P[wave], sm.T[buf], acc2, D, lane);
  };

  stream_tiles(t_begin, t_end, fetch, stash, body);

  if constexpr (ROLE == FWD) {
    // merge the 16 lanes of each accumulator row, fixed order
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) {
        const float m2 = __shfl_xor(run_m[r], x);
        const float s2 = __shfl_xor(run_s[r], x);
        lse_merge(run_m[r], run_s[r], m2, s2);
      }
      if ((lane & 15) == 0 && o_ok[r]) {
        const long row = base + lrow0 + r;
        a.ws[(long)split * a.B + row] = run_m[r];
        a.ws[((long)nsplit + split) * a.B + row] = run_s[r];
      }
    }
  } else {
    // Every wave is past the loop's last barrier, so the stream buffers are
    // idle: with one split, wave w parks its tile in rows 16w.. of buffer 0.
    if (nsplit == 1) {
      park_store<DP, VEC>(acc2, sm.T[0] + wave * 16 * G::XL,
                          (OWN_Q ? a.dq : a.dw) + base * D, wave * 16, n_here,
                          D, D, lane,
                          [](float v, int, const __bf16*) { return v; });
    } else {
      float* part =
          (OWN_Q ? a.part_q : a.part_w) + ((long)split * n_own + base) * D;
#pragma unroll
      for (int nt = 0; nt < G::NT; ++nt) {
        const int col = nt * 16 + frag_row(lane);
        if (col < D) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (o_ok[r]) part[(long)(lrow0 + r) * D + col] = acc2[nt][r];
        }
      }
    }
    if constexpr (ROLE == ROLE_W) {
      float* out = nsplit == 1 ? a.dbias : a.part_b + (long)split * n_own;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float s = row_sum16(run_s[r]);
        if ((lane & 15) == 0 && o_ok[r]) out[base + lrow0 + r] = s;
      }
    }
  }
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void dot_softmax_fwd_kernel(Args a) {
  __shared__ __align__(16) Smem<DP, false> sm;
  const int ntiles = (int)(((long)a.V + TILE - 1) / TILE);
  const int t0 = blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, ntiles);
  pass_loop<FWD, DP, VEC>(a, sm, blockIdx.x, t0, t1, blockIdx.y, gridDim.y);
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void dot_softmax_bwd_kernel(Args a) {
  __shared__ __align__(16) Smem<DP, true> sm;
  const long blocks_q = (long)a.nQ * a.nsplit_q;
  if ((long)blockIdx.x < blocks_q) {
    const int own = blockIdx.x % a.nQ, split = blockIdx.x / a.nQ;
    const int ntiles = (int)(((long)a.V + TILE - 1) / TILE);
    const int t0 = split * a.tps_q;
    pass_loop<ROLE_Q, DP, VEC>(a, sm, own, t0, min(t0 + a.tps_q, ntiles),
                               split, a.nsplit_q);
  } else {
    const unsigned bid = (unsigned)((long)blockIdx.x - blocks_q);
    const int own = bid % a.nW, split = bid / a.nW;
    const int ntiles = (a.B + TILE - 1) / TILE;
    const int t0 = split * a.tps_w;
    pass_loop<ROLE_W, DP, VEC>(a, sm, own, t0, min(t0 + a.tps_w, ntiles),
                               split, a.nsplit_w);
  }
}

// One thread an example: the splits merged in split order.
__global__ __launch_bounds__(WAVES * WAVE) void dot_softmax_finish_kernel(
    const float* __restrict__ ws, const float* __restrict__ s_true,
    const long* __restrict__ labels, int nsplit, int B,
    float* __restrict__ lse, float* __restrict__ loss) {
  const int b = blockIdx.x * (WAVES * WAVE) + threadIdx.x;
  if (b >= B) return;
  float M = ws[b];
  for (int k = 1; k < nsplit; ++k) M = fmaxf(M, ws[(long)k * B + b]);
  float sum = 0.f;
  for (int k = 0; k < nsplit; ++k)
    sum += ws[((long)nsplit + k) * B + b] * expf(ws[(long)k * B + b] - M);
  const float l = M + logf(sum);
  lse[b] = l;
  float out = 0.f;                  // an ignored example: +0, s_true not read
  if (labels[b] != -1) out = l - s_true[b];
  loss[b] = out;
}

// out [n][D] bf16 = the sum over the splits, in split order, of part
// [nsplit][n][D], rounded once; one thread per 8 columns of a row. Where
// out_b is not null, out_b [n] = the same sum of part_b [nsplit][n].
template <bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void dot_softmax_reduce_kernel(
    const float* __restrict__ part, const float* __restrict__ part_b,
    int nsplit, long n, int D, __bf16* __restrict__ out,
    float* __restrict__ out_b) {
  const int ppr = (D + 7) / 8;
  const long idx = (long)blockIdx.x * (WAVES * WAVE) + threadIdx.x;
  if (idx >= n * ppr) return;
  const long row = idx / ppr;
  const int c = (int)(idx % ppr) * 8;
  float s[8] = {};
  for (int k = 0; k < nsplit; ++k) {
    const float* p = part + ((long)k * n + row) * D + c;
    if (VEC) {
      const f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[e] += lo[e]; s[4 + e] += hi[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (c + e < D) s[e] += p[e];
    }
  }
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)s[e];
  st_piece<VEC>(out + row * D, 0, c, D, D, o);
  if (c == 0 && out_b) {
    float t = 0.f;
    for (int k = 0; k < nsplit; ++k) t += part_b[(long)k * n + row];
    out_b[row] = t;
  }
}

void launch_reduce(const float* part, const float* part_b, int nsplit, long n,
                   int D, __bf16* out, float* out_b, hipStream_t stream) {
  const long threads = n * ((D + 7) / 8);
  const dim3 grid((unsigned)((threads + WAVES * WAVE - 1) / (WAVES * WAVE)));
  const dim3 block(WAVES * WAVE);
  if ((D & 7) == 0 && aligned16(out) && aligned16(part))
    hipLaunchKernelGGL(dot_softmax_reduce_kernel<true>, grid, block, 0, stream,
                       part, part_b, nsplit, n, D, out, out_b);
  else
    hipLaunchKernelGGL(dot_softmax_reduce_kernel<false>, grid, block, 0,
                       stream, part, part_b, nsplit, n, D, out, out_b);
}

int tiles_of(long n) { return (int)((n + TILE - 1) / TILE); }

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

DotSoftmaxPlan dot_softmax_plan(long B, long V, long splits) {
  const int over_v =
      stream_splits(V, splits == 0 ? stream_default_splits(B) : splits);
  const int over_b =
      stream_splits(B, splits == 0 ? stream_default_splits(V) : splits);
  return {over_v, over_v, over_b};
}

// q [B,D], w [V,D] bf16 contiguous; bias fp32 [V] or null; labels int64 [B]
// (-1: ignored; any other value outside [0, V) is memory-safe and leaves the
// example's loss meaningless); ws fp32 [2 * nsplit * B] and s_true fp32 [B]
// workspaces, nsplit = dot_softmax_plan(B, V, .).fwd; lse, loss fp32 [B].
// 1 <= B <= INT_MAX - 64, 1 <= V < 2^31, 1 <= D <= kDotSoftmaxMaxD.
void launch_dot_softmax_fwd(const void* q, const void* w, const float* bias,
                            const long* labels, float* ws, float* s_true,
                            float* lse, float* loss, int B, int V, int D,
                            int nsplit, hipStream_t stream) {
  Args a = {};
  a.q = (const __bf16*)q; a.w = (const __bf16*)w; a.bias = bias;
  a.labels = labels; a.ws = ws; a.s_true = s_true;
  a.B = B; a.V = V; a.D = D;
  a.tiles_per_split = (tiles_of(V) + nsplit - 1) / nsplit;
  const bool vec = (D & 7) == 0 && aligned16(q) && aligned16(w);
  const dim3 grid(tiles_of(B), nsplit), block(WAVES * WAVE);
  dispatch_dp_vec<kDotSoftmaxMaxD>(D, vec, [&](auto c) {
    hipLaunchKernelGGL(
        (dot_softmax_fwd_kernel<decltype(c)::dp, decltype(c)::vec>), grid,
        block, 0, stream, a);
  });
  hipLaunchKernelGGL(dot_softmax_finish_kernel,
                     dim3((B + WAVES * WAVE - 1) / (WAVES * WAVE)),
                     dim3(WAVES * WAVE), 0, stream, ws, s_true, labels, nsplit,
                     B, lse, loss);
}

// lse, loss: the forward's; g = dloss fp32 [B]; dq [B,D], dw [V,D] bf16 and
// dbias fp32 [V], all written whole. nsplit_q, nsplit_w: the plan's bwd_q and
// bwd_w, with tiles(B) * nsplit_q + tiles(V) * nsplit_w <= INT_MAX. part_q
// fp32 [nsplit_q * B * D] where nsplit_q > 1; part_w fp32 [nsplit_w * V * D]
// and part_b fp32 [nsplit_w * V] where nsplit_w > 1. Same bounds as the
// forward.
void launch_dot_softmax_bwd(const void* q, const void* w, const float* bias,
                            const long* labels, const float* lse,
                            const float* loss, const float* g, float* part_q,
                            float* part_w, float* part_b, void* dq, void* dw,
                            float* dbias, int B, int V, int D, int nsplit_q,
                            int nsplit_w, hipStream_t stream) {
  Args a = {};
  a.q = (const __bf16*)q; a.w = (const __bf16*)w; a.bias = bias;
  a.labels = labels; a.lse = lse; a.loss = loss; a.g = g;
  a.part_q = part_q; a.part_w = part_w; a.part_b = part_b;
  a.dq = (__bf16*)dq; a.dw = (__bf16*)dw; a.dbias = dbias;
  a.B = B; a.V = V; a.D = D;
  a.nQ = tiles_of(B); a.nW = tiles_of(V);
  a.nsplit_q = nsplit_q; a.nsplit_w = nsplit_w;
  a.tps_q = (a.nW + nsplit_q - 1) / nsplit_q;
  a.tps_w = (a.nQ + nsplit_w - 1) / nsplit_w;
  const bool vec = (D & 7) == 0 && aligned16(q) && aligned16(w) &&
                   aligned16(dq) && aligned16(dw);
  const long blocks = (long)a.nQ * nsplit_q + (long)a.nW * nsplit_w;
  const dim3 grid((unsigned)blocks), block(WAVES * WAVE);
  dispatch_dp_vec<kDotSoftmaxMaxD>(D, vec, [&](auto c) {
    hipLaunchKernelGGL(
        (dot_softmax_bwd_kernel<decltype(c)::dp, decltype(c)::vec>), grid,
        block, 0, stream, a);
  });
  if (nsplit_q > 1)
    launch_reduce(part_q, nullptr, nsplit_q, B, D, a.dq, nullptr, stream);
  if (nsplit_w > 1)
    launch_reduce(part_w, part_b, nsplit_w, V, D, a.dw, dbias, stream);
}

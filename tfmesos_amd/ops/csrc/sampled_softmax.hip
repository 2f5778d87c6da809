// Sampled softmax loss (candidate sampling; with the batch's own items as
// candidates, the in-batch-negatives loss), forward and backward.
//
//   h [B,D], w_true [B,D], w_samp [S,D] bf16; true_adj [B], samp_adj [S] fp32
//   (null = 0); labels [B], sampled [S] int64 (both or neither).
//   t[b] = h[b].w_true[b] + true_adj[b],  l[b,s] = h[b].w_samp[s] + samp_adj[s],
//   the pair (b,s) is dropped where sampled[s] == labels[b],
//   lse[b] = log(exp t[b] + sum_kept exp l[b,s]),  loss[b] = lse[b] - t[b].
//   With g = dloss: p[b,s] = g[b] exp(l[b,s] - lse[b]) (0 where dropped),
//   q[b] = g[b] (exp(t[b] - lse[b]) - 1) = g[b] expm1(-loss[b]),
//   dh = P W_samp + q w_true, dw_samp = P^T H, dw_true = q h,
//   dsamp_adj = column sums of P, dtrue_adj = q.
//
// One loop (pair_loop) serves the forward and both backward products, on the
// scheme of mfma_stream.h (geometry, leaf helpers, dispatch and split rule
// from there; the loop's pieces are written out here, see that file). A
// block of 4 waves OWNS 64 rows of one set — wave w the rows 16w..16w+15, as
// MFMA A fragments loaded once from global memory into registers — and
// STREAMS the other set through LDS in tiles of 64 rows, row-major [row][d]
// with a padded stride, two buffers: the global loads of tile i+1 are issued
// before the arithmetic of tile i and written to the other buffer after it,
// one barrier per tile. The side values of the streamed rows (adjustment or
// -lse, g, id) ride along in LDS. Scores of a 16 x 64 tile: 16x16x32 bf16
// MFMAs whose B fragment is a 16-byte LDS read of a streamed row.
//
//   FWD     owns examples, streams its split of the candidate tiles. Every
//           lane keeps a running (max, sum) for its 4 accumulator rows over
//           its own columns; the 16 lanes of a row merge once at the end
//           (xor shuffles, fixed order) and the block writes (max, sum) per
//           example to the workspace ws [2][nsplit][B]. The finishing kernel
//           computes the true score (16 lanes per example, guarded scalar
//           loads) and merges it with the splits, in split order.
//   ROLE_H  owns examples, streams all candidates: p from the recomputed
//           scores, rounded to bf16 into a wave-private LDS image (the A
//           operand), dh += P . W_samp with B fragments read back from the
//           same row-major tile through ds_read_b64_tr_b16. The epilogue adds
//           q w_true and writes dh, dw_true (from the A fragments, which are
//           row-contiguous per lane) and dtrue_adj.
//   ROLE_W  owns candidates, streams all examples (with -lse and g): the
//           same tile is P^T, dw_samp += P^T . H, dsamp_adj = its row sums.
//   The backward is one launch: blocks [0, nH) take ROLE_H, the rest ROLE_W.
//   Output tiles are rounded once, parked in the (then idle) stream buffer
//   and leave as 16-byte row-contiguous stores.
//
// D % 8 == 0 with 16-byte-aligned row bases takes b128 global accesses;
// anything else the element-wise guarded form of the same loads and stores.
// 1 <= D <= 256 (kSampledMaxD), DP = 64 / 128 / 256 columns of registers.
// No atomics, fixed order => bit-reproducible; nothing is read back.
#include "sampled_softmax.h"

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are kept out of this
// file's kernels; everything here is scalar fp32 or MFMA.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

#include "mfma_stream.h"

enum { FWD = 0, ROLE_H = 1, ROLE_W = 2 };

struct Args {
  const __bf16* h; const __bf16* w_true; const __bf16* w_samp;
  const float* samp_adj;          // null = 0
  const long* labels; const long* sampled;   // both or neither null
  const float* lse; const float* loss; const float* g;     // backward
  float* ws;                      // forward: [2][nsplit][B]
  __bf16* dh; __bf16* dw_true; __bf16* dw_samp;
  float* dtrue_adj; float* dsamp_adj;
  int B, S, D;
  int tiles_per_split;            // forward
  int nH;                         // backward: blocks of ROLE_H
};

template <int DP> struct Smem {
  __bf16 T[2][TILE * (DP + 8)];   // streamed tiles, [row][d]
  __bf16 P[WAVES][16 * PL];       // probabilities, wave-private [row][col]
  long id[2][TILE];
  float add[2][TILE];
  float mul[2][TILE];
};

// (m, s) <- merge of (m, s) and (m2, s2): s exp(m) + s2 exp(m2), max-factored
DEVINL void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  s = s * __expf(m - M) + s2 * __expf(m2 - M);
  m = M;
}

// One block's pass: owned tile `own_tile`, streamed tiles [t_begin, t_end).
template <int ROLE, int DP, bool VEC>
DEVINL void pair_loop(const Args& a, Smem<DP>& sm, int own_tile, int t_begin,
                      int t_end, int split, int nsplit) {
  constexpr int XL = DP + 8;
  constexpr int KS = DP / 32;       // K steps of the scores
  constexpr int NT = DP / 16;       // 16-column tiles of the output rows
  constexpr int PIECES = TILE * (DP / 8) / (WAVES * WAVE);   // == KS
  constexpr int PPR = DP / 8;       // 16-byte pieces per image row
  constexpr bool OWN_EX = ROLE != ROLE_W;   // the owned rows are examples
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int D = a.D;
  const __bf16* own = OWN_EX ? a.h : a.w_samp;
  const __bf16* str = OWN_EX ? a.w_samp : a.h;
  const int n_own = OWN_EX ? a.B : a.S;
  const int n_str = OWN_EX ? a.S : a.B;
  const long* own_ids = OWN_EX ? a.labels : a.sampled;
  const long* str_ids = OWN_EX ? a.sampled : a.labels;
  const bool has_ids = a.labels != nullptr;
  const int row0 = own_tile * OWN + wave * 16;
  const int arow = row0 + (lane & 15);      // this lane's A-fragment row
  const int kq = (lane >> 4) << 3;          // its K offset inside a step

  bf16x8 af[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    af[ks] = ld_piece<VEC>(own, arow, n_own, ks * 32 + kq, D, D);

  // side values of this lane's 4 accumulator rows
  float o_add[4], o_mul[4];
  long o_id[4];
  bool o_ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + (lane >> 4) * 4 + r;
    o_ok[r] = row < n_own;
    const int rr = o_ok[r] ? row : 0;
    o_id[r] = has_ids ? own_ids[rr] : 0;
    if (ROLE == FWD) {
      o_add[r] = 0.f; o_mul[r] = 1.f;
    } else if (ROLE == ROLE_H) {
      o_add[r] = -a.lse[rr]; o_mul[r] = a.g[rr];
    } else {
      o_add[r] = a.samp_adj ? a.samp_adj[rr] : 0.f; o_mul[r] = 1.f;
    }
  }

  // streamed tile t: global -> registers (fetch), registers -> LDS (stash)
  bf16x8 pre[PIECES];
  float pre_add = 0.f, pre_mul = 1.f;
  long pre_id = 0;
  auto fetch = [&](int t) {
    const int c0 = t * TILE;
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int q = tid + WAVES * WAVE * i;
      pre[i] = ld_piece<VEC>(str, c0 + q / PPR, n_str, (q % PPR) * 8, D, D);
    }
    if (tid < TILE) {
      const int row = c0 + tid;
      const bool ok = row < n_str;
      const int rr = ok ? row : 0;
      pre_id = has_ids ? str_ids[rr] : 0;
      if (OWN_EX) {
        pre_add = a.samp_adj ? a.samp_adj[rr] : 0.f; pre_mul = 1.f;
      } else {
        pre_add = -a.lse[rr]; pre_mul = a.g[rr];
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int q = tid + WAVES * WAVE * i;
      *(bf16x8*)&sm.T[buf][(q / PPR) * XL + (q % PPR) * 8] = pre[i];
    }
    if (tid < TILE) {
      sm.id[buf][tid] = pre_id;
      sm.add[buf][tid] = pre_add;
      sm.mul[buf][tid] = pre_mul;
    }
  };

  float run_m[4], run_s[4];         // FWD: running max / sum; else s = row sum
#pragma unroll
  for (int r = 0; r < 4; ++r) { run_m[r] = NEG; run_s[r] = 0.f; }
  f32x4 acc2[NT] = {};              // backward: 16 x DP output tile
  __bf16* P = sm.P[wave];

  if (t_begin < t_end) {
    fetch(t_begin);
    stash(0);
  }
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const int buf = (t - t_begin) & 1;
    const bool more = t + 1 < t_end;    // block-uniform
    if (more) fetch(t + 1);
    const __bf16* T = sm.T[buf];

    f32x4 acc[TILE / 16] = {};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks * 32 < D) {
#pragma unroll
        for (int nt = 0; nt < TILE / 16; ++nt) {
          const bf16x8 b = *(const bf16x8*)&T[(nt * 16 + (lane & 15)) * XL +
                                              ks * 32 + kq];
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], b, acc[nt],
                                                            0, 0, 0);
        }
      }
    }

    float s_add[TILE / 16], s_mul[TILE / 16];
    long s_id[TILE / 16];
    bool s_ok[TILE / 16];
#pragma unroll
    for (int nt = 0; nt < TILE / 16; ++nt) {
      const int col = nt * 16 + (lane & 15);
      s_add[nt] = sm.add[buf][col];
      s_mul[nt] = sm.mul[buf][col];
      s_id[nt] = sm.id[buf][col];
      s_ok[nt] = t * TILE + col < n_str;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sc[TILE / 16];
      bool kept[TILE / 16];
#pragma unroll
      for (int nt = 0; nt < TILE / 16; ++nt) {
        // (dot + adjustment) - lse in every role
        sc[nt] = OWN_EX ? (acc[nt][r] + s_add[nt]) + o_add[r]
                        : (acc[nt][r] + o_add[r]) + s_add[nt];
        kept[nt] = o_ok[r] && s_ok[nt] && !(has_ids && s_id[nt] == o_id[r]);
      }
      if (ROLE == FWD) {
        float mx = run_m[r];
#pragma unroll
        for (int nt = 0; nt < TILE / 16; ++nt)
          if (kept[nt]) mx = fmaxf(mx, sc[nt]);
        float s = run_s[r] * __expf(run_m[r] - mx);
#pragma unroll
        for (int nt = 0; nt < TILE / 16; ++nt)
          if (kept[nt]) s += __expf(sc[nt] - mx);
        run_m[r] = mx;
        run_s[r] = s;
      } else {
#pragma unroll
        for (int nt = 0; nt < TILE / 16; ++nt) {
          const float p =
              kept[nt] ? (o_mul[r] * s_mul[nt]) * __expf(sc[nt]) : 0.f;
          run_s[r] += p;
          P[((lane >> 4) * 4 + r) * PL + nt * 16 + (lane & 15)] = (__bf16)p;
        }
      }
    }

    if (ROLE != FWD) {
      wave_lds_sync();
#pragma unroll
      for (int k2 = 0; k2 < TILE / 32; ++k2) {
        const bf16x8 pa =
            *(const bf16x8*)&P[(lane & 15) * PL + k2 * 32 + kq];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt * 16 < D) {
            const bf16x8 b = tr_frag<XL>(T, k2 * 32 + kq, nt * 16, lane);
            acc2[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, b, acc2[nt],
                                                               0, 0, 0);
          }
        }
      }
      wave_lds_sync();              // P is rewritten by the next tile
    }

    if (more) stash(buf ^ 1);
    __syncthreads();
  }

  if (ROLE == FWD) {
    // merge the 16 lanes of each accumulator row, fixed order
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) {
        const float m2 = __shfl_xor(run_m[r], x);
        const float s2 = __shfl_xor(run_s[r], x);
        lse_merge(run_m[r], run_s[r], m2, s2);
      }
      const int row = row0 + (lane >> 4) * 4 + r;
      if ((lane & 15) == 0 && row < n_own) {
        a.ws[(long)split * a.B + row] = run_m[r];
        a.ws[((long)nsplit + split) * a.B + row] = run_s[r];
      }
    }
    return;
  }

  // ---- backward epilogue. Every wave is past the loop's last barrier, so
  // the stream buffers are idle: wave w parks its tile in rows 16w.. of
  // buffer 0.
  __bf16* R = sm.T[0] + wave * 16 * XL;
  float o_q[4] = {};
  if (ROLE == ROLE_H) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + (lane >> 4) * 4 + r;
      o_q[r] = o_ok[r] ? o_mul[r] * expm1f(-a.loss[row]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int q = lane + WAVE * i;
      *(bf16x8*)&R[(q / PPR) * XL + (q % PPR) * 8] =
          ld_piece<VEC>(a.w_true, row0 + q / PPR, n_own, (q % PPR) * 8, D,
                        D);
    }
    wave_lds_sync();
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    if (nt * 16 < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = ((lane >> 4) * 4 + r) * XL + nt * 16 + (lane & 15);
        float v = acc2[nt][r];
        if (ROLE == ROLE_H) v += o_q[r] * (float)R[at];
        R[at] = (__bf16)v;
      }
    }
  }
  wave_lds_sync();
  __bf16* out = ROLE == ROLE_H ? a.dh : a.dw_samp;
#pragma unroll
  for (int i = 0; i < PIECES; ++i) {
    const int q = lane + WAVE * i;
    const int row = row0 + q / PPR, c = (q % PPR) * 8;
    if (row < n_own && c < D)
      st_piece<VEC>(out, row, c, D, D,
                    *(const bf16x8*)&R[(q / PPR) * XL + c]);
  }

  if (ROLE == ROLE_H) {
    // dw_true[b] = q[b] h[b]: the A fragments are 16 bytes of a row per lane
    if (arow < n_own) {
      const float q = a.g[arow] * expm1f(-a.loss[arow]);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int k = ks * 32 + kq;
        if (k < D) {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (__bf16)(q * (float)af[ks][e]);
          st_piece<VEC>(a.dw_true, arow, k, D, D, o);
        }
      }
      if (lane < 16) a.dtrue_adj[arow] = q;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s = row_sum16(run_s[r]);
      const int row = row0 + (lane >> 4) * 4 + r;
      if ((lane & 15) == 0 && row < n_own) a.dsamp_adj[row] = s;
    }
  }
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void sampled_softmax_fwd_kernel(
    Args a) {
  __shared__ __align__(16) Smem<DP> sm;
  const int ntiles = (a.S + TILE - 1) / TILE;
  const int t0 = blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, ntiles);
  pair_loop<FWD, DP, VEC>(a, sm, blockIdx.x, t0, t1, blockIdx.y, gridDim.y);
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void sampled_softmax_bwd_kernel(
    Args a) {
  __shared__ __align__(16) Smem<DP> sm;
  if ((int)blockIdx.x < a.nH)
    pair_loop<ROLE_H, DP, VEC>(a, sm, blockIdx.x, 0, (a.S + TILE - 1) / TILE,
                               0, 1);
  else
    pair_loop<ROLE_W, DP, VEC>(a, sm, (int)blockIdx.x - a.nH, 0,
                               (a.B + TILE - 1) / TILE, 0, 1);
}

// The true score and the merge: 16 lanes per example. The splits are merged
// in split order after the true score.
constexpr int FIN_EX = WAVES * WAVE / 16;   // examples per block

__global__ __launch_bounds__(WAVES * WAVE) void sampled_softmax_finish_kernel(
    const __bf16* __restrict__ h, const __bf16* __restrict__ w_true,
    const float* __restrict__ true_adj, const float* __restrict__ ws,
    int nsplit, int B, int D, float* __restrict__ lse,
    float* __restrict__ loss) {
  const int b = blockIdx.x * FIN_EX + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const bool live = b < B;
  float dot = 0.f;
  if (live) {
    const __bf16* hb = h + (long)b * D;
    const __bf16* wb = w_true + (long)b * D;
    for (int d = sub; d < D; d += 16) dot += (float)hb[d] * (float)wb[d];
  }
  dot = row_sum16(dot);
  if (live && sub == 0) {
    const float t = dot + (true_adj ? true_adj[b] : 0.f);
    float M = t;
    for (int k = 0; k < nsplit; ++k) M = fmaxf(M, ws[(long)k * B + b]);
    float sum = expf(t - M);
    for (int k = 0; k < nsplit; ++k)
      sum += ws[((long)nsplit + k) * B + b] * expf(ws[(long)k * B + b] - M);
    const float l = M + logf(sum);
    lse[b] = l;
    loss[b] = l - t;
  }
}

template <int DP, bool VEC>
void launch_fwd_dp(const Args& a, int nsplit, hipStream_t stream) {
  const dim3 grid((a.B + OWN - 1) / OWN, nsplit), block(WAVES * WAVE);
  hipLaunchKernelGGL((sampled_softmax_fwd_kernel<DP, VEC>), grid, block, 0,
                     stream, a);
}

template <int DP, bool VEC>
void launch_bwd_dp(const Args& a, hipStream_t stream) {
  const dim3 grid(a.nH + (a.S + OWN - 1) / OWN), block(WAVES * WAVE);
  hipLaunchKernelGGL((sampled_softmax_bwd_kernel<DP, VEC>), grid, block, 0,
                     stream, a);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// the split rule of mfma_stream.h with its default number of splits
int sampled_softmax_nsplit(long B, long S) {
  return stream_splits(S, stream_default_splits(B));
}

// h, w_true [B,D], w_samp [S,D] bf16 contiguous; true_adj [B], samp_adj [S]
// fp32 or null; labels [B], sampled [S] int64, both or neither null;
// ws fp32 [2 * sampled_softmax_nsplit(B, S) * B]; lse, loss fp32 [B].
// B >= 1, S >= 1, 1 <= D <= kSampledMaxD.
void launch_sampled_softmax_fwd(const void* h, const void* w_true,
                                const void* w_samp, const float* true_adj,
                                const float* samp_adj, const long* labels,
                                const long* sampled, float* ws, float* lse,
                                float* loss, int B, int S, int D,
                                hipStream_t stream) {
  Args a = {};
  a.h = (const __bf16*)h; a.w_true = (const __bf16*)w_true;
  a.w_samp = (const __bf16*)w_samp;
  a.samp_adj = samp_adj; a.labels = labels; a.sampled = sampled;
  a.ws = ws; a.B = B; a.S = S; a.D = D;
  const int nsplit = sampled_softmax_nsplit(B, S);
  const int ntiles = (S + TILE - 1) / TILE;
  a.tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  const bool vec = (D & 7) == 0 && aligned16(h) && aligned16(w_samp);
  dispatch_dp_vec<kSampledMaxD>(D, vec, [&](auto c) {
    launch_fwd_dp<decltype(c)::dp, decltype(c)::vec>(a, nsplit, stream);
  });
  hipLaunchKernelGGL(sampled_softmax_finish_kernel,
                     dim3((B + FIN_EX - 1) / FIN_EX), dim3(WAVES * WAVE), 0,
                     stream, a.h, a.w_true, true_adj, ws, nsplit, B, D, lse,
                     loss);
}

// lse, loss: the forward's; g = dloss fp32 [B]; dh, dw_true [B,D] and
// dw_samp [S,D] bf16, dtrue_adj [B], dsamp_adj [S] fp32, all written whole.
// Same bounds as the forward.
void launch_sampled_softmax_bwd(const void* h, const void* w_true,
                                const void* w_samp, const float* samp_adj,
                                const long* labels, const long* sampled,
                                const float* lse, const float* loss,
                                const float* g, void* dh, void* dw_true,
                                void* dw_samp, float* dtrue_adj,
                                float* dsamp_adj, int B, int S, int D,
                                hipStream_t stream) {
  Args a = {};
  a.h = (const __bf16*)h; a.w_true = (const __bf16*)w_true;
  a.w_samp = (const __bf16*)w_samp;
  a.samp_adj = samp_adj; a.labels = labels; a.sampled = sampled;
  a.lse = lse; a.loss = loss; a.g = g;
  a.dh = (__bf16*)dh; a.dw_true = (__bf16*)dw_true;
  a.dw_samp = (__bf16*)dw_samp;
  a.dtrue_adj = dtrue_adj; a.dsamp_adj = dsamp_adj;
  a.B = B; a.S = S; a.D = D;
  a.nH = (B + OWN - 1) / OWN;
  const bool vec = (D & 7) == 0 && aligned16(h) && aligned16(w_true) &&
                   aligned16(w_samp) && aligned16(dh) && aligned16(dw_true) &&
                   aligned16(dw_samp);
  dispatch_dp_vec<kSampledMaxD>(D, vec, [&](auto c) {
    launch_bwd_dp<decltype(c)::dp, decltype(c)::vec>(a, stream);
  });
}

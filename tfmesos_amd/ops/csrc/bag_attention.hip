// Attention over CSR bags (ragged sequences), forward and backward.
//
//   q [n,H,D], k, v [m,H,D] bf16; offsets [B+1] over the n query rows,
//   kv_offsets [B+1] over the m key rows (the same array for self-attention).
//   For bag b, head h, query i and key j of that bag:
//   s = scale q[i,h].k[j,h], kept where !causal or pos(j) <= pos(i)
//   (positions inside the bag), p = softmax_j(s) over the kept keys,
//   out[i,h] = sum_j p v[j,h] (a query without kept keys: zero row),
//   lse[h,i] = log sum_j exp s (such a query: -1e30).
//   Backward: delta[h,i] = dout[i,h].out[i,h], p = exp(s - lse),
//   dP = dout V^T, dS = scale p (dP - delta), dq = dS K, dk = dS^T Q,
//   dv = P^T dout.
//
// Tile map: a bag of L rows has ceil(L/64) tiles; bag_tiles_kernel writes the
// exclusive prefix of the tile counts (queries and keys). The grid is sized
// from shapes alone ((n + 63 B) / 64 is an upper bound); a block finds its
// (bag, tile) by binary search in the prefix and leaves if it is past the
// total. blockIdx.y is the head; row r of head h starts at (r H + h) D.
//
// One loop (attn_loop) serves the three roles, on the scheme of
// mfma_stream.h. A block of 4 waves OWNS 64
// rows of one bag and head — wave w the rows 16w..16w+15, as MFMA A
// fragments in registers, one or two tensors — and STREAMS the bag's rows of
// the other side, two tensors, through LDS in tiles of 64 rows, row-major
// with a padded stride, two buffers each: the global loads of tile i+1 are
// issued before the arithmetic of tile i and written to the other buffer
// after it, one block barrier per tile.
//
//   FWD     owns Q, streams K and V. S = Q K^T (B fragment: 16-byte LDS read
//           of a K row); running row max, uniform over the 16 lanes of a row
//           (4 xor shuffles), the fp32 output tile O and the running sum l
//           are rescaled by exp(m_old - m_new); l adds the fp32 exp values;
//           P~ = exp(s - m) rounded to bf16 into a wave-private LDS image,
//           O += P~ V with B fragments read back from the row-major V tile
//           through ds_read_b64_tr_b16. Epilogue O / l, lse = m + log l.
//   ROLE_Q  owns Q and dO, streams K and V: p, dP = dO V^T, dS rounded into
//           the image, dQ += dS K (transpose reads of the K tile).
//   ROLE_K  owns K and V, streams Q and dO (lse and delta ride along in
//           LDS): the same tile is P^T / dS^T, dV += P^T dO, dK += dS^T Q,
//           through the one image, one after the other.
//   The backward is one launch after delta_kernel: blocks [0, nQ) take
//   ROLE_Q, the rest ROLE_K. Both roles evaluate p and dS by the same
//   operations. Causal: ROLE_Q and FWD stop at the diagonal tile, ROLE_K
//   starts there; every tile is masked per element.
//   Output tiles are rounded once, parked in the (then idle) stream buffer
//   and leave as 16-byte row-contiguous stores.
//
// D % 8 == 0 with 16-byte-aligned bases takes b128 global accesses; anything
// else the element-wise guarded form of the same loads and stores.
// 1 <= D <= 128 (kBagAttnMaxD), DP = 64 / 128 columns of registers. Every
// position derived from the offsets is clamped to the tensors, and a block
// whose tile lies past its bag leaves: offsets that break the CSR contract
// give an unspecified result inside the tensors' bounds.
// No atomics, fixed order => bit-reproducible; nothing is read back.
#include "bag_attention.h"

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are kept out of this
// file's kernels; everything here is scalar fp32 or MFMA.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

#include "mfma_stream.h"

enum { FWD = 0, ROLE_Q = 1, ROLE_K = 2 };

struct Args {
  const __bf16* q; const __bf16* k; const __bf16* v; const __bf16* dout;
  const long* qoff; const long* koff;     // CSR offsets [B+1]
  const int* qpre; const int* kpre;       // tile prefixes [B+1]
  const float* lse; const float* delta;   // backward, [H,n]
  __bf16* out; float* lse_out;            // forward
  __bf16* dq; __bf16* dk; __bf16* dv;
  int n, m, B, H, D;
  float scale;
  int causal;
  int nQ;                                 // backward: blocks of ROLE_Q
};

template <int DP> struct Smem {
  __bf16 T1[2][TILE * (DP + 8)];  // streamed tiles, [row][d]: K (Q in ROLE_K)
  __bf16 T2[2][TILE * (DP + 8)];  // V (dO in ROLE_K)
  __bf16 P[WAVES][16 * PL];       // wave-private [owned row][streamed row]
  float lse[2][TILE];             // ROLE_K: of the streamed queries
  float del[2][TILE];
};

// bag b of a CSR array over N rows, clamped: 0 <= s <= e <= N
DEVINL void bag_span(const long* __restrict__ off, int b, int N, int& s,
                     int& e) {
  long lo = off[b], hi = off[b + 1];
  lo = lo < 0 ? 0 : lo > N ? N : lo;
  hi = hi < lo ? lo : hi > N ? N : hi;
  s = (int)lo;
  e = (int)hi;
}

// block `bid` of a tile prefix pre[0..B] (pre[0] == 0, nondecreasing):
// pre[bag] <= bid < pre[bag + 1]; false when bid is past the total
DEVINL bool locate(const int* __restrict__ pre, int B, int bid, int& bag,
                   int& tile) {
  if (bid >= pre[B]) return false;
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= bid) lo = mid; else hi = mid - 1;
  }
  bag = lo;
  tile = bid - pre[lo];
  return true;
}

template <int ROLE, int DP, bool VEC>
DEVINL void attn_loop(const Args& a, Smem<DP>& sm, int bid, int head) {
  typedef Stream<DP> G;
  constexpr int NT = G::NT;
  constexpr bool OWN_Q = ROLE != ROLE_K;   // the owned rows are queries
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int D = a.D;
  const long rs = (long)a.H * D;

  int bag, tile;
  if (!locate(OWN_Q ? a.qpre : a.kpre, a.B, bid, bag, tile)) return;
  int q0, q1, k0, k1;
  bag_span(a.qoff, bag, a.n, q0, q1);
  bag_span(a.koff, bag, a.m, k0, k1);
  const int own_end = OWN_Q ? q1 : k1;
  const int str_lo = OWN_Q ? k0 : q0, str_end = OWN_Q ? k1 : q1;
  // a tile past the bag (offsets against the contract): nothing to own
  if (tile >= (own_end - (OWN_Q ? q0 : k0) + OWN - 1) / OWN) return;
  const int own0 = (OWN_Q ? q0 : k0) + tile * OWN;
  int t_begin = 0, t_end = (str_end - str_lo + TILE - 1) / TILE;
  if (a.causal) {
    if (OWN_Q) t_end = min(t_end, tile + 1); else t_begin = min(tile, t_end);
  }

  const long hd = (long)head * D;
  const __bf16* own1 = (OWN_Q ? a.q : a.k) + hd;
  const __bf16* own2 = (ROLE == ROLE_Q ? a.dout : a.v) + hd;
  const __bf16* str1 = (OWN_Q ? a.k : a.q) + hd;
  const __bf16* str2 = (OWN_Q ? a.v : a.dout) + hd;
  const long side = (long)head * a.n;       // lse / delta are [H,n]

  const int row0 = own0 + wave * 16;

  bf16x8 af1[G::KS], af2[G::KS];
  load_owned<DP, VEC>(af1, own1, row0, own_end, D, rs, lane);
  if (ROLE != FWD) load_owned<DP, VEC>(af2, own2, row0, own_end, D, rs, lane);

  // this lane's 4 accumulator rows: position inside the bag, side values
  int o_pos[4];
  bool o_ok[4];
  float o_lse[4], o_del[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + acc_row(lane, r);
    o_pos[r] = tile * OWN + wave * 16 + acc_row(lane, r);
    o_ok[r] = row < own_end;
    o_lse[r] = o_del[r] = 0.f;
    if (ROLE == ROLE_Q && o_ok[r]) {
      o_lse[r] = a.lse[side + row];
      o_del[r] = a.delta[side + row];
    }
  }

  // streamed tile t: global -> registers (fetch), registers -> LDS (stash)
  bf16x8 pre1[G::PIECES], pre2[G::PIECES];
  float pre_lse = 0.f, pre_del = 0.f;
  auto fetch = [&](int t) {
    const int c0 = str_lo + t * TILE;
    auto src = [&](int trow) { return c0 + trow < str_end ? c0 + trow : -1; };
    tile_fetch<DP, VEC>(pre1, str1, D, rs, tid, src);
    tile_fetch<DP, VEC>(pre2, str2, D, rs, tid, src);
    if (ROLE == ROLE_K && tid < TILE) {
      const int row = c0 + tid;
      const bool ok = row < str_end;
      pre_lse = ok ? a.lse[side + row] : 0.f;
      pre_del = ok ? a.delta[side + row] : 0.f;
    }
  };
  auto stash = [&](int buf) {
    tile_stash<DP>(sm.T1[buf], pre1, tid);
    tile_stash<DP>(sm.T2[buf], pre2, tid);
    if (ROLE == ROLE_K && tid < TILE) {
      sm.lse[buf][tid] = pre_lse;
      sm.del[buf][tid] = pre_del;
    }
  };

  float run_m[4], run_l[4];         // FWD: running max, per-lane part of l
#pragma unroll
  for (int r = 0; r < 4; ++r) { run_m[r] = NEG; run_l[r] = 0.f; }
  f32x4 accA[NT] = {};              // O (FWD), dQ (ROLE_Q), dV (ROLE_K)
  f32x4 accB[NT] = {};              // dK (ROLE_K only)
  __bf16* P = sm.P[wave];

  stream_tiles(t_begin, t_end, fetch, stash, [&](int t, int buf) {
    const __bf16* T1 = sm.T1[buf];
    const __bf16* T2 = sm.T2[buf];

    f32x4 acc[ST] = {};
    score_tile<DP>(af1, T1, acc, D, lane);

    bool kept[4][ST];
#pragma unroll
    for (int nt = 0; nt < ST; ++nt) {
      const int s_pos = t * TILE + nt * 16 + frag_row(lane);
      const bool s_ok = s_pos < str_end - str_lo;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        kept[r][nt] = o_ok[r] && s_ok &&
                      (!a.causal ||
                       (OWN_Q ? s_pos <= o_pos[r] : o_pos[r] <= s_pos));
    }

    if (ROLE == FWD) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sc[ST];
        float mx = run_m[r];
#pragma unroll
        for (int nt = 0; nt < ST; ++nt) {
          sc[nt] = a.scale * acc[nt][r];
          if (kept[r][nt]) mx = fmaxf(mx, sc[nt]);
        }
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x));
        const float alpha = __expf(run_m[r] - mx);
        run_m[r] = mx;
        float s = 0.f;
#pragma unroll
        for (int nt = 0; nt < ST; ++nt) {
          const float p = kept[r][nt] ? __expf(sc[nt] - mx) : 0.f;
          s += p;
          P[acc_row(lane, r) * PL + nt * 16 + frag_row(lane)] = (__bf16)p;
        }
        run_l[r] = run_l[r] * alpha + s;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) accA[nt][r] *= alpha;
      }
      image_times_tile<DP>(P, T2, accA, D, lane);
    } else {
      f32x4 accp[ST] = {};
      score_tile<DP>(af2, T2, accp, D, lane);
      float ds[4][ST];
#pragma unroll
      for (int nt = 0; nt < ST; ++nt) {
        const int col = nt * 16 + frag_row(lane);
        const float s_lse = ROLE == ROLE_K ? sm.lse[buf][col] : 0.f;
        const float s_del = ROLE == ROLE_K ? sm.del[buf][col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float lse = ROLE == ROLE_K ? s_lse : o_lse[r];
          const float del = ROLE == ROLE_K ? s_del : o_del[r];
          const float p =
              kept[r][nt] ? __expf(fmaf(a.scale, acc[nt][r], -lse)) : 0.f;
          ds[r][nt] = (a.scale * p) * (accp[nt][r] - del);
          if (ROLE == ROLE_K)
            P[acc_row(lane, r) * PL + col] = (__bf16)p;
        }
      }
      if (ROLE == ROLE_K)
        image_times_tile<DP>(P, T2, accA, D, lane);   // dV += P^T dO
#pragma unroll
      for (int nt = 0; nt < ST; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          P[acc_row(lane, r) * PL + nt * 16 + frag_row(lane)] =
              (__bf16)ds[r][nt];
      if (ROLE == ROLE_K)
        image_times_tile<DP>(P, T1, accB, D, lane);   // dK += dS^T Q
      else
        image_times_tile<DP>(P, T1, accA, D, lane);   // dQ += dS K
    }
  });

  // ---- epilogue. Every wave is past the loop's last barrier, so the stream
  // buffers are idle: wave w parks its tile in rows 16w.. of T1[0].
  __bf16* R = sm.T1[0] + wave * 16 * G::XL;
  float mul[4] = {1.f, 1.f, 1.f, 1.f};
  auto store = [&](const f32x4 (&acc)[NT], __bf16* dst) {
    park_store<DP, VEC>(acc, R, dst + hd, row0, own_end, D, rs, lane,
                        [&](float v, int r, const __bf16*) {
                          return v * mul[r];
                        });
    wave_lds_sync();                // R is rewritten by the next tile
  };
  if (ROLE == FWD) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float l = row_sum16(run_l[r]);
      mul[r] = l > 0.f ? 1.f / l : 0.f;
      const int row = row0 + acc_row(lane, r);
      if (frag_row(lane) == 0 && o_ok[r])
        a.lse_out[side + row] = l > 0.f ? run_m[r] + __logf(l) : NEG;
    }
    store(accA, a.out);
  } else if (ROLE == ROLE_Q) {
    store(accA, a.dq);
  } else {
    store(accA, a.dv);
    store(accB, a.dk);
  }
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void bag_attention_fwd_kernel(
    Args a) {
  __shared__ __align__(16) Smem<DP> sm;
  attn_loop<FWD, DP, VEC>(a, sm, blockIdx.x, blockIdx.y);
}

template <int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void bag_attention_bwd_kernel(
    Args a) {
  __shared__ __align__(16) Smem<DP> sm;
  if ((int)blockIdx.x < a.nQ)
    attn_loop<ROLE_Q, DP, VEC>(a, sm, blockIdx.x, blockIdx.y);
  else
    attn_loop<ROLE_K, DP, VEC>(a, sm, (int)blockIdx.x - a.nQ, blockIdx.y);
}

// delta[h,i] = sum_d dout[i,h,d] out[i,h,d]: 16 lanes per (row, head)
constexpr int DELTA_ROWS = WAVES * WAVE / 16;

__global__ __launch_bounds__(WAVES * WAVE) void bag_attention_delta_kernel(
    const __bf16* __restrict__ out, const __bf16* __restrict__ dout, int n,
    int H, int D, float* __restrict__ delta) {
  const long pair = (long)blockIdx.x * DELTA_ROWS + (threadIdx.x >> 4);
  const int sub = threadIdx.x & 15;
  const bool live = pair < (long)n * H;     // pair = row * H + head
  float dot = 0.f;
  if (live) {
    const __bf16* o = out + pair * D;
    const __bf16* g = dout + pair * D;
    for (int d = sub; d < D; d += 16) dot += (float)g[d] * (float)o[d];
  }
  dot = row_sum16(dot);
  if (live && sub == 0) delta[(pair % H) * n + pair / H] = dot;
}

// Exclusive prefix of the bags' tile counts, pre[0..B]; block 0 the query
// offsets, block 1 the key offsets. Thread t sums a contiguous run of bags,
// thread 0 scans the 256 partial sums, each thread writes its run.
constexpr int SCAN = 256;

__global__ __launch_bounds__(SCAN) void bag_tiles_kernel(
    const long* __restrict__ qoff, const long* __restrict__ koff, int n, int m,
    int B, int* __restrict__ qpre, int* __restrict__ kpre) {
  __shared__ int part[SCAN];
  const long* off = blockIdx.x ? koff : qoff;
  const int N = blockIdx.x ? m : n;
  int* pre = blockIdx.x ? kpre : qpre;
  const int tid = threadIdx.x;
  const int per = (B + SCAN - 1) / SCAN;
  const int b0 = (int)min((long)tid * per, (long)B), b1 = min(b0 + per, B);
  auto tiles = [&](int b) {
    int s, e;
    bag_span(off, b, N, s, e);
    return (e - s + OWN - 1) / OWN;
  };
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += tiles(b);
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < SCAN; ++i) {
      const int t = part[i];
      part[i] = run;
      run += t;
    }
  }
  __syncthreads();
  int run = part[tid];
  for (int b = b0; b < b1; ++b) {
    pre[b] = run;
    run += tiles(b);
  }
  if (tid == SCAN - 1) pre[B] = run;     // its run ends at B: the total
}

template <int DP, bool VEC>
void launch_fwd_dp(const Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)bag_attention_max_tiles(a.n, a.B), a.H);
  hipLaunchKernelGGL((bag_attention_fwd_kernel<DP, VEC>), grid,
                     dim3(WAVES * WAVE), 0, stream, a);
}

template <int DP, bool VEC>
void launch_bwd_dp(const Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)(a.nQ + bag_attention_max_tiles(a.m, a.B)), a.H);
  hipLaunchKernelGGL((bag_attention_bwd_kernel<DP, VEC>), grid,
                     dim3(WAVES * WAVE), 0, stream, a);
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// offsets, kv_offsets int64 [B+1] -> qpre, kpre int32 [B+1]. B >= 1.
void launch_bag_attention_tiles(const long* offsets, const long* kv_offsets,
                                int* qpre, int* kpre, int n, int m, int B,
                                hipStream_t stream) {
  hipLaunchKernelGGL(bag_tiles_kernel, dim3(2), dim3(SCAN), 0, stream, offsets,
                     kv_offsets, n, m, B, qpre, kpre);
}

// q [n,H,D], k, v [m,H,D] bf16 contiguous; out [n,H,D] bf16 and lse fp32
// [H,n], written whole when the offsets keep the CSR contract. n, m, B >= 1,
// 1 <= D <= kBagAttnMaxD, H <= 65535, bag_attention_max_tiles of both sides
// within int. qpre, kpre: launch_bag_attention_tiles, same stream.
void launch_bag_attention_fwd(const void* q, const void* k, const void* v,
                              const long* offsets, const long* kv_offsets,
                              const int* qpre, const int* kpre, void* out,
                              float* lse, int n, int m, int B, int H, int D,
                              float scale, bool causal, hipStream_t stream) {
  Args a = {};
  a.q = (const __bf16*)q; a.k = (const __bf16*)k; a.v = (const __bf16*)v;
  a.qoff = offsets; a.koff = kv_offsets; a.qpre = qpre; a.kpre = kpre;
  a.out = (__bf16*)out; a.lse_out = lse;
  a.n = n; a.m = m; a.B = B; a.H = H; a.D = D;
  a.scale = scale; a.causal = causal;
  const bool vec = (D & 7) == 0 && aligned16(q) && aligned16(k) &&
                   aligned16(v) && aligned16(out);
  dispatch_dp_vec<kBagAttnMaxD>(D, vec, [&](auto c) {
    launch_fwd_dp<decltype(c)::dp, decltype(c)::vec>(a, stream);
  });
}

// out, lse: the forward's; dout [n,H,D] bf16 contiguous; delta fp32 [H,n]
// workspace; dq [n,H,D], dk, dv [m,H,D] bf16. Same bounds as the forward.
void launch_bag_attention_bwd(const void* q, const void* k, const void* v,
                              const void* out, const void* dout,
                              const long* offsets, const long* kv_offsets,
                              const int* qpre, const int* kpre,
                              const float* lse, float* delta, void* dq,
                              void* dk, void* dv, int n, int m, int B, int H,
                              int D, float scale, bool causal,
                              hipStream_t stream) {
  Args a = {};
  a.q = (const __bf16*)q; a.k = (const __bf16*)k; a.v = (const __bf16*)v;
  a.dout = (const __bf16*)dout;
  a.qoff = offsets; a.koff = kv_offsets; a.qpre = qpre; a.kpre = kpre;
  a.lse = lse; a.delta = delta;
  a.dq = (__bf16*)dq; a.dk = (__bf16*)dk; a.dv = (__bf16*)dv;
  a.n = n; a.m = m; a.B = B; a.H = H; a.D = D;
  a.scale = scale; a.causal = causal;
  a.nQ = (int)bag_attention_max_tiles(n, B);
  const long pairs = (long)n * H;
  hipLaunchKernelGGL(bag_attention_delta_kernel,
                     dim3((unsigned)((pairs + DELTA_ROWS - 1) / DELTA_ROWS)),
                     dim3(WAVES * WAVE), 0, stream, (const __bf16*)out,
                     a.dout, n, H, D, delta);
  const bool vec = (D & 7) == 0 && aligned16(q) && aligned16(k) &&
                   aligned16(v) && aligned16(dout) && aligned16(dq) &&
                   aligned16(dk) && aligned16(dv);
  dispatch_dp_vec<kBagAttnMaxD>(D, vec, [&](auto c) {
    launch_bwd_dp<decltype(c)::dp, decltype(c)::vec>(a, stream);
  });
}

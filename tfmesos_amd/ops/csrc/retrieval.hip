// Scoring a query batch against a whole vocabulary without forming [B, V]:
// the k best items per query (dot_topk) and the rank of one given item per
// query (dot_rank).
//
//   q [B,D], w [V,D] bf16; bias [V] fp32 (null = 0, -inf masks an item out);
//   labels [B] int64 in [0, V).
//   s[b,j] = q[b].w[j] + bias[j]: fp32 dot product, then the bias.
//   Item j BEATS item i for a query iff s_j > s_i, or s_j == s_i and j < i.
//   dot_topk: the k items no k-th other item beats, best first;
//   dot_rank: the number of items that beat labels[b].
//   NaN scores are outside the contract.
//
// Keys. A score and its item index pack into one 64-bit key: the high word
// is the order-preserving image of the fp32 bits (all bits of a negative
// flipped, the sign bit of a non-negative set; -0 is read as +0), the low
// word is ~index. "Beats" is one unsigned compare and the score comes back
// exactly. Key 0 is "no item": a real -inf has the high word 0x007fffff.
//
// One loop (score_loop) serves three roles. On the scheme of mfma_stream.h a
// block of 4 waves OWNS 64 queries — wave w the rows 16w..16w+15, as MFMA A
// fragments in registers — and STREAMS item tiles of 64 rows through two
// row-major LDS buffers of stride DP + 8, the bias riding along: the global
// loads of tile i+1 are issued before the arithmetic of tile i and written to
// the other buffer after it, one block barrier per tile. The 64 scores of a
// row in a tile sit in the 16 lanes of ONE wave (4 accumulators x 1 column a
// lane), so everything per row below is wave-private.
//
//   TOPK   streams its split of the tiles. Each owned row has a candidate
//          buffer of CAP = 128 keys in LDS, a count and a threshold key (the
//          row's k-th best so far; 0 until a compaction has seen k items). A
//          key above the threshold is appended at a slot taken from the
//          row's integer LDS counter; the slot order does not reach the
//          result, since keys are distinct and only ever sorted. A tile
//          whose keys all fail (wave-uniform test) costs nothing more.
//          Otherwise the lanes first add up, per row, how many keys would
//          join (a second integer counter), and a row they would overflow is
//          COMPACTED before they do: the wave sorts its 128 slots descending
//          (bitonic network, two keys a lane, compare-exchange over
//          __shfl_xor), keeps the first k, and the k-th becomes the
//          threshold; at most 64 keys then join k <= 64. After the
//          last tile every row is compacted and its k keys go to the
//          workspace ws [nsplit][B][k]. dot_topk_merge_kernel (one wave a
//          query) folds the nsplit lists in split order through the same
//          sort and unpacks values and indices.
//   TRUE   one gathered tile: the block stages the rows w[labels[b]] of its
//          own 64 queries (and their biases) as the tile, runs the same K
//          steps, and keeps the diagonal as the key (s_true, labels[b]) in
//          true_key [B]. The score of the labelled item is thereby the very
//          number the other two roles compute for it.
//   COUNT  streams its split with no buffers: every lane counts, per
//          accumulator row, the keys above the row's true key (the item
//          itself compares equal). The 16 lanes of a row add up after the
//          last tile, ws [nsplit][B] takes the counts, dot_rank_finish_kernel
//          sums them in split order.
//
// D % 8 == 0 with 16-byte-aligned bases takes b128 global loads; anything
// else the element-wise guarded form. 1 <= D <= 256 (kDotTopkMaxD), DP = 64 /
// 128 / 256 columns of registers; 1 <= k <= 64 (kDotTopkMaxK) <= V < 2^31.
// No float atomics, nothing [B, V]-sized, nothing read back; results do not
// depend on the order of the integer slot counter => bit-reproducible.
#include "retrieval.h"

// The packed fp32 VALU forms (v_pk_add/mul/fma_f32) are kept out of this
// file's kernels; everything here is scalar fp32, integer or MFMA.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

#include "mfma_stream.h"

typedef unsigned long long u64;

constexpr int CAP = 128;          // candidate keys per owned row
constexpr int KROW = CAP + 2;     // buffer row stride: rows 4 banks apart
enum { TOPK = 0, TRUE_SCORE = 1, COUNT = 2 };

struct Args {
  const __bf16* q; const __bf16* w;
  const float* bias;              // null = 0
  const long* labels;             // TRUE_SCORE
  u64* true_key;                  // [B]: TRUE_SCORE writes, COUNT reads
  u64* ws;                        // TOPK [nsplit][B][k] keys, COUNT [nsplit][B]
  int B, V, D, k;
  int tiles_per_split;
};

template <int DP, bool SELECT> struct Smem {
  __bf16 T[2][TILE * (DP + 8)];   // streamed tiles, [row][d]
  float bias[2][TILE];
};
template <int DP> struct Smem<DP, true> : Smem<DP, false> {
  u64 keys[OWN][KROW];            // candidates, unordered past a row's first k
  u64 thr[OWN];                   // a key must exceed it to be appended
  int cnt[OWN];
  int pend[OWN];                  // keys of the tile at hand above thr
};

DEVINL u64 make_key(float s, unsigned j) {
  unsigned u = __float_as_uint(s);
  u = u == 0x80000000u ? 0u : u;                    // -0 orders as +0
  u ^= (unsigned)((int)u >> 31) | 0x80000000u;
  return ((u64)u << 32) | (unsigned)~j;
}
DEVINL float key_value(u64 key) {
  unsigned u = (unsigned)(key >> 32);
  u ^= (unsigned)((int)~u >> 31) | 0x80000000u;
  return __uint_as_float(u);
}
DEVINL long key_index(u64 key) { return (long)(unsigned)~(unsigned)key; }

DEVINL u64 umax(u64 a, u64 b) { return a > b ? a : b; }
DEVINL u64 umin(u64 a, u64 b) { return a > b ? b : a; }

// Sorts the wave's 128 keys descending: element e < 64 is x0 of lane e,
// element 64 + e is x1 of lane e. Bitonic network; a 2^j-block with bit j of
// its element index clear is sorted descending, the other ascending.
DEVINL void sort128(u64& x0, u64& x1, int lane) {
#pragma unroll
  for (int size = 2; size <= 2 * WAVE; size <<= 1) {
    const bool desc0 = (lane & size) == 0;          // true at size 64, 128
    const bool desc1 = size == 2 * WAVE || (size != WAVE && desc0);
#pragma unroll
    for (int stride = size >> 1; stride >= 1; stride >>= 1) {
      if (stride == WAVE) {                         // within the lane
        const u64 hi = umax(x0, x1), lo = umin(x0, x1);
        x0 = hi; x1 = lo;
      } else {
        const bool lower = (lane & stride) == 0;
        const u64 y0 = __shfl_xor(x0, stride), y1 = __shfl_xor(x1, stride);
        x0 = desc0 == lower ? umax(x0, y0) : umin(x0, y0);
        x1 = desc1 == lower ? umax(x1, y1) : umin(x1, y1);
      }
    }
  }
}

// The whole wave compacts one owned row: sort, keep the first k (slots past
// the count are "no item"). Returns lane e's key of rank e. The caller
// fences before (the appends) and after (the count and threshold).
template <class S>
DEVINL u64 compact_row(S& sm, int row, int k, int lane) {
  const int n = sm.cnt[row];
  u64* K = sm.keys[row];
  u64 x0 = lane < n ? K[lane] : 0, x1 = lane + WAVE < n ? K[lane + WAVE] : 0;
  sort128(x0, x1, lane);
  if (lane < k) K[lane] = x0;     // a lane rewrites only a slot it read
  if (lane == k - 1) sm.thr[row] = x0;
  if (lane == 0) sm.cnt[row] = k;
  return x0;
}

// One block's pass: owned tile `own_tile`, streamed tiles [t_begin, t_end)
// (TRUE_SCORE: the one gathered tile).
template <int ROLE, int DP, bool VEC>
DEVINL void score_loop(const Args& a, Smem<DP, ROLE == TOPK>& sm, int own_tile,
                       int t_begin, int t_end, int split) {
  typedef Stream<DP> G;
  constexpr int NT = ST;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int D = a.D, V = a.V, k = a.k;
  const int row0 = own_tile * OWN + wave * 16;
  const int lrow0 = wave * 16 + acc_row(lane, 0);   // first accumulator row

  bf16x8 af[G::KS];
  load_owned<DP, VEC>(af, a.q, row0, a.B, D, D, lane);

  bool o_ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o_ok[r] = own_tile * OWN + lrow0 + r < a.B;

  // the item staged as tile row `trow` of tile t, or -1
  auto item = [&](int t, int trow) -> long {
    if (ROLE == TRUE_SCORE) {
      const int b = own_tile * OWN + trow;
      const long j = b < a.B ? a.labels[b] : -1;
      return j >= 0 && j < V ? j : -1;      // memory-safe whatever the label
    }
    const long j = (long)t * TILE + trow;
    return j < V ? j : -1;
  };

  // streamed tile t: global -> registers (fetch), registers -> LDS (stash)
  bf16x8 pre[G::PIECES];
  float pre_bias = 0.f;
  auto fetch = [&](int t) {
    tile_fetch<DP, VEC>(pre, a.w, D, D, tid,
                        [&](int trow) { return item(t, trow); });
    if (tid < TILE) {
      const long j = item(t, tid);
      pre_bias = a.bias && j >= 0 ? a.bias[j] : 0.f;
    }
  };
  auto stash = [&](int buf) {
    tile_stash<DP>(sm.T[buf], pre, tid);
    if (tid < TILE) sm.bias[buf][tid] = pre_bias;
  };

  u64 tk[4] = {};                   // COUNT: the rows' true keys
  int above[4] = {};                // COUNT: keys seen above them
  if constexpr (ROLE == COUNT) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      tk[r] = o_ok[r] ? a.true_key[own_tile * OWN + lrow0 + r] : ~0ull;
  }
  if constexpr (ROLE == TOPK) {
    if (lane < 16) {
      sm.cnt[wave * 16 + lane] = 0;
      sm.pend[wave * 16 + lane] = 0;
      sm.thr[wave * 16 + lane] = 0;
    }
  }

  fetch(t_begin);
  stash(0);
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const int buf = (t - t_begin) & 1;
    const bool more = t + 1 < t_end;    // block-uniform
    if (more) fetch(t + 1);

    f32x4 acc[NT] = {};
    score_tile<DP>(af, sm.T[buf], acc, D, lane);

    float s_bias[NT];
    unsigned s_col[NT];             // < 2^31 + 64: no wrap
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      s_bias[nt] = sm.bias[buf][nt * 16 + frag_row(lane)];
      s_col[nt] = (unsigned)t * TILE + nt * 16 + frag_row(lane);
    }

    if constexpr (ROLE == TOPK) {
      u64 key[4][NT];
      int pass[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u64 thr = sm.thr[lrow0 + r];
        pass[r] = 0;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          key[r][nt] = o_ok[r] && s_col[nt] < (unsigned)V
                           ? make_key(acc[nt][r] + s_bias[nt], s_col[nt])
                           : 0;
          pass[r] += key[r][nt] > thr;
        }
      }
      // wave-uniform: most tiles of a long stream pass nothing
      if (__any((pass[0] | pass[1]) | (pass[2] | pass[3]))) {
        // a row that this tile's keys would overflow is compacted first;
        // its threshold rises, and at most 64 keys join its k <= 64
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pass[r]) atomicAdd(&sm.pend[lrow0 + r], pass[r]);
        wave_lds_sync();
        int c = 0;
        if (lane < 16) {
          c = sm.cnt[wave * 16 + lane] + sm.pend[wave * 16 + lane];
          sm.pend[wave * 16 + lane] = 0;
        }
        u64 full = __ballot(c > CAP);               // wave-uniform
        while (full) {
          compact_row(sm, wave * 16 + __ffsll((long long)full) - 1, k, lane);
          full &= full - 1;
        }
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const u64 thr = sm.thr[lrow0 + r];
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            if (key[r][nt] > thr)
              sm.keys[lrow0 + r][atomicAdd(&sm.cnt[lrow0 + r], 1)] =
                  key[r][nt];
        }
      }
    } else if constexpr (ROLE == COUNT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const u64 key = s_col[nt] < (unsigned)V
                              ? make_key(acc[nt][r] + s_bias[nt], s_col[nt])
                              : 0;
          above[r] += key > tk[r];
        }
      }
    } else {
      // the diagonal of the 64 x 64 tile: accumulator `wave`, the lane whose
      // column is its row
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt == wave && frag_row(lane) == acc_row(lane, r) && o_ok[r]) {
            const int b = own_tile * OWN + lrow0 + r;
            a.true_key[b] =
                make_key(acc[nt][r] + s_bias[nt], (unsigned)a.labels[b]);
          }
        }
      }
    }

    if (more) stash(buf ^ 1);
    __syncthreads();
  }

  if constexpr (ROLE == TOPK) {
    wave_lds_sync();
    for (int r = 0; r < 16; ++r) {
      const u64 x = compact_row(sm, wave * 16 + r, k, lane);
      const int b = row0 + r;
      if (b < a.B && lane < k) a.ws[((long)split * a.B + b) * k + lane] = x;
    }
  } else if constexpr (ROLE == COUNT) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int x = 1; x < 16; x <<= 1) above[r] += __shfl_xor(above[r], x);
      if ((lane & 15) == 0 && o_ok[r])
        a.ws[(long)split * a.B + own_tile * OWN + lrow0 + r] = (u64)above[r];
    }
  }
}

template <int ROLE, int DP, bool VEC>
__global__ __launch_bounds__(WAVES * WAVE) void dot_score_kernel(Args a) {
  __shared__ __align__(16) Smem<DP, ROLE == TOPK> sm;
  if (ROLE == TRUE_SCORE) {
    score_loop<ROLE, DP, VEC>(a, sm, blockIdx.x, 0, 1, 0);
  } else {
    const int ntiles = (int)(((long)a.V + TILE - 1) / TILE);
    const int t0 = blockIdx.y * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, ntiles);
    score_loop<ROLE, DP, VEC>(a, sm, blockIdx.x, t0, t1, blockIdx.y);
  }
}

// One wave a query: the running best 64 in x0, the next split's list in x1,
// one sort per split, in split order.
__global__ __launch_bounds__(WAVES * WAVE) void dot_topk_merge_kernel(
    const u64* __restrict__ ws, int nsplit, int B, int k,
    float* __restrict__ values, long* __restrict__ indices) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;               // wave-uniform; no block barrier below
  u64 x0 = 0;
  for (int s = 0; s < nsplit; ++s) {
    u64 x1 = lane < k ? ws[((long)s * B + b) * k + lane] : 0;
    sort128(x0, x1, lane);
  }
  if (lane < k) {
    values[(long)b * k + lane] = key_value(x0);
    indices[(long)b * k + lane] = key_index(x0);
  }
}

__global__ __launch_bounds__(WAVES * WAVE) void dot_rank_finish_kernel(
    const u64* __restrict__ ws, int nsplit, int B, long* __restrict__ rank) {
  const int b = blockIdx.x * (WAVES * WAVE) + threadIdx.x;
  if (b >= B) return;
  long n = 0;
  for (int s = 0; s < nsplit; ++s) n += (long)ws[(long)s * B + b];
  rank[b] = n;
}

template <int ROLE>
void launch_score(const Args& a, int nsplit, hipStream_t stream) {
  const bool vec = (a.D & 7) == 0 && aligned16(a.q) && aligned16(a.w);
  const dim3 grid((a.B + OWN - 1) / OWN, nsplit), block(WAVES * WAVE);
  dispatch_dp_vec<kDotTopkMaxD>(a.D, vec, [&](auto c) {
    hipLaunchKernelGGL(
        (dot_score_kernel<ROLE, decltype(c)::dp, decltype(c)::vec>), grid,
        block, 0, stream, a);
  });
}

Args make_args(const void* q, const void* w, const float* bias, int B, int V,
               int D, int nsplit) {
  Args a = {};
  a.q = (const __bf16*)q; a.w = (const __bf16*)w; a.bias = bias;
  a.B = B; a.V = V; a.D = D;
  const int ntiles = (int)(((long)V + TILE - 1) / TILE);
  a.tiles_per_split = (ntiles + nsplit - 1) / nsplit;
  return a;
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// the split rule of mfma_stream.h
int dot_topk_nsplit(long B, long V) { return dot_topk_splits(B, V, 0); }

int dot_topk_splits(long B, long V, long splits) {
  return stream_splits(V, splits == 0 ? stream_default_splits(B) : splits);
}

// q [B,D], w [V,D] bf16 contiguous; bias fp32 [V] or null; ws int64
// [nsplit * B * k] with nsplit = dot_topk_splits(B, V, .); values fp32 and
// indices int64 [B,k]. B >= 1, 1 <= k <= kDotTopkMaxK, k <= V < 2^31,
// 1 <= D <= kDotTopkMaxD.
void launch_dot_topk(const void* q, const void* w, const float* bias,
                     long* ws, float* values, long* indices, int B, int V,
                     int D, int k, int nsplit, hipStream_t stream) {
  Args a = make_args(q, w, bias, B, V, D, nsplit);
  a.k = k;
  a.ws = (u64*)ws;
  launch_score<TOPK>(a, nsplit, stream);
  hipLaunchKernelGGL(dot_topk_merge_kernel, dim3((B + WAVES - 1) / WAVES),
                     dim3(WAVES * WAVE), 0, stream, a.ws, nsplit, B, k, values,
                     indices);
}

// labels int64 [B] (a label outside [0, V) is scored as a zero row with no
// bias: memory-safe, meaningless); true_key int64 [B], ws int64
// [nsplit * B] workspaces; rank int64 [B]. Same bounds as above.
void launch_dot_rank(const void* q, const void* w, const float* bias,
                     const long* labels, long* true_key, long* ws, long* rank,
                     int B, int V, int D, int nsplit, hipStream_t stream) {
  Args a = make_args(q, w, bias, B, V, D, nsplit);
  a.labels = labels;
  a.true_key = (u64*)true_key;
  a.ws = (u64*)ws;
  launch_score<TRUE_SCORE>(a, 1, stream);
  launch_score<COUNT>(a, nsplit, stream);
  hipLaunchKernelGGL(dot_rank_finish_kernel,
                     dim3((B + WAVES * WAVE - 1) / (WAVES * WAVE)),
                     dim3(WAVES * WAVE), 0, stream, a.ws, nsplit, B, rank);
}

// Worker-side routing of requests to a row-sharded embedding table: the
// stable partition of the ids by owning shard, the matching permutation
// (and wire-dtype cast) of gradient rows, the per-shard CSR of a bagged
// request and the bag coefficients.
//
// Routing rule (route(), shared by every kernel) for V rows in S shards:
//   * mod: shard = id % S, local = id / S.
//   * div (TF's rule): q = V / S, x = V % S; the first x shards hold q+1
//     rows, the rest q. shard = max(id / (q+1), (id - x) / q),
//     local = id - start(shard), start(s) = s*q + min(s, x).
//   * an id outside [0, V) goes to shard 0 with local = -1 (out of range
//     on every shard: pulls give a zero row, pushes ignore it). The range
//     is tested before any % (C's remainder is negative for negative ids).
//
// Stable partition = count, scan, scatter, no atomics:
//   * count: one lane per position, one wave per 64-position window; the
//     wave ballots each shard and writes the popcounts shard-major
//     (counts[s * W + w], W = number of windows).
//   * the inclusive scan of that array is plumbing (torch.cumsum in the
//     binding): its element s*W + w - 1 is the first slot of window w's
//     members of shard s, so shards come out grouped and, inside a shard,
//     windows (and positions) stay in order.
//   * scatter: recomputes the shard, ranks the lane among the window's
//     lanes of the same shard (popcount of the ballot below the lane) and
//     writes local / perm / inv; the first wave also writes starts.
//   Fixed slots, no atomics => two runs give identical bits. Grids are
//   sized from n; nothing is read back.
//
// Row permute + cast: out[j] = cast(rows[perm[j]]), one wave per row, in
// 256-column tiles (tile.h): f32x4 / bf16x4 when D % 4 == 0 and the bases
// are 16-byte aligned, scalar otherwise.
//
// Per-shard CSR: the partition is stable, so perm is increasing inside a
// shard and every bag stays contiguous there:
// shard_offsets[s][b] = lower_bound(perm[starts[s]:starts[s+1]], offsets[b]),
// one thread per (s, b).
//
// Bag coefficients: c[i] of bag.h (bag_weight_sum / bag_coef), one wave
// per bag — the bits the pooled kernels compute internally.
#include "common.h"

#include "bag.h"
#include "partition.h"
#include "run_sum.h"

namespace {

constexpr int WAVES = 4;   // waves (64-position windows) per block

struct Route {
  long V;
  long q;      // V / S
  long x;      // V % S
  int S;
  int div;
};

DEVINL void route(const Route& r, long id, int& shard, long& local) {
  if (id < 0 || id >= r.V) {
    shard = 0;
    local = -1;
    return;
  }
  if (!r.div) {
    shard = (int)(id % r.S);
    local = id / r.S;
    return;
  }
  const long a = id / (r.q + 1), b = (id - r.x) / r.q;   // q >= 1: V >= S
  const long s = a > b ? a : b;
  shard = (int)s;
  local = id - (s * r.q + (s < r.x ? s : r.x));
}

__global__ __launch_bounds__(WAVES * WAVE) void shard_count_kernel(
    const long* __restrict__ ids, int* __restrict__ counts, long n, long W,
    Route r) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= W) return;   // wave-uniform
  const long i = w * WAVE + lane;
  int shard = -1;
  long local = -1;
  if (i < n) route(r, ids[i], shard, local);
  int mine = 0;
  for (int s = 0; s < r.S; ++s) {
    const unsigned long long m = __ballot(shard == s);
    if (lane == s) mine = __popcll(m);
  }
  if (lane < r.S) counts[(long)lane * W + w] = mine;
}

// incl: inclusive scan of counts. n > 0.
__global__ __launch_bounds__(WAVES * WAVE) void shard_scatter_kernel(
    const long* __restrict__ ids, const long* __restrict__ incl,
    long* __restrict__ local_out, long* __restrict__ perm,
    long* __restrict__ inv, long* __restrict__ starts, long n, long W,
    Route r) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= W) return;   // wave-uniform
  if (w == 0) {
    // starts[s] = members of the shards before s; lanes 0..63 cover S+1
    for (int s = lane; s <= r.S; s += WAVE)
      starts[s] = s == 0 ? 0 : incl[(long)s * W - 1];
  }
  const long i = w * WAVE + lane;
  int shard = -1;
  long local = -1;
  if (i < n) route(r, ids[i], shard, local);
  // the lanes of this window that share the lane's shard
  unsigned long long same = 0;
  unsigned long long todo = __ballot(shard >= 0);
  while (todo) {
    const int lead = __ffsll(todo) - 1;
    const int s0 = __shfl(shard, lead);
    const unsigned long long m = __ballot(shard == s0);
    if (shard == s0) same = m;
    todo &= ~m;
  }
  if (shard < 0) return;
  const long idx = (long)shard * W + w;
  const long base = idx == 0 ? 0 : incl[idx - 1];
  const long slot = base + __popcll(same & ((1ull << lane) - 1ull));
  if (slot < 0 || slot >= n) return;   // cannot happen with a true scan
  local_out[slot] = local;
  perm[slot] = i;
  inv[i] = slot;
}

template <typename T, typename O, int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void permute_rows_kernel(
    const T* __restrict__ rows, const long* __restrict__ perm,
    O* __restrict__ out, long n_out, long n_rows, int D) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long j = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (j >= n_out) return;   // wave-uniform
  long src = perm[j];
  if (src >= n_rows) src = -1;   // outside [0, n_rows): a zero row
  for (int c0 = 0; c0 < D; c0 += TILE) {
    float v[ACC];
    ld_row<T, VEC>(rows, src, c0, lane, D, v);
    st_tile<O, VEC>(out + j * D, c0, lane, D, v);
  }
}

// out[s * (B+1) + b], b in [0, B]: one thread per element.
__global__ __launch_bounds__(WAVES * WAVE) void shard_bag_offsets_kernel(
    const long* __restrict__ perm, const long* __restrict__ starts,
    const long* __restrict__ offsets, long* __restrict__ out, long n, long B,
    int S) {
  const long t = (long)blockIdx.x * (WAVES * WAVE) + threadIdx.x;
  if (t >= (long)S * (B + 1)) return;
  const int s = (int)(t / (B + 1));
  const long b = t % (B + 1);
  const long first = clamp_pos(starts[s], n);
  long last = clamp_pos(starts[s + 1], n);
  if (last < first) last = first;
  const long want = clamp_pos(offsets[b], n);
  long lo = first, hi = last;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (perm[mid] < want) lo = mid + 1; else hi = mid;
  }
  out[t] = lo - first;
}

// coef arrives zeroed: a position no bag covers keeps 0.
__global__ __launch_bounds__(WAVES * WAVE) void bag_coef_kernel(
    const long* __restrict__ offsets, const float* __restrict__ weights,
    float* __restrict__ coef, long B, long n, int mean) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long b = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;   // wave-uniform
  long s, e;
  bag_range(offsets, b, n, s, e);
  const float W = mean ? bag_weight_sum(weights, s, e, lane) : 0.f;
  for (long p = s + lane; p < e; p += WAVE)
    coef[p] = bag_coef(weights ? weights[p] : 1.f, W, mean != 0);
}

template <typename T, typename O>
void permute_typed(const T* rows, const long* perm, O* out, long n_out,
                   long n_rows, int D, hipStream_t stream) {
  const dim3 block(WAVES * WAVE);
  const dim3 grid((unsigned)((n_out + WAVES - 1) / WAVES));
  if (tile_vec4(D, rows, out))
    hipLaunchKernelGGL((permute_rows_kernel<T, O, 4>), grid, block, 0, stream,
                       rows, perm, out, n_out, n_rows, D);
  else
    hipLaunchKernelGGL((permute_rows_kernel<T, O, 1>), grid, block, 0, stream,
                       rows, perm, out, n_out, n_rows, D);
}

Route make_route(long V, int S, bool div) {
  Route r;
  r.V = V;
  r.q = V / S;
  r.x = V % S;
  r.S = S;
  r.div = div ? 1 : 0;
  return r;
}

}  // namespace

// Number of 64-position windows of n ids; counts is int32 [S * windows].
long shard_windows(long n) { return (n + WAVE - 1) / WAVE; }

// n > 0, 1 <= S <= 64, V >= S.
void launch_shard_count(const long* ids, int* counts, long n, long V, int S,
                        bool div, hipStream_t stream) {
  const long W = shard_windows(n);
  const dim3 grid((unsigned)((W + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(shard_count_kernel, grid, dim3(WAVES * WAVE), 0, stream,
                     ids, counts, n, W, make_route(V, S, div));
}

// incl: int64 inclusive scan of counts. local/perm/inv [n], starts [S+1].
void launch_shard_scatter(const long* ids, const long* incl, long* local,
                          long* perm, long* inv, long* starts, long n, long V,
                          int S, bool div, hipStream_t stream) {
  const long W = shard_windows(n);
  const dim3 grid((unsigned)((W + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(shard_scatter_kernel, grid, dim3(WAVES * WAVE), 0,
                     stream, ids, incl, local, perm, inv, starts, n, W,
                     make_route(V, S, div));
}

// rows [n_rows, D] fp32 or bf16 -> out [n_out, D] fp32 or bf16.
// n_out, D > 0.
void launch_permute_rows(const void* rows, bool r_bf16, const long* perm,
                         void* out, bool o_bf16, long n_out, long n_rows,
                         int D, hipStream_t stream) {
  if (r_bf16 && o_bf16)
    permute_typed((const bf16_t*)rows, perm, (bf16_t*)out, n_out, n_rows, D,
                  stream);
  else if (r_bf16)
    permute_typed((const bf16_t*)rows, perm, (float*)out, n_out, n_rows, D,
                  stream);
  else if (o_bf16)
    permute_typed((const float*)rows, perm, (bf16_t*)out, n_out, n_rows, D,
                  stream);
  else
    permute_typed((const float*)rows, perm, (float*)out, n_out, n_rows, D,
                  stream);
}

// perm [n], starts [S+1], offsets [B+1] -> out [S, B+1].
void launch_shard_bag_offsets(const long* perm, const long* starts,
                              const long* offsets, long* out, long n, long B,
                              int S, hipStream_t stream) {
  const long total = (long)S * (B + 1);
  const dim3 grid((unsigned)((total + WAVES * WAVE - 1) / (WAVES * WAVE)));
  hipLaunchKernelGGL(shard_bag_offsets_kernel, grid, dim3(WAVES * WAVE), 0,
                     stream, perm, starts, offsets, out, n, B, S);
}

// offsets [B+1] (+ weights [n] or null) -> coef [n], zeroed by the caller.
// B, n > 0.
void launch_bag_coef(const long* offsets, const float* weights, float* coef,
                     long B, long n, bool mean, hipStream_t stream) {
  const dim3 grid((unsigned)((B + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(bag_coef_kernel, grid, dim3(WAVES * WAVE), 0, stream,
                     offsets, weights, coef, B, n, (int)mean);
}

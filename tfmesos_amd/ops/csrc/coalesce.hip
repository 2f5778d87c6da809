// Worker-side coalescing of a row request: the distinct ids of a request
// (TF's unique before embedding_lookup) and the per-id sum of its gradient
// rows (TF's unsorted_segment_sum before SparseApply*), so that a pull or
// push carries one id and one row per DISTINCT id.
//
// coalesce_ids. The binding stable-sorts the ids (plumbing): sorted, perm.
// Position j of the sorted order is a HEAD when sorted[j] != sorted[j-1]
// (j == 0 is one); the rank of j is the number of heads at or before it,
// minus one = the index k of its id among the distinct ids, ascending.
// Ranks = count, scan, scatter, no atomics (the structure of partition.hip):
//   * count: one lane per sorted position, one wave per 64-position
//     window; the wave ballots the heads and writes the popcount.
//   * the inclusive scan of the window counts is plumbing (torch.cumsum in
//     the binding); its last element is u, the number of distinct ids.
//   * scatter: recomputes the heads; rank = heads of earlier windows +
//     popcount of the ballot at or below the lane - 1. Every position
//     writes inverse[perm[j]] = rank; a head also writes uniq[rank] and
//     seg[rank] = j; position j >= u writes the tails uniq[j] = -1 and
//     seg[j] = n; the first lane writes seg[n] = n and count = u.
//   Fixed slots, no atomics => two runs give identical bits. The ids' range
//   is never looked at: negative and too-large ids are distinct values like
//   any other. Grids are sized from n; nothing is read back.
//
// segment_sum_rows: out[k] = sum of rows[perm[j]], j in [seg[k], seg[k+1]),
// for k < num. One wave owns one (output row, 256-column tile) — tile.h:
// f32x4 / bf16x4 when D % 4 == 0 and the bases are 16-byte aligned, scalar
// otherwise. The wave reads the run's perm entries 64 at a time (one per
// lane), broadcasts each with a wave shuffle and keeps 4 row loads in
// flight.
//   * hot ids: a run longer than CHUNK positions is cut into CHUNK-position
//     pieces relative to the run start; the piece starting at sorted
//     position p is summed by the wave of p's aligned 256-position window
//     (SLOT_DIV is also the width of pass 1's windows) into fp32 scratch
//     slot start/256 + piece (the slot scheme of run_sum.h); the owning
//     wave then adds the partials. A window holds at most one piece head
//     per run; its wave finds the runs that overlap it by a binary search
//     of seg and tests 64 runs at a time, one per lane.
//   * SUMMATION ORDER. A run of at most CHUNK positions: fp32, starting
//     from 0, one row after the other in run order (= request order inside
//     an id: the sort is stable). A longer run: every piece that way, then
//     the partials added to 0 in piece order. One rounding to the output
//     dtype at the end. Fixed order, no atomics => bit-reproducible.
//   * a perm entry outside [0, n) contributes a zero row; seg entries are
//     clamped to [0, n]. The grids are sized from num, n and D.
#include "common.h"

#include "coalesce.h"
#include "run_sum.h"

namespace {

constexpr int WAVES = 4;       // waves per block

DEVINL bool is_head(const long* __restrict__ sorted, long j, long n) {
  return j < n && (j == 0 || sorted[j - 1] != sorted[j]);
}

__global__ __launch_bounds__(WAVES * WAVE) void coalesce_count_kernel(
    const long* __restrict__ sorted, int* __restrict__ counts, long n,
    long W) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= W) return;   // wave-uniform
  const unsigned long long heads =
      __ballot(is_head(sorted, w * WAVE + lane, n));
  if (lane == 0) counts[w] = __popcll(heads);
}

// incl: inclusive scan of counts. n > 0.
__global__ __launch_bounds__(WAVES * WAVE) void coalesce_scatter_kernel(
    const long* __restrict__ sorted, const long* __restrict__ perm,
    const long* __restrict__ incl, long* __restrict__ uniq,
    long* __restrict__ inverse, long* __restrict__ seg,
    long* __restrict__ count, long n, long W) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= W) return;   // wave-uniform
  const long u = incl[W - 1];
  const long j = w * WAVE + lane;
  const bool head = is_head(sorted, j, n);
  const unsigned long long heads = __ballot(head);
  if (j == 0) {
    seg[n] = n;
    count[0] = u;
  }
  if (j >= n) return;
  // heads at or below the lane: 2 << 63 wraps to 0, so lane 63 keeps all
  const long rank = (w == 0 ? 0 : incl[w - 1]) +
                    __popcll(heads & ((2ull << lane) - 1ull)) - 1;
  if (j >= u) {   // the tails; heads write below u
    uniq[j] = -1;
    seg[j] = n;
  }
  if (rank < 0 || rank >= n) return;   // cannot happen with a true scan
  if (head) {
    uniq[rank] = sorted[j];
    seg[rank] = j;
  }
  const long p = perm[j];
  if (p >= 0 && p < n) inverse[p] = rank;
}

// acc += rows[perm[j]] for j in [pos, pos + cnt), in that order. All 64
// lanes must call this (shuffles); cnt is wave-uniform.
template <typename T, int VEC>
DEVINL void sum_rows(const T* __restrict__ rows, const long* __restrict__ perm,
                     long n, long pos, int cnt, int c0, int lane, int D,
                     float (&acc)[ACC]) {
  for (int done = 0; done < cnt; done += WAVE) {
    const int here = cnt - done < WAVE ? cnt - done : WAVE;
    long src = lane < here ? perm[pos + done + lane] : -1;
    if (src >= n) src = -1;   // outside [0, n): a zero row
    int k = 0;
    for (; k + 4 <= here; k += 4) {
      const long r0 = __shfl(src, k), r1 = __shfl(src, k + 1);
      const long r2 = __shfl(src, k + 2), r3 = __shfl(src, k + 3);
      float v0[ACC], v1[ACC], v2[ACC], v3[ACC];
      ld_row<T, VEC>(rows, r0, c0, lane, D, v0);
      ld_row<T, VEC>(rows, r1, c0, lane, D, v1);
      ld_row<T, VEC>(rows, r2, c0, lane, D, v2);
      ld_row<T, VEC>(rows, r3, c0, lane, D, v3);
#pragma unroll
      for (int e = 0; e < ACC; ++e)
        acc[e] = (((acc[e] + v0[e]) + v1[e]) + v2[e]) + v3[e];
    }
    for (; k < here; ++k) {
      const long r = __shfl(src, k);
      float v[ACC];
      ld_row<T, VEC>(rows, r, c0, lane, D, v);
#pragma unroll
      for (int e = 0; e < ACC; ++e) acc[e] += v[e];
    }
  }
}

// Pass 1 (only launched when n > CHUNK): one wave per (aligned window of
// SLOT_DIV sorted positions, column tile) sums the pieces of long runs
// that start inside the window into their scratch slots.
template <typename T, int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void segment_partial_kernel(
    const T* __restrict__ rows, const long* __restrict__ perm,
    const long* __restrict__ seg, float* __restrict__ scratch, long n,
    long num, long slots, int D, int tiles) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= slots * tiles) return;   // wave-uniform
  const long first = (w / tiles) * SLOT_DIV;   // the window [first, last)
  const long last = first + SLOT_DIV;
  const int c0 = (int)(w % tiles) * TILE;
  if (first >= n) return;
  // the run that holds position `first`: the last k with seg[k] <= first
  long lo = 0, hi = num;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (clamp_pos(seg[mid], n) <= first) lo = mid + 1; else hi = mid;
  }
  for (long kb = lo > 0 ? lo - 1 : 0; kb < num; kb += WAVE) {
    if (clamp_pos(seg[kb], n) >= last) break;   // wave-uniform
    const long k = kb + lane;
    long s = 0, e = 0, p = 0;
    bool has = false;
    if (k < num) {
      s = clamp_pos(seg[k], n);
      e = clamp_pos(seg[k + 1], n);
      if (e - s > CHUNK) {
        // the run's first piece head at or after `first`
        p = s >= first ? s : s + (first - s + CHUNK - 1) / CHUNK * CHUNK;
        has = p < last && p < e;
      }
    }
    unsigned long long todo = __ballot(has);
    while (todo) {
      const int b = __ffsll(todo) - 1;
      todo &= todo - 1;
      const long rs = __shfl(s, b), re = __shfl(e, b), rp = __shfl(p, b);
      const long slot = rs / SLOT_DIV + (rp - rs) / CHUNK;
      const int cnt = re - rp < CHUNK ? (int)(re - rp) : CHUNK;
      float acc[ACC];
#pragma unroll
      for (int x = 0; x < ACC; ++x) acc[x] = 0.f;
      sum_rows<T, VEC>(rows, perm, n, rp, cnt, c0, lane, D, acc);
      if (slot < slots)   // always: see the slot scheme above
        st_tile<float, VEC>(scratch + slot * D, c0, lane, D, acc);
    }
  }
}

// Pass 2: one wave per (output row, column tile).
template <typename T, typename O, int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void segment_sum_kernel(
    const T* __restrict__ rows, const long* __restrict__ perm,
    const long* __restrict__ seg, const float* __restrict__ scratch,
    O* __restrict__ out, long n, long num, long slots, int D, int tiles) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= num * tiles) return;   // wave-uniform
  const long k = w / tiles;
  const int c0 = (int)(w % tiles) * TILE;
  const long s = clamp_pos(seg[k], n);
  long e = clamp_pos(seg[k + 1], n);
  if (e < s) e = s;
  float acc[ACC];
#pragma unroll
  for (int x = 0; x < ACC; ++x) acc[x] = 0.f;
  if (e - s <= CHUNK) {
    sum_rows<T, VEC>(rows, perm, n, s, (int)(e - s), c0, lane, D, acc);
  } else {
    // partial sums of pass 1, added in piece order
    long slot = s / SLOT_DIV;
    for (long q = s; q < e && slot < slots; q += CHUNK, ++slot) {
      float v[ACC];
      ld_tile<float, VEC>(scratch + slot * D, c0, lane, D, v);
#pragma unroll
      for (int x = 0; x < ACC; ++x) acc[x] += v[x];
    }
  }
  st_tile<O, VEC>(out + k * D, c0, lane, D, acc);   // empty run: zeros
}

template <typename T, typename O>
void segment_typed(const T* rows, const long* perm, const long* seg,
                   float* scratch, O* out, long n, long num, int D,
                   hipStream_t stream) {
  const int tiles = (D + TILE - 1) / TILE;
  const dim3 block(WAVES * WAVE);
  const long slots = run_scratch_rows(n);
  const dim3 grid1((unsigned)((slots * tiles + WAVES - 1) / WAVES));
  const dim3 grid2((unsigned)((num * tiles + WAVES - 1) / WAVES));
  if (tile_vec4(D, rows, out, scratch)) {
    if (slots > 0)
      hipLaunchKernelGGL((segment_partial_kernel<T, 4>), grid1, block, 0,
                         stream, rows, perm, seg, scratch, n, num, slots, D,
                         tiles);
    hipLaunchKernelGGL((segment_sum_kernel<T, O, 4>), grid2, block, 0, stream,
                       rows, perm, seg, scratch, out, n, num, slots, D, tiles);
  } else {
    if (slots > 0)
      hipLaunchKernelGGL((segment_partial_kernel<T, 1>), grid1, block, 0,
                         stream, rows, perm, seg, scratch, n, num, slots, D,
                         tiles);
    hipLaunchKernelGGL((segment_sum_kernel<T, O, 1>), grid2, block, 0, stream,
                       rows, perm, seg, scratch, out, n, num, slots, D, tiles);
  }
}

}  // namespace

// Number of 64-position windows of n sorted ids; counts is int32 [windows].
long coalesce_windows(long n) { return (n + WAVE - 1) / WAVE; }

// sorted [n], n > 0 -> counts [coalesce_windows(n)].
void launch_coalesce_count(const long* sorted, int* counts, long n,
                           hipStream_t stream) {
  const long W = coalesce_windows(n);
  const dim3 grid((unsigned)((W + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(coalesce_count_kernel, grid, dim3(WAVES * WAVE), 0,
                     stream, sorted, counts, n, W);
}

// incl: int64 inclusive scan of counts. uniq/inverse [n], seg [n+1],
// count [1].
void launch_coalesce_scatter(const long* sorted, const long* perm,
                             const long* incl, long* uniq, long* inverse,
                             long* seg, long* count, long n,
                             hipStream_t stream) {
  const long W = coalesce_windows(n);
  const dim3 grid((unsigned)((W + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(coalesce_scatter_kernel, grid, dim3(WAVES * WAVE), 0,
                     stream, sorted, perm, incl, uniq, inverse, seg, count, n,
                     W);
}

// rows [n,D] fp32 or bf16, perm [n], seg [>= num+1] -> out [num,D] fp32 or
// bf16. scratch: fp32 [run_scratch_rows(n), D] (may be null when 0 rows).
// n, num, D > 0.
void launch_segment_sum_rows(const void* rows, bool r_bf16, const long* perm,
                             const long* seg, float* scratch, void* out,
                             bool o_bf16, long n, long num, int D,
                             hipStream_t stream) {
  if (r_bf16 && o_bf16)
    segment_typed((const bf16_t*)rows, perm, seg, scratch, (bf16_t*)out, n,
                  num, D, stream);
  else if (r_bf16)
    segment_typed((const bf16_t*)rows, perm, seg, scratch, (float*)out, n,
                  num, D, stream);
  else if (o_bf16)
    segment_typed((const float*)rows, perm, seg, scratch, (bf16_t*)out, n,
                  num, D, stream);
  else
    segment_typed((const float*)rows, perm, seg, scratch, (float*)out, n, num,
                  D, stream);
}

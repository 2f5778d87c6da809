// Pooled (bag) embedding pull: out[b] = sum_i c_i * table[ids[i]] over the
// positions i of CSR bag b (TF's embedding_lookup_sparse, combiner sum or
// mean, optional per-id weights; coefficient rule in bag.h).
//
//   * one wave owns one (bag, 256-column tile): it reads the bag's ids
//     (and weights) 64 positions at a time, one per lane, broadcasts each
//     with a wave shuffle, keeps 4 row loads in flight and accumulates in
//     fp32 registers in position order (bag_walk.h, shared with the keyed
//     pooled pull of hash.hip); the row is rounded once on store.
//     Fixed order, no atomics => bit-reproducible.
//   * D % 4 == 0 and 16-byte aligned bases: lane l owns columns 4l..4l+3
//     of the tile (bf16x4 / f32x4 accesses). Otherwise a scalar path:
//     lane l owns columns l, l+64, l+128, l+192 (a vector access on an
//     odd-D row would be misaligned).
//   * ids outside [0, V) contribute nothing (their rows are never read)
//     but still count in W_b.
//   * the grid is sized from B and D only; nothing is read back.
//   * a single very long bag stays with one wave per tile (no chunk rule
//     on the forward side).
#include "common.h"
#include "embedding_bag.h"

#include "bag_walk.h"

namespace {

constexpr int WAVES = 4;    // waves per block

// bag_walk's source over a table indexed by id: position p names row ids[p].
template <typename T, int VEC>
struct TableRows {
  const T* __restrict__ table;
  const long* __restrict__ ids;
  long V;
  int D, c0, lane;

  DEVINL long item(long p, bool& valid) const {
    const long id = ids[p];
    valid = id >= 0 && id < V;
    return id;
  }
  DEVINL void fetch(long id, int, float (&v)[ACC]) const {
    ld_tile<T, VEC>(table + id * D, c0, lane, D, v);
  }
};

template <typename T, typename O, int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void embedding_bag_kernel(
    const T* __restrict__ table, const long* __restrict__ ids,
    const long* __restrict__ offsets, const float* __restrict__ weights,
    O* __restrict__ out, long B, long n, int D, long V, int tiles,
    int mean) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= B * tiles) return;   // wave-uniform
  const long b = w / tiles;
  const int c0 = (int)(w % tiles) * TILE;
  long s, e;
  bag_range(offsets, b, n, s, e);
  const float W = mean ? bag_weight_sum(weights, s, e, lane) : 0.f;
  float acc[ACC];
#pragma unroll
  for (int k = 0; k < ACC; ++k) acc[k] = 0.f;
  TableRows<T, VEC> src = {table, ids, V, D, c0, lane};
  bag_walk(src, weights, s, e, W, mean != 0, lane, acc);
  st_tile<O, VEC>(out + b * D, c0, lane, D, acc);   // empty bag: zeros
}

template <typename T, typename O>
void launch_typed(const T* table, const long* ids, const long* offsets,
                  const float* weights, O* out, long B, long n, int D, long V,
                  bool mean, hipStream_t stream) {
  const int tiles = (D + TILE - 1) / TILE;
  const long waves = B * tiles;
  const dim3 block(WAVES * WAVE);
  const dim3 grid((unsigned)((waves + WAVES - 1) / WAVES));
  if (tile_vec4(D, table, out))
    hipLaunchKernelGGL((embedding_bag_kernel<T, O, 4>), grid, block, 0,
                       stream, table, ids, offsets, weights, out, B, n, D, V,
                       tiles, (int)mean);
  else
    hipLaunchKernelGGL((embedding_bag_kernel<T, O, 1>), grid, block, 0,
                       stream, table, ids, offsets, weights, out, B, n, D, V,
                       tiles, (int)mean);
}

}  // namespace

// table [V,D] bf16 or fp32; out [B,D] in the table's dtype, or fp32 from
// a bf16 table. weights may be null (all 1). B, n, D > 0.
void launch_embedding_bag(const void* table, bool t_bf16, const long* ids,
                          const long* offsets, const float* weights,
                          void* out, bool o_bf16, long B, long n, int D,
                          long V, bool mean, hipStream_t stream) {
  if (t_bf16 && o_bf16)
    launch_typed((const bf16_t*)table, ids, offsets, weights, (bf16_t*)out, B,
                 n, D, V, mean, stream);
  else if (t_bf16)
    launch_typed((const bf16_t*)table, ids, offsets, weights, (float*)out, B,
                 n, D, V, mean, stream);
  else
    launch_typed((const float*)table, ids, offsets, weights, (float*)out, B,
                 n, D, V, mean, stream);
}

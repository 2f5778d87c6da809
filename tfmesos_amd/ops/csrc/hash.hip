// Hashed embedding tables: a device-resident index from arbitrary int64 keys
// to the dense rows 0 .. size-1 of a table of fixed capacity (TF's
// MutableHashTable / dynamic embedding variable on the PS), the serving
// gather through it, and the per-key row initialiser.
//
// Layout. H slots, H a power of two >= max(64, 2 * capacity): slot_keys[H]
// (EMPTY = INT64_MIN, the one value that is not a key) and slot_rows[H].
// The maximum load of 0.5 is a DESIGN CHOICE (short linear-probe chains at
// 16 bytes per slot), not a measured optimum. home(key) = mix64(key) &
// (H - 1), linear probing, no deletion: a key sits before the first EMPTY
// slot of its probe sequence. Rows are numbered in allocation order and
// row_keys[r] is the key that owns row r; WHERE a key hashes to is visible
// to nothing outside this file. size and dropped are int64 device words;
// no launcher reads anything back.
//
// Between two calls the slot array holds ONLY published (key, row) pairs:
// a key that found no room (row >= capacity) never enters it, so the array
// cannot fill with rowless keys and every probe ends at an EMPTY slot.
//
// find_or_insert(keys [n]) — four kernels, one lane per position, and one
// scan; no sort, no float atomics, and no loop that waits for another
// thread's store (every value a kernel needs from another thread was
// written by an EARLIER kernel):
//   1. lookup: rows[i] = the row of keys[i] or -1. An absent key is
//      deduplicated in a per-call scratch table of S >= 2n slots (filled
//      with EMPTY by the binding): 64-bit atomicCAS(EMPTY -> key) claims a
//      slot, a loser that reads back its own key joins it, and an unsigned
//      64-bit atomicMin records the smallest position per slot (EMPTY as an
//      unsigned number, 2^63, lies above every position).
//   2. flags: flag[i] = 1 where i is that smallest position — the first
//      occurrence of a new key in the request.
//   *  the inclusive scan of the flags is plumbing (torch.cumsum in the
//      binding): incl[i] - 1 is the rank of the new key among the
//      request's new keys, in order of first occurrence.
//   3. insert: a flagged position whose row = size + rank is below capacity
//      inserts (key, row) — the keys are distinct, so a plain CAS probe —,
//      writes row_keys[row] and is_new[i] = 1.
//   4. resolve: positions still at -1 look their key up again (duplicates
//      of a new key find the row its first occurrence published in 3);
//      lane 0 adds min(new, room) to size and the rest to dropped.
//   Which scratch slot or hash slot a racing key lands in may differ from
//   run to run; rows, is_new, row_keys, size and dropped cannot.
//
// hash_gather (serving): one wave per key. The wave reads 64 consecutive
// slots per step (one per lane), ballots "is my key" and "is EMPTY", takes
// the row from the first matching lane or stops at an EMPTY one, then
// copies the bf16 row (8 bytes per lane when D % 4 == 0 and the bases are
// 8-byte aligned) or writes zeros on a miss: one launch per pull.
//
// find_or_admit(keys [n], sketch, admit_after) — feature admission: a key
// earns a row only once it has been named by admit_after requests. The
// sketch is count-min: counters int32 [4, width], width a power of two, the
// cell of key k in sketch row j is mix64(k + (j + 1) * G) & (width - 1).
// Kernels 1 and 2 above run unchanged (flag = first occurrence of an ABSENT
// key: each distinct absent key of the request is counted once), then
//   A. count: a flagged position adds 1 to its four cells (integer atomics).
//   B. decide: a flagged position reads its four cells — all counts of the
//      request are in, they were written by kernel A —, and pass[i] = the
//      minimum >= admit_after; every wave adds its number of flagged
//      positions that did not pass to `filtered` (one integer atomic per
//      wave that has any).
//   then the scan, insert and resolve run on the PASS flags: an admitted
//   key is a new key of find_or_insert, every other absent key stays at -1.
//   Saturation at CAP = 2^30: a count is atomicAdd(cell, 1), and an add that
//   RETURNS a value >= CAP takes itself back (atomicSub). Why the final
//   value is min(c0 + a, CAP) for a cell that starts at c0 <= CAP and gets a
//   adds, in every interleaving: at any moment the cell holds c0 + kept +
//   pending, kept = the adds that returned a value < CAP, pending = the adds
//   that returned >= CAP and have not been taken back yet. An add is kept
//   only when it saw less than CAP, so c0 + kept <= CAP throughout. The
//   FIRST add that is not kept (in the order the memory system applies
//   them) saw no pending ones, hence c0 + kept >= CAP at that moment, hence
//   = CAP, and kept never shrinks. So either every add is kept (c0 + a <=
//   CAP) or c0 + kept = CAP at the end; pending is 0 when the kernel ends.
//   The cell is treated as unsigned: c0 + a < 2^30 + 2^31 does not wrap.
//   Nothing reads a cell during kernel A; kernel B sees final values only.
//   So rows, is_new, row_keys, size, dropped, filtered and every counter are
//   the same from run to run.
//
// hash_gather_init (training pull of a table with admission): hash_gather,
// but a miss on a key other than EMPTY writes the bf16 of the key's INITIAL
// row, computed in registers (the bits init_rows_kernel would have put into
// the shadow); with last_used given, lane 0 stores step into last_used[row]
// on a hit (a plain store, as in touch_kernel). One launch.
//
// hash_embedding_bag (pooled pull by key): embedding_bag.hip's kernel with
// the lookup fused in. Each lane probes the key of its own position, then
// the wave walks the rows exactly as embedding_bag_kernel does (bag_walk.h:
// one walk, two row sources). With an initialiser given, a key that has no
// row contributes bf2f(f2bf(initial value)), computed in registers; without
// one it contributes nothing but still counts in a mean's weight sum. EMPTY
// never contributes. Bit for bit embedding_bag over the table extended by
// the bf16 initial rows of the absent keys.
//
// Row initialiser: value(seed, k, c) =
//     float(mix64(mix64(mix64(seed + G) ^ k) + c * G) >> 40) * 2^-24 * scale
// with G = 0x9E3779B97F4A7C15, mix64 the splitmix64 finaliser, k =
// key * key_mul + key_add (the GLOBAL key of a shard-local one), all in
// wrapping uint64; the 24-bit integer and the product by 2^-24 are exact in
// fp32, the product by scale is one fp32 rounding. One wave per (position,
// 256-column tile) writes master, shadow and zeroed state rows for the
// positions with is_new set. Every bound is checked; grids are sized
// from n.
//
// Eviction. The slot array has no deletion, so keys leave by COMPACTION:
// the caller says which rows stay (keep bool [capacity], read below size
// only), the surviving rows are made dense again and the slot array is
// rebuilt from row_keys. hash_touch keeps the use stamps a policy builds
// keep from: last_used[rows[i]] = step, one lane per position, plain stores
// (duplicates store the same value).
//
// compact(keep, row tensors, last_used) — hole filling. With K kept rows
// below size, the evicted rows below K (holes, ascending) receive the kept
// rows at or above K (movers, ascending), pair by pair: sources and
// destinations are disjoint, so the move runs in place with no second copy
// of a table, and it moves min(evicted, survivors) rows at the most. Four
// kernels and one scan, nothing read back, no kernel reads what another
// lane of the same kernel writes:
//   1. flags: flag[r] = r < size and keep[r]; lane 0 saves size.
//   *  incl = the inclusive scan of the flags (torch.cumsum, plumbing);
//      K = incl[capacity - 1].
//   2. plan: an evicted row r < K is hole number r - incl[r]; a kept row
//      r >= K is mover number incl[r] - 1 - incl[K - 1].
//   3. move: one wave per (hole, mover) pair copies the row in EVERY row
//      tensor (master, shadow, state: raw bytes, 16 per lane when the row
//      size and the base allow, else one element per lane), and lane 0 the
//      row's key and stamp. The number of pairs is known on the device
//      only: a grid of fixed size (at most 2048 blocks of 4 waves) strides
//      over the pairs.
//   4. finalize: row_keys[K:size] = EMPTY; size = K, evicted += size - K,
//      from the size kernel 1 saved.
//   Then the slot arrays are cleared and rebuild_kernel inserts
//   row_keys[0:K]. Rows >= K of the row tensors keep stale data; the init
//   kernel overwrites a row when it is handed out again.
#include "common.h"
#include "hash.h"

#include <climits>

#include "bag_walk.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = 4;   // waves per block of the wave-per-item kernels
constexpr long EMPTY = LONG_MIN;
constexpr unsigned long long GOLD = 0x9E3779B97F4A7C15ull;
constexpr int SKETCH_ROWS = 4;
constexpr unsigned SKETCH_CAP = 1u << 30;   // counters saturate here

typedef unsigned long long u64;

DEVINL u64 mix64(u64 z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// slots: a power of two
DEVINL long home_slot(long key, long slots) {
  return (long)(mix64((u64)key) & (u64)(slots - 1));
}

// Read-only probe: the row of key, -1 when absent (or EMPTY).
DEVINL long probe_find(const long* __restrict__ slot_keys,
                       const long* __restrict__ slot_rows, long key, long H) {
  if (key == EMPTY) return -1;
  long s = home_slot(key, H);
  for (long t = 0; t < H; ++t) {
    const long k = slot_keys[s];
    if (k == key) return slot_rows[s];
    if (k == EMPTY) return -1;
    s = (s + 1) & (H - 1);
  }
  return -1;
}

// Claims a slot for key (or joins the slot that holds it): the slot, -1
// when all `slots` are taken by other keys.
DEVINL long probe_claim(long* __restrict__ slot_keys, long key, long slots) {
  long s = home_slot(key, slots);
  for (long t = 0; t < slots; ++t) {
    const u64 old = atomicCAS((u64*)&slot_keys[s], (u64)EMPTY, (u64)key);
    if (old == (u64)EMPTY || old == (u64)key) return s;
    s = (s + 1) & (slots - 1);
  }
  return -1;
}

__global__ __launch_bounds__(BLOCK) void find_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, long* __restrict__ rows, long n,
    long H) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  rows[i] = probe_find(slot_keys, slot_rows, keys[i], H);
}

// find_or_insert 1: lookup, and dedup of the absent keys in the scratch.
__global__ __launch_bounds__(BLOCK) void lookup_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, long* __restrict__ rows,
    long* __restrict__ skeys, long* __restrict__ spos, long n, long H,
    long S) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const long key = keys[i];
  const long r = probe_find(slot_keys, slot_rows, key, H);
  rows[i] = r;
  if (r >= 0 || key == EMPTY) return;
  const long s = probe_claim(skeys, key, S);
  if (s >= 0) atomicMin((u64*)&spos[s], (u64)i);   // always: S >= 2n
}

// find_or_insert 2: first occurrences of the new keys.
__global__ __launch_bounds__(BLOCK) void flag_kernel(
    const long* __restrict__ keys, const long* __restrict__ rows,
    const long* __restrict__ skeys, const long* __restrict__ spos,
    int* __restrict__ flags, long n, long S) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const long key = keys[i];
  int flag = 0;
  if (rows[i] < 0 && key != EMPTY) {
    long s = home_slot(key, S);
    for (long t = 0; t < S; ++t) {
      const long k = skeys[s];
      if (k == key) { flag = spos[s] == i; break; }
      if (k == EMPTY) break;   // cannot happen: kernel 1 claimed it
      s = (s + 1) & (S - 1);
    }
  }
  flags[i] = flag;
}

// The cell of key in sketch row j; width: a power of two
DEVINL long sketch_cell(long key, int j, long width) {
  return (long)(mix64((u64)key + (u64)(j + 1) * GOLD) & (u64)(width - 1));
}

// find_or_admit A: every flagged position (the first occurrence of an absent
// key) counts once in its four cells; saturating (file header).
__global__ __launch_bounds__(BLOCK) void count_kernel(
    const long* __restrict__ keys, const int* __restrict__ flags,
    unsigned* __restrict__ counters, long n, long width) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n || !flags[i]) return;
  const long key = keys[i];
#pragma unroll
  for (int j = 0; j < SKETCH_ROWS; ++j) {
    unsigned* cell = counters + j * width + sketch_cell(key, j, width);
    if (atomicAdd(cell, 1u) >= SKETCH_CAP) atomicSub(cell, 1u);
  }
}

// find_or_admit B: pass[i] = flagged and min of the four cells >=
// admit_after; the flagged positions that do not pass are counted in
// filtered, one atomic per wave that has any.
__global__ __launch_bounds__(BLOCK) void decide_kernel(
    const long* __restrict__ keys, const int* __restrict__ flags,
    const unsigned* __restrict__ counters, int* __restrict__ pass,
    long* __restrict__ filtered, long n, long width, unsigned admit_after) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  const bool flagged = i < n && flags[i];
  bool ok = false;
  if (flagged) {
    const long key = keys[i];
    unsigned est = counters[sketch_cell(key, 0, width)];
#pragma unroll
    for (int j = 1; j < SKETCH_ROWS; ++j) {
      const unsigned c = counters[j * width + sketch_cell(key, j, width)];
      est = c < est ? c : est;
    }
    ok = est >= admit_after;
  }
  if (i < n) pass[i] = ok;
  const unsigned long long out = __ballot(flagged && !ok);
  if (out && (threadIdx.x & (WAVE - 1)) == 0)
    atomicAdd((u64*)filtered, (u64)__popcll(out));
}

// find_or_insert 3: publish the new keys that have room.
__global__ __launch_bounds__(BLOCK) void insert_kernel(
    const long* __restrict__ keys, const int* __restrict__ flags,
    const long* __restrict__ incl, long* __restrict__ slot_keys,
    long* __restrict__ slot_rows, long* __restrict__ row_keys,
    const long* __restrict__ size, bool* __restrict__ is_new, long n, long H,
    long capacity) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  bool fresh = false;
  if (flags[i]) {
    const long row = size[0] + incl[i] - 1;
    if (row >= 0 && row < capacity) {
      const long key = keys[i];
      const long s = probe_claim(slot_keys, key, H);
      if (s >= 0) {   // always: at most capacity <= H / 2 keys
        slot_rows[s] = row;
        row_keys[row] = key;
        fresh = true;
      }
    }
  }
  is_new[i] = fresh;
}

// find_or_insert 4: the rows of this request's new keys; the counters.
__global__ __launch_bounds__(BLOCK) void resolve_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, const long* __restrict__ incl,
    long* __restrict__ rows, long* __restrict__ size,
    long* __restrict__ dropped, long n, long H, long capacity) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  if (rows[i] < 0) rows[i] = probe_find(slot_keys, slot_rows, keys[i], H);
  if (i == 0) {   // no lane of this kernel reads size
    const long fresh = incl[n - 1], old = size[0];
    const long room = capacity > old ? capacity - old : 0;
    const long added = fresh < room ? fresh : room;
    size[0] = old + added;
    dropped[0] += fresh - added;
  }
}

// row_keys[0:size] into a cleared slot array.
__global__ __launch_bounds__(BLOCK) void rebuild_kernel(
    const long* __restrict__ row_keys, const long* __restrict__ size,
    long* __restrict__ slot_keys, long* __restrict__ slot_rows, long H,
    long capacity) {
  const long r = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= capacity || r >= size[0]) return;
  const long key = row_keys[r];
  if (key == EMPTY) return;
  const long s = probe_claim(slot_keys, key, H);
  if (s >= 0) slot_rows[s] = r;
}

// The row of key (the same in all 64 lanes), -1 when absent or EMPTY: the
// wave reads 64 consecutive slots per step, one per lane.
DEVINL long wave_find(const long* __restrict__ slot_keys,
                      const long* __restrict__ slot_rows, long key, long H,
                      int lane) {
  long row = -1;
  if (key != EMPTY) {
    const long base = home_slot(key, H);
    for (long st = 0; st < H; st += WAVE) {
      const long s = (base + st + lane) & (H - 1);
      const long k = slot_keys[s];
      const unsigned long long hit = __ballot(k == key);
      const unsigned long long gap = __ballot(k == EMPTY);
      if (hit) {
        const int b = __ffsll(hit) - 1;
        if (!gap || b < __ffsll(gap) - 1) row = __shfl(slot_rows[s], b);
        break;
      }
      if (gap) break;
    }
  }
  return row;
}

template <int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void hash_gather_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, const bf16_t* __restrict__ table,
    bf16_t* __restrict__ out, long n, long H, long V, int D) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= n) return;   // wave-uniform
  const long row = wave_find(slot_keys, slot_rows, keys[w], H, lane);
  const bool live = row >= 0 && row < V;
  const bf16_t* src = table + (live ? row : 0) * D;
  bf16_t* dst = out + w * D;
  if constexpr (VEC == 4) {
    for (int c = lane * 4; c < D; c += WAVE * 4) {
      bf16x4 v = {};
      if (live) v = *(const bf16x4*)(const __bf16*)(src + c);
      *(bf16x4*)(__bf16*)(dst + c) = v;
    }
  } else {
    for (int c = lane; c < D; c += WAVE)
      dst[c] = live ? src[c] : f2bf(0.f);
  }
}

DEVINL float init_value(u64 b, int col, float scale) {
  const u64 z = mix64(b + (u64)col * GOLD);
  return (float)(unsigned)(z >> 40) * 0x1p-24f * scale;
}

// What the initialiser needs besides the key and the column.
struct InitArgs {
  long seed, key_mul, key_add;
  float scale;
};

// The per-key base of init_value: mix64(mix64(seed + G) ^ global key).
DEVINL u64 init_base(const InitArgs& a, long key) {
  const u64 k = (u64)key * (u64)a.key_mul + (u64)a.key_add;
  return mix64(mix64((u64)a.seed + GOLD) ^ k);
}

// The lane's ACC elements (tile.h layout) of the initial row of a key, as
// the bf16 shadow holds them; columns at or beyond D are 0.
template <int VEC>
DEVINL void init_tile(u64 b, float scale, int c0, int lane, int D,
                      float (&v)[ACC]) {
#pragma unroll
  for (int e = 0; e < ACC; ++e) {
    const int col = VEC == 4 ? c0 + lane * 4 + e : c0 + e * WAVE + lane;
    v[e] = col < D ? bf2f(f2bf(init_value(b, col, scale))) : 0.f;
  }
}

// hash_gather with the initial row on a miss; stamps hits. One wave per key.
// last_used may be null; stamps = its length.
template <int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void hash_gather_init_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, const bf16_t* __restrict__ table,
    bf16_t* __restrict__ out, long* __restrict__ last_used, long n, long H,
    long V, int D, long stamps, long step, InitArgs init) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= n) return;   // wave-uniform
  const long key = keys[w];
  const long row = wave_find(slot_keys, slot_rows, key, H, lane);
  const bool live = row >= 0 && row < V;
  bf16_t* dst = out + w * D;
  if (live) {
    if (last_used && lane == 0 && row < stamps) last_used[row] = step;
    const bf16_t* src = table + row * D;
    if constexpr (VEC == 4) {
      for (int c = lane * 4; c < D; c += WAVE * 4)
        *(bf16x4*)(__bf16*)(dst + c) = *(const bf16x4*)(const __bf16*)(src + c);
    } else {
      for (int c = lane; c < D; c += WAVE) dst[c] = src[c];
    }
    return;
  }
  // a row the table cannot hold (row >= V) reads as zeros, like EMPTY
  const bool fresh = row < 0 && key != EMPTY;
  const u64 b = fresh ? init_base(init, key) : 0;
  for (int c0 = 0; c0 < D; c0 += TILE) {
    float v[ACC];
#pragma unroll
    for (int e = 0; e < ACC; ++e) v[e] = 0.f;
    if (fresh) init_tile<VEC>(b, init.scale, c0, lane, D, v);
    st_tile<bf16_t, VEC>(dst, c0, lane, D, v);
  }
}

// bag_walk's source over a table indexed by KEY: position p names the row
// of keys[p]; a key without a row names its initial row when has_init.
template <int VEC>
struct KeyedRows {
  const long* __restrict__ keys;
  const long* __restrict__ slot_keys;
  const long* __restrict__ slot_rows;
  const bf16_t* __restrict__ table;
  long* __restrict__ last_used;   // stamped by the wave of tile 0; or null
  long H, V, stamps, step;
  int D, c0, lane;
  bool has_init;
  InitArgs init;
  long key;                       // the lane's own

  DEVINL long item(long p, bool& valid) {
    key = keys[p];
    const long r = probe_find(slot_keys, slot_rows, key, H);
    if (r >= 0) {
      valid = r < V;
      if (last_used && c0 == 0 && r < stamps) last_used[r] = step;
      return r;
    }
    valid = has_init && key != EMPTY;
    return -1;
  }
  // the load is issued before the (wave-uniform) branch, so that four of
  // them stay in flight when every key has a row; V >= 1
  DEVINL void fetch(long r, int k, float (&v)[ACC]) {
    ld_tile<bf16_t, VEC>(table + (r > 0 ? r : 0) * D, c0, lane, D, v);
    if (r < 0)
      init_tile<VEC>(init_base(init, __shfl(key, k)), init.scale, c0, lane, D,
                     v);
  }
};

// One wave per (bag, 256-column tile), as embedding_bag_kernel.
template <typename O, int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void hash_bag_kernel(
    const long* __restrict__ keys, const long* __restrict__ slot_keys,
    const long* __restrict__ slot_rows, const bf16_t* __restrict__ table,
    const long* __restrict__ offsets, const float* __restrict__ weights,
    O* __restrict__ out, long* __restrict__ last_used, long B, long n, long H,
    long V, int D, int tiles, int mean, long stamps, long step, int has_init,
    InitArgs init) {
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
  KeyedRows<VEC> src = {keys, slot_keys, slot_rows, table, last_used, H, V,
                        stamps, step, D, c0, lane, has_init != 0, init,
                        EMPTY};
  bag_walk(src, weights, s, e, W, mean != 0, lane, acc);
  st_tile<O, VEC>(out + b * D, c0, lane, D, acc);   // empty bag: zeros
}

// One wave per (position, 256-column tile); s1 / s2 may be null.
template <int VEC>
__global__ __launch_bounds__(WAVES * WAVE) void init_rows_kernel(
    const long* __restrict__ keys, const long* __restrict__ rows,
    const bool* __restrict__ is_new, float* __restrict__ master,
    bf16_t* __restrict__ shadow, float* __restrict__ s1,
    float* __restrict__ s2, long n, long V, int D, int tiles, long seed,
    long key_mul, long key_add, float scale) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (w >= n * tiles) return;   // wave-uniform
  const long i = w / tiles;
  const int c0 = (int)(w % tiles) * TILE;
  if (!is_new[i]) return;
  const long row = rows[i];
  if (row < 0 || row >= V) return;
  const u64 k = (u64)keys[i] * (u64)key_mul + (u64)key_add;
  const u64 b = mix64(mix64((u64)seed + GOLD) ^ k);
  float v[ACC], zero[ACC];
#pragma unroll
  for (int e = 0; e < ACC; ++e) {
    const int col = VEC == 4 ? c0 + lane * 4 + e : c0 + e * WAVE + lane;
    v[e] = init_value(b, col, scale);
    zero[e] = 0.f;
  }
  st_tile<float, VEC>(master + row * D, c0, lane, D, v);
  st_tile<bf16_t, VEC>(shadow + row * D, c0, lane, D, v);
  if (s1) st_tile<float, VEC>(s1 + row * D, c0, lane, D, zero);
  if (s2) st_tile<float, VEC>(s2 + row * D, c0, lane, D, zero);
}

// Use stamps: last_used[rows[i]] = step. Duplicates store the same value.
__global__ __launch_bounds__(BLOCK) void touch_kernel(
    const long* __restrict__ rows, long* __restrict__ last_used, long n,
    long capacity, long step) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const long r = rows[i];
  if (r >= 0 && r < capacity) last_used[r] = step;
}

// compact 1: flags[r] = row r is live and kept; lane 0 saves the size the
// later kernels work from (no lane of this kernel reads old_size).
__global__ __launch_bounds__(BLOCK) void keep_flag_kernel(
    const bool* __restrict__ keep, const long* __restrict__ size,
    int* __restrict__ flags, long* __restrict__ old_size, long capacity) {
  const long r = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= capacity) return;
  long sz = size[0];
  sz = sz < 0 ? 0 : (sz > capacity ? capacity : sz);
  flags[r] = r < sz && keep[r];
  if (r == 0) old_size[0] = sz;
}

// compact 2: holes (evicted rows below K) and movers (kept rows at or above
// K), each written at its rank. incl is the inclusive scan of flags, K =
// incl[capacity - 1]; both lists have K - incl[K - 1] entries.
__global__ __launch_bounds__(BLOCK) void plan_kernel(
    const int* __restrict__ flags, const long* __restrict__ incl,
    const long* __restrict__ old_size, long* __restrict__ holes,
    long* __restrict__ movers, long capacity) {
  const long r = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= capacity || r >= old_size[0]) return;
  const long K = incl[capacity - 1];
  if (r < K) {
    if (!flags[r]) holes[r - incl[r]] = r;    // evicted rows in [0, r] - 1
  } else if (flags[r]) {
    const long below = K > 0 ? incl[K - 1] : 0;
    movers[incl[r] - 1 - below] = r;          // kept rows in [K, r] - 1
  }
}

// The row tensors that travel with a row: base, bytes per row, and the
// access width (16, or the element size when D or the base rule 16 out).
struct CompactTabs {
  char* base[4];
  int row_bytes[4];
  int width[4];
  int count;
};

template <typename U>
DEVINL void copy_row(const char* __restrict__ src, char* __restrict__ dst,
                     int row_bytes, int lane) {
  for (int c = lane * (int)sizeof(U); c < row_bytes; c += WAVE * (int)sizeof(U))
    *(U*)(dst + c) = *(const U*)(src + c);
}

// compact 3: one wave per mover copies row movers[j] onto row holes[j] in
// every tensor; sources (>= K) and destinations (< K) are disjoint. The
// number of movers lives on the device, so a grid of fixed size strides
// over them.
__global__ __launch_bounds__(WAVES * WAVE) void move_kernel(
    CompactTabs tabs, const long* __restrict__ incl,
    const long* __restrict__ holes, const long* __restrict__ movers,
    long* __restrict__ row_keys, long* __restrict__ last_used,
    long capacity) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long w0 = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const long stride = (long)gridDim.x * WAVES;
  const long K = incl[capacity - 1];
  const long M = K > 0 && K <= capacity ? K - incl[K - 1] : 0;
  for (long j = w0; j < M && j < capacity; j += stride) {   // wave-uniform
    const long h = holes[j], m = movers[j];
    if (h < 0 || h >= capacity || m < 0 || m >= capacity) continue;
    if (lane == 0) {
      row_keys[h] = row_keys[m];
      if (last_used) last_used[h] = last_used[m];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < tabs.count) {
        const int rb = tabs.row_bytes[t];
        const char* src = tabs.base[t] + m * rb;
        char* dst = tabs.base[t] + h * rb;
        if (tabs.width[t] == 16) copy_row<uint4>(src, dst, rb, lane);
        else if (tabs.width[t] == 4) copy_row<unsigned>(src, dst, rb, lane);
        else copy_row<unsigned short>(src, dst, rb, lane);
      }
    }
  }
}

// compact 4: EMPTY behind the survivors, and the counters. No lane reads
// size or evicted: the old size comes from kernel 1's copy.
__global__ __launch_bounds__(BLOCK) void finalize_kernel(
    const long* __restrict__ incl, const long* __restrict__ old_size,
    long* __restrict__ row_keys, long* __restrict__ size,
    long* __restrict__ evicted, long capacity) {
  const long r = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (r >= capacity) return;
  const long sz = old_size[0], K = incl[capacity - 1];
  if (r >= K && r < sz) row_keys[r] = EMPTY;
  if (r == 0) {
    size[0] = K;
    evicted[0] += sz - K;
  }
}

inline dim3 lanes_grid(long n) {
  return dim3((unsigned)((n + BLOCK - 1) / BLOCK));
}

}  // namespace

// rows [n], n > 0; last_used [capacity].
void launch_hash_touch(const long* rows, long* last_used, long n,
                       long capacity, long step, hipStream_t stream) {
  hipLaunchKernelGGL(touch_kernel, lanes_grid(n), dim3(BLOCK), 0, stream, rows,
                     last_used, n, capacity, step);
}

// Kernel 1 of a compaction. keep bool [capacity], flags int32 [capacity],
// old_size int64 [1]; capacity > 0.
void launch_hash_compact_flags(const bool* keep, const long* size, int* flags,
                               long* old_size, long capacity,
                               hipStream_t stream) {
  hipLaunchKernelGGL(keep_flag_kernel, lanes_grid(capacity), dim3(BLOCK), 0,
                     stream, keep, size, flags, old_size, capacity);
}

// Kernels 2 to 4. incl: int64 inclusive scan of flags; holes / movers int64
// [capacity]; bases / row_bytes / elem_bytes describe count <= 4 row tensors
// of capacity rows; last_used [capacity] or null.
void launch_hash_compact_move(const int* flags, const long* incl,
                              const long* old_size, long* holes, long* movers,
                              void* const* bases, const int* row_bytes,
                              const int* elem_bytes, int count,
                              long* row_keys, long* last_used, long* size,
                              long* evicted, long capacity,
                              hipStream_t stream) {
  hipLaunchKernelGGL(plan_kernel, lanes_grid(capacity), dim3(BLOCK), 0, stream,
                     flags, incl, old_size, holes, movers, capacity);
  CompactTabs tabs = {};
  tabs.count = count;
  for (int t = 0; t < count; ++t) {
    tabs.base[t] = (char*)bases[t];
    tabs.row_bytes[t] = row_bytes[t];
    const bool wide = (row_bytes[t] % 16) == 0 &&
                      ((uintptr_t)bases[t] % 16) == 0;
    tabs.width[t] = wide ? 16 : elem_bytes[t];
  }
  // at most capacity / 2 movers; MOVE_BLOCKS blocks fill the device
  constexpr long MOVE_BLOCKS = 2048;
  long blocks = (capacity / 2 + WAVES) / WAVES;
  if (blocks > MOVE_BLOCKS) blocks = MOVE_BLOCKS;
  hipLaunchKernelGGL(move_kernel, dim3((unsigned)blocks), dim3(WAVES * WAVE),
                     0, stream, tabs, incl, holes, movers, row_keys,
                     last_used, capacity);
  hipLaunchKernelGGL(finalize_kernel, lanes_grid(capacity), dim3(BLOCK), 0,
                     stream, incl, old_size, row_keys, size, evicted,
                     capacity);
}

// keys [n], n > 0 -> rows [n].
void launch_hash_find(const long* keys, const long* slot_keys,
                      const long* slot_rows, long* rows, long n, long H,
                      hipStream_t stream) {
  hipLaunchKernelGGL(find_kernel, lanes_grid(n), dim3(BLOCK), 0, stream, keys,
                     slot_keys, slot_rows, rows, n, H);
}

// Kernels 1 and 2. skeys / spos: int64 [S] filled with INT64_MIN, S a power
// of two >= 2n; flags int32 [n]. n > 0.
void launch_hash_lookup(const long* keys, const long* slot_keys,
                        const long* slot_rows, long* rows, long* skeys,
                        long* spos, int* flags, long n, long H, long S,
                        hipStream_t stream) {
  hipLaunchKernelGGL(lookup_kernel, lanes_grid(n), dim3(BLOCK), 0, stream,
                     keys, slot_keys, slot_rows, rows, skeys, spos, n, H, S);
  hipLaunchKernelGGL(flag_kernel, lanes_grid(n), dim3(BLOCK), 0, stream, keys,
                     rows, skeys, spos, flags, n, S);
}

// Kernels 3 and 4. incl: int64 inclusive scan of flags; is_new bool [n].
void launch_hash_insert(const long* keys, const int* flags, const long* incl,
                        long* slot_keys, long* slot_rows, long* row_keys,
                        long* size, long* dropped, long* rows, bool* is_new,
                        long n, long H, long capacity, hipStream_t stream) {
  hipLaunchKernelGGL(insert_kernel, lanes_grid(n), dim3(BLOCK), 0, stream,
                     keys, flags, incl, slot_keys, slot_rows, row_keys, size,
                     is_new, n, H, capacity);
  hipLaunchKernelGGL(resolve_kernel, lanes_grid(n), dim3(BLOCK), 0, stream,
                     keys, slot_keys, slot_rows, incl, rows, size, dropped, n,
                     H, capacity);
}

// Kernels A and B of find_or_admit, between launch_hash_lookup and the scan:
// counters int32 [4, width], width a power of two; flags / pass int32 [n];
// filtered int64 [1]; 1 <= admit_after <= 2^30; n > 0.
void launch_hash_admit(const long* keys, const int* flags, int* counters,
                       int* pass, long* filtered, long n, long width,
                       long admit_after, hipStream_t stream) {
  hipLaunchKernelGGL(count_kernel, lanes_grid(n), dim3(BLOCK), 0, stream,
                     keys, flags, (unsigned*)counters, n, width);
  hipLaunchKernelGGL(decide_kernel, lanes_grid(n), dim3(BLOCK), 0, stream,
                     keys, flags, (const unsigned*)counters, pass, filtered,
                     n, width, (unsigned)admit_after);
}

// slot_keys filled with INT64_MIN by the caller; capacity > 0.
void launch_hash_rebuild(const long* row_keys, const long* size,
                         long* slot_keys, long* slot_rows, long H,
                         long capacity, hipStream_t stream) {
  hipLaunchKernelGGL(rebuild_kernel, lanes_grid(capacity), dim3(BLOCK), 0,
                     stream, row_keys, size, slot_keys, slot_rows, H,
                     capacity);
}

// table bf16 [V,D] -> out bf16 [n,D]; n, D > 0.
void launch_hash_gather(const long* keys, const long* slot_keys,
                        const long* slot_rows, const bf16_t* table,
                        bf16_t* out, long n, long H, long V, int D,
                        hipStream_t stream) {
  const dim3 grid((unsigned)((n + WAVES - 1) / WAVES));
  const uintptr_t bases = (uintptr_t)table | (uintptr_t)out;
  if ((D % 4) == 0 && (bases % 8) == 0)
    hipLaunchKernelGGL(hash_gather_kernel<4>, grid, dim3(WAVES * WAVE), 0,
                       stream, keys, slot_keys, slot_rows, table, out, n, H,
                       V, D);
  else
    hipLaunchKernelGGL(hash_gather_kernel<1>, grid, dim3(WAVES * WAVE), 0,
                       stream, keys, slot_keys, slot_rows, table, out, n, H,
                       V, D);
}

// master fp32 / shadow bf16 [V,D], s1 / s2 fp32 [V,D] or null; n, D > 0.
void launch_hash_init_rows(const long* keys, const long* rows,
                           const bool* is_new, float* master, bf16_t* shadow,
                           float* s1, float* s2, long n, long V, int D,
                           long seed, long key_mul, long key_add, float scale,
                           hipStream_t stream) {
  const int tiles = (D + TILE - 1) / TILE;
  const dim3 grid((unsigned)((n * tiles + WAVES - 1) / WAVES));
  if (tile_vec4(D, master, shadow, s1, s2))
    hipLaunchKernelGGL(init_rows_kernel<4>, grid, dim3(WAVES * WAVE), 0,
                       stream, keys, rows, is_new, master, shadow, s1, s2, n,
                       V, D, tiles, seed, key_mul, key_add, scale);
  else
    hipLaunchKernelGGL(init_rows_kernel<1>, grid, dim3(WAVES * WAVE), 0,
                       stream, keys, rows, is_new, master, shadow, s1, s2, n,
                       V, D, tiles, seed, key_mul, key_add, scale);
}

// table bf16 [V,D] -> out bf16 [n,D], a miss reads the key's initial row;
// last_used int64 [stamps] or null; n, D > 0.
void launch_hash_gather_init(const long* keys, const long* slot_keys,
                             const long* slot_rows, const bf16_t* table,
                             bf16_t* out, long* last_used, long n, long H,
                             long V, int D, long stamps, long step, long seed,
                             long key_mul, long key_add, float scale,
                             hipStream_t stream) {
  const dim3 grid((unsigned)((n + WAVES - 1) / WAVES));
  const InitArgs init = {seed, key_mul, key_add, scale};
  const uintptr_t bases = (uintptr_t)table | (uintptr_t)out;
  if ((D % 4) == 0 && (bases % 8) == 0)
    hipLaunchKernelGGL(hash_gather_init_kernel<4>, grid, dim3(WAVES * WAVE),
                       0, stream, keys, slot_keys, slot_rows, table, out,
                       last_used, n, H, V, D, stamps, step, init);
  else
    hipLaunchKernelGGL(hash_gather_init_kernel<1>, grid, dim3(WAVES * WAVE),
                       0, stream, keys, slot_keys, slot_rows, table, out,
                       last_used, n, H, V, D, stamps, step, init);
}

namespace {

template <typename O>
void launch_bag_typed(const long* keys, const long* slot_keys,
                      const long* slot_rows, const bf16_t* table,
                      const long* offsets, const float* weights, O* out,
                      long* last_used, long B, long n, long H, long V, int D,
                      bool mean, long stamps, long step, bool has_init,
                      const InitArgs& init, hipStream_t stream) {
  const int tiles = (D + TILE - 1) / TILE;
  const dim3 block(WAVES * WAVE);
  const dim3 grid((unsigned)((B * tiles + WAVES - 1) / WAVES));
  if (tile_vec4(D, table, out))
    hipLaunchKernelGGL((hash_bag_kernel<O, 4>), grid, block, 0, stream, keys,
                       slot_keys, slot_rows, table, offsets, weights, out,
                       last_used, B, n, H, V, D, tiles, (int)mean, stamps,
                       step, (int)has_init, init);
  else
    hipLaunchKernelGGL((hash_bag_kernel<O, 1>), grid, block, 0, stream, keys,
                       slot_keys, slot_rows, table, offsets, weights, out,
                       last_used, B, n, H, V, D, tiles, (int)mean, stamps,
                       step, (int)has_init, init);
}

}  // namespace

// table bf16 [V,D], V >= 1; out [B,D] bf16 or fp32; weights may be null;
// last_used int64 [stamps] or null; B, n, D > 0.
void launch_hash_embedding_bag(const long* keys, const long* slot_keys,
                               const long* slot_rows, const bf16_t* table,
                               const long* offsets, const float* weights,
                               void* out, bool o_bf16, long* last_used,
                               long B, long n, long H, long V, int D,
                               bool mean, long stamps, long step,
                               bool has_init, long seed, long key_mul,
                               long key_add, float scale,
                               hipStream_t stream) {
  const InitArgs init = {seed, key_mul, key_add, scale};
  if (o_bf16)
    launch_bag_typed(keys, slot_keys, slot_rows, table, offsets, weights,
                     (bf16_t*)out, last_used, B, n, H, V, D, mean, stamps,
                     step, has_init, init, stream);
  else
    launch_bag_typed(keys, slot_keys, slot_rows, table, offsets, weights,
                     (float*)out, last_used, B, n, H, V, D, mean, stamps,
                     step, has_init, init, stream);
}

// Fused sparse optimizer apply for embedding tables (PS push path).
//
// TF's SparseApply* semantics: duplicate ids are SUMMED first, then the
// optimizer runs once per touched row — which a scatter-add cannot
// express (Adagrad/Adam/momentum need the row's summed gradient). This
// is the store-and-sum shape instead of float atomics: the binding
// stable-sorts the ids (the inverted index: every destination row's
// contributions become one contiguous run of the permutation, in
// original-position order), and everything after it is here:
//
//   * one wave owns one destination row: it walks the row's run in
//     order, accumulates in fp32 registers, applies the optimizer with
//     the exact per-element formulas of apply.hip, and writes master,
//     state and the bf16 shadow row in the same pass. Fixed order, no
//     atomics => bit-reproducible. Untouched rows are never accessed.
//   * hot ids: a run longer than CHUNK contributions is cut into CHUNK-
//     row pieces (relative to the run start) that separate waves sum
//     into an fp32 scratch; the owning wave adds the partials in chunk
//     order (one wave per destination otherwise runs as long as the
//     longest list).
//   * no compaction and no device->host sync: each wave inspects a
//     window of 64 sorted positions (one per lane), ballots the run
//     heads among them and processes those; grids are sized from n.
//     A long run starting at sorted position s owns the scratch slots
//     s/256 + k (k = chunk index): the slot scheme of run_sum.h.
//   * a lane owns VEC consecutive columns per step (ld_vec / st_vec of
//     tile.h): f32x4 / bf16x4 accesses and 256 columns per step when
//     D % 4 == 0 and the bases are 16-byte aligned (VEC == 4); otherwise
//     one column per lane and 64 per step (a vector access on an odd-D
//     row would be misaligned).
//   * ids outside [0, V) are ignored (they sort to the ends and are
//     never heads).
//   * bag mode (pooled push): grads holds one row per CSR bag; position i
//     contributes coef[i] * grads[bag_of[i]]. bag_expand_kernel derives
//     bag_of / coef from the offsets (+ weights, combiner); the run
//     summation takes them as a trailing BagIdx argument. An EMPTY
//     trailing pack is row mode: the row-mode kernels keep their
//     signature and compile to the code they had before bag mode.
#include "common.h"

#include "bag.h"
#include "ftrl.h"
#include "run_sum.h"
#include "sparse_apply.h"

namespace {

constexpr int WAVES = 4;       // waves (64-position windows) per block

// Bag mode's per-position indirection: position i of the push reads bag
// gradient row bag_of[i], scaled by coef[i].
struct BagIdx {
  const int* __restrict__ bag_of;
  const float* __restrict__ coef;
};

DEVINL const BagIdx& bag_idx(const BagIdx& b) { return b; }

// acc += sum of grads[perm[j]] over the leading positions j in
// [pos, pos+cap) whose sorted id equals id, in position order. The wave
// reads the index 64 positions at a time (one per lane) and broadcasts
// each source row; 4 row loads are kept in flight. All 64 lanes must
// call this (ballot/shuffle); `active` lanes own the VEC columns at col.
// Bag mode (one trailing BagIdx): the term of position i = perm[j] is
// coef[i] * grads[bag_of[i]] instead.
template <typename G, int VEC, typename... BagP>
DEVINL void sum_run(const long* __restrict__ sorted,
                    const long* __restrict__ perm,
                    const G* __restrict__ grads, long n, long pos, int cap,
                    long id, int D, int col, bool active, int lane,
                    float (&acc)[VEC], BagP... bagp) {
  constexpr bool BAG = sizeof...(BagP) != 0;
  for (int done = 0; done < cap; done += WAVE) {
    const long j = pos + done + lane;
    const bool match = (done + lane < cap) && j < n && sorted[j] == id;
    long src = match ? perm[j] : 0;
    float cf = 0.f;
    if constexpr (BAG) {
      const BagIdx& bi = bag_idx(bagp...);
      if (match) {
        cf = bi.coef[src];
        src = bi.bag_of[src];
      }
    }
    const unsigned long long miss = ~__ballot(match);
    const int cnt = miss ? __ffsll(miss) - 1 : WAVE;
    int k = 0;
    for (; k + 4 <= cnt; k += 4) {
      const long r0 = __shfl(src, k), r1 = __shfl(src, k + 1);
      const long r2 = __shfl(src, k + 2), r3 = __shfl(src, k + 3);
      float f0 = 1.f, f1 = 1.f, f2 = 1.f, f3 = 1.f;
      if constexpr (BAG) {   // shuffles stay outside the divergent branch
        f0 = __shfl(cf, k), f1 = __shfl(cf, k + 1);
        f2 = __shfl(cf, k + 2), f3 = __shfl(cf, k + 3);
      }
      if (active) {
        float v0[VEC], v1[VEC], v2[VEC], v3[VEC];
        ld_vec<G, VEC>(grads + r0 * D + col, v0);
        ld_vec<G, VEC>(grads + r1 * D + col, v1);
        ld_vec<G, VEC>(grads + r2 * D + col, v2);
        ld_vec<G, VEC>(grads + r3 * D + col, v3);
        if constexpr (BAG) {
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            acc[e] = (((acc[e] + f0 * v0[e]) + f1 * v1[e]) + f2 * v2[e]) +
                     f3 * v3[e];
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            acc[e] = (((acc[e] + v0[e]) + v1[e]) + v2[e]) + v3[e];
        }
      }
    }
    for (; k < cnt; ++k) {
      const long r = __shfl(src, k);
      float f = 1.f;
      if constexpr (BAG) f = __shfl(cf, k);
      if (active) {
        float v[VEC];
        ld_vec<G, VEC>(grads + r * D + col, v);
        if constexpr (BAG) {
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += f * v[e];
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] += v[e];
        }
      }
    }
    if (cnt < WAVE) break;
  }
}

// One element of the optimizer step: the formulas of apply.hip's dense
// kernels, on the row's summed gradient g. (Adam's 1-beta and bias
// corrections arrive rounded from double: a hot row's summed gradient
// is large enough to show fp32's error in 1.f - 0.999f.) FTRL-Proximal is
// the rule of ftrl.h (a = accumulator, c = linear term; no weight decay).
template <int OPT>
DEVINL void apply_elem(float& pv, float& a, float& c, float g,
                       const SparseHp& hp) {
  if (OPT == SPARSE_FTRL) {
    ftrl_elem(pv, a, c, g, FtrlHp{hp.lr, hp.l1, hp.l2, hp.acc0, hp.gscale});
    return;
  }
  float gv = g * hp.gscale;
  if (hp.wd != 0.f) gv += hp.wd * pv;
  if (OPT == SPARSE_SGD) {
    pv -= hp.lr * gv;
  } else if (OPT == SPARSE_SGD_MOM) {
    const float m = a * hp.beta1 + gv;
    a = m;
    pv -= hp.lr * m;
  } else if (OPT == SPARSE_ADAGRAD) {
    const float acc = a + gv * gv;
    a = acc;
    pv -= hp.lr * gv / (__builtin_sqrtf(acc) + hp.eps);
  } else {
    const float mv = hp.beta1 * a + hp.omb1 * gv;
    const float vv = hp.beta2 * c + hp.omb2 * gv * gv;
    a = mv;
    c = vv;
    pv -= hp.lr * (mv / hp.bc1) / (__builtin_sqrtf(vv / hp.bc2) + hp.eps);
  }
}

// Pass 1 (only launched when n > CHUNK): the chunk heads of LONG runs
// sum their <= CHUNK contributions into scratch[slot].
template <typename G, int VEC, typename... BagP>
__global__ __launch_bounds__(WAVES * WAVE) void sparse_partial_kernel(
    const long* __restrict__ sorted, const long* __restrict__ perm,
    const G* __restrict__ grads, float* __restrict__ scratch, long n, int D,
    long V, BagP... bagp) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long base = ((long)blockIdx.x * WAVES + (threadIdx.x >> 6)) * WAVE;
  const long i = base + lane;
  long rs = -1;  // run start, set iff position i heads a chunk of a long run
  if (i < n) {
    const long id = sorted[i];
    if (id >= 0 && id < V) {
      if (i == 0 || sorted[i - 1] != id) {
        if (i + CHUNK < n && sorted[i + CHUNK] == id) rs = i;
      } else if (i >= CHUNK && sorted[i - CHUNK] == id) {
        // deep inside a long run: find its start (lower bound of id)
        long lo = 0, hi = i - CHUNK;
        while (lo < hi) {
          const long mid = (lo + hi) >> 1;
          if (sorted[mid] < id) lo = mid + 1; else hi = mid;
        }
        if ((i - lo) % CHUNK == 0) rs = lo;
      }
    }
  }
  unsigned long long heads = __ballot(rs >= 0);
  while (heads) {
    const int b = __ffsll(heads) - 1;
    heads &= heads - 1;
    const long pos = base + b;
    const long start = __shfl(rs, b);
    const long id = sorted[pos];
    const long slot = start / SLOT_DIV + (pos - start) / CHUNK;
    for (int c0 = 0; c0 < D; c0 += WAVE * VEC) {
      const int col = c0 + lane * VEC;
      const bool active = col < D;
      float acc[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
      sum_run<G, VEC>(sorted, perm, grads, n, pos, CHUNK, id, D, col, active,
                      lane, acc, bagp...);
      if (active) st_vec<float, VEC>(scratch + slot * D + col, acc);
    }
  }
}

// Pass 2: one wave per touched row (run head) — sum, apply, store.
template <typename G, int VEC, int OPT, typename... BagP>
__global__ __launch_bounds__(WAVES * WAVE) void sparse_apply_kernel(
    float* __restrict__ table, const long* __restrict__ sorted,
    const long* __restrict__ perm, const G* __restrict__ grads,
    const float* __restrict__ scratch, float* __restrict__ s1,
    float* __restrict__ s2, bf16_t* __restrict__ shadow, long n, int D,
    long V, SparseHp hp, BagP... bagp) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long base = ((long)blockIdx.x * WAVES + (threadIdx.x >> 6)) * WAVE;
  const long i = base + lane;
  bool head = false;
  if (i < n) {
    const long id = sorted[i];
    head = id >= 0 && id < V && (i == 0 || sorted[i - 1] != id);
  }
  unsigned long long heads = __ballot(head);
  while (heads) {
    const int b = __ffsll(heads) - 1;
    heads &= heads - 1;
    const long pos = base + b;
    const long id = sorted[pos];
    const bool is_long = pos + CHUNK < n && sorted[pos + CHUNK] == id;
    for (int c0 = 0; c0 < D; c0 += WAVE * VEC) {
      const int col = c0 + lane * VEC;
      const bool active = col < D;
      const long off = id * D + col;
      // row state first: independent of the index walk below
      float p[VEC], a[VEC], c[VEC];
      if (active) {
        ld_vec<float, VEC>(table + off, p);
        if (OPT >= SPARSE_SGD_MOM) ld_vec<float, VEC>(s1 + off, a);
        if (OPT >= SPARSE_ADAM) ld_vec<float, VEC>(s2 + off, c);
      }
      float g[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) g[e] = 0.f;
      if (!is_long) {
        sum_run<G, VEC>(sorted, perm, grads, n, pos, CHUNK, id, D, col, active,
                        lane, g, bagp...);
      } else {
        // partial sums of pass 1, added in chunk order
        long slot = pos / SLOT_DIV;
        for (long q = pos; q < n && sorted[q] == id; q += CHUNK, ++slot) {
          if (active) {
            float v[VEC];
            ld_vec<float, VEC>(scratch + slot * D + col, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) g[e] += v[e];
          }
        }
      }
      if (active) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          apply_elem<OPT>(p[e], a[e], c[e], g[e], hp);
        st_vec<float, VEC>(table + off, p);
        if (OPT >= SPARSE_SGD_MOM) st_vec<float, VEC>(s1 + off, a);
        if (OPT >= SPARSE_ADAM) st_vec<float, VEC>(s2 + off, c);
        if (shadow != nullptr) st_vec<bf16_t, VEC>(shadow + off, p);
      }
    }
  }
}

// Bag mode's expansion: one wave per bag writes, for each of its
// positions, the bag's row number and the coefficient c_i (bag.h), after
// reducing W_b for mean. Unweighted bags read no weights. bag_of / coef
// arrive zeroed, so a position no bag covers (an offsets contract
// violation) contributes 0 * grads[0].
__global__ __launch_bounds__(WAVES * WAVE) void bag_expand_kernel(
    const long* __restrict__ offsets, const float* __restrict__ weights,
    int* __restrict__ bag_of, float* __restrict__ coef, long B, long n,
    int mean) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long b = (long)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;   // wave-uniform
  long s, e;
  bag_range(offsets, b, n, s, e);
  const float W = mean ? bag_weight_sum(weights, s, e, lane) : 0.f;
  for (long p = s + lane; p < e; p += WAVE) {
    bag_of[p] = (int)b;
    coef[p] = bag_coef(weights ? weights[p] : 1.f, W, mean != 0);
  }
}

template <typename G, int VEC, typename... BagP>
void launch_typed(int opt, float* table, const long* sorted, const long* perm,
                  const G* grads, float* scratch, float* s1, float* s2,
                  bf16_t* shadow, long n, int D, long V, const SparseHp& hp,
                  hipStream_t stream, BagP... bagp) {
  const dim3 block(WAVES * WAVE);
  const dim3 grid((unsigned)((n + WAVES * WAVE - 1) / (WAVES * WAVE)));
  if (n > CHUNK)
    hipLaunchKernelGGL((sparse_partial_kernel<G, VEC, BagP...>), grid, block,
                       0, stream, sorted, perm, grads, scratch, n, D, V,
                       bagp...);
#define DISP(OPTV)                                                          \
  hipLaunchKernelGGL((sparse_apply_kernel<G, VEC, OPTV, BagP...>), grid,    \
                     block, 0, stream, table, sorted, perm, grads, scratch, \
                     s1, s2, shadow, n, D, V, hp, bagp...)
  switch (opt) {
    case SPARSE_SGD: DISP(SPARSE_SGD); break;
    case SPARSE_SGD_MOM: DISP(SPARSE_SGD_MOM); break;
    case SPARSE_ADAGRAD: DISP(SPARSE_ADAGRAD); break;
    case SPARSE_ADAM: DISP(SPARSE_ADAM); break;
    case SPARSE_FTRL: DISP(SPARSE_FTRL); break;
    default: break;   // no such code: the binding has rejected it
  }
#undef DISP
}

template <typename... BagP>
void launch_any(int opt, float* table, const long* sorted, const long* perm,
                const void* grads, bool g_bf16, float* scratch, float* s1,
                float* s2, bf16_t* shadow, long n, int D, long V,
                const SparseHp& hp, hipStream_t stream, BagP... bagp) {
  const bool vec = tile_vec4(D, table, grads, scratch, s1, s2, shadow);
  if (g_bf16) {
    if (vec) launch_typed<bf16_t, 4>(opt, table, sorted, perm,
                                     (const bf16_t*)grads, scratch, s1, s2,
                                     shadow, n, D, V, hp, stream, bagp...);
    else launch_typed<bf16_t, 1>(opt, table, sorted, perm,
                                 (const bf16_t*)grads, scratch, s1, s2,
                                 shadow, n, D, V, hp, stream, bagp...);
  } else {
    if (vec) launch_typed<float, 4>(opt, table, sorted, perm,
                                    (const float*)grads, scratch, s1, s2,
                                    shadow, n, D, V, hp, stream, bagp...);
    else launch_typed<float, 1>(opt, table, sorted, perm,
                                (const float*)grads, scratch, s1, s2, shadow,
                                n, D, V, hp, stream, bagp...);
  }
}

}  // namespace

// sorted/perm: the stable sort of the ids and its permutation (n > 0).
// scratch: fp32 [run_scratch_rows(n), D] (may be null when 0 rows).
void launch_sparse_apply(int opt, float* table, const long* sorted,
                         const long* perm, const void* grads, bool g_bf16,
                         float* scratch, float* s1, float* s2, bf16_t* shadow,
                         long n, int D, long V, const SparseHp& hp,
                         hipStream_t stream) {
  launch_any(opt, table, sorted, perm, grads, g_bf16, scratch, s1, s2, shadow,
             n, D, V, hp, stream);
}

// offsets [B+1] (+ weights [n] or null) -> bag_of / coef [n], both zeroed
// by the caller. B, n > 0.
void launch_bag_expand(const long* offsets, const float* weights, int* bag_of,
                       float* coef, long B, long n, bool mean,
                       hipStream_t stream) {
  const dim3 grid((unsigned)((B + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(bag_expand_kernel, grid, dim3(WAVES * WAVE), 0, stream,
                     offsets, weights, bag_of, coef, B, n, (int)mean);
}

// launch_sparse_apply with grads = [B,D] bag gradients and the per-position
// bag_of / coef of launch_bag_expand.
void launch_sparse_apply_bag(int opt, float* table, const long* sorted,
                             const long* perm, const void* grads, bool g_bf16,
                             const int* bag_of, const float* coef,
                             float* scratch, float* s1, float* s2,
                             bf16_t* shadow, long n, int D, long V,
                             const SparseHp& hp, hipStream_t stream) {
  launch_any(opt, table, sorted, perm, grads, g_bf16, scratch, s1, s2, shadow,
             n, D, V, hp, stream, BagIdx{bag_of, coef});
}

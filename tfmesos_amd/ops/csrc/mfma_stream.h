// The scheme shared by the kernels that own 64 rows as MFMA A fragments and
// stream another row set through row-major LDS tiles (sampled_softmax.hip,
// bag_attention.hip, retrieval.hip), written once: the geometry, guarded
// 16-byte row pieces with a row stride, the owned-fragment load, the tile's
// fetch and stash, the 16 x 64 score block, the image-times-tile block with
// its transpose reads, the park-and-store epilogue, the double-buffer loop,
// and on the host the DP x VEC dispatch and the split rule.
// sampled_softmax.hip takes the geometry, the leaf helpers and the host side
// from here and keeps its own text of the device pieces: built from the
// functions below its backward kernels measured 1 to 16 % slower.
// Included after common.h, inside the including file's anonymous namespace
// and its no-packed-fp32-ops attribute region, so that the helpers carry the
// target features of the kernels they are inlined into; callables passed to
// the helpers are defined inside that region for the same reason.
#pragma once

// A block of WAVES waves owns OWN rows: wave w the rows 16w..16w+15.
constexpr int WAVES = 4;
constexpr int OWN = WAVES * 16;   // owned rows per block
constexpr int TILE = 64;          // streamed rows per tile
constexpr int ST = TILE / 16;     // 16-column tiles of the scores
constexpr int PL = TILE + 8;      // P image row stride
[[maybe_unused]] constexpr float NEG = -1e30f;   // "no kept score yet": finite,
                                  // so that the merge of two empty halves is
                                  // exp(0) * 0

// What follows from DP, the columns of registers a row takes.
template <int DP> struct Stream {
  static constexpr int XL = DP + 8;     // tile row stride
  static constexpr int KS = DP / 32;    // K steps of the scores
  static constexpr int NT = DP / 16;    // 16-column tiles of the output rows
  static constexpr int PPR = DP / 8;    // 16-byte pieces per tile row
  static constexpr int PIECES = TILE * PPR / (WAVES * WAVE);   // == KS
};

// Lane coordinates inside a wave's 16 rows. An A or B fragment: row
// frag_row, K offset frag_k inside a 32-wide step. An accumulator: column
// frag_row, rows acc_row(lane, 0..3).
DEVINL int frag_row(int lane) { return lane & 15; }
DEVINL int frag_k(int lane) { return (lane >> 4) << 3; }
DEVINL int acc_row(int lane, int r) { return (lane >> 4) * 4 + r; }

// rows[row * rs + k .. +8) where live, zero where not or outside [0,D);
// rs = row stride
template <bool VEC>
DEVINL bf16x8 ld_piece_if(bool live, const __bf16* __restrict__ rows, long row,
                          int k, int D, long rs) {
  bf16x8 z = {};
  if (VEC) {     // D % 8 == 0: a piece that starts inside the row ends inside
    const bool ok = live && k < D;
    const bf16x8 g = *(const bf16x8*)(rows + (ok ? row * rs + k : 0));
    return ok ? g : z;
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) z[e] = rows[row * rs + k + e];
  }
  return z;
}

// the same, zero outside [0,nrows) x [0,D)
template <bool VEC>
DEVINL bf16x8 ld_piece(const __bf16* __restrict__ rows, int row, int nrows,
                       int k, int D, long rs) {
  return ld_piece_if<VEC>(row < nrows, rows, row, k, D, rs);
}

template <bool VEC>
DEVINL void st_piece(__bf16* __restrict__ rows, int row, int k, int D, long rs,
                     bf16x8 v) {
  __bf16* dst = rows + (long)row * rs + k;
  if (VEC) {
    *(bf16x8*)dst = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k + e < D) dst[e] = v[e];
  }
}

DEVINL bf16x4 tr_read(const __bf16* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)p);
}

// MFMA B fragment out of a [row][d] image of stride XL: rows kfrag..kfrag+7
// at column cb + (lane & 15), two transpose-reads of four image rows each
// (lane mapping: gemm.hip, interaction.hip)
template <int XL>
DEVINL bf16x8 tr_frag(const __bf16* X, int kfrag, int cb, int lane) {
  const int a = (kfrag + ((lane & 15) >> 2)) * XL + cb + 4 * (lane & 3);
  const bf16x4 f0 = tr_read(&X[a]);
  const bf16x4 f1 = tr_read(&X[a + 4 * XL]);
  return __builtin_shufflevector(f0, f1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// orders a wave's own LDS writes before its own LDS reads of other lanes'
// data (the P image, the epilogue's parked tile)
DEVINL void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the 16 lanes that share an accumulator row, fixed order
DEVINL float row_sum16(float v) {
#pragma unroll
  for (int x = 1; x < 16; x <<= 1) v += __shfl_xor(v, x);
  return v;
}

// The A fragments of this lane's owned row: row row0 + frag_row of a row set
// of nrows rows, loaded once from global memory.
template <int DP, bool VEC>
DEVINL void load_owned(bf16x8 (&af)[DP / 32], const __bf16* rows, int row0,
                       int nrows, int D, long rs, int lane) {
#pragma unroll
  for (int ks = 0; ks < DP / 32; ++ks)
    af[ks] = ld_piece<VEC>(rows, row0 + frag_row(lane), nrows,
                           ks * 32 + frag_k(lane), D, rs);
}

// A streamed tile, global -> registers. src(tile row) is the row of `rows`
// staged there, or negative for none (a row of zeros).
template <int DP, bool VEC, class Src>
DEVINL void tile_fetch(bf16x8 (&pre)[DP / 32], const __bf16* rows, int D,
                       long rs, int tid, Src src) {
  typedef Stream<DP> G;
#pragma unroll
  for (int i = 0; i < G::PIECES; ++i) {
    const int p = tid + WAVES * WAVE * i;
    const long j = src(p / G::PPR);
    pre[i] = ld_piece_if<VEC>(j >= 0, rows, j, (p % G::PPR) * 8, D, rs);
  }
}

// registers -> the tile buffer T, [row][d] of stride DP + 8
template <int DP>
DEVINL void tile_stash(__bf16* T, const bf16x8 (&pre)[DP / 32], int tid) {
  typedef Stream<DP> G;
#pragma unroll
  for (int i = 0; i < G::PIECES; ++i) {
    const int p = tid + WAVES * WAVE * i;
    *(bf16x8*)&T[(p / G::PPR) * G::XL + (p % G::PPR) * 8] = pre[i];
  }
}

// acc += 16 x 64 scores of the owned fragments against the tile T: the B
// fragment is a 16-byte LDS read of a streamed row
template <int DP>
DEVINL void score_tile(const bf16x8 (&af)[DP / 32], const __bf16* T,
                       f32x4 (&acc)[ST], int D, int lane) {
  typedef Stream<DP> G;
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) {
    if (ks * 32 < D) {
#pragma unroll
      for (int nt = 0; nt < ST; ++nt) {
        const bf16x8 b = *(const bf16x8*)&T[(nt * 16 + frag_row(lane)) * G::XL +
                                            ks * 32 + frag_k(lane)];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], b, acc[nt],
                                                          0, 0, 0);
      }
    }
  }
}

// acc += P . T: the wave's image P (16 x 64, stride PL) is the A operand, the
// B fragments come back from the row-major tile through transpose reads
template <int DP>
DEVINL void image_times_tile(const __bf16* P, const __bf16* T,
                             f32x4 (&acc)[DP / 16], int D, int lane) {
  typedef Stream<DP> G;
  wave_lds_sync();
#pragma unroll
  for (int k2 = 0; k2 < TILE / 32; ++k2) {
    const bf16x8 pa =
        *(const bf16x8*)&P[frag_row(lane) * PL + k2 * 32 + frag_k(lane)];
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt) {
      if (nt * 16 < D) {
        const bf16x8 b =
            tr_frag<G::XL>(T, k2 * 32 + frag_k(lane), nt * 16, lane);
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, b, acc[nt], 0, 0,
                                                          0);
      }
    }
  }
  wave_lds_sync();                  // the image is rewritten next
}

// A wave's 16 x DP output tile acc leaves through R, its 16 rows of an idle
// tile buffer: val(v, r, slot) is the value stored for the accumulator
// element v of row r, whose slot in R it may read first; rounded to bf16
// once, then 16-byte row-contiguous stores to rows row0.. of dst, those
// below nrows.
template <int DP, bool VEC, class Val>
DEVINL void park_store(const f32x4 (&acc)[DP / 16], __bf16* R, __bf16* dst,
                       int row0, int nrows, int D, long rs, int lane,
                       Val val) {
  typedef Stream<DP> G;
#pragma unroll
  for (int nt = 0; nt < G::NT; ++nt) {
    if (nt * 16 < D) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        __bf16* slot = &R[acc_row(lane, r) * G::XL + nt * 16 + frag_row(lane)];
        *slot = (__bf16)val(acc[nt][r], r, slot);
      }
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < G::PIECES; ++i) {
    const int p = lane + WAVE * i;
    const int row = row0 + p / G::PPR, c = (p % G::PPR) * 8;
    if (row < nrows && c < D)
      st_piece<VEC>(dst, row, c, D, rs,
                    *(const bf16x8*)&R[(p / G::PPR) * G::XL + c]);
  }
}

// The double-buffer loop over the tiles [t_begin, t_end): fetch(t) issues the
// global loads of tile t, stash(buf) writes them to buffer buf, body(t, buf)
// is the arithmetic on tile t. The loads of tile t+1 are issued before the
// arithmetic of tile t and stashed after it, one block barrier per tile.
// (retrieval.hip writes the same loop out: through this function its
// counting kernel measured 1 to 1.5 % slower.)
template <class Fetch, class Stash, class Body>
DEVINL void stream_tiles(int t_begin, int t_end, Fetch fetch, Stash stash,
                         Body body) {
  if (t_begin < t_end) {
    fetch(t_begin);
    stash(0);
  }
  __syncthreads();
  for (int t = t_begin; t < t_end; ++t) {
    const int buf = (t - t_begin) & 1;
    const bool more = t + 1 < t_end;    // block-uniform
    if (more) fetch(t + 1);
    body(t, buf);
    if (more) stash(buf ^ 1);
    __syncthreads();
  }
}

// ---- host side

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// fn(DpVec<DP, VEC>()) with the smallest DP in {64, 128, 256} that holds D;
// MAXDP (128 or 256) is the largest the kernel is built for, D <= MAXDP
template <int DP, bool VEC> struct DpVec {
  static constexpr int dp = DP;
  static constexpr bool vec = VEC;
};
template <int MAXDP, class Fn>
inline void dispatch_dp_vec(int D, bool vec, Fn fn) {
  if (D <= 64) {
    if (vec) fn(DpVec<64, true>()); else fn(DpVec<64, false>());
  } else if (MAXDP == 128 || D <= 128) {
    if (vec) fn(DpVec<128, true>()); else fn(DpVec<128, false>());
  } else if constexpr (MAXDP == 256) {
    if (vec) fn(DpVec<256, true>()); else fn(DpVec<256, false>());
  }
}

// The split rule of a streamed row set of n_str rows. The default number of
// splits, for n_own owned rows: 256 blocks' worth.
inline long stream_default_splits(long n_own) {
  const long n = 256 / ((n_own + OWN - 1) / OWN);
  return n < 1 ? 1 : n;
}
// `splits` clamped to [1, tiles] and to the grid's y limit, then the fewest
// splits of that many tiles each (no split is empty)
inline int stream_splits(long n_str, long splits) {
  const long ntiles = (n_str + TILE - 1) / TILE;
  long n = splits < 1 ? 1 : splits > ntiles ? ntiles : splits;
  n = n > 65535 ? 65535 : n;
  const long per = (ntiles + n - 1) / n;
  return (int)((ntiles + per - 1) / per);
}

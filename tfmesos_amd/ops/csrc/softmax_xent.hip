// Fused softmax + cross-entropy (fwd: mean loss + probs; bwd: dlogits).
//
// The reference workload's loss (softmax_cross_entropy_with_logits,
// examples/mnist/mnist_replica.py:143-145). One wave64 per row; the
// class dimension (10 for mnist, up to 4096 supported) is reduced with
// wave shuffles — no LDS round trip, no separate log-softmax pass.
#include "common.h"
#include "softmax_xent.h"
#include "mlp_head.h"

namespace {

DEVINL float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

DEVINL float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    v += __shfl_xor(v, off, WAVE);
  return v;
}

// rows B, classes C; loss_out accumulates sum(-log p[label]) / B
__global__ void softmax_xent_fwd_kernel(const bf16_t* __restrict__ logits,
                                        const long* __restrict__ labels,
                                        bf16_t* __restrict__ probs,
                                        float* __restrict__ loss_out,
                                        int B, int C) {
  const int row = blockIdx.x;
  if (row >= B) return;
  const int lane = threadIdx.x;
  const bf16_t* lrow = logits + (long)row * C;
  bf16_t* prow = probs + (long)row * C;

  float mx = -1e30f;
  for (int c = lane; c < C; c += WAVE) mx = fmaxf(mx, bf2f(lrow[c]));
  mx = wave_max(mx);

  float sum = 0.f;
  for (int c = lane; c < C; c += WAVE) sum += __expf(bf2f(lrow[c]) - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;

  const long label = labels[row];
  float neglogp = 0.f;
  for (int c = lane; c < C; c += WAVE) {
    float p = __expf(bf2f(lrow[c]) - mx) * inv;
    prow[c] = f2bf(p);
    if (c == (int)label) neglogp = -__logf(fmaxf(p, 1e-30f));
  }
  neglogp = wave_sum(neglogp);
  if (lane == 0) atomicAdd(loss_out, neglogp / B);
}

// dlogits = (probs - onehot(label)) * scale
__global__ void softmax_xent_bwd_kernel(const bf16_t* __restrict__ probs,
                                        const long* __restrict__ labels,
                                        bf16_t* __restrict__ dlogits,
                                        float scale, int B, int C) {
  const int row = blockIdx.x;
  if (row >= B) return;
  const int lane = threadIdx.x;
  const bf16_t* prow = probs + (long)row * C;
  bf16_t* drow = dlogits + (long)row * C;
  const long label = labels[row];
  for (int c = lane; c < C; c += WAVE) {
    float v = bf2f(prow[c]) - (c == (int)label ? 1.f : 0.f);
    drow[c] = f2bf(v * scale);
  }
}

// Fully fused fwd+bwd for small class counts (mnist C=10): ONE kernel
// computes mean loss AND dlogits = (softmax - onehot)*scale, replacing
// the fwd kernel + bwd kernel + per-step loss zero-fill of the unfused
// path (each launch costs ~5us at this size — see profiles/). One
// workgroup, one row per thread (B<=256, C<=32): loss is tree-reduced in
// LDS and written once, so no atomics and no pre-zeroed buffer needed.
__global__ __launch_bounds__(256)
void softmax_xent_fused_kernel(const bf16_t* __restrict__ logits,
                               const long* __restrict__ labels,
                               bf16_t* __restrict__ dlogits,
                               float* __restrict__ loss_out, float scale,
                               int B, int C) {
  __shared__ float lsum[256];
  const int r = threadIdx.x;
  float neglogp = 0.f;
  if (r < B) {
    const bf16_t* lrow = logits + (long)r * C;
    bf16_t* drow = dlogits + (long)r * C;
    const int label = (int)labels[r];
    float mx = -1e30f;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, bf2f(lrow[c]));
    float sum = 0.f;
    for (int c = 0; c < C; ++c) sum += __expf(bf2f(lrow[c]) - mx);
    const float inv = 1.f / sum;
    for (int c = 0; c < C; ++c) {
      const float p = __expf(bf2f(lrow[c]) - mx) * inv;
      drow[c] = f2bf((p - (c == label ? 1.f : 0.f)) * scale);
      if (c == label) neglogp = -__logf(fmaxf(p, 1e-30f));
    }
  }
  lsum[r] = neglogp;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (r < s) lsum[r] += lsum[r + s];
    __syncthreads();
  }
  if (r == 0) *loss_out = lsum[0] / B;
}

}  // namespace

void launch_softmax_xent_fused(const bf16_t* logits, const long* labels,
                               bf16_t* dlogits, float* loss, float scale,
                               int B, int C, hipStream_t stream) {
  hipLaunchKernelGGL(softmax_xent_fused_kernel, dim3(1), dim3(256), 0, stream,
                     logits, labels, dlogits, loss, scale, B, C);
}

void launch_softmax_xent_fwd(const bf16_t* logits, const long* labels,
                             bf16_t* probs, float* loss, int B, int C,
                             hipStream_t stream) {
  hipLaunchKernelGGL(softmax_xent_fwd_kernel, dim3(B), dim3(WAVE), 0, stream,
                     logits, labels, probs, loss, B, C);
}

void launch_softmax_xent_bwd(const bf16_t* probs, const long* labels,
                             bf16_t* dlogits, float scale, int B, int C,
                             hipStream_t stream) {
  hipLaunchKernelGGL(softmax_xent_bwd_kernel, dim3(B), dim3(WAVE), 0, stream,
                     probs, labels, dlogits, scale, B, C);
}

namespace {

// Fully fused MLP classifier head for the mnist_replica hot step:
//   logits = h @ w + b ; softmax ; mean xent loss ;
//   dlogits = (p - onehot)/B ; dh = (dlogits @ w^T) * (h > 0)
// ONE single-workgroup kernel replacing three ~5-6 us launches (the
// per-kernel execution floor dominates at these sizes — see profiles/).
// One THREAD per row; h is staged through LDS with COALESCED
// cooperative copies (per-thread row walks over global memory are
// 64-way divergent and ran 10x slower), weights are read as f32x4
// broadcasts, dh is written back through the same LDS staging. Every
// class loop is unrolled to the 16-class cap: runtime-bounded loops
// over register arrays would demote acc[]/dl[] to scratch.
// Constraints: C <= 16, H <= 512, B <= 512, B*(H+8) <= 15000.
__global__ __launch_bounds__(512)
void mlp_head_fused_kernel(const bf16_t* __restrict__ h,
                           const bf16_t* __restrict__ w,
                           const bf16_t* __restrict__ bias,
                           const long* __restrict__ labels,
                           bf16_t* __restrict__ dlogits,
                           bf16_t* __restrict__ dh,
                           float* __restrict__ loss_out,
                           float scale, int B, int H, int C) {
  __shared__ __align__(16) float ws[512][16];    // 32 KB, f32x4 reads
  __shared__ __align__(16) __bf16 hs[15000];     // [B][H+8] staged rows
  __shared__ float lsum[512];
  const int t = threadIdx.x;
  const int hp = H + 8;
  for (int i = t; i < H * C; i += 512)
    ws[i / C][i % C] = bf2f(w[i]);
  for (int i = t; i < B * H; i += 512)
    hs[(i / H) * hp + (i % H)] = *(const __bf16*)&h[i];
  __syncthreads();

  float neglogp = 0.f;
  if (t < B) {
    __bf16* hrow = &hs[t * hp];
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = (j < C) ? bf2f(bias[j]) : 0.f;
    for (int e = 0; e < H; ++e) {
      const float hv = (float)hrow[e];
      const f32x4* wrow = (const f32x4*)ws[e];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q * 4 >= C) break;
        const f32x4 wv = wrow[q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (q * 4 + j < C) acc[q * 4 + j] += hv * wv[j];
      }
    }
    float mx = -1e30f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j >= C) break;
      mx = fmaxf(mx, acc[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j >= C) break;
      acc[j] = __expf(acc[j] - mx);
      sum += acc[j];
    }
    const float inv = 1.f / sum;
    const int label = (int)labels[t];
    float dl[16];
    bf16_t* drow = dlogits + (long)t * C;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j >= C) break;
      const float p = acc[j] * inv;
      dl[j] = (p - (j == label ? 1.f : 0.f)) * scale;
      drow[j] = f2bf(dl[j]);
      if (j == label) neglogp = -__logf(fmaxf(p, 1e-30f));
    }
    // dh into the LDS staging (overwrite h rows in place)
    for (int e = 0; e < H; ++e) {
      const float hv = (float)hrow[e];
      const f32x4* wrow = (const f32x4*)ws[e];
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q * 4 >= C) break;
        const f32x4 wv = wrow[q];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (q * 4 + j < C) v += dl[q * 4 + j] * wv[j];
      }
      hrow[e] = (__bf16)(hv > 0.f ? v : 0.f);
    }
  }
  lsum[t] = neglogp;
  __syncthreads();
  // coalesced writeback of dh
  for (int i = t; i < B * H; i += 512)
    dh[i] = *(bf16_t*)&hs[(i / H) * hp + (i % H)];
#pragma unroll
  for (int s = 256; s > 0; s >>= 1) {
    if (t < s) lsum[t] += lsum[t + s];
    __syncthreads();
  }
  if (t == 0) *loss_out = lsum[0] / B;
}

// MFMA rewrite of the fused head for the benchmark geometry (B<=128,
// H<=128, C<=16): one 256-thread workgroup where all four waves
// cooperate — logits and dh are v_mfma_f32_32x32x16_bf16 tiles instead
// of the per-thread serial H-loops that made the first version 40 us
// (100 of 512 threads active). Cuts the mnist step's critical path
// from {logits GEMM, softmax, dh GEMM} = three ~5-7 us launches to one
// kernel.
// phase-stamp debug hook (tools/headbench.py --phases): wall_clock64
// per phase per workgroup, written when the pointer is armed
__device__ unsigned long long* g_head_dbg = nullptr;

DEVINL void head_stamp(int t, int phase) {
  if (g_head_dbg != nullptr && t == 0)
    g_head_dbg[blockIdx.x * 16 + phase] = wall_clock64();
}

// tile constants (HB, HP, CP, LSP) and the logits / softmax / dh
// phases live in mlp_head.h, shared with the fused head+tail kernel

// dw2/db2 (optional): the weight/bias grads of the classifier are
// computed IN the same kernel (both operands already live in LDS),
// removing the dW2 GEMM launch from the step entirely. GF32 selects
// fp32 vs bf16 grad stores (the trainer's flat grad buffer dtype).
// FROMWS: h arrives as the fwd GEMM's fp32 split-K stripes (wsrc,
// nslice of them, [B*H] each) instead of a materialized tensor — the
// stripe reduce + bias1 + relu happen while staging hs into LDS, so h
// never touches global memory and the separate reduce kernel is gone.
// Requires H % 4 == 0 (f32x4 chunks stay within one row).
template <bool GF32, bool FROMWS>
__global__ __launch_bounds__(256)
void mlp_head_mfma_kernel(const bf16_t* __restrict__ h,
                          const float* __restrict__ wsrc, int nslice,
                          const bf16_t* __restrict__ bias1,
                          const bf16_t* __restrict__ w,
                          const bf16_t* __restrict__ bias,
                          const long* __restrict__ labels,
                          bf16_t* __restrict__ dlogits,
                          bf16_t* __restrict__ dh,
                          float* __restrict__ loss_out,
                          void* __restrict__ dw2v,
                          void* __restrict__ db2v,
                          float scale, int B, int H, int C) {
  __shared__ __align__(16) __bf16 hs[HB * HP];      // [row][k]
  // 32 rows (not CP): the B-fragment's lane index spans the full
  // 32-wide MFMA tile, so cols C..31 must read zeros, not neighbors
  __shared__ __align__(16) __bf16 wtp[32 * HP];     // [c][k]  (w^T)
  __shared__ __align__(16) __bf16 wpad[HB * CP];    // [hrow][c]
  __shared__ __align__(16) __bf16 dls[HB * CP];     // [row][c]
  // transposed copy for the dW2 B-fragments: [c][b] rows make the
  // fragment reads aligned b128 instead of 8 latency-exposed scalar
  // gathers per MFMA step (32 rows: fragment lanes span a full tile)
  __shared__ __align__(16) __bf16 dlsT[32 * HP];
  // transposed h copy [col][row]: b64 relu-mask reads in the dh phase
  // and b128 A-fragments in dW2 (both were 64 serial scalar LDS
  // gathers per thread — the dh phase alone measured 4.4 us of the
  // 11 us kernel, see tools/headbench.py --phases)
  __shared__ __align__(16) __bf16 hsT[HB * HP];
  __shared__ float ls[HB * LSP];   // fp32 logits staging
  __shared__ float lsum[256];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wr = t >> 6;
  head_stamp(t, 0);

  // zero the padded operand tiles (b128 stores — the scalar version
  // was ~28K LDS writes), then stage h and w (scalar; tiny tensors)
  {
    const bf16x8 z8 = {};
    for (int i = t * 8; i < HB * HP; i += 256 * 8)
      *(bf16x8*)&hs[i] = z8;
    for (int i = t * 8; i < 32 * HP; i += 256 * 8)
      *(bf16x8*)&wtp[i] = z8;
    for (int i = t * 8; i < HB * CP; i += 256 * 8)
      *(bf16x8*)&wpad[i] = z8;
    for (int i = t * 8; i < HB * CP; i += 256 * 8)
      *(bf16x8*)&dls[i] = z8;
    for (int i = t * 8; i < 32 * HP; i += 256 * 8)
      *(bf16x8*)&dlsT[i] = z8;
    for (int i = t * 8; i < HB * HP; i += 256 * 8)
      *(bf16x8*)&hsT[i] = z8;
  }
  __syncthreads();
  head_stamp(t, 1);
  // staging walks 4-element row chunks (H % 4 == 0, binding-checked):
  // chunks never cross a row, so each is ONE aligned b64 global load +
  // ONE b64 LDS store with a single division per chunk. The previous
  // flat-index walk paid 2 integer divisions (~30 VALU each) plus an
  // 8-scalar-store carry loop per chunk — the head's PMC showed ~6.7k
  // issue slots per wave on a ~0.5 MFLOP kernel.
  {
    const int H4 = H >> 2;
    const int nch = B * H4;
    const int rstep = 256 / H4;          // uniform per-iteration walk:
    const int cstep = 256 - rstep * H4;  // ONE division per thread total
    int row = t / H4;
    int c4i = t - row * H4;
    for (int k = t; k < nch; k += 256) {
      const int c4 = c4i * 4;
      if (FROMWS) {
        const int BH = B * H;
        const int i = row * H + c4;
        f32x4 v = {};
        for (int z = 0; z < nslice; ++z) {
          const f32x4 sv = *(const f32x4*)&wsrc[(long)z * BH + i];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += sv[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float f = v[j] + (float)bias1[c4 + j];
          const __bf16 r = (__bf16)(f > 0.f ? f : 0.f);
          hs[row * HP + c4 + j] = r;
          hsT[(c4 + j) * HP + row] = r;
        }
      } else {
        const bf16x4 v4 = *(const bf16x4*)&h[(long)row * H + c4];
        *(bf16x4*)&hs[row * HP + c4] = v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) hsT[(c4 + j) * HP + row] = v4[j];
      }
      row += rstep;
      c4i += cstep;
      if (c4i >= H4) { c4i -= H4; ++row; }
    }
  }
  // w rows are C elements: one thread per h-row, no divisions
  for (int hr = t; hr < H; hr += 256) {
    for (int c = 0; c < C; ++c) {
      const __bf16 v = *(const __bf16*)&w[hr * C + c];
      wtp[c * HP + hr] = v;
      wpad[hr * CP + c] = v;
    }
  }
  __syncthreads();
  head_stamp(t, 2);

  // logits[B,C] = hs @ w: wave wr owns rows 32wr..32wr+31
  {
    const f32x16v acc = head_logits_tile(
        &hs[(wr * 32 + (lane & 31)) * HP], &wtp[(lane & 31) * HP], lane);
    const int col = lane & 31;
    const float bc = col < C ? bf2f(bias[col]) : 0.f;
    head_store_logits(ls, acc, wr * 32, bc, lane);
  }
  __syncthreads();
  head_stamp(t, 3);

  // rowwise softmax + dlogits (one thread per row, C <= 16 scalar).
  // Two-workgroup split: WG0 owns {loss, dlogits store, dh}, WG1 owns
  // {dW2, db2} — both recompute the cheap logits/softmax (22 KB of
  // reads) so the two expensive output phases run in parallel.
  const bool wg0 = blockIdx.x == 0;
  const bool wg1 = blockIdx.x + 1 == gridDim.x;
  float neglogp = 0.f;
  if (t < B) {
    const int label = (int)labels[t];
    neglogp = head_softmax_row(
        &ls[t * LSP], C, label, scale, [&](int c, float d) {
          dls[t * CP + c] = (__bf16)d;
          dlsT[c * HP + t] = (__bf16)d;
          if (wg0) dlogits[(long)t * C + c] = f2bf(d);
        });
  }
  lsum[t] = neglogp;
  __syncthreads();
  head_stamp(t, 4);

  // dh[B,H] = dls @ w^T, relu-masked by h>0: wave wr owns rows
  // 32wr..+31, loops the four 32-wide H column tiles; K = C (one MFMA)
  if (wg0) {
    const int arow = wr * 32 + (lane & 31);
#pragma unroll
    for (int ct = 0; ct < HB / 32; ++ct) {
      const f32x16v acc = head_dh_tile(
          &dls[arow * CP], &wpad[(ct * 32 + (lane & 31)) * CP], lane);
      const int colh = ct * 32 + (lane & 31);
      if (colh < H) {
        // relu mask: 4 b64 reads of the transposed copy (one per
        // 4-consecutive-row group of the D fragment) instead of 16
        // serial scalar gathers across hs rows
        const int rbase = wr * 32 + ((lane >> 5) << 2);
        bf16x4 mk[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
          mk[g] = *(const bf16x4*)&hsT[colh * HP + rbase + g * 8];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = wr * 32 + head_frag_row(v, lane);
          if (row < B) {
            const float m =
                (float)mk[v >> 2][v & 3] > 0.f ? acc[v] : 0.f;
            dh[(long)row * H + colh] = f2bf(m);
          }
        }
      }
    }
  }
  head_stamp(t, 5);

  // dW2[H,C] = h^T @ dls (K = B, one 32-row tile per wave) — both
  // operands are in LDS already, so the step's separate dW2 GEMM
  // launch disappears. Transposed A reads are scalar gathers (tiny).
  if (wg1 && dw2v != nullptr) {
    f32x16v acc = {};
#pragma unroll
    for (int kh = 0; kh < HB / 16; ++kh) {
      const int k0 = kh * 16 + ((lane >> 5) << 3);
      bf16x8 a = *(const bf16x8*)&hsT[(wr * 32 + (lane & 31)) * HP + k0];
      bf16x8 bv = *(const bf16x8*)&dlsT[(lane & 31) * HP + k0];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bv, acc, 0, 0, 0);
    }
    const int c = lane & 31;
    if (c < C) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int hrow = wr * 32 + ((v >> 2) << 3) + ((lane >> 5) << 2) +
                         (v & 3);
        if (hrow < H) {
          if (GF32) ((float*)dw2v)[hrow * C + c] = acc[v];
          else ((bf16_t*)dw2v)[hrow * C + c] = f2bf(acc[v]);
        }
      }
    }
    // db2[c] = sum_b dls[b][c]: 16 partial lanes per class (the serial
    // B-loop was ~100 dependent LDS reads on 10 threads)
    __shared__ float db2p[CP * 16];
    if (t < C * 16) {
      const int c = t >> 4, part = t & 15;
      float s = 0.f;
      for (int b2 = part; b2 < B; b2 += 16) s += (float)dlsT[c * HP + b2];
      db2p[t] = s;
    }
    __syncthreads();
    if (t < C) {
      float s = 0.f;
#pragma unroll
      for (int p2 = 0; p2 < 16; ++p2) s += db2p[t * 16 + p2];
      if (GF32) ((float*)db2v)[t] = s;
      else ((bf16_t*)db2v)[t] = f2bf(s);
    }
  }
  head_stamp(t, 6);

  // mean loss
  if (!wg0) return;
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) lsum[t] += lsum[t + s];
    __syncthreads();
  }
  if (t == 0) *loss_out = lsum[0] / B;
  head_stamp(t, 7);
}

}  // namespace

void launch_mlp_head_fused(const bf16_t* h, const bf16_t* w,
                           const bf16_t* bias, const long* labels,
                           bf16_t* dlogits, bf16_t* dh, float* loss,
                           void* dw2, void* db2, bool grads_f32,
                           float scale, int B, int H, int C,
                           hipStream_t stream) {
  if (B <= 128 && H <= 128 && C <= 16 && (H & 3) == 0) {
    dim3 hg(dw2 != nullptr ? 2 : 1);
    if (grads_f32)
      hipLaunchKernelGGL((mlp_head_mfma_kernel<true, false>), hg,
                         dim3(256), 0, stream, h, nullptr, 0, nullptr, w,
                         bias, labels, dlogits, dh, loss, dw2, db2, scale,
                         B, H, C);
    else
      hipLaunchKernelGGL((mlp_head_mfma_kernel<false, false>), hg,
                         dim3(256), 0, stream, h, nullptr, 0, nullptr, w,
                         bias, labels, dlogits, dh, loss, dw2, db2, scale,
                         B, H, C);
    return;
  }
  hipLaunchKernelGGL(mlp_head_fused_kernel, dim3(1), dim3(512), 0, stream,
                     h, w, bias, labels, dlogits, dh, loss, scale, B, H, C);
}

// head fed by the fwd GEMM's split-K stripes (see FROMWS above);
// bounds checked by the binding: B<=128, H<=128 (H%4==0), C<=16
void launch_mlp_fwd_head(const float* ws, int nslice, const bf16_t* b1,
                         const bf16_t* w, const bf16_t* bias,
                         const long* labels, bf16_t* dlogits, bf16_t* dh,
                         float* loss, void* dw2, void* db2, bool grads_f32,
                         float scale, int B, int H, int C,
                         hipStream_t stream) {
  dim3 hg(dw2 != nullptr ? 2 : 1);
  if (grads_f32)
    hipLaunchKernelGGL((mlp_head_mfma_kernel<true, true>), hg,
                       dim3(256), 0, stream, nullptr, ws, nslice, b1, w,
                       bias, labels, dlogits, dh, loss, dw2, db2, scale,
                       B, H, C);
  else
    hipLaunchKernelGGL((mlp_head_mfma_kernel<false, true>), hg,
                       dim3(256), 0, stream, nullptr, ws, nslice, b1, w,
                       bias, labels, dlogits, dh, loss, dw2, db2, scale,
                       B, H, C);
}

void set_head_debug(void* ptr) {
  // arm/disarm the per-phase wall_clock64 stamps (tools/headbench.py)
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_head_dbg), &ptr, sizeof(ptr));
}

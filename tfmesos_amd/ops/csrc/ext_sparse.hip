// Python bindings of the embedding and sparse parameter-server kernels:
// gather / scatter-add, pooled (bag) pull, fused sparse applies, shard
// partition, coalescing and hashed tables. Pure dispatch + shape checking;
// bind_sparse adds them to the module of ext.hip.
#include <climits>

#include "ext_util.h"

#include "coalesce.h"
#include "embedding.h"
#include "embedding_bag.h"
#include "hash.h"
#include "partition.h"
#include "run_sum.h"
#include "sparse_apply.h"

namespace {

// The fp32 scratch [run_scratch_rows(n), D] of a run sum over n positions
// (run_sum.h) and its pointer: undefined / null when no run can be long.
std::pair<torch::Tensor, float*> run_scratch(
    long n, long D, const torch::TensorOptions& options) {
  const long rows = run_scratch_rows(n);
  if (rows == 0) return {torch::Tensor(), nullptr};
  auto scratch = torch::empty({rows, D}, options.dtype(torch::kFloat32));
  return {scratch, scratch.data_ptr<float>()};
}

torch::Tensor embedding_gather(torch::Tensor table, torch::Tensor ids) {
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous(),
              "table must be contiguous [V,D] on GPU");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.dim() == 1,
              "ids must be i64 [N]");
  long n = ids.numel(), V = table.size(0);
  int D = table.size(1);
  auto out = torch::empty({n, (long)D}, table.options());
  if (n == 0) return out;
  if (table.scalar_type() == torch::kBFloat16)
    launch_gather_bf16((const bf16_t*)table.data_ptr(), ids.data_ptr<long>(),
                       (bf16_t*)out.data_ptr(), n, D, V, cur_stream());
  else if (table.scalar_type() == torch::kFloat32)
    launch_gather_f32(table.data_ptr<float>(), ids.data_ptr<long>(),
                      out.data_ptr<float>(), n, D, V, cur_stream());
  else
    TORCH_CHECK(false, "table must be bf16 or fp32");
  return out;
}

void embedding_scatter_add(torch::Tensor table, torch::Tensor ids,
                           torch::Tensor rows) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 &&
              table.is_contiguous(), "scatter-add table must be fp32 [V,D]");
  TORCH_CHECK(ids.scalar_type() == torch::kInt64, "ids must be i64");
  long n = ids.numel(), V = table.size(0);
  int D = table.size(1);
  if (n == 0) return;
  TORCH_CHECK(rows.is_contiguous() && rows.numel() == n * D,
              "rows shape mismatch");
  if (rows.scalar_type() == torch::kBFloat16)
    launch_scatter_add_bf16(table.data_ptr<float>(), ids.data_ptr<long>(),
                            (const bf16_t*)rows.data_ptr(), n, D, V,
                            cur_stream());
  else
    launch_scatter_add_f32(table.data_ptr<float>(), ids.data_ptr<long>(),
                           rows.data_ptr<float>(), n, D, V, cur_stream());
}

// Hyper-parameters of one sparse apply (row or bag mode).
SparseHp sparse_hp(long step, double lr, double beta1, double beta2,
                   double eps, double weight_decay, double grad_scale,
                   double l1, double l2, double acc0) {
  SparseHp hp;
  hp.lr = (float)lr;
  hp.gscale = (float)grad_scale;
  hp.wd = (float)weight_decay;
  hp.beta1 = (float)beta1;
  hp.beta2 = (float)beta2;
  hp.eps = (float)eps;
  // Adam constants in double, rounded once: fp32 (1.f - 0.999f) is off by
  // 4.7e-5 relative, which a hot row's large summed gradient makes
  // visible in exp_avg_sq
  hp.omb1 = (float)(1.0 - beta1);
  hp.omb2 = (float)(1.0 - beta2);
  hp.bc1 = (float)(1.0 - std::pow(beta1, (double)step));
  hp.bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  hp.l1 = (float)l1;
  hp.l2 = (float)l2;
  hp.acc0 = (float)acc0;
  return hp;
}

// CSR bag arguments shared by embedding_bag and sparse_apply_bag: ids i64
// [n], offsets i64 [B+1], weights fp32 [n] or empty. The contents of
// offsets are a caller contract (not read back: no device->host sync; the
// kernels clamp what they derive from it). Returns the weights pointer.
const float* bag_args(const char* op, const torch::Tensor& ids,
                      const torch::Tensor& offsets,
                      const torch::Tensor& weights) {
  TORCH_CHECK(i64_vec(ids), op, ": ids must be contiguous i64 [n] on GPU");
  TORCH_CHECK(i64_vec(offsets) && offsets.numel() >= 1,
              op, ": offsets must be contiguous i64 [B+1] on GPU");
  TORCH_CHECK(offsets.numel() - 1 <= (long)INT_MAX,
              op, ": too many bags");
  if (weights.numel() == 0) return nullptr;   // unweighted (or n == 0)
  TORCH_CHECK(weights.is_cuda() && weights.scalar_type() == torch::kFloat32 &&
              weights.is_contiguous() && weights.numel() == ids.numel(),
              op, ": weights must be contiguous fp32 [n] on GPU");
  return weights.data_ptr<float>();
}

// Pooled pull (embedding_bag.hip): out[b] = sum_i c_i * table[ids[i]] over
// bag b, fp32 accumulation in position order, rounded once. out is the
// table's dtype, or fp32 from a bf16 table with out_f32.
torch::Tensor embedding_bag(torch::Tensor table, torch::Tensor ids,
                            torch::Tensor offsets, torch::Tensor weights,
                            bool mean, bool out_f32) {
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous(),
              "embedding_bag: table must be contiguous [V,D] on GPU");
  const bool t_bf16 = table.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(t_bf16 || table.scalar_type() == torch::kFloat32,
              "embedding_bag: table must be bf16 or fp32");
  const float* w = bag_args("embedding_bag", ids, offsets, weights);
  const long n = ids.numel(), V = table.size(0), B = offsets.numel() - 1;
  const int D = table.size(1);
  const bool o_bf16 = t_bf16 && !out_f32;
  auto out = torch::empty({B, (long)D},
                          table.options().dtype(o_bf16 ? torch::kBFloat16
                                                       : torch::kFloat32));
  if (B == 0 || D == 0) return out;   // a zero-size grid is a launch error
  if (n == 0) return out.zero_();
  TORCH_CHECK(B * ((D + 255) / 256) / 4 < (long)INT_MAX,
              "embedding_bag: B x D too large for one grid");
  launch_embedding_bag(table.data_ptr(), t_bf16, ids.data_ptr<long>(),
                       offsets.data_ptr<long>(), w, out.data_ptr(), o_bf16, B,
                       n, D, V, mean, cur_stream());
  return out;
}

// Fused sparse optimizer apply (sparse_apply.hip), row and bag mode:
// duplicates summed, then ONE optimizer step per touched row, master + state
// + bf16 shadow in the same pass. The stable sort of the ids is the inverted
// index (plumbing; stays on the device, no host sync); everything after it
// is our HIP. state1/state2/shadow: empty tensors when unused.
// Row mode (offsets == nullptr): grads is [n,D], one row per id.
// Bag mode (pooled push): grads is [B,D]; position i of bag b contributes
// c_i * grads[b] (coefficient rule in bag.h). One expansion kernel derives
// bag row and coefficient per position from the offsets.
void sparse_apply_any(const char* op, torch::Tensor& table,
                      const torch::Tensor& ids, const torch::Tensor* offsets,
                      const torch::Tensor* weights, bool mean,
                      const torch::Tensor& grads, torch::Tensor& state1,
                      torch::Tensor& state2, torch::Tensor& shadow, long opt,
                      long step, double lr, double beta1, double beta2,
                      double eps, double weight_decay, double grad_scale,
                      double l1, double l2, double acc0) {
  const bool bag = offsets != nullptr;
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous() &&
              table.scalar_type() == torch::kFloat32,
              op, ": table must be contiguous fp32 [V,D] on GPU");
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == torch::kInt64 &&
              ids.dim() == 1, op, ": ids must be i64 [n] on GPU");
  TORCH_CHECK(opt >= SPARSE_SGD && opt <= SPARSE_FTRL,
              op, ": unknown optimizer code ", opt);
  const float* w = bag ? bag_args(op, ids, *offsets, *weights) : nullptr;
  const long n = ids.numel(), V = table.size(0);
  const long B = bag ? offsets->numel() - 1 : n;   // gradient rows
  const int D = table.size(1);
  TORCH_CHECK(grads.is_cuda() && grads.numel() == B * D,
              op, ": grads must be [", bag ? "B" : "n", ",D] on GPU");
  const long total = table.numel();
  float* s1 = opt_f32(state1, total, "state1");
  float* s2 = opt_f32(state2, total, "state2");
  bf16_t* shp = opt_bf16(shadow, total, "bf16_out");
  TORCH_CHECK((s1 == nullptr || state1.is_contiguous()) &&
              (s2 == nullptr || state2.is_contiguous()) &&
              (shp == nullptr || shadow.is_contiguous()),
              op, ": state/shadow must be contiguous");
  TORCH_CHECK(opt == SPARSE_SGD || s1 != nullptr,
              op, ": optimizer state tensor missing");
  TORCH_CHECK(opt != SPARSE_ADAM || (s2 != nullptr && step >= 1),
              op, ": adam needs exp_avg_sq and step >= 1");
  TORCH_CHECK(opt != SPARSE_FTRL ||
              (s2 != nullptr && lr > 0 && l1 >= 0 && l2 >= 0 && acc0 > 0),
              op, ": ftrl_proximal needs the linear state and lr > 0, "
              "l1 >= 0, l2 >= 0, initial_accumulator_value > 0");
  if (n == 0 || B == 0 || D == 0) return;   // zero-size grid: launch error
  bool gb;
  const void* g = grad_ptr(grads, &gb);
  torch::Tensor bag_of, coef;
  if (bag) {
    bag_of = torch::zeros({n}, ids.options().dtype(torch::kInt32));
    coef = torch::zeros({n}, ids.options().dtype(torch::kFloat32));
    launch_bag_expand(offsets->data_ptr<long>(), w, bag_of.data_ptr<int>(),
                      coef.data_ptr<float>(), B, n, mean, cur_stream());
  }
  const auto [sorted, perm] = stable_sort_ids(ids);
  const auto [scratch, scratch_p] = run_scratch(n, D, table.options());
  const SparseHp hp = sparse_hp(step, lr, beta1, beta2, eps, weight_decay,
                                grad_scale, l1, l2, acc0);
  if (bag)
    launch_sparse_apply_bag((int)opt, table.data_ptr<float>(),
                            sorted.data_ptr<long>(), perm.data_ptr<long>(), g,
                            gb, bag_of.data_ptr<int>(), coef.data_ptr<float>(),
                            scratch_p, s1, s2, shp, n, D, V, hp, cur_stream());
  else
    launch_sparse_apply((int)opt, table.data_ptr<float>(),
                        sorted.data_ptr<long>(), perm.data_ptr<long>(), g, gb,
                        scratch_p, s1, s2, shp, n, D, V, hp, cur_stream());
}

void sparse_apply(torch::Tensor table, torch::Tensor ids, torch::Tensor grads,
                  torch::Tensor state1, torch::Tensor state2,
                  torch::Tensor shadow, long opt, long step, double lr,
                  double beta1, double beta2, double eps, double weight_decay,
                  double grad_scale, double l1, double l2, double acc0) {
  sparse_apply_any("sparse_apply", table, ids, nullptr, nullptr, false, grads,
                   state1, state2, shadow, opt, step, lr, beta1, beta2, eps,
                   weight_decay, grad_scale, l1, l2, acc0);
}

void sparse_apply_bag(torch::Tensor table, torch::Tensor ids,
                      torch::Tensor offsets, torch::Tensor weights,
                      torch::Tensor grads, torch::Tensor state1,
                      torch::Tensor state2, torch::Tensor shadow, long opt,
                      long step, bool mean, double lr, double beta1,
                      double beta2, double eps, double weight_decay,
                      double grad_scale, double l1, double l2, double acc0) {
  sparse_apply_any("sparse_apply_bag", table, ids, &offsets, &weights, mean,
                   grads, state1, state2, shadow, opt, step, lr, beta1, beta2,
                   eps, weight_decay, grad_scale, l1, l2, acc0);
}

// Stable partition of ids by owning shard (partition.hip): count kernel,
// cumsum of the per-window counts (plumbing; stays on the device), scatter
// kernel. Returns local, perm, inv [n] and starts [S+1]; no host sync.
std::vector<torch::Tensor> shard_partition(torch::Tensor ids, long rows,
                                           long num_shards, bool div) {
  TORCH_CHECK(i64_vec(ids),
              "shard_partition: ids must be contiguous i64 [n] on GPU");
  TORCH_CHECK(num_shards >= 1 && num_shards <= 64 && rows >= num_shards,
              "shard_partition: need 1 <= num_shards <= 64 and "
              "rows >= num_shards");
  const long n = ids.numel();
  TORCH_CHECK(n < (long)INT_MAX, "shard_partition: n must be below 2^31");
  const int S = (int)num_shards;
  auto opt = ids.options();
  auto local = torch::empty({n}, opt), perm = torch::empty({n}, opt);
  auto inv = torch::empty({n}, opt);
  if (n == 0)   // a zero-size grid is a launch error
    return {local, perm, inv, torch::zeros({S + 1}, opt)};
  auto starts = torch::empty({S + 1}, opt);
  auto counts = torch::empty({S * shard_windows(n)},
                             opt.dtype(torch::kInt32));
  launch_shard_count(ids.data_ptr<long>(), counts.data_ptr<int>(), n, rows, S,
                     div, cur_stream());
  auto incl = torch::cumsum(counts, 0, torch::kInt64);
  launch_shard_scatter(ids.data_ptr<long>(), incl.data_ptr<long>(),
                       local.data_ptr<long>(), perm.data_ptr<long>(),
                       inv.data_ptr<long>(), starts.data_ptr<long>(), n, rows,
                       S, div, cur_stream());
  return {local, perm, inv, starts};
}

// out[j] = cast(rows[perm[j]]): a push's gradient rows in wire order and
// wire dtype in one pass. A perm entry outside [0, n_rows) gives a zero row.
torch::Tensor permute_rows(torch::Tensor rows, torch::Tensor perm,
                           bool out_bf16) {
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 2 && rows.is_contiguous(),
              "permute_rows: rows must be contiguous [n,D] on GPU");
  const bool r_bf16 = rows.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(r_bf16 || rows.scalar_type() == torch::kFloat32,
              "permute_rows: rows must be bf16 or fp32");
  TORCH_CHECK(i64_vec(perm),
              "permute_rows: perm must be contiguous i64 [m] on GPU");
  const long m = perm.numel(), D = rows.size(1);
  TORCH_CHECK(D <= (long)INT_MAX && (m + 3) / 4 < (long)INT_MAX,
              "permute_rows: too large for one grid");
  auto out = torch::empty({m, D},
                          rows.options().dtype(out_bf16 ? torch::kBFloat16
                                                        : torch::kFloat32));
  if (m == 0 || D == 0) return out;
  launch_permute_rows(rows.data_ptr(), r_bf16, perm.data_ptr<long>(),
                      out.data_ptr(), out_bf16, m, rows.size(0), (int)D,
                      cur_stream());
  return out;
}

// shard_offsets [S, B+1]: the CSR of a bagged request inside each shard's
// slice of the partition.
torch::Tensor shard_bag_offsets(torch::Tensor perm, torch::Tensor starts,
                                torch::Tensor offsets) {
  TORCH_CHECK(i64_vec(perm) && i64_vec(starts) && i64_vec(offsets),
              "shard_bag_offsets: perm, starts, offsets must be contiguous "
              "i64 vectors on GPU");
  TORCH_CHECK(starts.numel() >= 2 && starts.numel() <= 65 &&
              offsets.numel() >= 1, "shard_bag_offsets: starts must be "
              "[S+1], 1 <= S <= 64, offsets [B+1]");
  const long S = starts.numel() - 1, B = offsets.numel() - 1;
  TORCH_CHECK(S * (B + 1) / 256 < (long)INT_MAX,
              "shard_bag_offsets: too many bags");
  auto out = torch::empty({S, B + 1}, perm.options());
  launch_shard_bag_offsets(perm.data_ptr<long>(), starts.data_ptr<long>(),
                           offsets.data_ptr<long>(), out.data_ptr<long>(),
                           perm.numel(), B, (int)S, cur_stream());
  return out;
}

// c [n] fp32: the per-position coefficients of bag.h.
torch::Tensor bag_coefficients(long n, torch::Tensor offsets,
                               torch::Tensor weights, bool mean) {
  TORCH_CHECK(i64_vec(offsets) && offsets.numel() >= 1,
              "bag_coefficients: offsets must be contiguous i64 [B+1] on GPU");
  TORCH_CHECK(n >= 0 && offsets.numel() - 1 <= (long)INT_MAX,
              "bag_coefficients: bad n or too many bags");
  const float* w = nullptr;
  if (weights.numel() > 0) {
    TORCH_CHECK(weights.is_cuda() &&
                weights.scalar_type() == torch::kFloat32 &&
                weights.is_contiguous() && weights.numel() == n,
                "bag_coefficients: weights must be contiguous fp32 [n] on "
                "GPU");
    w = weights.data_ptr<float>();
  }
  const long B = offsets.numel() - 1;
  auto coef = torch::zeros({n}, offsets.options().dtype(torch::kFloat32));
  if (n == 0 || B == 0) return coef;
  launch_bag_coef(offsets.data_ptr<long>(), w, coef.data_ptr<float>(), B, n,
                  mean, cur_stream());
  return coef;
}

// The distinct ids of a request (coalesce.hip): stable sort of the ids and
// cumsum of the per-window head counts are plumbing (they stay on the
// device), the count and scatter kernels are ours. Returns uniq, inverse,
// perm [n], seg [n+1] and count [1]; no host sync.
std::vector<torch::Tensor> coalesce_ids(torch::Tensor ids) {
  TORCH_CHECK(i64_vec(ids),
              "coalesce_ids: ids must be contiguous i64 [n] on GPU");
  const long n = ids.numel();
  TORCH_CHECK(n < (long)INT_MAX, "coalesce_ids: n must be below 2^31");
  auto opt = ids.options();
  if (n == 0)   // a zero-size grid is a launch error
    return {torch::empty({0}, opt), torch::empty({0}, opt),
            torch::empty({0}, opt), torch::zeros({1}, opt),
            torch::zeros({1}, opt)};
  const auto [sorted, perm] = stable_sort_ids(ids);
  auto uniq = torch::empty({n}, opt), inverse = torch::empty({n}, opt);
  auto seg = torch::empty({n + 1}, opt), count = torch::empty({1}, opt);
  auto counts = torch::empty({coalesce_windows(n)}, opt.dtype(torch::kInt32));
  launch_coalesce_count(sorted.data_ptr<long>(), counts.data_ptr<int>(), n,
                        cur_stream());
  auto incl = torch::cumsum(counts, 0, torch::kInt64);
  launch_coalesce_scatter(sorted.data_ptr<long>(), perm.data_ptr<long>(),
                          incl.data_ptr<long>(), uniq.data_ptr<long>(),
                          inverse.data_ptr<long>(), seg.data_ptr<long>(),
                          count.data_ptr<long>(), n, cur_stream());
  return {uniq, inverse, perm, seg, count};
}

// out[k] = sum of rows[perm[j]] over j in [seg[k], seg[k+1]), k < num: fp32
// accumulation in that order, rounded once (coalesce.hip). The contents of
// perm and seg are a caller contract (not read back); the kernels clamp
// what they derive from them.
torch::Tensor segment_sum_rows(torch::Tensor rows, torch::Tensor perm,
                               torch::Tensor seg, long num, bool out_bf16) {
  TORCH_CHECK(rows.is_cuda() && rows.dim() == 2 && rows.is_contiguous(),
              "segment_sum_rows: rows must be contiguous [n,D] on GPU");
  const bool r_bf16 = rows.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(r_bf16 || rows.scalar_type() == torch::kFloat32,
              "segment_sum_rows: rows must be bf16 or fp32");
  TORCH_CHECK(i64_vec(perm) && i64_vec(seg),
              "segment_sum_rows: perm and seg must be contiguous i64 vectors "
              "on GPU");
  const long n = rows.size(0), D = rows.size(1);
  TORCH_CHECK(perm.numel() == n, "segment_sum_rows: perm must be [n]");
  TORCH_CHECK(num >= 0 && seg.numel() >= num + 1,
              "segment_sum_rows: seg must hold num + 1 entries");
  const long tiles = (D + 255) / 256;
  TORCH_CHECK(n < (long)INT_MAX && D <= (long)INT_MAX &&
              num * tiles / 4 < (long)INT_MAX &&
              (n / 256 + 1) * tiles / 4 < (long)INT_MAX,
              "segment_sum_rows: too large for one grid");
  auto out = torch::empty({num, D},
                          rows.options().dtype(out_bf16 ? torch::kBFloat16
                                                        : torch::kFloat32));
  if (num == 0 || D == 0) return out;   // a zero-size grid is a launch error
  if (n == 0) return out.zero_();
  const auto [scratch, scratch_p] = run_scratch(n, D, rows.options());
  launch_segment_sum_rows(rows.data_ptr(), r_bf16, perm.data_ptr<long>(),
                          seg.data_ptr<long>(), scratch_p, out.data_ptr(),
                          out_bf16, n, num, (int)D, cur_stream());
  return out;
}

// ---- hashed embedding tables (hash.hip) ----------------------------------

// The slot arrays of an index: equal length, a power of two >= 64.
long hash_slots(const torch::Tensor& slot_keys,
                const torch::Tensor& slot_rows) {
  TORCH_CHECK(i64_vec(slot_keys) && i64_vec(slot_rows) &&
              slot_keys.numel() == slot_rows.numel(),
              "hash: slot_keys and slot_rows must be contiguous i64 [H] on "
              "GPU");
  const long H = slot_keys.numel();
  TORCH_CHECK(H >= 64 && (H & (H - 1)) == 0,
              "hash: H must be a power of two >= 64");
  return H;
}

long hash_keys(const torch::Tensor& keys) {
  TORCH_CHECK(i64_vec(keys), "hash: keys must be contiguous i64 [n] on GPU");
  TORCH_CHECK(keys.numel() < (long)INT_MAX, "hash: n must be below 2^31");
  return keys.numel();
}

void hash_counters(const torch::Tensor& row_keys, const torch::Tensor& size,
                   long H) {
  TORCH_CHECK(i64_vec(row_keys) && i64_vec(size) && size.numel() == 1,
              "hash: row_keys [capacity] and size [1] must be contiguous i64 "
              "on GPU");
  TORCH_CHECK(row_keys.numel() >= 1 && 2 * row_keys.numel() <= H,
              "hash: need 1 <= capacity <= H / 2");
}

// rows [n]: the row of every key, -1 when absent. Read-only.
torch::Tensor hash_find(torch::Tensor slot_keys, torch::Tensor slot_rows,
                        torch::Tensor keys) {
  const long H = hash_slots(slot_keys, slot_rows), n = hash_keys(keys);
  auto rows = torch::empty({n}, keys.options());
  if (n == 0) return rows;   // a zero-size grid is a launch error
  launch_hash_find(keys.data_ptr<long>(), slot_keys.data_ptr<long>(),
                   slot_rows.data_ptr<long>(), rows.data_ptr<long>(), n, H,
                   cur_stream());
  return rows;
}

// An admission sketch in front of the insert: counters i32 [4, width] and
// filtered i64 [1] on the keys' GPU.
struct Admission {
  torch::Tensor counters, filtered;
  long admit_after;
};

// find_or_insert, behind a sketch when one is given (hash.hip). The scratch
// fill and the scan of the flags are plumbing; no host sync.
std::vector<torch::Tensor> find_or_insert(
    const torch::Tensor& slot_keys, const torch::Tensor& slot_rows,
    const torch::Tensor& row_keys, const torch::Tensor& size,
    const torch::Tensor& dropped, const torch::Tensor& keys,
    const Admission* admit) {
  const long H = hash_slots(slot_keys, slot_rows), n = hash_keys(keys);
  hash_counters(row_keys, size, H);
  TORCH_CHECK(i64_vec(dropped) && dropped.numel() == 1,
              "hash: dropped must be i64 [1] on GPU");
  auto opt = keys.options();
  auto rows = torch::empty({n}, opt);
  auto is_new = torch::empty({n}, opt.dtype(torch::kBool));
  if (n == 0) return {rows, is_new};
  long S = 64;
  while (S < 2 * n) S <<= 1;
  // [0] keys, [1] smallest position: both start at INT64_MIN
  auto scratch = torch::full({2, S}, (int64_t)LONG_MIN, opt);
  // [0:n] first occurrences of absent keys, [n:2n] those of them that pass
  auto flags = torch::empty({admit ? 2 * n : n}, opt.dtype(torch::kInt32));
  long* sk = scratch.data_ptr<long>();
  int* fresh = flags.data_ptr<int>();
  launch_hash_lookup(keys.data_ptr<long>(), slot_keys.data_ptr<long>(),
                     slot_rows.data_ptr<long>(), rows.data_ptr<long>(), sk,
                     sk + S, fresh, n, H, S, cur_stream());
  if (admit) {
    launch_hash_admit(keys.data_ptr<long>(), fresh,
                      admit->counters.data_ptr<int>(), fresh + n,
                      admit->filtered.data_ptr<long>(), n,
                      admit->counters.size(1), admit->admit_after,
                      cur_stream());
    fresh += n;
    flags = flags.narrow(0, n, n);
  }
  auto incl = torch::cumsum(flags, 0, torch::kInt64);
  launch_hash_insert(keys.data_ptr<long>(), fresh, incl.data_ptr<long>(),
                     slot_keys.data_ptr<long>(), slot_rows.data_ptr<long>(),
                     row_keys.data_ptr<long>(), size.data_ptr<long>(),
                     dropped.data_ptr<long>(), rows.data_ptr<long>(),
                     is_new.data_ptr<bool>(), n, H, row_keys.numel(),
                     cur_stream());
  return {rows, is_new};
}

// rows [n] and is_new bool [n]; absent keys get the rows size, size + 1, ..
// in order of first occurrence while they are below capacity (hash.hip).
std::vector<torch::Tensor> hash_find_or_insert(
    torch::Tensor slot_keys, torch::Tensor slot_rows, torch::Tensor row_keys,
    torch::Tensor size, torch::Tensor dropped, torch::Tensor keys) {
  return find_or_insert(slot_keys, slot_rows, row_keys, size, dropped, keys,
                        nullptr);
}

// find_or_insert behind a count-min admission sketch (hash.hip): an absent
// key is counted once per request in counters int32 [4, width] and gets a
// row only when its estimate has reached admit_after; the distinct keys
// that did not are added to filtered.
std::vector<torch::Tensor> hash_find_or_admit(
    torch::Tensor slot_keys, torch::Tensor slot_rows, torch::Tensor row_keys,
    torch::Tensor size, torch::Tensor dropped, torch::Tensor counters,
    torch::Tensor filtered, torch::Tensor keys, long admit_after) {
  TORCH_CHECK(i64_vec(filtered) && filtered.numel() == 1,
              "hash_find_or_admit: filtered must be i64 [1] on GPU");
  TORCH_CHECK(counters.is_cuda() && counters.scalar_type() == torch::kInt32 &&
              counters.dim() == 2 && counters.size(0) == 4 &&
              counters.is_contiguous() && counters.device() == keys.device(),
              "hash_find_or_admit: counters must be contiguous i32 "
              "[4, width] on the keys' GPU");
  const long width = counters.size(1);
  TORCH_CHECK(width >= 64 && (width & (width - 1)) == 0,
              "hash_find_or_admit: width must be a power of two >= 64");
  TORCH_CHECK(admit_after >= 1 && admit_after <= (1L << 30),
              "hash_find_or_admit: admit_after must lie in [1, 2^30]");
  const Admission admit = {counters, filtered, admit_after};
  return find_or_insert(slot_keys, slot_rows, row_keys, size, dropped, keys,
                        &admit);
}

// Clears the slot arrays and inserts row_keys[0:size] with their rows.
void hash_rebuild(torch::Tensor slot_keys, torch::Tensor slot_rows,
                  torch::Tensor row_keys, torch::Tensor size) {
  const long H = hash_slots(slot_keys, slot_rows);
  hash_counters(row_keys, size, H);
  slot_keys.fill_((int64_t)LONG_MIN);
  slot_rows.fill_(-1);
  launch_hash_rebuild(row_keys.data_ptr<long>(), size.data_ptr<long>(),
                      slot_keys.data_ptr<long>(), slot_rows.data_ptr<long>(),
                      H, row_keys.numel(), cur_stream());
}

// out [n,D] bf16: the table row of every key, zeros on a miss; one launch.
torch::Tensor hash_gather(torch::Tensor slot_keys, torch::Tensor slot_rows,
                          torch::Tensor table, torch::Tensor keys) {
  const long H = hash_slots(slot_keys, slot_rows), n = hash_keys(keys);
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous() &&
              table.scalar_type() == torch::kBFloat16,
              "hash_gather: table must be contiguous bf16 [V,D] on GPU");
  const long V = table.size(0), D = table.size(1);
  TORCH_CHECK(D <= (long)INT_MAX, "hash_gather: D too large");
  auto out = torch::empty({n, D}, table.options());
  if (n == 0 || D == 0) return out;
  launch_hash_gather(keys.data_ptr<long>(), slot_keys.data_ptr<long>(),
                     slot_rows.data_ptr<long>(),
                     (const bf16_t*)table.data_ptr(), (bf16_t*)out.data_ptr(),
                     n, H, V, (int)D, cur_stream());
  return out;
}

// The use stamps of a serving kernel: null / 0 for an empty tensor.
long* hash_stamps(const char* op, const torch::Tensor& last_used,
                  const torch::Tensor& keys, long& count) {
  count = last_used.numel();
  if (count == 0) return nullptr;
  TORCH_CHECK(i64_vec(last_used) && last_used.device() == keys.device(), op,
              ": last_used must be contiguous i64 [capacity] on the keys' "
              "GPU");
  return last_used.data_ptr<long>();
}

// hash_gather with the key's initial row (bf16) on a miss; a hit stores step
// into last_used[row] (numel 0: no stamps). One launch.
torch::Tensor hash_gather_init(torch::Tensor slot_keys,
                               torch::Tensor slot_rows, torch::Tensor table,
                               torch::Tensor keys, torch::Tensor last_used,
                               long step, long seed, long key_mul,
                               long key_add, double scale) {
  const long H = hash_slots(slot_keys, slot_rows), n = hash_keys(keys);
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous() &&
              table.scalar_type() == torch::kBFloat16,
              "hash_gather_init: table must be contiguous bf16 [V,D] on GPU");
  const long V = table.size(0), D = table.size(1);
  TORCH_CHECK(D <= (long)INT_MAX, "hash_gather_init: D too large");
  long stamps = 0;
  long* lu = hash_stamps("hash_gather_init", last_used, keys, stamps);
  auto out = torch::empty({n, D}, table.options());
  if (n == 0 || D == 0) return out;
  launch_hash_gather_init(keys.data_ptr<long>(), slot_keys.data_ptr<long>(),
                          slot_rows.data_ptr<long>(),
                          (const bf16_t*)table.data_ptr(),
                          (bf16_t*)out.data_ptr(), lu, n, H, V, (int)D,
                          stamps, step, seed, key_mul, key_add, (float)scale,
                          cur_stream());
  return out;
}

// Pooled pull by key (hash.hip): embedding_bag with the lookup fused in; with
// has_init a key without a row contributes its bf16 initial row. out bf16,
// or fp32 with out_f32.
torch::Tensor hash_embedding_bag(torch::Tensor slot_keys,
                                 torch::Tensor slot_rows, torch::Tensor table,
                                 torch::Tensor keys, torch::Tensor offsets,
                                 torch::Tensor weights, bool mean,
                                 bool out_f32, torch::Tensor last_used,
                                 long step, bool has_init, long seed,
                                 long key_mul, long key_add, double scale) {
  const long H = hash_slots(slot_keys, slot_rows);
  TORCH_CHECK(table.is_cuda() && table.dim() == 2 && table.is_contiguous() &&
              table.scalar_type() == torch::kBFloat16 && table.size(0) >= 1,
              "hash_embedding_bag: table must be contiguous bf16 [V,D], "
              "V >= 1, on GPU");
  const float* w = bag_args("hash_embedding_bag", keys, offsets, weights);
  const long n = hash_keys(keys), V = table.size(0);
  const long B = offsets.numel() - 1, D = table.size(1);
  TORCH_CHECK(D <= (long)INT_MAX, "hash_embedding_bag: D too large");
  long stamps = 0;
  long* lu = hash_stamps("hash_embedding_bag", last_used, keys, stamps);
  auto out = torch::empty({B, D}, table.options().dtype(
      out_f32 ? torch::kFloat32 : torch::kBFloat16));
  if (B == 0 || D == 0) return out;   // a zero-size grid is a launch error
  if (n == 0) return out.zero_();
  TORCH_CHECK(B * ((D + 255) / 256) / 4 < (long)INT_MAX,
              "hash_embedding_bag: B x D too large for one grid");
  launch_hash_embedding_bag(keys.data_ptr<long>(), slot_keys.data_ptr<long>(),
                            slot_rows.data_ptr<long>(),
                            (const bf16_t*)table.data_ptr(),
                            offsets.data_ptr<long>(), w, out.data_ptr(),
                            !out_f32, lu, B, n, H, V, (int)D, mean, stamps,
                            step, has_init, seed, key_mul, key_add,
                            (float)scale, cur_stream());
  return out;
}

// Initial master / shadow rows and zeroed state rows for the positions of
// a find_or_insert that allocated a row. states: 0, 1 or 2 fp32 [V,D].
void hash_init_new_rows(torch::Tensor keys, torch::Tensor rows,
                        torch::Tensor is_new, torch::Tensor master,
                        torch::Tensor shadow,
                        std::vector<torch::Tensor> states, long seed,
                        long key_mul, long key_add, double scale) {
  const long n = hash_keys(keys);
  TORCH_CHECK(i64_vec(rows) && rows.numel() == n && is_new.is_cuda() &&
              is_new.scalar_type() == torch::kBool && is_new.dim() == 1 &&
              is_new.is_contiguous() && is_new.numel() == n,
              "hash_init_new_rows: rows i64 [n] and is_new bool [n] must be "
              "contiguous on GPU");
  TORCH_CHECK(master.is_cuda() && master.dim() == 2 &&
              master.is_contiguous() &&
              master.scalar_type() == torch::kFloat32,
              "hash_init_new_rows: master must be contiguous fp32 [V,D] on "
              "GPU");
  TORCH_CHECK(shadow.is_cuda() && shadow.is_contiguous() &&
              shadow.scalar_type() == torch::kBFloat16 &&
              shadow.sizes() == master.sizes(),
              "hash_init_new_rows: shadow must be contiguous bf16 [V,D]");
  TORCH_CHECK(states.size() <= 2, "hash_init_new_rows: at most 2 states");
  float* sp[2] = {nullptr, nullptr};
  for (size_t k = 0; k < states.size(); ++k) {
    const auto& s = states[k];
    TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                s.scalar_type() == torch::kFloat32 &&
                s.sizes() == master.sizes(),
                "hash_init_new_rows: states must be contiguous fp32 [V,D]");
    sp[k] = s.data_ptr<float>();
  }
  const long V = master.size(0), D = master.size(1);
  const long tiles = (D + 255) / 256;
  TORCH_CHECK(D <= (long)INT_MAX && n * tiles / 4 < (long)INT_MAX,
              "hash_init_new_rows: too large for one grid");
  if (n == 0 || D == 0 || V == 0) return;
  launch_hash_init_rows(keys.data_ptr<long>(), rows.data_ptr<long>(),
                        is_new.data_ptr<bool>(), master.data_ptr<float>(),
                        (bf16_t*)shadow.data_ptr(), sp[0], sp[1], n, V,
                        (int)D, seed, key_mul, key_add, (float)scale,
                        cur_stream());
}

// last_used[rows[i]] = step for every rows[i] in [0, capacity).
void hash_touch(torch::Tensor rows, torch::Tensor last_used, long step) {
  const long n = hash_keys(rows);
  TORCH_CHECK(i64_vec(last_used) && last_used.device() == rows.device(),
              "hash_touch: last_used must be contiguous i64 [capacity] on "
              "the rows' GPU");
  if (n == 0 || last_used.numel() == 0) return;
  launch_hash_touch(rows.data_ptr<long>(), last_used.data_ptr<long>(), n,
                    last_used.numel(), step, cur_stream());
}

// Compaction by hole filling (hash.hip): the rows of [0, size) with keep set
// become rows [0, K) in every tensor of tables, in row_keys and in last_used
// (numel 0: none); then the slot arrays are rebuilt. The scan of the flags
// and the slot clear are plumbing; no host sync.
void hash_compact(torch::Tensor slot_keys, torch::Tensor slot_rows,
                  torch::Tensor row_keys, torch::Tensor size,
                  torch::Tensor evicted, torch::Tensor keep,
                  std::vector<torch::Tensor> tables,
                  torch::Tensor last_used) {
  const long H = hash_slots(slot_keys, slot_rows);
  hash_counters(row_keys, size, H);
  const long capacity = row_keys.numel();
  const auto dev = row_keys.device();
  TORCH_CHECK(i64_vec(evicted) && evicted.numel() == 1 &&
              evicted.device() == dev && size.device() == dev &&
              slot_keys.device() == dev && slot_rows.device() == dev,
              "hash_compact: evicted must be i64 [1] on the index's GPU");
  TORCH_CHECK(keep.is_cuda() && keep.device() == dev &&
              keep.scalar_type() == torch::kBool && keep.dim() == 1 &&
              keep.is_contiguous() && keep.numel() == capacity,
              "hash_compact: keep must be contiguous bool [capacity] = [",
              capacity, "] on the index's GPU");
  TORCH_CHECK(tables.size() <= 4, "hash_compact: at most 4 row tensors");
  void* bases[4] = {nullptr, nullptr, nullptr, nullptr};
  int row_bytes[4] = {0, 0, 0, 0}, elem_bytes[4] = {0, 0, 0, 0};
  int count = 0;
  for (const auto& t : tables) {
    const bool f32 = t.scalar_type() == torch::kFloat32;
    TORCH_CHECK(t.is_cuda() && t.device() == dev && t.dim() == 2 &&
                t.is_contiguous() && t.size(0) == capacity &&
                (f32 || t.scalar_type() == torch::kBFloat16),
                "hash_compact: every row tensor must be contiguous fp32 or "
                "bf16 [capacity, D] on the index's GPU");
    TORCH_CHECK(t.size(1) == tables[0].size(1),
                "hash_compact: the row tensors must share one width D");
    const long bytes = t.size(1) * (f32 ? 4 : 2);
    TORCH_CHECK(bytes <= (long)INT_MAX, "hash_compact: D too large");
    if (bytes == 0) continue;
    bases[count] = t.data_ptr();
    row_bytes[count] = (int)bytes;
    elem_bytes[count] = f32 ? 4 : 2;
    ++count;
  }
  long* stamps = nullptr;
  if (last_used.numel() != 0) {
    TORCH_CHECK(i64_vec(last_used) && last_used.device() == dev &&
                last_used.numel() == capacity,
                "hash_compact: last_used must be contiguous i64 [capacity] "
                "on the index's GPU");
    stamps = last_used.data_ptr<long>();
  }
  auto opt = row_keys.options();
  auto flags = torch::empty({capacity}, opt.dtype(torch::kInt32));
  auto old_size = torch::empty({1}, opt);
  auto plan = torch::empty({2, capacity}, opt);   // [0] holes, [1] movers
  launch_hash_compact_flags(keep.data_ptr<bool>(), size.data_ptr<long>(),
                            flags.data_ptr<int>(), old_size.data_ptr<long>(),
                            capacity, cur_stream());
  auto incl = torch::cumsum(flags, 0, torch::kInt64);
  long* pp = plan.data_ptr<long>();
  launch_hash_compact_move(flags.data_ptr<int>(), incl.data_ptr<long>(),
                           old_size.data_ptr<long>(), pp, pp + capacity,
                           bases, row_bytes, elem_bytes, count,
                           row_keys.data_ptr<long>(), stamps,
                           size.data_ptr<long>(), evicted.data_ptr<long>(),
                           capacity, cur_stream());
  slot_keys.fill_((int64_t)LONG_MIN);
  slot_rows.fill_(-1);
  launch_hash_rebuild(row_keys.data_ptr<long>(), size.data_ptr<long>(),
                      slot_keys.data_ptr<long>(), slot_rows.data_ptr<long>(),
                      H, capacity, cur_stream());
}

}  // namespace

void bind_sparse(pybind11::module_& m) {
  m.def("embedding_gather", &embedding_gather);
  m.def("embedding_scatter_add", &embedding_scatter_add);
  m.def("sparse_apply", &sparse_apply,
        "fused sparse SGD/momentum/Adagrad/Adam/FTRL-Proximal apply + bf16 "
        "shadow",
        py::arg("table"), py::arg("ids"), py::arg("grads"),
        py::arg("state1"), py::arg("state2"), py::arg("bf16_out"),
        py::arg("opt"), py::arg("step"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("grad_scale"), py::arg("l1") = 0.0, py::arg("l2") = 0.0,
        py::arg("initial_accumulator_value") = 0.1);
  m.def("embedding_bag", &embedding_bag,
        "pooled (bag) embedding pull: sum / mean, optional weights",
        py::arg("table"), py::arg("ids"), py::arg("offsets"),
        py::arg("weights"), py::arg("mean"), py::arg("out_f32"));
  m.def("sparse_apply_bag", &sparse_apply_bag,
        "sparse_apply fed [B,D] bag gradients (pooled push)",
        py::arg("table"), py::arg("ids"), py::arg("offsets"),
        py::arg("weights"), py::arg("grads"), py::arg("state1"),
        py::arg("state2"), py::arg("bf16_out"), py::arg("opt"),
        py::arg("step"), py::arg("mean"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("grad_scale"), py::arg("l1") = 0.0, py::arg("l2") = 0.0,
        py::arg("initial_accumulator_value") = 0.1);
  m.def("shard_partition", &shard_partition,
        "stable partition of ids by owning shard: local, perm, inv, starts",
        py::arg("ids"), py::arg("rows"), py::arg("num_shards"),
        py::arg("div"));
  m.def("permute_rows", &permute_rows, "out[j] = cast(rows[perm[j]])",
        py::arg("rows"), py::arg("perm"), py::arg("out_bf16"));
  m.def("shard_bag_offsets", &shard_bag_offsets,
        "per-shard CSR offsets [S,B+1] of a partitioned bagged request",
        py::arg("perm"), py::arg("starts"), py::arg("offsets"));
  m.def("bag_coefficients", &bag_coefficients,
        "per-position bag coefficients c [n]",
        py::arg("n"), py::arg("offsets"), py::arg("weights"),
        py::arg("mean"));
  m.def("coalesce_ids", &coalesce_ids,
        "distinct ids of a request: uniq, inverse, perm, seg, count",
        py::arg("ids"));
  m.def("segment_sum_rows", &segment_sum_rows,
        "out[k] = sum of rows[perm[seg[k]:seg[k+1]]], rounded once",
        py::arg("rows"), py::arg("perm"), py::arg("seg"), py::arg("num"),
        py::arg("out_bf16"));
  m.def("hash_find", &hash_find, "rows of int64 keys, -1 when absent",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("keys"));
  m.def("hash_find_or_insert", &hash_find_or_insert,
        "rows of int64 keys, absent keys get the next free rows: rows, is_new",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("row_keys"),
        py::arg("size"), py::arg("dropped"), py::arg("keys"));
  m.def("hash_find_or_admit", &hash_find_or_admit,
        "find_or_insert behind a count-min admission sketch: rows, is_new",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("row_keys"),
        py::arg("size"), py::arg("dropped"), py::arg("counters"),
        py::arg("filtered"), py::arg("keys"), py::arg("admit_after"));
  m.def("hash_gather_init", &hash_gather_init,
        "bf16 table rows of int64 keys, the initial row when absent",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("table"),
        py::arg("keys"), py::arg("last_used"), py::arg("step"),
        py::arg("seed"), py::arg("key_mul"), py::arg("key_add"),
        py::arg("scale"));
  m.def("hash_embedding_bag", &hash_embedding_bag,
        "pooled pull by int64 key, optional initial rows for absent keys",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("table"),
        py::arg("keys"), py::arg("offsets"), py::arg("weights"),
        py::arg("mean"), py::arg("out_f32"), py::arg("last_used"),
        py::arg("step"), py::arg("has_init"), py::arg("seed"),
        py::arg("key_mul"), py::arg("key_add"), py::arg("scale"));
  m.def("hash_rebuild", &hash_rebuild,
        "clear the slots and insert row_keys[0:size]",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("row_keys"),
        py::arg("size"));
  m.def("hash_gather", &hash_gather,
        "bf16 table rows of int64 keys, zeros when absent",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("table"),
        py::arg("keys"));
  m.def("hash_init_new_rows", &hash_init_new_rows,
        "initial master/shadow/state rows of newly allocated rows",
        py::arg("keys"), py::arg("rows"), py::arg("is_new"),
        py::arg("master"), py::arg("shadow"), py::arg("states"),
        py::arg("seed"), py::arg("key_mul"), py::arg("key_add"),
        py::arg("scale"));
  m.def("hash_touch", &hash_touch, "last_used[rows] = step",
        py::arg("rows"), py::arg("last_used"), py::arg("step"));
  m.def("hash_compact", &hash_compact,
        "keep the flagged rows, dense again, in every row tensor; rebuild",
        py::arg("slot_keys"), py::arg("slot_rows"), py::arg("row_keys"),
        py::arg("size"), py::arg("evicted"), py::arg("keep"),
        py::arg("tables"), py::arg("last_used"));
}

// Helpers shared by the binding translation units (ext.hip, ext_sparse.hip).
#pragma once

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <tuple>
#include <utility>

#include "common.h"

// The sparse bindings (ext_sparse.hip), added to the one module of ext.hip.
void bind_sparse(pybind11::module_& m);

inline hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

inline const void* grad_ptr(const torch::Tensor& g, bool* is_bf16) {
  TORCH_CHECK(g.is_contiguous(), "grad must be contiguous");
  if (g.scalar_type() == torch::kBFloat16) {
    *is_bf16 = true;
    return g.data_ptr();
  }
  TORCH_CHECK(g.scalar_type() == torch::kFloat32, "grad must be fp32 or bf16");
  *is_bf16 = false;
  return g.data_ptr();
}

inline float* opt_f32(torch::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  TORCH_CHECK(t.numel() == n && t.scalar_type() == torch::kFloat32,
              name, " must be fp32 with same numel as param");
  return t.data_ptr<float>();
}

inline bf16_t* opt_bf16(torch::Tensor& t, long n, const char* name) {
  if (t.numel() == 0) return nullptr;
  TORCH_CHECK(t.numel() == n && t.scalar_type() == torch::kBFloat16,
              name, " must be bf16 with same numel as param");
  return (bf16_t*)t.data_ptr();
}

// A contiguous int64 vector on the GPU.
inline bool i64_vec(const torch::Tensor& t) {
  return t.is_cuda() && t.scalar_type() == torch::kInt64 && t.dim() == 1 &&
         t.is_contiguous();
}

// The stable sort of the ids and its permutation: the inverted index of a
// request (plumbing; it stays on the device, no host sync).
inline std::pair<torch::Tensor, torch::Tensor> stable_sort_ids(
    const torch::Tensor& ids) {
  auto st = torch::sort(ids, /*stable=*/true, /*dim=*/0,
                        /*descending=*/false);
  return {std::get<0>(st), std::get<1>(st)};
}

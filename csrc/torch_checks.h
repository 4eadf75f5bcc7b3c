// The check vocabulary of the PyTorch bindings: csrc/bindings.cpp and every csrc/*/bindings.cpp.
//
// Every entry point validates device, dtype, contiguity, shape and range on the host BEFORE
// launching (a bad shape must never reach a kernel: an out-of-bounds access can reset the whole
// node), names the offending argument by its Python keyword name at the start of the message, and
// launches on the current HIP stream of its anchor tensor's device under a device guard.  Every
// tensor whose pointer goes to a launcher passes through one of the checks below, so an entry point
// reads as the list of what it requires.  `a` is the entry point's anchor: the tensor given to
// DeviceGuard and cur_stream (checked against itself); `name` is the argument's keyword name.
#pragma once
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

namespace vwa::checks {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

// torch-ROCm exposes GPUs as device type "cuda"; the masquerading accessor returns the stream
// torch itself launches on (including the capture stream inside torch.cuda.graph).
inline hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}
inline bool aligned(const Tensor& t, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & (bytes - 1)) == 0;
}
// byte ranges [p, p + n) and [q, q + m)
inline bool overlaps(const void* p, int64_t n, const void* q, int64_t m) {
  const char* a = static_cast<const char*>(p);
  const char* b = static_cast<const char*>(q);
  return a < b + m && b < a + n;
}

inline void check_anchor(const Tensor& a, const char* name) { TORCH_CHECK(a.is_cuda(), name, " must be a GPU tensor"); }
// GPU tensor: on the anchor's device, with the dtype the kernel reads
inline void check_gpu(const Tensor& t, const Tensor& a, at::ScalarType dt, const char* name) {
  check_anchor(t, name);
  TORCH_CHECK(t.device() == a.device(), name, " must be on ", a.device(), " (the device this call launches on), not ",
              t.device());
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", not ", t.scalar_type());
}
// Vector: contiguous GPU tensor of >= n (exact: == n) elements, of any shape ...
inline void check_vec(const Tensor& t, const Tensor& a, at::ScalarType dt, int64_t n, const char* name,
                      bool exact = false) {
  check_gpu(t, a, dt, name);
  TORCH_CHECK(t.is_contiguous() && (exact ? t.numel() == n : t.numel() >= n), name, " must be contiguous with ",
              exact ? "" : ">= ", n, " elements, not ", t.sizes());
}
// ... or 1-D only (n = 0: any length, for a vector whose length sets the call's row count)
inline void check_vec_1d(const Tensor& t, const Tensor& a, at::ScalarType dt, int64_t n, const char* name,
                         bool exact = false) {
  check_gpu(t, a, dt, name);
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous() && (exact ? t.numel() == n : t.numel() >= n), name,
              " must be contiguous 1-D with ", exact ? "" : ">= ", n, " elements, not ", t.sizes());
}
// Matrix: 2-D [>= rows, >= cols] with unit inner stride and rows that do not overlap (the kernels
// take a row stride).  rows = cols = 0: any size, for a matrix the entry point measures itself.
inline void check_mat(const Tensor& t, const Tensor& a, at::ScalarType dt, int64_t rows, int64_t cols,
                      const char* name) {
  check_gpu(t, a, dt, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) >= t.size(1), name, " must be 2-D with contiguous rows");
  TORCH_CHECK(t.size(0) >= rows && t.size(1) >= cols, name, " must be [>= ", rows, ", >= ", cols, "], not ",
              t.sizes());
}
// The sampler's packed allow-mask: int32 [1 or rows, >= ceil(vocab / 32)] with unit inner stride.
// Returns the row stride for the launcher: 0 for one shared row.  exact_rows: a mask of more than
// one row has exactly `rows` (else at least `rows`); expanded_ok: its rows may also be one row
// expanded (stride 0) -- otherwise they must not overlap.
inline int64_t check_mask(const Tensor& m, const Tensor& a, int64_t rows, int64_t vocab, bool exact_rows,
                          bool expanded_ok, const char* name = "mask") {
  check_gpu(m, a, at::kInt, name);
  const int64_t words = (vocab + 31) / 32;
  TORCH_CHECK(m.dim() == 2 && m.stride(1) == 1 && m.size(1) >= words &&
                  (m.size(0) == 1 || (exact_rows ? m.size(0) == rows : m.size(0) >= rows)),
              name, " must be [1 or ", exact_rows ? "" : ">= ", rows, ", >= ", words, " (vocab = ", vocab,
              " bits)] with contiguous rows, not ", m.sizes());
  if (m.size(0) == 1) return 0;
  TORCH_CHECK(m.stride(0) >= m.size(1) || (expanded_ok && m.stride(0) == 0), name, " rows must not overlap");
  return m.stride(0);
}
inline void check_rc(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " launch failed with code ", rc); }

}  // namespace vwa::checks

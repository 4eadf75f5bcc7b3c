// PyTorch bindings of the keyterm boosting library (_vwa_boost.so).
//
// Same rules as csrc/bindings.cpp and the align / sot / beam bindings: the entry point validates
// device, dtype, contiguity, shape and range on the host BEFORE launching (a bad shape must never
// reach a kernel), names the offending argument, and launches on the current HIP stream of the
// anchor tensor's device under a device guard.  The few checks needed are a copy of those files'
// vocabulary.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include "boost/boost.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<Tensor>;

hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}
// GPU tensor: on the anchor's device, with the dtype the kernel reads
void check_gpu(const Tensor& t, const Tensor& a, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.device() == a.device(), name, " must be on ", a.device(), " (the device this call launches on), not ",
              t.device());
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", not ", t.scalar_type());
}
// Vector: contiguous 1-D GPU tensor of exactly / at least n elements
void check_vec(const Tensor& t, const Tensor& a, at::ScalarType dt, int64_t n, bool exact, const char* name) {
  check_gpu(t, a, dt, name);
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous() && (exact ? t.numel() == n : t.numel() >= n), name,
              " must be contiguous 1-D with ", exact ? "" : ">= ", n, " elements, not ", t.sizes());
}
void check_rc(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " launch failed with code ", rc); }

bool overlaps(const Tensor& a, const Tensor& b, int64_t n) {
  const int* pa = a.data_ptr<int>();
  const int* pb = b.data_ptr<int>();
  return pa < pb + n && pb < pa + n;
}

void boost_step(const Tensor& logits, int64_t vocab, const Tensor& edge_off, const Tensor& edge_tok,
                const Tensor& edge_next, const Tensor& edge_bias, const Tensor& state_root, const Tensor& roots,
                const Tensor& state_in, const Tensor& state_out, const OptTensor& tokens, const OptTensor& parents,
                int64_t W) {
  check_gpu(logits, logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) >= logits.size(1),
              "logits must be 2-D with contiguous rows");
  check_gpu(roots, logits, at::kInt, "roots");
  TORCH_CHECK(roots.dim() == 1 && roots.is_contiguous(), "roots must be contiguous 1-D, not ", roots.sizes());
  const int64_t rows = roots.numel();
  TORCH_CHECK(rows >= 1 && rows <= kBoostMaxRows, "roots: rows must be in [1, ", kBoostMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per root), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kBoostMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kBoostMaxVocab, ")], not ", vocab);
  check_gpu(state_root, logits, at::kInt, "state_root");
  TORCH_CHECK(state_root.dim() == 1 && state_root.is_contiguous(), "state_root must be contiguous 1-D");
  const int64_t S = state_root.numel();
  TORCH_CHECK(S >= 1 && S <= kBoostMaxStates, "state_root: states must be in [1, ", kBoostMaxStates, "], not ", S);
  check_vec(edge_off, logits, at::kInt, S + 1, true, "edge_off");
  check_gpu(edge_tok, logits, at::kInt, "edge_tok");
  TORCH_CHECK(edge_tok.dim() == 1 && edge_tok.is_contiguous(), "edge_tok must be contiguous 1-D");
  const int64_t E = edge_tok.numel();
  TORCH_CHECK(E >= 1 && E <= kBoostMaxEdges, "edge_tok: edges must be in [1, ", kBoostMaxEdges, "], not ", E);
  check_vec(edge_next, logits, at::kInt, E, true, "edge_next");
  check_vec(edge_bias, logits, at::kFloat, E, true, "edge_bias");
  check_vec(state_in, logits, at::kInt, rows, false, "state_in");
  check_vec(state_out, logits, at::kInt, rows, false, "state_out");
  if (tokens.has_value()) check_vec(*tokens, logits, at::kInt, rows, false, "tokens");
  if (parents.has_value()) {
    check_vec(*parents, logits, at::kInt, rows, false, "parents");
    TORCH_CHECK(W >= 1 && W <= rows && rows % W == 0, "W: ", rows, " rows are not groups of W = ", W);
    TORCH_CHECK(!overlaps(state_in, state_out, rows), "state_out must not overlap state_in when parents are given");
  } else {
    TORCH_CHECK(state_in.data_ptr<int>() == state_out.data_ptr<int>() || !overlaps(state_in, state_out, rows),
                "state_out must be state_in itself or not overlap it");
  }
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_boost_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, edge_off.data_ptr<int>(),
                          edge_tok.data_ptr<int>(), edge_next.data_ptr<int>(), edge_bias.data_ptr<float>(),
                          state_root.data_ptr<int>(), (int)S, (int)E, roots.data_ptr<int>(), state_in.data_ptr<int>(),
                          state_out.data_ptr<int>(), tokens.has_value() ? tokens->data_ptr<int>() : nullptr,
                          parents.has_value() ? parents->data_ptr<int>() : nullptr, parents.has_value() ? (int)W : 1,
                          cur_stream(logits)),
           "boost_step");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 keyterm boosting: one launch per decode step moving the rows' keyterm automata and biasing their logits";
  m.attr("MAX_ROWS") = kBoostMaxRows;
  m.attr("MAX_STATES") = kBoostMaxStates;
  m.attr("MAX_EDGES") = kBoostMaxEdges;
  m.attr("MAX_VOCAB") = kBoostMaxVocab;
  m.def("boost_step", &boost_step, py::arg("logits"), py::arg("vocab"), py::arg("edge_off"), py::arg("edge_tok"),
        py::arg("edge_next"), py::arg("edge_bias"), py::arg("state_root"), py::arg("roots"), py::arg("state_in"),
        py::arg("state_out"), py::arg("tokens"), py::arg("parents"), py::arg("W"));
}

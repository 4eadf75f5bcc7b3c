// PyTorch bindings of the timestamp rules library (_vwa_tsrules.so).
//
// Same rules as csrc/bindings.cpp and the align / sot / beam / boost bindings: the entry point
// validates device, dtype, contiguity, shape and range on the host BEFORE launching (a bad shape must
// never reach a kernel), names the offending argument, and launches on the current HIP stream of the
// anchor tensor's device under a device guard.  The few checks needed are a copy of those files'
// vocabulary.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include "tsrules/tsrules.h"

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
// State: contiguous [>= rows, 4] int32
void check_state(const Tensor& t, const Tensor& a, int64_t rows, const char* name) {
  check_gpu(t, a, at::kInt, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 4 && t.is_contiguous() && t.size(0) >= rows, name,
              " must be contiguous [>= ", rows, ", 4], not ", t.sizes());
}
void check_rc(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " launch failed with code ", rc); }

void ts_rules_step(const Tensor& logits, int64_t vocab, int64_t eot, int64_t ts_begin, int64_t max_initial,
                   const Tensor& mask, const Tensor& enable, const Tensor& state_in, const Tensor& state_out,
                   const OptTensor& tokens) {
  check_gpu(logits, logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) >= logits.size(1),
              "logits must be 2-D with contiguous rows");
  check_gpu(enable, logits, at::kInt, "enable");
  TORCH_CHECK(enable.dim() == 1 && enable.is_contiguous(), "enable must be contiguous 1-D, not ", enable.sizes());
  const int64_t rows = enable.numel();
  TORCH_CHECK(rows >= 1 && rows <= kTsMaxRows, "enable: rows must be in [1, ", kTsMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per enable), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kTsMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kTsMaxVocab, ")], not ", vocab);
  TORCH_CHECK(eot >= 0 && eot < ts_begin, "eot must be in [0, ts_begin = ", ts_begin, "), not ", eot);
  TORCH_CHECK(ts_begin < vocab, "ts_begin must be below vocab = ", vocab, ", not ", ts_begin);
  TORCH_CHECK(max_initial >= INT32_MIN && max_initial <= INT32_MAX, "max_initial must fit int32, not ", max_initial);
  check_gpu(mask, logits, at::kInt, "mask");
  const int64_t words = (vocab + 31) / 32;
  TORCH_CHECK(mask.dim() == 2 && mask.stride(1) == 1 && mask.size(1) >= words &&
                  (mask.size(0) == 1 || (mask.size(0) >= rows && mask.stride(0) >= mask.size(1))),
              "mask must be [1 or >= ", rows, ", >= ", words, "] with contiguous rows, not ", mask.sizes());
  check_state(state_in, logits, rows, "state_in");
  check_state(state_out, logits, rows, "state_out");
  if (tokens.has_value()) {
    check_gpu(*tokens, logits, at::kInt, "tokens");
    TORCH_CHECK(tokens->dim() == 1 && tokens->is_contiguous() && tokens->numel() >= rows,
                "tokens must be contiguous 1-D with >= ", rows, " elements, not ", tokens->sizes());
  }
  const int* pi = state_in.data_ptr<int>();
  const int* po = state_out.data_ptr<int>();
  TORCH_CHECK(pi == po || !(pi < po + 4 * rows && po < pi + 4 * rows),
              "state_out must be state_in itself or not overlap it");
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_ts_rules_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, (int)eot, (int)ts_begin,
                             (int)max_initial, mask.data_ptr<int>(), mask.size(0) == 1 ? 0 : mask.stride(0),
                             enable.data_ptr<int>(), pi, state_out.data_ptr<int>(),
                             tokens.has_value() ? tokens->data_ptr<int>() : nullptr, cur_stream(logits)),
           "ts_rules_step");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 Whisper timestamp rules: one launch per decode step moving the rows' states and banning logits";
  m.attr("MAX_ROWS") = kTsMaxRows;
  m.attr("MAX_VOCAB") = kTsMaxVocab;
  m.def("ts_rules_step", &ts_rules_step, py::arg("logits"), py::arg("vocab"), py::arg("eot"), py::arg("ts_begin"),
        py::arg("max_initial"), py::arg("mask"), py::arg("enable"), py::arg("state_in"), py::arg("state_out"),
        py::arg("tokens"));
}

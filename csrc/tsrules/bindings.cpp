// PyTorch bindings of the timestamp rules library (_vwa_tsrules.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "tsrules/tsrules.h"

namespace {

using namespace vwa::checks;

// State: contiguous [>= rows, 4] int32
void check_state(const Tensor& t, const Tensor& a, int64_t rows, const char* name) {
  check_gpu(t, a, at::kInt, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 4 && t.is_contiguous() && t.size(0) >= rows, name,
              " must be contiguous [>= ", rows, ", 4], not ", t.sizes());
}

void ts_rules_step(const Tensor& logits, int64_t vocab, int64_t eot, int64_t ts_begin, int64_t max_initial,
                   const Tensor& mask, const Tensor& enable, const Tensor& state_in, const Tensor& state_out,
                   const OptTensor& tokens) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  check_vec_1d(enable, logits, at::kInt, 0, "enable");
  const int64_t rows = enable.numel();
  TORCH_CHECK(rows >= 1 && rows <= kTsMaxRows, "enable: rows must be in [1, ", kTsMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per enable), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kTsMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kTsMaxVocab, ")], not ", vocab);
  TORCH_CHECK(eot >= 0 && eot < ts_begin, "eot must be in [0, ts_begin = ", ts_begin, "), not ", eot);
  TORCH_CHECK(ts_begin < vocab, "ts_begin must be below vocab = ", vocab, ", not ", ts_begin);
  TORCH_CHECK(max_initial >= INT32_MIN && max_initial <= INT32_MAX, "max_initial must fit int32, not ", max_initial);
  const int64_t mask_stride = check_mask(mask, logits, rows, vocab, false, false);
  check_state(state_in, logits, rows, "state_in");
  check_state(state_out, logits, rows, "state_out");
  if (tokens.has_value()) check_vec_1d(*tokens, logits, at::kInt, rows, "tokens");
  const int* pi = state_in.data_ptr<int>();
  const int* po = state_out.data_ptr<int>();
  TORCH_CHECK(pi == po || !overlaps(pi, 16 * rows, po, 16 * rows),
              "state_out must be state_in itself or not overlap it");
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_ts_rules_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, (int)eot, (int)ts_begin,
                             (int)max_initial, mask.data_ptr<int>(), mask_stride,
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

// PyTorch bindings of the set log-probability library (_vwa_turn.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "turn/turn.h"

namespace {

using namespace vwa::checks;

void set_logprob(const Tensor& logits, int64_t vocab, const Tensor& set, const Tensor& out) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  check_gpu(out, logits, at::kFloat, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 2 && out.is_contiguous(), "out must be contiguous [rows, 2], not ",
              out.sizes());
  const int64_t rows = out.size(0);
  TORCH_CHECK(rows >= 1 && rows <= kTurnMaxRows, "out: rows must be in [1, ", kTurnMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per row of out), not ",
              logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kTurnMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kTurnMaxVocab, ")], not ", vocab);
  const int64_t set_stride = check_mask(set, logits, rows, vocab, false, false, "set");
  const int64_t words = (vocab + 31) / 32;
  TORCH_CHECK(!overlaps(out.data_ptr(), 8 * rows, logits.data_ptr(), 4 * ((rows - 1) * logits.stride(0) + vocab)),
              "out must not overlap logits");
  TORCH_CHECK(!overlaps(out.data_ptr(), 8 * rows, set.data_ptr(), 4 * ((rows - 1) * set_stride + words)),
              "out must not overlap set");
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_set_logprob(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, set.data_ptr<int>(),
                           set_stride, out.data_ptr<float>(), cur_stream(logits)),
           "set_logprob");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 set log-probability: per logits row, the log of the softmax mass on a packed set of ids";
  m.attr("MAX_ROWS") = kTurnMaxRows;
  m.attr("MAX_VOCAB") = kTurnMaxVocab;
  m.def("set_logprob", &set_logprob, py::arg("logits"), py::arg("vocab"), py::arg("set"), py::arg("out"));
}

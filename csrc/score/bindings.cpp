// PyTorch bindings of the transcript score library (_vwa_score.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "score/score.h"

namespace {

using namespace vwa::checks;

// Counts: contiguous [>= rows, 2] int32
void check_cnt(const Tensor& t, const Tensor& a, int64_t rows, const char* name) {
  check_gpu(t, a, at::kInt, name);
  TORCH_CHECK(t.dim() == 2 && t.size(1) == 2 && t.is_contiguous() && t.size(0) >= rows, name,
              " must be contiguous [>= ", rows, ", 2], not ", t.sizes());
}

void score_step(const Tensor& logits, int64_t vocab, int64_t eot, const Tensor& mask, const Tensor& enable,
                const Tensor& tokens, const Tensor& sum_in, const Tensor& sum_out, const Tensor& cnt_in,
                const Tensor& cnt_out, const OptTensor& step_lp) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  check_vec_1d(enable, logits, at::kInt, 0, "enable");
  const int64_t rows = enable.numel();
  TORCH_CHECK(rows >= 1 && rows <= kScoreMaxRows, "enable: rows must be in [1, ", kScoreMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per enable), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kScoreMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kScoreMaxVocab, ")], not ", vocab);
  TORCH_CHECK(eot >= 0 && eot < vocab, "eot must be in [0, vocab = ", vocab, "), not ", eot);
  const int64_t mask_stride = check_mask(mask, logits, rows, vocab, false, false);
  check_vec_1d(tokens, logits, at::kInt, rows, "tokens");
  check_vec_1d(sum_in, logits, at::kFloat, rows, "sum_in");
  check_vec_1d(sum_out, logits, at::kFloat, rows, "sum_out");
  check_cnt(cnt_in, logits, rows, "cnt_in");
  check_cnt(cnt_out, logits, rows, "cnt_out");
  if (step_lp.has_value()) check_vec_1d(*step_lp, logits, at::kFloat, rows, "step_lp");
  // the in-place pairs may coincide exactly; nothing else among the state tensors and step_lp may overlap
  struct Span { const char* name; const char* p; int64_t n; };
  const Span sp[5] = {{"sum_in", (const char*)sum_in.data_ptr(), 4 * rows},
                      {"sum_out", (const char*)sum_out.data_ptr(), 4 * rows},
                      {"cnt_in", (const char*)cnt_in.data_ptr(), 8 * rows},
                      {"cnt_out", (const char*)cnt_out.data_ptr(), 8 * rows},
                      {"step_lp", step_lp.has_value() ? (const char*)step_lp->data_ptr() : nullptr, 4 * rows}};
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j) {
      if (!sp[i].p || !sp[j].p) continue;
      if (sp[i].p == sp[j].p && ((i == 0 && j == 1) || (i == 2 && j == 3))) continue;
      TORCH_CHECK(!overlaps(sp[i].p, sp[i].n, sp[j].p, sp[j].n), sp[j].name, " must not overlap ",
                  sp[i].name, " (sum_out may be sum_in itself and cnt_out may be cnt_in itself, nothing else)");
    }
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_score_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, (int)eot,
                          mask.data_ptr<int>(), mask_stride, enable.data_ptr<int>(),
                          tokens.data_ptr<int>(), sum_in.data_ptr<float>(), sum_out.data_ptr<float>(),
                          cnt_in.data_ptr<int>(), cnt_out.data_ptr<int>(),
                          step_lp.has_value() ? step_lp->data_ptr<float>() : nullptr, cur_stream(logits)),
           "score_step");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 transcript scores: one launch per decode step adding the sampled tokens' log-probabilities";
  m.attr("MAX_ROWS") = kScoreMaxRows;
  m.attr("MAX_VOCAB") = kScoreMaxVocab;
  m.def("score_step", &score_step, py::arg("logits"), py::arg("vocab"), py::arg("eot"), py::arg("mask"),
        py::arg("enable"), py::arg("tokens"), py::arg("sum_in"), py::arg("sum_out"), py::arg("cnt_in"),
        py::arg("cnt_out"), py::arg("step_lp"));
}

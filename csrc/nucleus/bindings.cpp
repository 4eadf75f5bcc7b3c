// PyTorch bindings of the nucleus step library (_vwa_nucleus.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "nucleus/nucleus.h"

namespace {

using namespace vwa::checks;

struct Range {
  const void* p;
  int64_t bytes;
  const char* name;
};

// logits is the anchor; its row count is the call's
void nucleus_step(const Tensor& logits, int64_t vocab, const OptTensor& mask_in, const Tensor& mask_out,
                  const Tensor& n_kept, const Tensor& temperature, const Tensor& top_p, const Tensor& top_k,
                  const Tensor& penalty, const Tensor& history) {
  check_mat(logits, logits, at::kFloat, 1, 1, "logits");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(rows <= kNucleusMaxRows, "logits: rows must be in [1, ", kNucleusMaxRows, "], not ", rows);
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kNucleusMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kNucleusMaxVocab, ")], not ", vocab);
  const int64_t words = (vocab + 31) / 32;
  const int64_t n1 = rows - 1;
  int64_t mask_ld = 0;
  if (mask_in.has_value()) {
    // a GPU tensor or pinned host rows (the engine's zero-copy grammar masks)
    const Tensor& m = *mask_in;
    if (m.is_cuda()) {
      check_gpu(m, logits, at::kInt, "mask_in");
    } else {
      TORCH_CHECK(m.is_pinned(), "mask_in must be a GPU or pinned host tensor");
      TORCH_CHECK(m.scalar_type() == at::kInt, "mask_in must be ", at::kInt, ", not ", m.scalar_type());
    }
    TORCH_CHECK(m.dim() == 2 && m.stride(1) == 1 && m.size(1) >= words && (m.size(0) == 1 || m.size(0) >= rows),
                "mask_in must be [1 or >= ", rows, ", >= ", words, " (vocab = ", vocab,
                " bits)] with contiguous rows, not ", m.sizes());
    if (m.size(0) > 1) {
      TORCH_CHECK(m.stride(0) >= m.size(1), "mask_in rows must not overlap");
      mask_ld = m.stride(0);
    }
  }
  check_mat(mask_out, logits, at::kInt, rows, words, "mask_out");
  check_vec_1d(n_kept, logits, at::kInt, rows, "n_kept");
  check_vec_1d(temperature, logits, at::kFloat, rows, "temperature");
  check_vec_1d(top_p, logits, at::kFloat, rows, "top_p");
  check_vec_1d(top_k, logits, at::kInt, rows, "top_k");
  check_vec_1d(penalty, logits, at::kFloat, rows, "penalty");
  check_gpu(history, logits, at::kInt, "history");
  TORCH_CHECK(history.dim() == 2 && history.size(0) >= rows && history.size(1) <= kNucleusMaxHistory &&
                  (history.size(1) == 0 || (history.stride(1) == 1 && history.stride(0) >= history.size(1))),
              "history must be [>= ", rows, ", <= ", kNucleusMaxHistory, "] with contiguous rows, not ",
              history.sizes());
  const int64_t H = history.size(1);
  const int64_t hist_ld = H > 0 ? history.stride(0) : 0;

  const Range outs[2] = {{mask_out.data_ptr(), 4 * (n1 * mask_out.stride(0) + mask_out.size(1)), "mask_out"},
                         {n_kept.data_ptr(), 4 * rows, "n_kept"}};
  const Range ins[7] = {{logits.data_ptr(), 4 * (n1 * logits.stride(0) + vocab), "logits"},
                        {mask_in.has_value() ? mask_in->data_ptr() : nullptr,
                         mask_in.has_value() ? 4 * (n1 * mask_ld + words) : 0, "mask_in"},
                        {temperature.data_ptr(), 4 * rows, "temperature"},
                        {top_p.data_ptr(), 4 * rows, "top_p"},
                        {top_k.data_ptr(), 4 * rows, "top_k"},
                        {penalty.data_ptr(), 4 * rows, "penalty"},
                        {H > 0 ? history.data_ptr() : nullptr, H > 0 ? 4 * (n1 * hist_ld + H) : 0, "history"}};
  TORCH_CHECK(!overlaps(outs[0].p, outs[0].bytes, outs[1].p, outs[1].bytes), "mask_out must not overlap n_kept");
  for (const Range& o : outs)
    for (const Range& i : ins)
      TORCH_CHECK(i.bytes == 0 || !overlaps(o.p, o.bytes, i.p, i.bytes), o.name, " must not overlap ", i.name);

  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_nucleus_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab,
                            mask_in.has_value() ? mask_in->data_ptr<int>() : nullptr, mask_ld,
                            mask_out.data_ptr<int>(), mask_out.stride(0), (int)mask_out.size(1),
                            n_kept.data_ptr<int>(), temperature.data_ptr<float>(), top_p.data_ptr<float>(),
                            top_k.data_ptr<int>(), penalty.data_ptr<float>(), H > 0 ? history.data_ptr<int>() : nullptr,
                            hist_ld, (int)H, cur_stream(logits)),
           "nucleus_step");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 nucleus step: repetition penalty, top-k and top-p narrowing of the sampler's allow-mask";
  m.attr("MAX_ROWS") = kNucleusMaxRows;
  m.attr("MAX_VOCAB") = kNucleusMaxVocab;
  m.attr("MAX_TOP_K") = kNucleusMaxTopK;
  m.attr("MAX_HISTORY") = kNucleusMaxHistory;
  m.def("nucleus_step", &nucleus_step, py::arg("logits"), py::arg("vocab"), py::arg("mask_in"), py::arg("mask_out"),
        py::arg("n_kept"), py::arg("temperature"), py::arg("top_p"), py::arg("top_k"), py::arg("penalty"),
        py::arg("history"));
}

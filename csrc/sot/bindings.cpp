// PyTorch bindings of the start-of-transcript probe library (_vwa_sot.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include <vector>

#include "torch_checks.h"
#include "sot/sot.h"

namespace {

using namespace vwa::checks;

void sot_probe(const Tensor& logits, int64_t vocab, int64_t lang0, int64_t n_lang, const std::vector<int64_t>& allow,
               int64_t no_speech_id, const Tensor& lang_probs, const Tensor& lang_tok, const Tensor& lang_conf,
               const Tensor& no_speech, const OptTensor& tok_dst, const OptTensor& dst_rows) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(rows >= 1 && rows < (1 << 24), "logits: the row count must be in [1, 2^24), not ", rows);
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab < (int64_t(1) << 31), "vocab must be in [1, ",
              logits.size(1), "] (the logits' row length), not ", vocab);
  TORCH_CHECK(n_lang >= 1 && n_lang <= kSotMaxLangs, "n_lang must be in [1, ", kSotMaxLangs, "], not ", n_lang);
  TORCH_CHECK(lang0 >= 0 && lang0 + n_lang <= vocab, "lang0 = ", lang0, " with n_lang = ", n_lang,
              " must lie in [0, vocab = ", vocab, "]");
  TORCH_CHECK(no_speech_id >= 0 && no_speech_id < vocab, "no_speech_id must be in [0, vocab = ", vocab, "), not ",
              no_speech_id);
  TORCH_CHECK(allow.size() == 4, "allow must be 4 words of 32 bits, not ", allow.size());
  uint32_t words[4];
  bool any = false;
  for (int i = 0; i < 4; ++i) {
    TORCH_CHECK(allow[i] >= 0 && allow[i] <= 0xffffffffLL, "allow[", i, "] must be a 32-bit word, not ", allow[i]);
    words[i] = (uint32_t)allow[i];
    for (int b = 0; b < 32; ++b) any = any || (((words[i] >> b) & 1u) && 32 * i + b < n_lang);
  }
  TORCH_CHECK(any, "allow admits no language below n_lang = ", n_lang);
  check_mat(lang_probs, logits, at::kFloat, rows, n_lang, "lang_probs");
  check_vec(lang_tok, logits, at::kInt, rows, "lang_tok");
  check_vec(lang_conf, logits, at::kFloat, rows, "lang_conf");
  check_vec(no_speech, logits, at::kFloat, rows, "no_speech");
  TORCH_CHECK(tok_dst.has_value() == dst_rows.has_value(), "tok_dst and dst_rows are given together or not at all");
  int* dst = nullptr;
  const int* drows = nullptr;
  int64_t n_dst = 0;
  if (tok_dst.has_value()) {
    check_vec(*tok_dst, logits, at::kInt, 1, "tok_dst");
    check_vec(*dst_rows, logits, at::kInt, rows, "dst_rows");
    n_dst = tok_dst->numel();
    TORCH_CHECK(n_dst < (int64_t(1) << 31), "tok_dst is too large");
    dst = tok_dst->data_ptr<int>();
    drows = dst_rows->data_ptr<int>();
  }
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_sot_probe(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, (int)lang0, (int)n_lang,
                         words, (int)no_speech_id, lang_probs.data_ptr<float>(), lang_probs.stride(0),
                         lang_tok.data_ptr<int>(), lang_conf.data_ptr<float>(), no_speech.data_ptr<float>(), dst, drows,
                         (int)n_dst, cur_stream(logits)),
           "sot_probe");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 start-of-transcript probe: no-speech probability and language distribution of Whisper's SOT logits";
  m.def("sot_probe", &sot_probe, py::arg("logits"), py::arg("vocab"), py::arg("lang0"), py::arg("n_lang"),
        py::arg("allow"), py::arg("no_speech_id"), py::arg("lang_probs"), py::arg("lang_tok"), py::arg("lang_conf"),
        py::arg("no_speech"), py::arg("tok_dst") = py::none(), py::arg("dst_rows") = py::none());
}

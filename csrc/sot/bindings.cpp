// PyTorch bindings of the start-of-transcript probe library (_vwa_sot.so).
//
// Same rules as csrc/bindings.cpp and csrc/align/bindings.cpp: the entry point validates device,
// dtype, contiguity, shape and range on the host BEFORE launching (a bad shape must never reach a
// kernel), names the offending argument, and launches on the current HIP stream of the anchor
// tensor's device under a device guard.  The few checks needed are a copy of those files' vocabulary.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "sot/sot.h"

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
// Vector: contiguous GPU tensor of >= n elements
void check_vec(const Tensor& t, const Tensor& a, at::ScalarType dt, int64_t n, const char* name) {
  check_gpu(t, a, dt, name);
  TORCH_CHECK(t.is_contiguous() && t.numel() >= n, name, " must be contiguous with >= ", n, " elements, not ",
              t.sizes());
}
// f32 matrix with unit inner stride and non-overlapping rows
void check_f32_rows(const Tensor& t, const Tensor& a, const char* name) {
  check_gpu(t, a, at::kFloat, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) >= t.size(1), name, " must be 2-D with contiguous rows");
}
void check_rc(int rc, const char* what) { TORCH_CHECK(rc == 0, what, " launch failed with code ", rc); }

void sot_probe(const Tensor& logits, int64_t vocab, int64_t lang0, int64_t n_lang, const std::vector<int64_t>& allow,
               int64_t no_speech_id, const Tensor& lang_probs, const Tensor& lang_tok, const Tensor& lang_conf,
               const Tensor& no_speech, const OptTensor& tok_dst, const OptTensor& dst_rows) {
  check_f32_rows(logits, logits, "logits");
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
  check_f32_rows(lang_probs, logits, "lang_probs");
  TORCH_CHECK(lang_probs.size(0) >= rows && lang_probs.size(1) >= n_lang, "lang_probs must be [>= ", rows, ", >= ",
              n_lang, "], not ", lang_probs.sizes());
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

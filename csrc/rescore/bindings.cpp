// PyTorch bindings of the per-sequence log-probability library (_vwa_rescore.so).  Rules and check
// vocabulary: csrc/torch_checks.h.
#include "rescore/rescore.h"
#include "torch_checks.h"

namespace {

using namespace vwa::checks;

void seq_logprob(const Tensor& logits, int64_t vocab, const Tensor& target, const Tensor& end_set, const Tensor& seq,
                 int64_t n_seq, const OptTensor& acc_in, const Tensor& lp, const Tensor& acc_out) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  check_vec_1d(target, logits, at::kInt, 0, "target");
  const int64_t rows = target.numel();
  TORCH_CHECK(rows >= 1 && rows <= kRescoreMaxRows, "target: rows must be in [1, ", kRescoreMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per target), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kRescoreMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kRescoreMaxVocab, ")], not ", vocab);
  TORCH_CHECK(n_seq >= 1 && n_seq <= kRescoreMaxSeq, "n_seq must be in [1, ", kRescoreMaxSeq, "], not ", n_seq);
  const int64_t words = (vocab + 31) / 32;
  check_vec(end_set, logits, at::kInt, words, "end_set");
  check_vec_1d(seq, logits, at::kInt, rows, "seq", true);
  check_vec_1d(lp, logits, at::kFloat, rows, "lp", true);
  check_vec_1d(acc_out, logits, at::kFloat, n_seq, "acc_out", true);
  if (acc_in) check_vec_1d(*acc_in, logits, at::kFloat, n_seq, "acc_in", true);
  const struct {
    const char* name;
    const void* p;
    int64_t n;
  } ins[] = {{"logits", logits.data_ptr(), 4 * ((rows - 1) * logits.stride(0) + vocab)},
             {"target", target.data_ptr(), 4 * rows},
             {"end_set", end_set.data_ptr(), 4 * words},
             {"seq", seq.data_ptr(), 4 * rows},
             {"acc_in", acc_in ? acc_in->data_ptr() : nullptr, acc_in ? 4 * n_seq : 0}};
  for (const auto& in : ins) {
    if (!in.n) continue;
    TORCH_CHECK(!overlaps(lp.data_ptr(), 4 * rows, in.p, in.n), "lp must not overlap ", in.name);
    TORCH_CHECK(!overlaps(acc_out.data_ptr(), 4 * n_seq, in.p, in.n), "acc_out must not overlap ", in.name);
  }
  TORCH_CHECK(!overlaps(lp.data_ptr(), 4 * rows, acc_out.data_ptr(), 4 * n_seq), "acc_out must not overlap lp");
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_seq_logprob(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, target.data_ptr<int>(),
                           end_set.data_ptr<int>(), seq.data_ptr<int>(), (int)n_seq,
                           acc_in ? acc_in->data_ptr<float>() : nullptr, lp.data_ptr<float>(),
                           acc_out.data_ptr<float>(), cur_stream(logits)),
           "seq_logprob");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 per-sequence log-probabilities: per logits row, the log-probability of a target id or of the end "
            "set; per sequence, their running sum";
  m.attr("MAX_ROWS") = kRescoreMaxRows;
  m.attr("MAX_SEQ") = kRescoreMaxSeq;
  m.attr("MAX_VOCAB") = kRescoreMaxVocab;
  m.def("seq_logprob", &seq_logprob, py::arg("logits"), py::arg("vocab"), py::arg("target"), py::arg("end_set"),
        py::arg("seq"), py::arg("n_seq"), py::arg("acc_in"), py::arg("lp"), py::arg("acc_out"));
}

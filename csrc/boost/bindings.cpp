// PyTorch bindings of the keyterm boosting library (_vwa_boost.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "boost/boost.h"

namespace {

using namespace vwa::checks;

void boost_step(const Tensor& logits, int64_t vocab, const Tensor& edge_off, const Tensor& edge_tok,
                const Tensor& edge_next, const Tensor& edge_bias, const Tensor& state_root, const Tensor& roots,
                const Tensor& state_in, const Tensor& state_out, const OptTensor& tokens, const OptTensor& parents,
                int64_t W) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  check_vec_1d(roots, logits, at::kInt, 0, "roots");
  const int64_t rows = roots.numel();
  TORCH_CHECK(rows >= 1 && rows <= kBoostMaxRows, "roots: rows must be in [1, ", kBoostMaxRows, "], not ", rows);
  TORCH_CHECK(logits.size(0) >= rows, "logits must have >= ", rows, " rows (one per root), not ", logits.size(0));
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kBoostMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kBoostMaxVocab, ")], not ", vocab);
  check_vec_1d(state_root, logits, at::kInt, 0, "state_root");
  const int64_t S = state_root.numel();
  TORCH_CHECK(S >= 1 && S <= kBoostMaxStates, "state_root: states must be in [1, ", kBoostMaxStates, "], not ", S);
  check_vec_1d(edge_off, logits, at::kInt, S + 1, "edge_off", true);
  check_vec_1d(edge_tok, logits, at::kInt, 0, "edge_tok");
  const int64_t E = edge_tok.numel();
  TORCH_CHECK(E >= 1 && E <= kBoostMaxEdges, "edge_tok: edges must be in [1, ", kBoostMaxEdges, "], not ", E);
  check_vec_1d(edge_next, logits, at::kInt, E, "edge_next", true);
  check_vec_1d(edge_bias, logits, at::kFloat, E, "edge_bias", true);
  check_vec_1d(state_in, logits, at::kInt, rows, "state_in");
  check_vec_1d(state_out, logits, at::kInt, rows, "state_out");
  if (tokens.has_value()) check_vec_1d(*tokens, logits, at::kInt, rows, "tokens");
  const int* pi = state_in.data_ptr<int>();
  const int* po = state_out.data_ptr<int>();
  if (parents.has_value()) {
    check_vec_1d(*parents, logits, at::kInt, rows, "parents");
    TORCH_CHECK(W >= 1 && W <= rows && rows % W == 0, "W: ", rows, " rows are not groups of W = ", W);
    TORCH_CHECK(!overlaps(pi, 4 * rows, po, 4 * rows), "state_out must not overlap state_in when parents are given");
  } else {
    TORCH_CHECK(pi == po || !overlaps(pi, 4 * rows, po, 4 * rows),
                "state_out must be state_in itself or not overlap it");
  }
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_boost_step(logits.data_ptr<float>(), logits.stride(0), (int)rows, (int)vocab, edge_off.data_ptr<int>(),
                          edge_tok.data_ptr<int>(), edge_next.data_ptr<int>(), edge_bias.data_ptr<float>(),
                          state_root.data_ptr<int>(), (int)S, (int)E, roots.data_ptr<int>(), pi,
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

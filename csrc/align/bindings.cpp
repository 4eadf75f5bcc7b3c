// PyTorch bindings of the word-alignment kernel library (_vwa_align.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "align/align.h"

namespace {

using namespace vwa::checks;
constexpr auto kBF16 = at::kBFloat16;

// f32 [planes, rows, cols] with unit inner stride, rows and planes that do not overlap
void check_planes(const Tensor& t, const Tensor& a, const char* name) {
  check_gpu(t, a, at::kFloat, name);
  TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 && t.stride(1) >= t.size(2), name,
              " must be 3-D with contiguous rows");
  TORCH_CHECK(t.stride(0) >= t.size(1) * t.stride(1), name, " planes must not overlap");
}

void attn_probs(const Tensor& q, const Tensor& k, const Tensor& heads, int64_t n_keys, double scale, const Tensor& out) {
  check_gpu(q, q, kBF16, "q");
  TORCH_CHECK(q.dim() == 2 && q.stride(1) == 1 && q.stride(0) % 8 == 0 && aligned(q, 16), "q",
              " must be 2-D with contiguous 16-byte aligned rows");
  check_gpu(k, q, kBF16, "k");
  TORCH_CHECK(k.dim() == 3 && k.is_contiguous() && aligned(k, 16), "k must be contiguous [S_max, H, 64]");
  TORCH_CHECK(k.size(2) == kAlignHeadDim, "k: head_dim must be 64, not ", k.size(2));
  const int64_t S = k.size(0), H = k.size(1), T = q.size(0);
  TORCH_CHECK(H >= 1 && q.size(1) == H * kAlignHeadDim, "q must be [T, H * 64] with k's H = ", H, ", not ", q.sizes());
  TORCH_CHECK(T >= 1 && T < (1 << 20), "q: T must be in [1, 2^20), not ", T);
  check_vec(heads, q, at::kInt, 1, "heads");
  TORCH_CHECK(heads.dim() == 1 && heads.numel() <= 65535, "heads must be 1-D with 1..65535 entries");
  TORCH_CHECK(n_keys >= 1 && n_keys <= S, "n_keys must be in [1, S_max = ", S, "], not ", n_keys);
  check_planes(out, q, "out");
  TORCH_CHECK(out.size(0) == heads.numel() && out.size(1) == T && out.size(2) == S, "out must be [n_sel, T, S_max] = [",
              heads.numel(), ", ", T, ", ", S, "], not ", out.sizes());
  const c10::DeviceGuard guard(q.device());
  check_rc(vwa_attn_probs(reinterpret_cast<const uint16_t*>(q.data_ptr()), q.stride(0),
                          reinterpret_cast<const uint16_t*>(k.data_ptr()), heads.data_ptr<int>(), (int)heads.numel(),
                          (int)H, (int)T, (int)n_keys, (float)scale, out.data_ptr<float>(), out.stride(0),
                          out.stride(1), cur_stream(q)),
           "attn_probs");
}

void align_cost(const Tensor& probs, int64_t n_tokens, int64_t n_keys, const Tensor& out) {
  check_planes(probs, probs, "probs");
  const int64_t Hs = probs.size(0), T = probs.size(1), S = probs.size(2);
  TORCH_CHECK(Hs >= 1 && Hs < (1 << 20), "probs: the head count must be in [1, 2^20), not ", Hs);
  TORCH_CHECK(n_tokens >= 1 && n_tokens <= T, "n_tokens must be in [1, T = ", T, "], not ", n_tokens);
  TORCH_CHECK(n_keys >= 1 && n_keys <= S, "n_keys must be in [1, S_max = ", S, "], not ", n_keys);
  TORCH_CHECK(S < (1 << 24), "probs: S_max too large");
  check_mat(out, probs, at::kFloat, 0, 0, "out");
  TORCH_CHECK(out.size(0) == T && out.size(1) == S, "out must be [T, S_max] = [", T, ", ", S, "], not ", out.sizes());
  const c10::DeviceGuard guard(probs.device());
  check_rc(vwa_align_cost(probs.data_ptr<float>(), probs.stride(0), probs.stride(1), (int)Hs, (int)n_tokens,
                          (int)n_keys, out.data_ptr<float>(), out.stride(0), cur_stream(probs)),
           "align_cost");
}

void dtw_path(const Tensor& cost, int64_t n_tokens, int64_t n_keys, const Tensor& first_frame,
              const Tensor& last_frame, const OptTensor& workspace) {
  check_mat(cost, cost, at::kFloat, 0, 0, "cost");
  const int64_t T = cost.size(0), S = cost.size(1);
  TORCH_CHECK(n_tokens >= 1 && n_tokens <= T && n_tokens <= kDtwMaxRows, "n_tokens must be in [1, min(T = ", T, ", ",
              kDtwMaxRows, ")], not ", n_tokens);
  TORCH_CHECK(n_keys >= 1 && n_keys <= S && S < (1 << 24), "n_keys must be in [1, S_max = ", S, "], not ", n_keys);
  check_vec(first_frame, cost, at::kInt, n_tokens, "first_frame");
  check_vec(last_frame, cost, at::kInt, n_tokens, "last_frame");
  uint8_t* ws = nullptr;
  if (n_tokens * n_keys > kDtwLdsTrace) {
    TORCH_CHECK(workspace.has_value(), "workspace (uint8, >= n_tokens * n_keys bytes) is required above ",
                kDtwLdsTrace, " cells");
    check_vec(*workspace, cost, at::kByte, n_tokens * n_keys, "workspace");
    ws = workspace->data_ptr<uint8_t>();
  } else if (workspace.has_value()) {
    check_vec(*workspace, cost, at::kByte, 0, "workspace");
  }
  const c10::DeviceGuard guard(cost.device());
  check_rc(vwa_dtw_path(cost.data_ptr<float>(), cost.stride(0), (int)n_tokens, (int)n_keys, first_frame.data_ptr<int>(),
                        last_frame.data_ptr<int>(), ws, cur_stream(cost)),
           "dtw_path");
}

void token_logprob(const Tensor& logits, const Tensor& targets, const OptTensor& mask, int64_t vocab,
                   const Tensor& out) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  const int64_t N = logits.size(0);
  TORCH_CHECK(N >= 1 && N < (1 << 24), "logits: the row count must be in [1, 2^24), not ", N);
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1), "vocab must be in [1, ", logits.size(1), "], not ", vocab);
  check_vec(targets, logits, at::kInt, N, "targets");
  // ([N, words] may be one row expanded: stride 0)
  const int64_t mask_stride = mask.has_value() ? check_mask(*mask, logits, N, vocab, true, true) : 0;
  check_vec(out, logits, at::kFloat, N, "out");
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_token_logprob(logits.data_ptr<float>(), logits.stride(0), (int)N, (int)vocab, targets.data_ptr<int>(),
                             mask.has_value() ? reinterpret_cast<const uint32_t*>(mask->data_ptr<int>()) : nullptr,
                             mask_stride, out.data_ptr<float>(), cur_stream(logits)),
           "token_logprob");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 word-alignment kernels: attention probabilities, alignment cost, DTW, token log-probabilities";
  m.def("attn_probs", &attn_probs, py::arg("q"), py::arg("k"), py::arg("heads"), py::arg("n_keys"), py::arg("scale"),
        py::arg("out"));
  m.def("align_cost", &align_cost, py::arg("probs"), py::arg("n_tokens"), py::arg("n_keys"), py::arg("out"));
  m.def("dtw_path", &dtw_path, py::arg("cost"), py::arg("n_tokens"), py::arg("n_keys"), py::arg("first_frame"),
        py::arg("last_frame"), py::arg("workspace") = py::none());
  m.def("token_logprob", &token_logprob, py::arg("logits"), py::arg("targets"), py::arg("mask"), py::arg("vocab"),
        py::arg("out"));
}

// PyTorch bindings of the beam search library (_vwa_beam.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "beam/beam.h"

namespace {

using namespace vwa::checks;

// int32 [G, W], contiguous
void check_gw(const Tensor& t, const Tensor& a, int64_t G, int64_t W, const char* name) {
  check_gpu(t, a, at::kInt, name);
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous() && t.size(0) == G && t.size(1) == W, name, " must be contiguous [", G,
              ", ", W, "], not ", t.sizes());
}
void check_width(int64_t G, int64_t W) {
  TORCH_CHECK(W >= 2 && W <= kBeamMaxWidth, "W (beams per group) must be in [2, ", kBeamMaxWidth, "], not ", W);
  TORCH_CHECK(G >= 1 && G * W <= kBeamMaxRows, "G x W must be in [1, ", kBeamMaxRows, "] rows, not ", G, " x ", W);
}

int64_t beam_select_workspace(int64_t rows, int64_t vocab) {
  TORCH_CHECK(rows >= 1 && rows <= kBeamMaxRows, "rows must be in [1, ", kBeamMaxRows, "], not ", rows);
  TORCH_CHECK(vocab >= 1 && vocab <= kBeamMaxVocab, "vocab must be in [1, ", kBeamMaxVocab, "], not ", vocab);
  return vwa_beam_select_workspace((int)rows, (int)vocab);
}

void beam_select(const Tensor& logits, const Tensor& cum, const OptTensor& mask, int64_t vocab, int64_t W,
                 const Tensor& cand_score, const Tensor& cand_beam, const Tensor& cand_tok, const Tensor& workspace) {
  check_mat(logits, logits, at::kFloat, 0, 0, "logits");
  const int64_t N = logits.size(0);
  TORCH_CHECK(W >= 2 && W <= kBeamMaxWidth, "W (beams per group) must be in [2, ", kBeamMaxWidth, "], not ", W);
  TORCH_CHECK(N >= W && N % W == 0, "logits: ", N, " rows are not groups of W = ", W);
  const int64_t G = N / W;
  check_width(G, W);
  TORCH_CHECK(vocab >= 1 && vocab <= logits.size(1) && vocab <= kBeamMaxVocab, "vocab must be in [1, min(",
              logits.size(1), " (the logits' row length), ", kBeamMaxVocab, ")], not ", vocab);
  check_vec(cum, logits, at::kFloat, N, "cum");
  const int64_t mask_stride = mask.has_value() ? check_mask(*mask, logits, N, vocab, true, false) : 0;
  const int64_t K = 2 * W;
  check_mat(cand_score, logits, at::kFloat, G, K, "cand_score");
  check_mat(cand_beam, logits, at::kInt, G, K, "cand_beam");
  check_mat(cand_tok, logits, at::kInt, G, K, "cand_tok");
  const int64_t ldc = cand_score.stride(0);
  TORCH_CHECK(cand_beam.stride(0) == ldc && cand_tok.stride(0) == ldc,
              "cand_score, cand_beam and cand_tok must have one row stride");
  const int64_t need = vwa_beam_select_workspace((int)N, (int)vocab);
  check_gpu(workspace, logits, at::kInt, "workspace");
  TORCH_CHECK(workspace.is_contiguous() && workspace.numel() * 4 >= need, "workspace must be contiguous int32 with >= ",
              need / 4, " elements (beam_select_workspace), not ", workspace.sizes());
  const c10::DeviceGuard guard(logits.device());
  check_rc(vwa_beam_select(logits.data_ptr<float>(), logits.stride(0), (int)G, (int)W, (int)vocab,
                           mask.has_value() ? reinterpret_cast<const uint32_t*>(mask->data_ptr<int>()) : nullptr,
                           mask_stride, cum.data_ptr<float>(), cand_score.data_ptr<float>(), cand_beam.data_ptr<int>(),
                           cand_tok.data_ptr<int>(), ldc, workspace.data_ptr<int>(), workspace.numel() * 4,
                           cur_stream(logits)),
           "beam_select");
}

void kv_beam_gather(const Tensor& k_cache, const Tensor& v_cache, const Tensor& block_table, const Tensor& slots,
                    const Tensor& parents, const Tensor& n_ctx, int64_t max_ctx) {
  check_gpu(k_cache, k_cache, at::kBFloat16, "k_cache");
  check_gpu(v_cache, k_cache, at::kBFloat16, "v_cache");
  TORCH_CHECK(k_cache.dim() == 5 && k_cache.is_contiguous(), "k_cache must be contiguous [L, n_blocks, H, bs, hd]");
  TORCH_CHECK(v_cache.is_contiguous() && v_cache.sizes() == k_cache.sizes(), "v_cache must be contiguous ",
              k_cache.sizes(), ", not ", v_cache.sizes());
  const int64_t L = k_cache.size(0), n_blocks = k_cache.size(1), H = k_cache.size(2), bs = k_cache.size(3),
                hd = k_cache.size(4);
  TORCH_CHECK(L >= 1 && n_blocks >= 2 && n_blocks < (1 << 24) && H >= 1 && bs >= 1 && hd >= 1,
              "k_cache: empty or too large ", k_cache.sizes());
  TORCH_CHECK((bs * hd * 2) % 16 == 0, "k_cache: a head's block (bs x hd = ", bs, " x ", hd,
              " bf16) must be a multiple of 16 bytes");
  TORCH_CHECK(H * bs * hd * 2 / 16 <= (1 << 24), "k_cache: a block is too large");
  TORCH_CHECK(aligned(k_cache, 16) && aligned(v_cache, 16), "k_cache and v_cache must be 16-byte aligned");
  TORCH_CHECK(slots.dim() == 2, "slots must be [G, W], not ", slots.sizes());
  const int64_t G = slots.size(0), W = slots.size(1);
  check_width(G, W);
  check_gw(slots, k_cache, G, W, "slots");
  check_gw(parents, k_cache, G, W, "parents");
  check_vec(n_ctx, k_cache, at::kInt, G, "n_ctx");
  check_mat(block_table, k_cache, at::kInt, 1, 1, "block_table");
  TORCH_CHECK(block_table.size(0) < (1 << 24), "block_table: too many sessions, ", block_table.size(0));
  const int64_t bps = block_table.size(1);
  TORCH_CHECK(max_ctx >= 0 && max_ctx <= bps * bs, "max_ctx = ", max_ctx, " exceeds the block table's ", bps,
              " blocks of ", bs, " positions");
  const int64_t max_blocks = (max_ctx + bs - 1) / bs;
  TORCH_CHECK(L * max_blocks <= 65535, "k_cache: ", L, " layers x ", max_blocks, " blocks exceed the grid");
  const c10::DeviceGuard guard(k_cache.device());
  check_rc(vwa_kv_beam_gather(k_cache.data_ptr(), v_cache.data_ptr(), (int)L, (int)n_blocks, (int)H, (int)bs, (int)hd,
                              block_table.data_ptr<int>(), (int)block_table.size(0), block_table.stride(0), (int)bps,
                              slots.data_ptr<int>(), parents.data_ptr<int>(), n_ctx.data_ptr<int>(), (int)G, (int)W,
                              (int)max_blocks, cur_stream(k_cache)),
           "kv_beam_gather");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 beam search steps: the best continuations of a group of beams, and the beams' K/V following their parents";
  m.attr("MAX_WIDTH") = kBeamMaxWidth;
  m.attr("MAX_ROWS") = kBeamMaxRows;
  m.attr("MAX_VOCAB") = kBeamMaxVocab;
  m.def("beam_select_workspace", &beam_select_workspace, py::arg("rows"), py::arg("vocab"));
  m.def("beam_select", &beam_select, py::arg("logits"), py::arg("cum"), py::arg("mask"), py::arg("vocab"),
        py::arg("W"), py::arg("cand_score"), py::arg("cand_beam"), py::arg("cand_tok"), py::arg("workspace"));
  m.def("kv_beam_gather", &kv_beam_gather, py::arg("k_cache"), py::arg("v_cache"), py::arg("block_table"),
        py::arg("slots"), py::arg("parents"), py::arg("n_ctx"), py::arg("max_ctx"));
}

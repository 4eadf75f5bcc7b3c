// PyTorch bindings for the gfx950 kernel library.
//
// The rules every entry point follows, and the check vocabulary shared with the small libraries'
// bindings (check_gpu / check_vec / check_mat / ...), are in torch_checks.h; the checks only this
// library needs (check_gpu_or_pinned / check_rows / check_slots / check_cache / check_qkv) are below.
// Each op launches on the current HIP stream of its anchor's device, so it is capturable in a
// torch.cuda.CUDAGraph (= hipGraph on ROCm).
#include <mutex>
#include <string>

#include "torch_checks.h"
#include "kernels/vwa_kernels.h"

namespace {

using namespace vwa::checks;
constexpr auto kBF16 = at::kBFloat16;
constexpr auto kF8 = at::kFloat8_e4m3fn;

const uint16_t* bfp(const Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* bfp_mut(const Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }
const uint16_t* bfp_opt(const OptTensor& t) { return t.has_value() ? bfp(*t) : nullptr; }
uint16_t* bfp_mut_opt(const OptTensor& t) { return t.has_value() ? bfp_mut(*t) : nullptr; }
template <class T>
T* ptr_opt(const OptTensor& t) { return t.has_value() ? t->data_ptr<T>() : nullptr; }
unsigned long long* u64p(const Tensor& t) { return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()); }

// ---- the checks only this library needs (the shared ones: torch_checks.h)
// GPU tensor or pinned host memory (zero-copy grammar masks, token readback)
void check_gpu_or_pinned(const Tensor& t, const Tensor& a, at::ScalarType dt, const char* name) {
  if (t.is_cuda()) return check_gpu(t, a, dt, name);
  TORCH_CHECK(t.is_pinned(), name, " must be a GPU or pinned host tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", not ", t.scalar_type());
}
// the dtype to demand of an output the kernels write as bf16 or f32
at::ScalarType bf16_or_f32(const Tensor& t) { return t.scalar_type() == at::kFloat ? at::kFloat : kBF16; }
// Rows, weak form: 2-D with unit inner stride (the kernels take a row stride)
void check_rows_weak(const Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, name, " must be 2-D with contiguous rows");
}
// Rows: + 16-byte rows (they enter / leave the kernels as 16-byte chunks)
void check_rows(const Tensor& t, const char* name) {
  check_rows_weak(t, name);
  TORCH_CHECK(t.stride(0) % 8 == 0, name, " row stride must be a multiple of 8 elements");
  TORCH_CHECK(aligned(t, 16), name, " must be 16-byte aligned");
}
void check_sizes(const Tensor& t, std::initializer_list<int64_t> want, const char* name) {
  TORCH_CHECK(t.sizes() == at::IntArrayRef(want), name, " must be ", at::IntArrayRef(want), ", not ", t.sizes());
}
// Tensor lists (wdec_run): (index, dtype, minimum length) of each slot
struct Slot { int i; at::ScalarType dt; int64_t n; };
void check_slots(const std::vector<Tensor>& v, const Tensor& a, const char* list, std::initializer_list<Slot> slots) {
  for (const Slot& s : slots)
    check_vec(v[(size_t)s.i], a, s.dt, s.n, (std::string(list) + "[" + std::to_string(s.i) + "]").c_str());
}
// paged KV cache: any block / head / token strides (the kernels address by stride), contiguous head_dim rows
void check_cache(const Tensor& c, const Tensor& a, const char* name) {
  check_gpu(c, a, kBF16, name);
  TORCH_CHECK(c.dim() == 4 && c.stride(3) == 1 && c.stride(0) > 0 && c.stride(1) > 0 && c.stride(2) > 0, name,
              " must be [blocks, kv_heads, block_size, head_dim] with contiguous head_dim rows");
}

int device_cus(const Tensor& t) {
  static int cached[64] = {0};
  const int d = t.device().index();
  if (d >= 0 && d < 64 && cached[d]) return cached[d];
  int cus = 0;
  TORCH_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess, "CU count");
  if (d >= 0 && d < 64) cached[d] = cus;
  return cus;
}

// ---- QKV epilogue operands (RoPE table, positions, paged-KV slots, q rows and cache strides) of the
// skinny / chained kernels, the tiled GEMM's QKV epilogue and rope_kv_write: checked once, here.
// rows_name / q_name: the caller's names of the QKV row count's owner and of q_out.
struct QkvOperands {
  int n_q_heads, n_kv_heads, head_dim, use_rope;
  const int* positions;
  const int64_t* slots;
  const float* rope;
  uint16_t* q_out; int ldq;
  uint16_t* k_cache; uint16_t* v_cache;
  int block_size;
  int64_t sb, sh, st;
};
QkvOperands check_qkv(const Tensor& a, int64_t M, int64_t qkv_rows, const char* rows_name, int64_t n_q_heads,
                      int64_t n_kv_heads, int64_t head_dim, bool use_rope, const Tensor& positions, const Tensor& slots,
                      const OptTensor& rope, const Tensor& q_out, const Tensor& k_cache, const Tensor& v_cache,
                      const char* q_name = "q_out") {
  TORCH_CHECK(n_q_heads >= 1 && n_kv_heads >= 1 && head_dim >= 16 && head_dim % 16 == 0,
              "head_dim must be a multiple of 16, n_q_heads and n_kv_heads positive");
  TORCH_CHECK(qkv_rows == (n_q_heads + 2 * n_kv_heads) * head_dim, rows_name, " has ", qkv_rows,
              ", not (n_q_heads + 2 n_kv_heads) * head_dim");
  check_vec(positions, a, at::kInt, M, "positions");
  check_vec(slots, a, at::kLong, M, "slots");
  check_gpu(q_out, a, kBF16, q_name);
  check_rows_weak(q_out, q_name);
  TORCH_CHECK(q_out.size(0) >= M && q_out.size(1) == n_q_heads * head_dim, q_name,
              " must be [>= M, n_q_heads * head_dim]");
  const Tensor* caches[2] = {&k_cache, &v_cache};
  for (int i = 0; i < 2; ++i) {
    const char* name = i ? "v_cache" : "k_cache";
    check_cache(*caches[i], a, name);
    TORCH_CHECK(caches[i]->size(1) == n_kv_heads && caches[i]->size(3) == head_dim, name,
                " must have n_kv_heads heads of head_dim columns");
  }
  if (use_rope) {
    TORCH_CHECK(rope.has_value(), "rope table required");
    check_vec(*rope, a, at::kFloat, 0, "rope");
    TORCH_CHECK(rope->dim() >= 2 && rope->size(-2) == head_dim / 2 && rope->size(-1) == 2,
                "rope table must be [max_pos, head_dim/2, 2]");
  }
  return {(int)n_q_heads, (int)n_kv_heads, (int)head_dim, use_rope ? 1 : 0, positions.data_ptr<int>(),
          slots.data_ptr<int64_t>(), use_rope ? rope->data_ptr<float>() : nullptr, bfp_mut(q_out), (int)q_out.stride(0),
          bfp_mut(k_cache), bfp_mut(v_cache), (int)k_cache.size(2), k_cache.stride(0), k_cache.stride(1),
          k_cache.stride(2)};
}
template <class P>
void set_qkv_common(P& p, const QkvOperands& q) {
  p.n_q_heads = q.n_q_heads;
  p.n_kv_heads = q.n_kv_heads;
  p.head_dim = q.head_dim;
  p.use_rope = q.use_rope;
  p.positions = q.positions;
  p.slots = q.slots;
  p.rope = q.rope;
  p.q_out = q.q_out;
  p.ldq = q.ldq;
  p.k_cache = q.k_cache;
  p.v_cache = q.v_cache;
  p.block_size = q.block_size;
}
void set_qkv(SkinnyParams& p, const QkvOperands& q) {
  set_qkv_common(p, q);
  p.cache_stride_block = q.sb;
  p.cache_stride_head = q.sh;
  p.cache_stride_tok = q.st;
}
void set_qkv(GemmParams& p, const QkvOperands& q) {
  set_qkv_common(p, q);
  p.cache_sb = q.sb;
  p.cache_sh = q.sh;
  p.cache_st = q.st;
}

// ---- skinny (<= 16 row, small-weight <= 64 row) GEMMs
// skinny GEMM dispatch: 1 = persistent streaming kernel when the shape fits (default), 0 = one-tile kernel
int g_skinny_mode = 1;
int g_grid_cap = 256;
int g_ks = 0;  // K-split waves of the streaming kernel; 0 = by shape (skinny_ks)
int g_w_first = 2;  // 0: never, 1: only with the fused RMSNorm prologue, 2: always (measured best)
void set_skinny_mode(int64_t mode, int64_t grid_cap, int64_t ks, int64_t w_first) {
  g_skinny_mode = (int)mode;
  g_grid_cap = (int)grid_cap;
  g_ks = (int)ks;
  g_w_first = (int)w_first;
}
// Small weights (<= g_small_bytes, e.g. every Whisper-tiny projection): the one-tile kernel.
// Measured (tools/bench_kernels.py --only small, M = 1, weights cache-resident as in the ASR
// decode loop): 2.2 vs 4.3 us for 384-1536 wide projections, 3.3 vs 5.0 us for 1280 x 1280.
size_t g_small_bytes = 4u << 20;
void set_small_gemm_bytes(int64_t n) { g_small_bytes = (size_t)(n > 0 ? n : 0); }
// Also every K < 1024: the streaming kernel splits K over its 8 waves in 128-wide groups, so
// with fewer than 8 groups most of its waves idle (Whisper-tiny's 40 MB LM head, K = 384).
// Streaming-kernel K split: 4 waves when K < 2048, else 8.  Its waves take 128-wide k-groups, so
// at K = 1280 (Whisper-large-v3's decoder) 8 waves leave 6 idle in the second round; measured
// (tools/bench_whisper_decode.py, tiled weights, HBM-resident) 6.45 vs 6.83 us for QKV, 8.33 vs
// 8.97 for fc1, 27.9 vs 34.2 for the 133 MB LM head; K >= 4096 (Llama) stays at 8.
// (> 16 rows: the many-row form exists for 8 waves only)
int skinny_ks(const SkinnyParams& p) { return g_ks ? g_ks : (p.K < 2048 && p.M <= 16 ? 4 : 8); }

bool small_gemm(const SkinnyParams& p) {
  return !p.w_scale && g_small_bytes && p.M <= 64 && ((size_t)p.N * p.K * 2 <= g_small_bytes || p.K < 1024);
}

int run_skinny(int epi, const SkinnyParams& p, hipStream_t st) {
  if (g_skinny_mode == 1 && !small_gemm(p)) {
    const int r = vwa_skinny_stream(epi, &p, g_grid_cap, skinny_ks(p), st);
    if (r != -10) return r;
  }
  return vwa_skinny_gemm(epi, &p, st);
}

// x (the anchor), w and bias of a skinny GEMM; xn / wn / bn: the entry point's names for them
SkinnyParams base_params(const Tensor& x, const char* xn, const Tensor& w, const char* wn, const OptTensor& bias,
                         const char* bn, bool fuse_rms, double eps, const OptTensor& w_scale = c10::nullopt,
                         bool w_tiled = false, bool w_nt = false) {
  check_gpu(x, x, kBF16, xn);
  check_rows(x, xn);
  check_gpu(w, x, w_scale.has_value() ? kF8 : kBF16, wn);
  TORCH_CHECK(w.is_contiguous() && w.dim() == 2, wn, " must be contiguous [N, K]");
  if (w_scale.has_value()) check_vec(*w_scale, x, at::kFloat, w.size(0), "w_scale", true);
  TORCH_CHECK(x.size(1) == w.size(1), "K mismatch: ", xn, " ", x.sizes(), " ", wn, " ", w.sizes());
  // (17..64 rows: the one-tile kernel only, small bf16 weights -- ops._small_rows)
  TORCH_CHECK(x.size(0) >= 1 && x.size(0) <= 64, "skinny_gemm supports 1..64 rows (more: the tiled GEMM), got ", x.size(0));
  TORCH_CHECK(x.size(0) <= 16 || (!w_scale.has_value() && !w_tiled),
              "17..64 rows: bf16 row-major weights (the one-tile kernel) only");
  TORCH_CHECK(w.size(1) % 128 == 0, "K must be a multiple of 128");
  if (bias.has_value()) check_vec(*bias, x, kBF16, w.size(0), bn, true);
  // (fp8 + tiled: the fp8 tiled layout, which only the streaming kernel's W8A8 path reads)
  if (w_tiled) TORCH_CHECK(w.size(0) % 16 == 0, "pre-tiled weights need N % 16 == 0, K % 128 == 0");
  // (the nt weight policy reads whole lines once per instruction: the pre-tiled layouts only)
  TORCH_CHECK(!w_nt || w_tiled, wn, ": w_nt (non-temporal weight loads) needs a pre-tiled weight");
  SkinnyParams p{};
  p.X = bfp(x);
  p.ldx = (int)x.stride(0);
  p.W = bfp(w);
  p.M = (int)x.size(0);
  p.N = (int)w.size(0);
  p.K = (int)w.size(1);
  p.bias = bfp_opt(bias);
  p.fuse_rms = fuse_rms ? 1 : 0;
  p.eps = (float)eps;
  p.w_scale = ptr_opt<float>(w_scale);
  p.w_first = g_w_first == 2 || (g_w_first == 1 && fuse_rms);
  p.w_tiled = w_tiled ? 1 : 0;
  p.w_nt = w_nt ? 1 : 0;
  return p;
}

// fp8 weights run only on the streaming kernel; a shape it cannot take is an error, never a
// silent bf16 fallback (the Python layer routes those shapes to the dequantising path).
int run_skinny_checked(int epi, const SkinnyParams& p, hipStream_t st) {
  if (p.M > 16) return vwa_skinny_gemm(epi, &p, st);  // (17..64 rows: the one-tile kernel's MT row tiles)
  // pre-tiled weights (bf16 or fp8) exist only for the streaming kernel (a shape it rejects is an error)
  if (p.w_tiled) return vwa_skinny_stream(epi, &p, g_grid_cap, skinny_ks(p), st);
  if (p.w_scale || (p.fuse_rms == 2 && !small_gemm(p))) return vwa_skinny_stream(epi, &p, g_grid_cap, skinny_ks(p), st);
  return run_skinny(epi, p, st);
}

// Folded LayerNorm (fuse_rms = 2): bf16 weights, <= 16 rows (17..64: the one-tile kernel); runs on the streaming kernel, or on
// the one-tile kernel for the small GEMMs it takes (run_skinny_checked: small_gemm).
void set_ln_fold(SkinnyParams& p, const Tensor& a, const OptTensor& ln_c, int epi) {
  if (!ln_c.has_value()) return;
  TORCH_CHECK(p.w_scale == nullptr, "folded LayerNorm needs bf16 weights");
  TORCH_CHECK(epi != 2, "folded LayerNorm is not supported with the SwiGLU epilogue");
  TORCH_CHECK(p.M <= 64, "folded LayerNorm takes <= 64 rows (17..64: the one-tile kernel)");
  check_vec(*ln_c, a, at::kFloat, p.N, "ln_c", true);
  p.fuse_rms = 2;
  p.ln_c = ln_c->data_ptr<float>();
}

// epi: 0 store, 1 residual add, 3 gelu
// col_mask (epi 0): int32 token bitmask rows [>= rows_used, words]; column n of y is the mask's bit
// col_mask_off * 32 + n (vocab shard offset under TP) -- tiles without an admissible bit in any of
// the first mask_rows rows are not computed (their y columns are left as they were)
void skinny_gemm(Tensor x, Tensor w, OptTensor bias, Tensor y, int64_t epi, bool fuse_rms, double eps,
                 OptTensor residual, OptTensor w_scale, OptTensor ln_c, bool w_tiled, OptTensor col_mask,
                 int64_t col_mask_off, int64_t mask_rows, bool w_nt) {
  c10::DeviceGuard g(x.device());
  SkinnyParams p = base_params(x, "x", w, "w", bias, "bias", fuse_rms, eps, w_scale, w_tiled, w_nt);
  TORCH_CHECK(epi == 0 || epi == 1 || epi == 3, "bad epilogue");
  set_ln_fold(p, x, ln_c, (int)epi);
  check_gpu(y, x, bf16_or_f32(y), "y");
  check_rows_weak(y, "y");
  check_sizes(y, {p.M, p.N}, "y");
  p.Y = y.data_ptr();
  p.ldy = (int)y.stride(0);
  p.y_f32 = y.scalar_type() == at::kFloat;
  if (epi == 1) {
    TORCH_CHECK(residual.has_value(), "residual epilogue needs residual");
    check_gpu(*residual, x, kBF16, "residual");
    check_rows_weak(*residual, "residual");
    check_sizes(*residual, {p.M, p.N}, "residual");
    p.R = bfp(*residual);
    p.ldr = (int)residual->stride(0);
  }
  if (col_mask.has_value()) {
    const Tensor& cm = *col_mask;
    TORCH_CHECK(epi == 0, "col_mask needs the store epilogue");
    check_gpu_or_pinned(cm, x, at::kInt, "col_mask");
    check_rows_weak(cm, "col_mask");
    TORCH_CHECK(mask_rows >= 1 && mask_rows <= cm.size(0) && col_mask_off >= 0 &&
                    (col_mask_off + (w.size(0) + 31) / 32) <= cm.size(1),
                "col_mask does not cover the output columns");
    p.col_mask = reinterpret_cast<const uint32_t*>(cm.data_ptr<int>()) + col_mask_off;
    p.col_mask_ld = (int)cm.stride(0);
    p.col_mask_rows = (int)mask_rows;
  }
  check_rc(run_skinny_checked((int)epi, p, cur_stream(x)), "skinny_gemm");
}

void skinny_gemm_swiglu(Tensor x, Tensor w_gu, OptTensor bias, Tensor h, bool fuse_rms, double eps, OptTensor w_scale,
                        bool w_tiled, bool w_nt) {
  c10::DeviceGuard g(x.device());
  SkinnyParams p = base_params(x, "x", w_gu, "w_gu", bias, "bias", fuse_rms, eps, w_scale, w_tiled, w_nt);
  check_gpu(h, x, kBF16, "h");
  check_rows_weak(h, "h");
  TORCH_CHECK(w_gu.size(0) % 32 == 0, "gate/up rows must be a multiple of 32");
  check_sizes(h, {p.M, p.N / 2}, "h");
  p.Y = h.data_ptr();
  p.ldy = (int)h.stride(0);
  check_rc(run_skinny_checked(2, p, cur_stream(x)), "skinny_gemm_swiglu");
}

void skinny_gemm_qkv(Tensor x, Tensor w_qkv, OptTensor bias, bool fuse_rms, double eps, int64_t n_q_heads,
                     int64_t n_kv_heads, int64_t head_dim, bool use_rope, Tensor positions, Tensor slots,
                     OptTensor rope, Tensor q_out, Tensor k_cache, Tensor v_cache, OptTensor w_scale, OptTensor ln_c,
                     bool w_tiled, bool w_nt) {
  c10::DeviceGuard g(x.device());
  SkinnyParams p = base_params(x, "x", w_qkv, "w_qkv", bias, "bias", fuse_rms, eps, w_scale, w_tiled, w_nt);
  set_ln_fold(p, x, ln_c, 4);
  set_qkv(p, check_qkv(x, p.M, p.N, "w_qkv", n_q_heads, n_kv_heads, head_dim, use_rope, positions, slots, rope, q_out,
                       k_cache, v_cache));
  check_rc(run_skinny_checked(4, p, cur_stream(x)), "skinny_gemm_qkv");
}

// ---- LDS-tiled MFMA GEMM (gemm.hip), M > 16 rows: the operands its entry points share
// w: bf16 [N, K] row-major or pre-tiled, or (sw set) the fp8 tiled layout with per-row scales sw
void set_gemm_w(GemmParams& p, const Tensor& a, const Tensor& w, const char* wn, const OptTensor& sw, bool w_tiled,
                int64_t K) {
  check_gpu(w, a, sw.has_value() ? kF8 : kBF16, wn);
  TORCH_CHECK(w.dim() == 2 && w.is_contiguous() && w.size(1) == K, wn, " must be contiguous [N, K = ", K, "], not ",
              w.sizes());
  TORCH_CHECK(w.size(0) % 16 == 0 && K % 128 == 0, wn, ": N % 16 == 0 and K % 128 == 0 required");
  p.W = bfp(w);
  p.w_tiled = w_tiled ? 1 : 0;
  p.N = (int)w.size(0);
  p.K = (int)K;
  if (sw.has_value()) {
    TORCH_CHECK(w_tiled, wn, ": fp8 weights exist in the tiled layout only");
    check_vec(*sw, a, at::kFloat, p.N, "sw", true);
    p.sw = sw->data_ptr<float>();
  }
}
void set_gemm_bias(GemmParams& p, const Tensor& a, const OptTensor& bias, const char* name = "bias") {
  if (bias.has_value()) check_vec(*bias, a, kBF16, p.N, name, true);
  p.bias = bfp_opt(bias);
}
// x (the anchor): bf16 rows, or (sx set: W8A8, needs sw) fp8 e4m3 codes with per-row scales sx; bf16 x
// with sw is W8A16 (the weights convert to bf16 on the LDS read, no quantised copy of x).  rstd: f32
// [M] per-row RMSNorm scale applied to the product (gammas folded into w).  ws: f32 split-K
// workspace (the launcher splits K only when the output tiles alone cannot fill the CUs).
GemmParams gemm_params(const Tensor& x, const char* xn, const OptTensor& sx, const Tensor& w, const char* wn,
                       const OptTensor& sw, bool w_tiled, const OptTensor& bias, const OptTensor& rstd,
                       const OptTensor& ws) {
  GemmParams p{};
  if (sx.has_value()) {
    check_gpu(x, x, kF8, xn);
    check_rows_weak(x, xn);
    TORCH_CHECK(x.stride(0) % 16 == 0 && aligned(x, 16), xn, " rows must be 16-byte aligned");
    TORCH_CHECK(sw.has_value(), "sx (fp8 x) needs fp8 tiled weights and their scales sw");
    check_vec(*sx, x, at::kFloat, x.size(0), "sx");
  } else {
    check_gpu(x, x, kBF16, xn);
    check_rows(x, xn);
  }
  p.X = bfp(x);
  p.ldx = (int)x.stride(0);
  p.M = (int)x.size(0);
  p.sx = ptr_opt<float>(sx);
  set_gemm_w(p, x, w, wn, sw, w_tiled, x.size(1));
  set_gemm_bias(p, x, bias);
  if (rstd.has_value()) check_vec(*rstd, x, at::kFloat, p.M, "rstd");
  p.rstd = ptr_opt<float>(rstd);
  p.splits = 1;
  p.cus = device_cus(x);
  if (ws.has_value()) {
    check_vec(*ws, x, at::kFloat, 0, "ws");
    p.ws = ws->data_ptr<float>();
    p.ws_cap = ws->numel();
    p.splits = vwa_gemm_splits(p.M, p.N, p.K, p.cus, p.ws_cap, p.sw ? 1 : 0);
  }
  return p;
}

// y and the epilogue of the two plain tiled GEMMs.  epi: 0 store (+bias, bf16 / f32 out), 1 residual
// add (+bias), 2 SwiGLU over interleaved gate/up tiles (y [M, N/2]), 3 GELU (+bias).
void set_gemm_epilogue(GemmParams& p, const Tensor& a, int64_t epi, const Tensor& y, const OptTensor& residual) {
  TORCH_CHECK(epi >= 0 && epi <= 3, "bad epilogue ", epi);
  if (epi == 2) TORCH_CHECK(p.N % 32 == 0, "SwiGLU epilogue: gate/up rows must be a multiple of 32");
  check_gpu(y, a, epi == 2 ? kBF16 : bf16_or_f32(y), "y");
  check_rows(y, "y");  // (bf16 rows leave the kernel as 16-byte chunks)
  check_sizes(y, {p.M, epi == 2 ? p.N / 2 : p.N}, "y");
  p.Y = y.data_ptr();
  p.ldy = (int)y.stride(0);
  p.y_f32 = y.scalar_type() == at::kFloat;
  if (epi == 1) {
    TORCH_CHECK(residual.has_value(), "residual epilogue needs residual");
    TORCH_CHECK(!p.y_f32, "y: the residual epilogue writes bf16");
    check_gpu(*residual, a, kBF16, "residual");
    check_rows(*residual, "residual");
    check_sizes(*residual, {p.M, p.N}, "residual");
    p.R = bfp(*residual);
    p.ldr = (int)residual->stride(0);
  }
}

// RMS statistics hand-off of the tiled GEMM (GemmParams::ss_*): ss_out (residual epilogue) gets
// the squares of the output rows added, ss_zero is zeroed (whole tensor), ss_in replaces rstd
// (each an int64 [>= M] vector: u64 fixed point, 2^-24 units)
void set_ss(GemmParams& p, const Tensor& a, int64_t epi, const OptTensor& ss_out, const OptTensor& ss_zero,
            const OptTensor& ss_in, double eps) {
  if (ss_out.has_value()) {
    check_vec(*ss_out, a, at::kLong, p.M, "ss_out");
    TORCH_CHECK(epi == 1 && !p.y_f32, "ss_out: residual epilogue (bf16 rows) only");
    p.ss_out = u64p(*ss_out);
  }
  if (ss_zero.has_value()) {
    check_vec(*ss_zero, a, at::kLong, p.M, "ss_zero");
    p.ss_zero = u64p(*ss_zero);
    p.ss_zero_n = (int)ss_zero->numel();
  }
  if (ss_in.has_value()) {
    check_vec(*ss_in, a, at::kLong, p.M, "ss_in");
    TORCH_CHECK(p.rstd == nullptr && p.sx == nullptr, "ss_in replaces rstd, bf16 x only");
    p.ss_in = u64p(*ss_in);
    p.ss_eps = (float)eps;
  }
}

void gemm(Tensor x, Tensor w, OptTensor bias, Tensor y, int64_t epi, OptTensor rstd, OptTensor residual, bool w_tiled,
          OptTensor ws, OptTensor ss_out, OptTensor ss_zero, OptTensor ss_in, double ss_eps) {
  c10::DeviceGuard g(x.device());
  GemmParams p = gemm_params(x, "x", c10::nullopt, w, "w", c10::nullopt, w_tiled, bias, rstd, ws);
  set_gemm_epilogue(p, x, epi, y, residual);
  set_ss(p, x, epi, ss_out, ss_zero, ss_in, ss_eps);
  check_rc(vwa_gemm((int)epi, &p, cur_stream(x)), "gemm");
}

// fp8 tiled GEMM: w8 the fp8 tiled layout [N, K] with per-row scales sw, and either x8 OCP e4m3
// [M, K] with per-row scales sx (W8A8, quant_fp8_rows) or bf16 rows with sx = None (W8A16)
void gemm_fp8(Tensor x8, OptTensor sx, Tensor w8, Tensor sw, OptTensor bias, Tensor y, int64_t epi, OptTensor rstd,
              OptTensor residual, OptTensor ws, OptTensor ss_out, OptTensor ss_zero, OptTensor ss_in, double ss_eps) {
  c10::DeviceGuard g(x8.device());
  GemmParams p = gemm_params(x8, "x8", sx, w8, "w8", sw, true, bias, rstd, ws);
  set_gemm_epilogue(p, x8, epi, y, residual);
  set_ss(p, x8, epi, ss_out, ss_zero, ss_in, ss_eps);
  check_rc(vwa_gemm((int)epi, &p, cur_stream(x8)), "gemm_fp8");
}

// QKV projection on the tiled GEMM with the rotary + paged-KV write in its epilogue (gemm.hip
// EPI_QKV; > 16 rows): x bf16 (sx null) or fp8 codes x8 with per-row scales sx (W8A8); w bf16 or
// fp8 tiled with row scales sw (bf16 x + sw: W8A16).  Replaces gemm -> qkv scratch -> rope_kv_write.
void gemm_qkv(Tensor x, OptTensor sx, Tensor w, OptTensor sw, OptTensor bias, OptTensor rstd, bool w_tiled, Tensor ws,
              int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim, bool use_rope, Tensor positions, Tensor slots,
              OptTensor rope, Tensor q_out, Tensor k_cache, Tensor v_cache, OptTensor ss_in, double ss_eps) {
  c10::DeviceGuard g(x.device());
  GemmParams p = gemm_params(x, "x", sx, w, "w", sw, w_tiled, bias, rstd, ws);
  set_qkv(p, check_qkv(x, p.M, p.N, "w", n_q_heads, n_kv_heads, head_dim, use_rope, positions, slots, rope, q_out,
                       k_cache, v_cache));
  // (this path only: q rows and cache token rows leave the kernel as 16-byte chunks, one set of strides)
  check_rows(q_out, "q_out");
  TORCH_CHECK(k_cache.stride(0) % 8 == 0 && k_cache.stride(1) % 8 == 0 && k_cache.stride(2) % 8 == 0 &&
                  k_cache.strides() == v_cache.strides() && aligned(k_cache, 16) && aligned(v_cache, 16),
              "k_cache / v_cache: 16-byte aligned token rows and equal strides");
  set_ss(p, x, 5, c10::nullopt, c10::nullopt, ss_in, ss_eps);
  check_rc(vwa_gemm(5, &p, cur_stream(x)), "gemm_qkv");
}

void row_rstd(Tensor x, Tensor rstd, double eps) {
  c10::DeviceGuard g(x.device());
  check_gpu(x, x, kBF16, "x");
  check_rows(x, "x");
  check_vec(rstd, x, at::kFloat, x.size(0), "rstd");
  check_rc(vwa_row_rstd(bfp(x), (int)x.stride(0), (int)x.size(0), (int)x.size(1), (float)eps, rstd.data_ptr<float>(),
                        cur_stream(x)),
           "row_rstd");
}

void quant_fp8_rows(Tensor x, Tensor q, Tensor scale, OptTensor rstd, double eps) {
  c10::DeviceGuard g(x.device());
  check_gpu(x, x, kBF16, "x");
  check_rows(x, "x");
  check_gpu(q, x, kF8, "q");
  TORCH_CHECK(q.is_contiguous() && q.sizes() == x.sizes(), "q must be contiguous [rows, D] like x");
  check_vec(scale, x, at::kFloat, x.size(0), "scale");
  if (rstd.has_value()) check_vec(*rstd, x, at::kFloat, x.size(0), "rstd");
  check_rc(vwa_quant_fp8_rows(bfp(x), (int)x.stride(0), (int)x.size(0), (int)x.size(1),
                              reinterpret_cast<uint8_t*>(q.data_ptr()), scale.data_ptr<float>(), ptr_opt<float>(rstd),
                              (float)eps, cur_stream(x)),
           "quant_fp8_rows");
}

// Whisper conv stem (K3): conv1d(k=3, pad=1, stride) + bias + GELU (+ pos) as a batched implicit
// GEMM on the tiled MFMA GEMM (gemm.hip, row-major weights).  x [B, Tin, Cin] must be a view
// of a zero-padded channels-last buffer (ops.padded_rows): one zero row in front of and behind
// every batch's Tin rows, so GEMM row t is the 3*Cin contiguous elements starting at padded
// row t*stride (ldx = stride*Cin).  w [Cout, 3*Cin] in (kk, ci) order, row-major or pre-tiled.
void conv1d_gelu(Tensor x, Tensor w, OptTensor b, OptTensor pos, Tensor y, int64_t stride, bool w_tiled) {
  c10::DeviceGuard g(x.device());
  check_gpu(x, x, kBF16, "x");
  check_gpu(y, x, kBF16, "y");
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1 && x.stride(1) == x.size(2),
              "x must be [B, T, Cin] with contiguous rows");
  const int64_t B = x.size(0), Tin = x.size(1), Cin = x.size(2);
  TORCH_CHECK(B == 1 || x.stride(0) >= (Tin + 2) * Cin, "x batches must be (Tin + 2)-row padded slabs");
  TORCH_CHECK(x.storage_offset() >= Cin &&
                  (int64_t)(x.storage().nbytes() / 2) >= x.storage_offset() + (B - 1) * x.stride(0) + (Tin + 1) * Cin,
              "x must be a view of a zero-padded buffer (a pad row before and after each batch)");
  TORCH_CHECK(stride == 1 || stride == 2, "stride 1 or 2");
  TORCH_CHECK(Cin % 8 == 0, "x: Cin % 8 == 0 required");
  GemmParams p{};
  // w [Cout, 3*Cin] ([co][kk][ci]); tiled: the ops.tile_weight layout, 1 KB contiguous B-fragment DMA per instruction
  set_gemm_w(p, x, w, "w", c10::nullopt, w_tiled, 3 * Cin);
  const int64_t Tout = (Tin + 2 - 3) / stride + 1, Cout = w.size(0);
  TORCH_CHECK(y.dim() == 3 && y.size(0) == B && y.size(1) == Tout && y.size(2) == Cout && y.stride(2) == 1 &&
                  y.stride(1) % 8 == 0 && (B == 1 || y.stride(0) % 8 == 0) && aligned(y, 16),
              "y [B, Tout, Cout] with 16-byte aligned rows");
  p.X = bfp(x) - Cin;  // the zero row in front
  p.ldx = (int)(stride * Cin);
  p.M = (int)Tout;
  p.Y = y.data_ptr();
  p.ldy = (int)y.stride(1);
  p.splits = 1;
  p.nbatch = (int)B;
  p.bsx = x.stride(0);
  p.bsy = y.stride(0);
  set_gemm_bias(p, x, b, "b");
  // one utterance: split-K when the output tiles alone cannot fill the CUs (large-v3 conv2: 120
  // tiles x 30 k-groups); the f32 slabs are summed by gemm_reduce_kernel with the same epilogue
  Tensor ws;
  if (B == 1 && p.K >= 1024) {  // (K = 384: the split's f32 reduce costs more than it saves)
    const int s = vwa_gemm_splits(p.M, p.N, p.K, device_cus(x), (int64_t)1 << 25, 0);
    if (s > 1) {
      ws = at::empty({(int64_t)s * p.M * p.N}, x.options().dtype(at::kFloat));
      p.ws = ws.data_ptr<float>();
      p.splits = s;
    }
  }
  int epi = 3;
  if (pos.has_value()) {
    check_gpu(*pos, x, kBF16, "pos");
    check_rows(*pos, "pos");
    TORCH_CHECK(pos->size(0) >= Tout && pos->size(1) == Cout, "pos must be [>= Tout, Cout]");
    p.R = bfp(*pos);
    p.ldr = (int)pos->stride(0);
    p.bsr = 0;
    epi = 4;
  }
  check_rc(vwa_gemm(epi, &p, cur_stream(x)), "conv1d_gelu");
}

// ---- attention
KVView make_view(const Tensor& a, const Tensor& k, const Tensor& v, const Tensor& table, int64_t block_size, int64_t sb,
                 int64_t sh, int64_t stok) {
  check_gpu(k, a, kBF16, "k");
  check_gpu(v, a, kBF16, "v");
  check_vec(table, a, at::kInt, 0, "table");
  TORCH_CHECK(table.dim() == 2, "table (block table) must be 2-D");
  KVView kv{};
  kv.k = bfp(k);
  kv.v = bfp(v);
  kv.block_table = table.data_ptr<int>();
  kv.table_stride = (int)table.stride(0);
  kv.block_size = (int)block_size;
  kv.stride_block = sb;
  kv.stride_head = sh;
  kv.stride_tok = stok;
  return kv;
}

// q is the anchor
DecodeAttnParams decode_params(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& table,
                               int64_t block_size, int64_t sb, int64_t sh, int64_t stok, const Tensor& ctx_lens,
                               const Tensor& seq_ids, int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim,
                               double scale, int64_t n_splits, const Tensor& part_o, const Tensor& part_ml,
                               const Tensor& counters, const Tensor& out) {
  check_gpu(q, q, kBF16, "q");
  check_rows(q, "q");  // (vector loads)
  TORCH_CHECK(q.size(1) == n_q_heads * head_dim, "q must be [rows, n_q_heads * head_dim]");
  const int rows = (int)q.size(0);
  check_vec(ctx_lens, q, at::kInt, rows, "ctx_lens");
  check_vec(seq_ids, q, at::kInt, rows, "seq_ids");
  check_gpu(out, q, kBF16, "out");
  check_rows_weak(out, "out");
  TORCH_CHECK(out.size(0) >= rows && out.size(1) == n_q_heads * head_dim,
              "out must be [>= rows, n_q_heads * head_dim]");
  TORCH_CHECK(n_splits >= 1 && n_splits <= 64,
              "n_splits: decode attention merges 1..64 chunks (context <= 16384 tokens)");
  // partials and chunk tickets are read only when the keys are split
  // (counters: zero-initialised, left zero by the kernel)
  const int64_t parts = n_splits > 1 ? (int64_t)rows * n_splits * n_q_heads : 0;
  check_vec(part_o, q, at::kFloat, parts * head_dim, "part_o");
  check_vec(part_ml, q, at::kFloat, parts * 2, "part_ml");
  check_vec(counters, q, at::kInt, n_splits > 1 ? rows * n_kv_heads : 0, "counters");
  DecodeAttnParams p{};
  p.q = bfp(q);
  p.ldq = (int)q.stride(0);
  p.kv = make_view(q, k, v, table, block_size, sb, sh, stok);
  p.ctx_lens = ctx_lens.data_ptr<int>();
  p.seq_ids = seq_ids.data_ptr<int>();
  p.rows = rows;
  p.n_q_heads = (int)n_q_heads;
  p.n_kv_heads = (int)n_kv_heads;
  p.head_dim = (int)head_dim;
  p.scale = (float)scale;
  p.split_tokens = vwa_attention_split_tokens();
  p.n_splits = (int)n_splits;
  p.part_o = part_o.data_ptr<float>();
  p.part_ml = part_ml.data_ptr<float>();
  p.counters = counters.data_ptr<int>();
  p.out = bfp_mut(out);
  p.ldo = (int)out.stride(0);
  return p;
}

void decode_attention(Tensor q, Tensor k, Tensor v, Tensor table, int64_t block_size, int64_t sb, int64_t sh,
                      int64_t stok, Tensor ctx_lens, Tensor seq_ids, int64_t n_q_heads, int64_t n_kv_heads,
                      int64_t head_dim, double scale, int64_t n_splits, Tensor part_o, Tensor part_ml, Tensor counters,
                      Tensor out, OptTensor shared) {
  c10::DeviceGuard g(q.device());
  DecodeAttnParams p = decode_params(q, k, v, table, block_size, sb, sh, stok, ctx_lens, seq_ids, n_q_heads,
                                     n_kv_heads, head_dim, scale, n_splits, part_o, part_ml, counters, out);
  if (shared.has_value()) check_vec(*shared, q, at::kInt, 2, "shared");  // [P, n_real]
  p.shared = ptr_opt<int>(shared);
  check_rc(vwa_decode_attention(&p, cur_stream(q)), "decode_attention");
}

void flash_attention(Tensor q, Tensor k, Tensor v, Tensor table, int64_t block_size, int64_t sb, int64_t sh,
                     int64_t stok, Tensor out, int64_t Sk, int64_t n_kv_heads, bool causal, int64_t q_offset,
                     OptTensor q_offsets, OptTensor k_lens, double scale) {
  c10::DeviceGuard g(q.device());
  check_gpu(q, q, kBF16, "q");
  check_gpu(out, q, kBF16, "out");
  TORCH_CHECK(q.dim() == 4, "q must be [B, S, H, D]");
  TORCH_CHECK(q.stride(3) == 1 && out.sizes() == q.sizes() && out.stride(3) == 1,
              "q / out layout: out like q, contiguous D");
  TORCH_CHECK((q.stride(2) % 8) == 0 && (q.stride(1) % 8) == 0, "q strides must be 16-byte multiples");
  if (q_offsets.has_value()) check_vec(*q_offsets, q, at::kInt, q.size(0), "q_offsets");
  if (k_lens.has_value()) check_vec(*k_lens, q, at::kInt, q.size(0), "k_lens");
  FlashAttnParams p{};
  p.q = bfp(q);
  p.q_stride_b = q.stride(0);
  p.q_stride_s = q.stride(1);
  p.q_stride_h = q.stride(2);
  p.kv = make_view(q, k, v, table, block_size, sb, sh, stok);
  p.o = bfp_mut(out);
  p.o_stride_b = out.stride(0);
  p.o_stride_s = out.stride(1);
  p.o_stride_h = out.stride(2);
  p.B = (int)q.size(0);
  p.Sq = (int)q.size(1);
  p.Sk = (int)Sk;
  p.n_q_heads = (int)q.size(2);
  p.n_kv_heads = (int)n_kv_heads;
  p.head_dim = (int)q.size(3);
  p.causal = causal ? 1 : 0;
  p.q_offset = (int)q_offset;
  p.q_offsets = ptr_opt<int>(q_offsets);
  p.k_lens = ptr_opt<int>(k_lens);
  p.scale = (float)scale;
  check_rc(vwa_flash_attention(&p, cur_stream(q)), "flash_attention");
}

// ---- chained launches (skinny_stream.hip, vwa_chain_*)
// Workgroups of a chained launch: one per CU, or CUs / VWA_CHAIN_GRID_DIV when several processes
// share one GPU (the two-rank tensor-parallel test on a single device: both ranks' persistent
// launches must be resident at once, or their in-launch rounds wait for each other until the
// bounded spin gives up)
int chain_grid(const Tensor& a) {
  const char* e = std::getenv("VWA_CHAIN_GRID_DIV");
  const int div = e ? std::atoi(e) : 1, cus = device_cus(a);
  return div > 1 ? cus / div : cus;
}

// Chained-launch schedule (ChainParams): the measured-best settings of the round-2 A/B runs
// (profiles/r2_*): two weight items issued ahead of each barrier, phase 1's item 0 in the free
// register set of a one-item phase 0, X staged by one wave with LDS-DMA, o_proj units only on
// workgroups without an attention item, LDS items for phases 1 and 2, attention -> o_proj
// hand-off by completion count.
void chain_schedule(ChainParams& cp) {
  cp.pre2 = 1;
  cp.next0 = 1;
  cp.xdma = 1;
  cp.osub = 1;
  cp.lds_item_req = 1;
  cp.lds_item2_req = 1;
  cp.attn_flag = 1;
  // round 5 (profiles/r5_chain_xwait.md): nothing but the X pieces in a CU's memory queue until X is
  // in LDS -- chained layer 103.2-103.6 vs 105.6 us, bench GPU wait 3462-3471 vs 3558 us per step
  cp.xfirst = 1;
  cp.xwait = 1;
  // o_proj in 32-column tiles: one epilogue per workgroup (1 row 102.3 / 102.1 vs 103.5 / 103.0 us,
  // 4 rows 107.0 vs 107.5 us per layer, profiles/r5_chain_o_nt2.jsonl)
  cp.o_nt2 = 1;
  // 5..16 rows: the X-streaming down projection in 32-column tiles, half the X bytes per weight
  // byte -- 8 / 13 / 16 rows 107.8 / 113.8 / 117.1 vs 110.4 / 119.0 / 125.4 us per layer
  // (profiles/r5_chain_d_nt2.jsonl)
  cp.d_nt2 = 1;
  // the QKV phase's two items go out at the down -> QKV barrier (half the workgroups take two of its
  // 384 tiles): 100.96 / 100.84 vs 101.38 / 101.57 us (profiles/r5_chain_pre_mask.jsonl)
  cp.pre_mask = 8;
  // round 6 schedule options, all measured no better than the defaults: the
  // multi-layer launch's QKV -> next-attention hand-off by per-kv-group counters instead of the
  // grid barrier, a K/V prefetch while the attention workgroups wait, and (fp8) gate/up's item 0
  // issued by the attention workgroups during their attention
  cp.qkv_flags = 0;  // (per-kv-group counters measured 99.5 -> 100.9 us per layer: the barrier stays)
  cp.kv_prefetch = 0;  // (neutral: 99.47 vs 99.53 us per layer, profiles/r6_chain_multi_variants.jsonl)
  cp.attn_pre = 0;  // (fp8 chain: 2503.7 vs 2471.6 us GPU wait per step with it, bench.py --dtype fp8)
  // diagnostic override of the schedule (tools/chain_probe.py A/B runs): "name=value,..."
  if (const char* e = std::getenv("VWA_CHAIN_SCHED")) {
    std::string s(e);
    size_t at = 0;
    while (at < s.size()) {
      const size_t comma = s.find(',', at), eq = s.find('=', at);
      const size_t end = comma == std::string::npos ? s.size() : comma;
      if (eq != std::string::npos && eq < end) {
        const std::string k = s.substr(at, eq - at);
        const int v = std::atoi(s.substr(eq + 1, end - eq - 1).c_str());
        if (k == "pre2") cp.pre2 = v;
        else if (k == "next0") cp.next0 = v;
        else if (k == "xdma") cp.xdma = v;
        else if (k == "osub") cp.osub = v;
        else if (k == "lds1") cp.lds_item_req = v;
        else if (k == "lds2") cp.lds_item2_req = v;
        else if (k == "aflag") cp.attn_flag = v;
        else if (k == "pre_mask") cp.pre_mask = v;
        else if (k == "pre_waves") cp.pre_waves = v;
        else if (k == "xfirst") cp.xfirst = v;
        else if (k == "xwait") cp.xwait = v;
        else if (k == "xw_late") cp.xw_late = v;
        else if (k == "poll_free") cp.poll_free = v;
        else if (k == "o_nt2") cp.o_nt2 = v;
        else if (k == "d_nt2") cp.d_nt2 = v;
        else if (k == "qkv_flags") cp.qkv_flags = v;
        else if (k == "kv_pf") cp.kv_prefetch = v;
        else if (k == "attn_pre") cp.attn_pre = v;
      }
      at = end + 1;
    }
  }
}

void set_resid(SkinnyParams& p, const Tensor& h) {
  p.Y = h.data_ptr();
  p.ldy = (int)h.stride(0);
  p.R = bfp(h);
  p.ldr = (int)h.stride(0);
}

// bar: 128-byte aligned barrier words; work: [0, 8192) u32 split-tile tickets (zeroed, self-resetting) |
// f32 partial slots
void set_chain_sync(ChainParams& cp, const Tensor& a, const Tensor& bar, const Tensor& work, int64_t bar_mode) {
  check_vec(bar, a, at::kInt, 384, "bar");
  TORCH_CHECK(aligned(bar, 128), "bar must be 128-byte aligned");
  check_vec(work, a, at::kInt, 8192 + 4096 + 1, "work");
  cp.bar = reinterpret_cast<unsigned*>(bar.data_ptr<int>());
  cp.bar_mode = (int)bar_mode;
  cp.tickets = reinterpret_cast<unsigned*>(work.data_ptr<int>());
  cp.max_tiles = 8192;
  cp.part = reinterpret_cast<float*>(work.data_ptr<int>() + 8192);
  cp.part_floats = (int)(work.numel() - 8192);
}

// The descriptor built on the host, copied to a device tensor (graph replays then only launch), and
// its dynamic LDS bytes; the empty tensor when the shapes do not fit the chain (the caller keeps the
// per-kernel path).
Tensor chain_upload(ChainParams& cp, const Tensor& a, int64_t& lds) {
  lds = vwa_chain_prepare(&cp, chain_grid(a));
  if (lds < 0) {
    lds = 0;
    return torch::empty({0}, torch::dtype(torch::kUInt8).device(a.device()));
  }
  Tensor host = torch::empty({(int64_t)sizeof(ChainParams)}, torch::dtype(torch::kUInt8));
  std::memcpy(host.data_ptr(), &cp, sizeof(ChainParams));
  return host.to(a.device());
}

// Chained Llama decode layer tail, M <= 4, bf16 / fp8 tiled weights, one GPU or the in-launch TP
// all-reduce.  Returns (descriptor uint8 tensor, dynamic LDS bytes + flag bits).
std::tuple<Tensor, int64_t> chain_make(Tensor h, Tensor att, Tensor act, Tensor w_o, Tensor w_gu, Tensor w_down,
                                       double eps, OptTensor w_qkv, int64_t n_q_heads, int64_t n_kv_heads,
                                       int64_t head_dim, OptTensor positions, OptTensor slots, OptTensor rope,
                                       OptTensor q_out, OptTensor k_cache, OptTensor v_cache, Tensor bar, Tensor work,
                                       OptTensor ts, int64_t bar_mode, OptTensor a_q, OptTensor a_k, OptTensor a_v,
                                       OptTensor a_table, int64_t a_block_size, int64_t a_sb, int64_t a_sh,
                                       int64_t a_st, OptTensor a_ctx, OptTensor a_seq, double a_scale,
                                       int64_t a_n_splits, OptTensor a_part_o, OptTensor a_part_ml,
                                       OptTensor a_counters, bool w_tiled,
                                       OptTensor a_row_table, OptTensor s_o, OptTensor s_gu, OptTensor s_down,
                                       OptTensor s_qkv, int64_t tp_ar, OptTensor a_plan, int64_t a_plan_mode,
                                       OptTensor p_o, OptTensor p_gu, OptTensor p_down, OptTensor p_qkv,
                                       std::vector<int64_t> p_base, bool w_nt) {
  c10::DeviceGuard g(h.device());
  ChainParams cp{};
  // w_nt: the launch streams its weights non-temporally where it has that instantiation (the tails
  // with the attention phase: packed, bf16 with o_nt2, fp8); other forms keep the default policy
  TORCH_CHECK(!w_nt || w_tiled, "chain: w_nt (non-temporal weight loads) needs pre-tiled weights");
  // s_*: per-row scales of fp8 tiled weights (ops.tile_weight_fp8) -> the W8A16 chain
  TORCH_CHECK(s_o.has_value() == s_gu.has_value() && s_o.has_value() == s_down.has_value() &&
                  (!w_qkv.has_value() || s_qkv.has_value() == s_o.has_value()),
              "fp8 chain: every phase's weight needs its scales");
  TORCH_CHECK(!s_o.has_value() || w_tiled, "fp8 chain: tiled fp8 weights only");
  cp.ph[1].p = base_params(h, "h", w_gu, "w_gu", c10::nullopt, "", true, eps, s_gu, w_tiled);
  cp.ph[1].epi = 2;
  const int64_t M = h.size(0);
  cp.ph[0].p = base_params(att, "att", w_o, "w_o", c10::nullopt, "", false, eps, s_o, w_tiled);
  cp.ph[0].epi = 1;
  set_resid(cp.ph[0].p, h);
  check_gpu(act, h, kBF16, "act");
  check_rows_weak(act, "act");
  TORCH_CHECK(att.size(0) == M && act.size(0) == M, "att / act: row counts differ from h's");
  TORCH_CHECK(act.size(1) * 2 == w_gu.size(0) && w_gu.size(0) % 32 == 0, "act must be [M, gate_up rows / 2]");
  cp.ph[1].p.Y = act.data_ptr();
  cp.ph[1].p.ldy = (int)act.stride(0);
  cp.ph[2].p = base_params(act, "act", w_down, "w_down", c10::nullopt, "", false, eps, s_down, w_tiled);
  cp.ph[2].epi = 1;
  set_resid(cp.ph[2].p, h);
  TORCH_CHECK(w_down.size(0) == h.size(1) && w_o.size(0) == h.size(1), "w_down / w_o must have h's columns as rows");
  cp.n = 3;
  cp.seq = 0;
  chain_schedule(cp);
  if (bar.numel() < 640) cp.qkv_flags = 0;  // (the per-group QKV counters live up to u64 word 304)
  if (w_qkv.has_value()) {
    TORCH_CHECK(positions.has_value() && slots.has_value() && q_out.has_value() && k_cache.has_value() &&
                    v_cache.has_value(),
                "the QKV phase needs positions, slots, q_out and the KV caches");
    cp.ph[3].p = base_params(h, "h", *w_qkv, "w_qkv", c10::nullopt, "", true, eps, s_qkv, w_tiled);
    cp.ph[3].epi = 4;
    set_qkv(cp.ph[3].p, check_qkv(h, M, w_qkv->size(0), "w_qkv", n_q_heads, n_kv_heads, head_dim, rope.has_value(),
                                  *positions, *slots, rope, *q_out, *k_cache, *v_cache));
    cp.n = 4;
  }
  if (tp_ar) {
    // tensor parallel (o_proj / down row-parallel): the two phases write this rank's f32 partial
    // rows into its chain regions, the in-launch rounds all-reduce them into h (chain_tp_reduce)
    TORCH_CHECK(vwa_ar_chain_tp(reinterpret_cast<void*>(tp_ar), &cp.tp) == 0, "chain TP: peers not mapped");
    TORCH_CHECK(h.stride(1) == 1 && M * h.size(1) <= cp.tp.region, "chain TP: rows exceed the chain region");
    for (int i : {0, 2}) {
      SkinnyParams& q = cp.ph[i].p;
      q.Y = cp.tp.stage[cp.tp.rank] + (i == 2 ? cp.tp.region : 0);
      q.y_f32 = 1;
      q.ldy = (int)h.size(1);
      q.R = nullptr;
    }
  }
  set_chain_sync(cp, h, bar, work, bar_mode);
  if (ts.has_value()) {
    check_vec(*ts, h, at::kLong, 1024 * 64, "ts");  // (64 stamp slots per workgroup)
    cp.ts = u64p(*ts);
  }
  if (a_q.has_value()) {  // decode attention as the launch's first phase (its output is `att`)
    TORCH_CHECK(a_k && a_v && a_table && a_ctx && a_seq && a_part_o && a_part_ml && a_counters,
                "attention phase: every a_* tensor is required");
    TORCH_CHECK(head_dim == 128 && (n_q_heads / n_kv_heads == 4 || n_q_heads / n_kv_heads == 8) &&
                    n_q_heads % n_kv_heads == 0 && a_q->size(0) == M && M <= 64,
                "attention phase: head_dim 128, GQA group 4 or 8, one query row per chained row");
    check_gpu(*a_q, h, kBF16, "a_q");
    cp.attn = decode_params(*a_q, *a_k, *a_v, *a_table, a_block_size, a_sb, a_sh, a_st, *a_ctx, *a_seq, n_q_heads,
                            n_kv_heads, head_dim, a_scale, a_n_splits, *a_part_o, *a_part_ml, *a_counters, att);
    TORCH_CHECK(a_n_splits > 1, "attention phase: the in-launch chunk merge needs n_splits > 1");
    cp.attn_g = (int)(n_q_heads / n_kv_heads);
    TORCH_CHECK(a_row_table.has_value(), "attention phase: a_row_table (per-row block tables) is required");
    TORCH_CHECK(a_block_size == 16, "attention phase: 16-token KV blocks (mq_attention.h FINE addressing)");
    const Tensor& rtab = *a_row_table;
    check_vec(rtab, h, at::kInt, 0, "a_row_table");
    TORCH_CHECK(rtab.dim() == 2 && rtab.size(0) >= M && rtab.size(1) <= 128 && rtab.size(1) % 2 == 0,
                "a_row_table must be int32 [>= rows, <= 128 (even)] contiguous");
    cp.attn.row_table = rtab.data_ptr<int>();
    cp.attn.rt_stride = (int)rtab.size(1);
    // step plan of the attention partition (mq_attention.h): layer 0 writes it, layers 1.. read it
    if (a_plan_mode) {
      TORCH_CHECK(a_plan_mode == 1 || a_plan_mode == 2, "a_plan_mode: 1 write, 2 read");
      TORCH_CHECK(a_plan.has_value(), "a_plan_mode needs a_plan");
      check_vec(*a_plan, h, at::kInt, (int64_t)chain_grid(h) * 16, "a_plan");
      cp.attn.plan = a_plan->data_ptr<int>();
      cp.attn.plan_mode = (int)a_plan_mode;
    }
  }
  // p_*: the packed form of each phase's bf16 tiled weight (ops.pack_weight: uint8 [blocks x 3328
  // bytes | one flag byte per block], p_base: its exponent base), streamed instead of the weight by
  // the one launch form that decodes it -- attention phase, o_proj in 32-column tiles, one rank;
  // every other form of the chain ignores them and streams the bf16 weights as before
  const bool pk = p_o.has_value() && a_q.has_value() && cp.o_nt2 && !s_o.has_value() && !tp_ar && w_tiled &&
                  w_o.size(0) % 32 == 0;
  if (pk) {
    TORCH_CHECK(p_gu.has_value() && p_down.has_value() && p_qkv.has_value() == w_qkv.has_value() &&
                    (int64_t)p_base.size() == cp.n,
                "packed chain: every phase's weight needs its packed form and base");
    const Tensor* pw[4] = {&*p_o, &*p_gu, &*p_down, w_qkv.has_value() ? &*p_qkv : nullptr};
    for (int i = 0; i < cp.n; ++i) {
      SkinnyParams& q = cp.ph[i].p;
      const int64_t blocks = (int64_t)(q.N / 16) * (q.K / 128);
      check_vec(*pw[i], h, at::kByte, blocks * 3329, "p_* (packed weight)", true);
      TORCH_CHECK(p_base[i] >= 0 && p_base[i] <= 112, "p_base: an exponent base in 0..112");
      q.w_pack = pw[i]->data_ptr<uint8_t>();
      q.w_pack_flag = q.w_pack + blocks * 3328;
      q.w_pack_base = (int)p_base[i];
    }
  }
  for (int i = 0; i < cp.n; ++i) cp.ph[i].p.w_nt = w_nt ? 1 : 0;
  int64_t lds = 0;
  Tensor desc = chain_upload(cp, h, lds);
  if (!desc.numel()) return {desc, 0};
  const bool nt = w_nt && cp.attn_g > 0 && !cp.ph[2].xg && (pk || s_o.has_value() != (cp.o_nt2 != 0));
  // (bit 24 of the returned LDS size: the down phase streams X with the weights, bit 25: fp8
  // weights, bit 26: o_proj in 32-column tiles, bit 28: packed weights, bit 29: nt weight loads --
  // chain_run launches that instantiation)
  return {desc, lds | (cp.n >= 3 && cp.ph[2].xg ? (int64_t)1 << 24 : 0) | (cp.d_nt2 ? (int64_t)1 << 27 : 0) |
                    (s_o.has_value() ? (int64_t)1 << 25 : 0) | (cp.o_nt2 ? (int64_t)1 << 26 : 0) |
                    (pk ? (int64_t)1 << 28 : 0) | (nt ? (int64_t)1 << 29 : 0)};
}

// Whisper decoder chains (skinny_stream.hip chain_kernel SEQ 1 / 2): phase i computes
// Y[i] (=|+=) X[i] . W[i]^T + bias[i] with the epilogue epi[i] (0 store, 1 residual into Y, 3 GELU,
// 4 QKV + self-KV write, no RoPE); ln_c[i] set = LayerNorm folded into W[i] (fuse_rms 2).
std::tuple<Tensor, int64_t> chain_make_seq(int64_t seq, std::vector<Tensor> X, std::vector<Tensor> W,
                                           std::vector<OptTensor> bias, std::vector<OptTensor> ln_c,
                                           std::vector<Tensor> Y, std::vector<int64_t> epi, double eps, int64_t n_heads,
                                           int64_t head_dim, OptTensor positions, OptTensor slots, OptTensor k_cache,
                                           OptTensor v_cache, Tensor bar, Tensor work, int64_t bar_mode, bool w_tiled) {
  const size_t n = X.size();
  TORCH_CHECK(n >= 2 && n <= (size_t)kChainMaxPhases && W.size() == n && bias.size() == n && ln_c.size() == n &&
                  Y.size() == n && epi.size() == n,
              "chain_make_seq: one X/W/bias/ln_c/Y/epi per phase");
  TORCH_CHECK(seq == 1 || seq == 2, "chain_make_seq: seq 1 (Whisper tail) or 2 (Whisper middle)");
  const Tensor& a = X[0];
  c10::DeviceGuard g(a.device());
  check_anchor(a, "X");
  ChainParams cp{};
  set_chain_sync(cp, a, bar, work, bar_mode);
  for (size_t i = 0; i < n; ++i) {
    check_gpu(X[i], a, kBF16, "X");
    SkinnyParams& p = cp.ph[i].p;
    p = base_params(X[i], "X", W[i], "W", bias[i], "bias", false, eps, c10::nullopt, w_tiled);
    cp.ph[i].epi = (int)epi[i];
    set_ln_fold(p, a, ln_c[i], (int)epi[i]);
    TORCH_CHECK(p.M == cp.ph[0].p.M && Y[i].dim() == 2 && Y[i].size(0) == p.M, "X / Y: row counts differ");
    if (epi[i] == 4) {
      TORCH_CHECK(positions && slots && k_cache && v_cache, "the QKV phase needs positions, slots and the KV caches");
      set_qkv(p, check_qkv(a, p.M, p.N, "W", n_heads, n_heads, head_dim, false, *positions, *slots, c10::nullopt, Y[i],
                           *k_cache, *v_cache, "Y"));
      continue;
    }
    check_gpu(Y[i], a, kBF16, "Y");
    check_rows_weak(Y[i], "Y");
    TORCH_CHECK(Y[i].size(1) == p.N, "Y must be [M, N] rows");
    if (epi[i] == 1) {
      set_resid(p, Y[i]);
    } else {
      p.Y = Y[i].data_ptr();
      p.ldy = (int)Y[i].stride(0);
    }
  }
  cp.n = (int)n;
  cp.seq = (int)seq;
  cp.pre2 = 1;  // (the Llama schedule without its attention-phase and LDS-item parts)
  cp.next0 = 1;
  cp.xdma = 1;
  cp.osub = 1;
  int64_t lds = 0;
  Tensor desc = chain_upload(cp, a, lds);
  return {desc, lds};
}

// n_layers > 1: desc holds n_layers consecutive descriptors (torch.cat of chain_make outputs of
// consecutive layers, same flags) run by ONE launch (skinny_stream.hip chain_kernel MULTI)
void chain_run(Tensor desc, int64_t n_phases, int64_t lds, Tensor like, int64_t attn_g, int64_t seq, int64_t n_layers) {
  c10::DeviceGuard g(like.device());
  check_anchor(like, "like");
  check_vec(desc, like, at::kByte, 0, "desc");
  TORCH_CHECK(n_layers >= 1 && desc.numel() == n_layers * (int64_t)sizeof(ChainParams) && aligned(desc, 64),
              "desc: bad chain descriptor (n_layers x sizeof(ChainParams) bytes, 64-byte aligned)");
  // one workgroup per CU: the barrier needs every workgroup resident
  check_rc(vwa_chain_launch(reinterpret_cast<const ChainParams*>(desc.data_ptr()), (int)seq, (int)n_phases, (int)attn_g,
                            (int)(lds & 0xFFFFFF), chain_grid(like), cur_stream(like),
                            (int)((lds >> 24) & 1) * (((lds >> 27) & 1) ? 2 : 1), (int)((lds >> 25) & 1),
                            (int)((lds >> 26) & 1), (int)n_layers, (int)((lds >> 28) & 1), (int)((lds >> 29) & 1) * 2),
           "chain");
}

// One-row device-resident decode loop step (see elementwise.hip decode_advance_kernel)
void decode_advance(Tensor tokens, Tensor positions, Tensor ctx_lens, Tensor slots, Tensor sampled, Tensor out,
                    Tensor counter, int64_t base_block, int64_t block_size) {
  c10::DeviceGuard g(tokens.device());
  check_vec(tokens, tokens, at::kInt, 1, "tokens");
  check_vec(positions, tokens, at::kInt, 1, "positions");
  check_vec(ctx_lens, tokens, at::kInt, 1, "ctx_lens");
  check_vec(slots, tokens, at::kLong, 1, "slots");
  check_vec(sampled, tokens, at::kInt, 1, "sampled");
  check_vec(out, tokens, at::kInt, 1, "out");
  check_vec(counter, tokens, at::kInt, 1, "counter");
  TORCH_CHECK(block_size > 0 && base_block >= 0, "bad block geometry");
  check_rc(vwa_decode_advance(tokens.data_ptr<int>(), positions.data_ptr<int>(), ctx_lens.data_ptr<int>(),
                              slots.data_ptr<int64_t>(), sampled.data_ptr<int>(), out.data_ptr<int>(),
                              counter.data_ptr<int>(), (int)out.numel(), (int)base_block, (int)block_size,
                              cur_stream(tokens)),
           "decode_advance");
}

// Device memory the L2 does not cache (hipDeviceMallocUncached): chain barrier words polled with
// scalar loads.  Returned as an int32 tensor whose deleter DEFERS the hipFree to the next
// allocation: the tensor may die in a garbage collection that runs inside another model's graph
// capture, where a hipFree is not permitted (seen: the whole process aborted in the GC of an
// earlier test's model during the next test's capture).
std::mutex g_uncached_mu;
std::vector<void*> g_uncached_pending;

Tensor alloc_uncached_i32(int64_t n, Tensor like) {
  check_anchor(like, "like");
  TORCH_CHECK(n >= 1, "n must be positive");
  c10::DeviceGuard g(like.device());
  {
    std::lock_guard<std::mutex> lk(g_uncached_mu);
    for (void* p : g_uncached_pending) (void)hipFree(p);
    g_uncached_pending.clear();
  }
  void* ptr = nullptr;
  TORCH_CHECK(hipExtMallocWithFlags(&ptr, (size_t)n * 4, hipDeviceMallocUncached) == hipSuccess, "uncached malloc");
  TORCH_CHECK(hipMemset(ptr, 0, (size_t)n * 4) == hipSuccess, "memset");
  return torch::from_blob(ptr, {n}, [](void* p) {
        std::lock_guard<std::mutex> lk(g_uncached_mu);
        g_uncached_pending.push_back(p);
      }, torch::dtype(torch::kInt).device(like.device()));
}

// ---- persistent Whisper decoder (whisper_dec.hip): per-layer descriptors from a flat list of
// 3 kWdGemms + 4 tensors per layer -- (W, bias, ln_c) of each WdecLayer::g (pre-tiled bf16 weights;
// bias / ln_c may be None), then k_cache, v_cache, cross K, cross V.
Tensor wdec_layers(std::vector<OptTensor> flat, int64_t n_layers, Tensor like) {
  constexpr int kPer = 3 * kWdGemms + 4;
  check_anchor(like, "like");
  TORCH_CHECK(n_layers >= 1 && (int64_t)flat.size() == n_layers * kPer, "flat: 3 kWdGemms + 4 entries per layer");
  auto ptr = [&](int64_t i, at::ScalarType dt, bool need) -> void* {
    const auto& t = flat[(size_t)i];
    const std::string name = "flat[" + std::to_string(i) + "]";
    TORCH_CHECK(t.has_value() || !need, name, " is required");
    if (!t.has_value()) return nullptr;
    check_vec(*t, like, dt, 0, name.c_str());
    return t->data_ptr();
  };
  Tensor host = torch::zeros({n_layers * (int64_t)sizeof(WdecLayer)}, torch::dtype(torch::kUInt8));
  auto* L = reinterpret_cast<WdecLayer*>(host.data_ptr());
  for (int64_t li = 0; li < n_layers; ++li) {
    const int64_t b = li * kPer;
    for (int g = 0; g < kWdGemms; ++g) {
      L[li].g[g].W = static_cast<const uint16_t*>(ptr(b + 3 * g, kBF16, true));
      L[li].g[g].bias = static_cast<const uint16_t*>(ptr(b + 3 * g + 1, kBF16, false));
      L[li].g[g].ln_c = static_cast<const float*>(ptr(b + 3 * g + 2, at::kFloat, false));
    }
    constexpr int c0 = 3 * kWdGemms;
    L[li].k_cache = static_cast<uint16_t*>(ptr(b + c0, kBF16, true));
    L[li].v_cache = static_cast<uint16_t*>(ptr(b + c0 + 1, kBF16, true));
    L[li].xk = static_cast<const uint16_t*>(ptr(b + c0 + 2, kBF16, true));
    L[li].xv = static_cast<const uint16_t*>(ptr(b + c0 + 3, kBF16, true));
  }
  return host.to(like.device());
}

// bufs: x0, x1, q, att, f, xpart, seq_ids, ctx_lens, slots, block_table, cross_table, cnt
// ints: n_layers, d, H, ffn, T, block_size, bt_stride, nch, ch_len, sessions, grid
// lm (optional): [W pre-tiled bf16 [V, d], bias bf16 [V] or None-as-empty, column sums f32 [V], logits f32 [>= V]]
// emb (optional): [tok_emb bf16 [rows, d], pos_emb bf16 [>= max position + 1, d], tokens int32, positions int32]
// smp (optional, needs lm): [mask u32-as-int32 [>= V / 32], out_tok int32, step int32, part f32 [2 grid],
//   loop_out int32, loop_cnt int32, adv_tokens, adv_positions, adv_ctx int32, adv_slots int64]
void wdec_run(Tensor layers, Tensor roles, std::vector<Tensor> bufs, std::vector<int64_t> ints, double eps,
              double scale, std::vector<int64_t> n_prod, OptTensor ts, int64_t opt,
              c10::optional<std::vector<Tensor>> lm, c10::optional<std::vector<Tensor>> emb,
              c10::optional<std::vector<Tensor>> smp, int64_t loop_base_block) {
  TORCH_CHECK(bufs.size() == 12 && ints.size() == 11 && n_prod.size() == kWdLevels, "wdec_run: argument counts");
  const Tensor& like = bufs[0];
  c10::DeviceGuard g(like.device());
  const int64_t grid = ints[10];
  WdecParams p{};
  p.n_layers = (int)ints[0];
  p.d = (int)ints[1];
  p.H = (int)ints[2];
  p.ffn = (int)ints[3];
  p.T = (int)ints[4];
  p.block_size = (int)ints[5];
  p.bt_stride = (int)ints[6];
  p.nch = (int)ints[7];
  p.ch_len = (int)ints[8];
  p.sessions = (int)ints[9];
  p.eps = (float)eps;
  p.scale = (float)scale;
  // (one hidden row each; xpart: cross partials + the cross query's two f32 halves + x1 tile sums; cnt,
  // uncached: levels, error word, sampler counters at u64 1152..1279, per-head QKV counters)
  check_slots(bufs, like, "bufs",
              {{0, kBF16, p.d}, {1, kBF16, p.d}, {2, kBF16, p.d}, {3, kBF16, p.d}, {4, kBF16, p.ffn},
               {5, at::kFloat, (int64_t)p.H * p.nch * 68 + 3 * p.d}, {6, at::kInt, 1}, {7, at::kInt, 1},
               {8, at::kLong, 1}, {9, at::kInt, p.bt_stride}, {10, at::kInt, 1},
               {11, at::kInt, 2 * (1280 + 16 * (int64_t)p.H)}});
  check_vec(layers, like, at::kByte, p.n_layers * (int64_t)sizeof(WdecLayer), "layers", true);
  check_vec(roles, like, at::kInt, grid * kWdRole, "roles", true);
  p.layers = reinterpret_cast<const WdecLayer*>(layers.data_ptr());
  p.roles = roles.data_ptr<int>();
  p.x0 = bfp_mut(bufs[0]);
  p.x1 = bfp_mut(bufs[1]);
  p.q = bfp_mut(bufs[2]);
  p.att = bfp_mut(bufs[3]);
  p.f = bfp_mut(bufs[4]);
  p.xpart = bufs[5].data_ptr<float>();
  p.seq_ids = bufs[6].data_ptr<int>();
  p.ctx_lens = bufs[7].data_ptr<int>();
  p.slots = bufs[8].data_ptr<int64_t>();
  p.block_table = bufs[9].data_ptr<int>();
  p.cross_table = bufs[10].data_ptr<int>();
  p.cnt = reinterpret_cast<unsigned long long*>(bufs[11].data_ptr());
  for (int l = 0; l < kWdLevels; ++l) {
    TORCH_CHECK(n_prod[(size_t)l] > 0, "n_prod: every level needs a producer");
    p.n_prod[l] = (int)n_prod[(size_t)l];
  }
  if (ts.has_value()) {
    check_vec(*ts, like, at::kLong, grid * ints[0] * kWdLevels * 4, "ts");  // [grid * n_layers * 8 * 4]
    p.ts = u64p(*ts);
  }
  p.opt[0] = (int)opt;
  if (lm.has_value()) {
    const std::vector<Tensor>& L = *lm;
    TORCH_CHECK(L.size() == 4 && L[0].dim() == 2 && L[0].size(1) == p.d && L[0].size(0) % 16 == 0,
                "lm = [W [V % 16 == 0, d] (pre-tiled), bias, ln_c, logits]");
    const int64_t V = L[0].size(0);
    check_slots(L, like, "lm", {{0, kBF16, V * p.d}, {2, at::kFloat, V}, {3, at::kFloat, V}});
    TORCH_CHECK(L[2].numel() == V, "lm[2] (ln_c) must be [V]");
    p.lm_W = bfp(L[0]);
    if (L[1].numel()) {
      check_vec(L[1], like, kBF16, V, "lm[1]", true);
      p.lm_b = bfp(L[1]);
    }
    p.lm_c = L[2].data_ptr<float>();
    p.logits = L[3].data_ptr<float>();
    p.n_vocab = (int)V;
  }
  if (emb.has_value()) {
    const std::vector<Tensor>& Em = *emb;
    TORCH_CHECK(Em.size() == 4, "emb = [tok_emb, pos_emb, tokens, positions]");
    check_slots(Em, like, "emb", {{0, kBF16, p.d}, {1, kBF16, p.d}, {2, at::kInt, 1}, {3, at::kInt, 1}});
    TORCH_CHECK(Em[0].dim() == 2 && Em[0].size(1) == p.d && Em[1].dim() == 2 && Em[1].size(1) == p.d,
                "emb[0] / emb[1]: embedding tables [rows, d] contiguous");
    TORCH_CHECK(p.block_size > 0 && Em[1].size(0) >= (int64_t)p.bt_stride * p.block_size,
                "emb[1]: the position table covers every KV position");
    p.tok_emb = bfp(Em[0]);
    p.pos_emb = bfp(Em[1]);
    p.tokens = Em[2].data_ptr<int>();
    p.positions = Em[3].data_ptr<int>();
    p.emb_rows = (int)Em[0].size(0);
  }
  if (smp.has_value()) {
    const std::vector<Tensor>& S = *smp;
    TORCH_CHECK(S.size() == 10 && p.lm_W, "smp = 10 tensors, with the LM head");
    check_slots(S, like, "smp",
                {{0, at::kInt, (p.n_vocab + 31) / 32}, {1, at::kInt, 1}, {2, at::kInt, 1}, {3, at::kFloat, 2 * grid},
                 {4, at::kInt, 1}, {5, at::kInt, 1}, {6, at::kInt, 1}, {7, at::kInt, 1}, {8, at::kInt, 1},
                 {9, at::kLong, 1}});
    p.smp_mask = reinterpret_cast<const uint32_t*>(S[0].data_ptr());
    p.smp_tok = S[1].data_ptr<int>();
    p.smp_step = S[2].data_ptr<int>();
    p.smp_part = S[3].data_ptr<float>();
    p.loop_out = S[4].data_ptr<int>();
    p.loop_max = (int)S[4].numel();
    p.loop_cnt = S[5].data_ptr<int>();
    p.adv_tokens = S[6].data_ptr<int>();
    p.adv_positions = S[7].data_ptr<int>();
    p.adv_ctx = S[8].data_ptr<int>();
    p.adv_slots = S[9].data_ptr<int64_t>();
    p.loop_base_block = (int)loop_base_block;
  }
  check_rc(vwa_wdec_launch(&p, (int)grid, cur_stream(like)), "wdec");
}

// ---- norms / elementwise
// optional residual in, updated residual out: both bf16, contiguous, like x
void check_residual_pair(const Tensor& x, const OptTensor& residual, const OptTensor& residual_out) {
  if (!residual.has_value()) return;
  TORCH_CHECK(residual_out.has_value(), "residual needs residual_out");
  check_vec(*residual, x, kBF16, 0, "residual");
  check_vec(*residual_out, x, kBF16, 0, "residual_out");
  TORCH_CHECK(residual->sizes() == x.sizes() && residual_out->sizes() == x.sizes(), "residual / residual_out shapes");
}

void rmsnorm(Tensor x, OptTensor residual, OptTensor residual_out, OptTensor w, Tensor y, double eps) {
  c10::DeviceGuard g(x.device());
  check_gpu(x, x, kBF16, "x");
  check_rows(x, "x");
  check_vec(y, x, kBF16, 0, "y");
  TORCH_CHECK(y.sizes() == x.sizes(), "y shape");
  check_residual_pair(x, residual, residual_out);
  if (w.has_value()) check_vec(*w, x, kBF16, x.size(1), "w", true);
  check_rc(vwa_rmsnorm(bfp(x), bfp_opt(residual), bfp_mut_opt(residual_out), bfp_opt(w), bfp_mut(y), (int)x.size(0),
                       (int)x.size(1), (int)x.stride(0), (float)eps, cur_stream(x)),
           "rmsnorm");
}

void layernorm(Tensor x, OptTensor residual, OptTensor residual_out, Tensor w, Tensor b, Tensor y, double eps) {
  c10::DeviceGuard g(x.device());
  check_gpu(x, x, kBF16, "x");
  check_rows(x, "x");
  check_vec(y, x, kBF16, 0, "y");
  TORCH_CHECK(y.sizes() == x.sizes(), "y shape");
  check_vec(w, x, kBF16, x.size(1), "w", true);
  check_vec(b, x, kBF16, x.size(1), "b", true);
  check_residual_pair(x, residual, residual_out);
  check_rc(vwa_layernorm(bfp(x), bfp_opt(residual), bfp_mut_opt(residual_out), bfp(w), bfp(b), bfp_mut(y),
                         (int)x.size(0), (int)x.size(1), (int)x.stride(0), (float)eps, cur_stream(x)),
           "layernorm");
}

void rope_kv_write(Tensor qkv, int64_t n_q_heads, int64_t n_kv_heads, int64_t head_dim, bool use_rope, Tensor positions,
                   Tensor slots, OptTensor rope, Tensor q_out, Tensor k_cache, Tensor v_cache) {
  c10::DeviceGuard g(qkv.device());
  check_gpu(qkv, qkv, kBF16, "qkv");
  check_rows_weak(qkv, "qkv");
  const int rows = (int)qkv.size(0);
  const QkvOperands q = check_qkv(qkv, rows, qkv.size(1), "qkv columns", n_q_heads, n_kv_heads, head_dim, use_rope,
                                  positions, slots, rope, q_out, k_cache, v_cache);
  check_rc(vwa_rope_kv_write(bfp(qkv), (int)qkv.stride(0), rows, q.n_q_heads, q.n_kv_heads, q.head_dim, q.use_rope,
                             q.positions, q.slots, q.rope, q.q_out, q.ldq, q.k_cache, q.v_cache, q.block_size, q.sb,
                             q.sh, q.st, cur_stream(qkv)),
           "rope_kv_write");
}

void swiglu(Tensor gu, Tensor h) {
  c10::DeviceGuard g(gu.device());
  check_vec(gu, gu, kBF16, 0, "gu");
  check_vec(h, gu, kBF16, 0, "h");
  TORCH_CHECK(gu.dim() == 2 && h.dim() == 2 && gu.size(0) == h.size(0) && gu.size(1) == 2 * h.size(1),
              "swiglu shapes: gu [rows, 2 F], h [rows, F]");
  check_rc(vwa_swiglu(bfp(gu), bfp_mut(h), (int)h.size(0), (int)h.size(1), cur_stream(gu)), "swiglu");
}

void bias_act(Tensor x, OptTensor bias, OptTensor residual, Tensor y, int64_t act) {
  c10::DeviceGuard g(x.device());
  check_vec(x, x, kBF16, 0, "x");
  check_vec(y, x, kBF16, 0, "y");
  TORCH_CHECK(x.dim() == 2 && y.sizes() == x.sizes(), "bias_act shapes: x, y [rows, N]");
  if (bias.has_value()) check_vec(*bias, x, kBF16, x.size(1), "bias", true);
  if (residual.has_value()) {
    check_vec(*residual, x, kBF16, 0, "residual");
    TORCH_CHECK(residual->sizes() == x.sizes(), "residual shape");
  }
  check_rc(vwa_bias_act(bfp(x), bfp_opt(bias), bfp_opt(residual), bfp_mut(y), (int)x.size(0), (int)x.size(1),
                        (int)act, cur_stream(x)),
           "bias_act");
}

void embedding(Tensor ids, Tensor table, OptTensor pos_table, OptTensor positions, Tensor out, int64_t vocab_start) {
  c10::DeviceGuard g(ids.device());
  check_gpu(ids, ids, at::kInt, "ids");
  check_vec(table, ids, kBF16, 0, "table");
  check_vec(out, ids, kBF16, 0, "out");
  TORCH_CHECK(table.dim() == 2 && out.dim() == 2 && out.size(1) == table.size(1),
              "embedding shapes: out [rows, D], table [V, D]");
  const int rows = (int)out.size(0);
  check_vec(ids, ids, at::kInt, rows, "ids");
  if (pos_table.has_value()) {
    check_vec(*pos_table, ids, kBF16, 0, "pos_table");
    TORCH_CHECK(pos_table->dim() == 2 && pos_table->size(1) == table.size(1), "pos_table must be [positions, D]");
    TORCH_CHECK(positions.has_value(), "pos_table needs positions");
  }
  if (positions.has_value()) check_vec(*positions, ids, at::kInt, rows, "positions");
  check_rc(vwa_embedding(ids.data_ptr<int>(), bfp(table), bfp_opt(pos_table), ptr_opt<int>(positions), bfp_mut(out),
                         rows, (int)table.size(1), (int)vocab_start, (int)(vocab_start + table.size(0)),
                         cur_stream(ids)),
           "embedding");
}

// ---- sampling
struct SampleArgs {
  int rows = 0, V = 0, mask_words = 0;
  const uint32_t* mask = nullptr;
  const float* temperature = nullptr;
  const int64_t* fail = nullptr;
};

// logits is the anchor
SampleArgs check_sample(const Tensor& logits, const OptTensor& mask, const OptTensor& temperature, const Tensor& seed,
                        const Tensor& step, const Tensor& out_tokens, const OptTensor& fail_word, int64_t v_offset) {
  check_gpu(logits, logits, at::kFloat, "logits");
  check_rows_weak(logits, "logits");
  SampleArgs a;
  a.rows = (int)logits.size(0);
  a.V = (int)logits.size(1);
  TORCH_CHECK(a.rows >= 1, "logits has no rows");
  TORCH_CHECK(v_offset >= 0 && v_offset % 32 == 0, "v_offset must be a non-negative multiple of 32");
  if (mask.has_value()) {
    // (pinned host rows allowed: zero-copy grammar masks)
    check_gpu_or_pinned(*mask, logits, at::kInt, "mask");
    TORCH_CHECK(mask->dim() == 2 && mask->is_contiguous() && mask->size(0) >= a.rows,
                "mask must be int32 [rows, words]");
    a.mask_words = (int)mask->size(1);
    TORCH_CHECK((int64_t)a.mask_words * 32 >= v_offset + a.V, "mask too short");
    a.mask = reinterpret_cast<const uint32_t*>(mask->data_ptr<int>());
  }
  if (temperature.has_value()) check_vec(*temperature, logits, at::kFloat, a.rows, "temperature");
  a.temperature = ptr_opt<float>(temperature);
  check_vec(seed, logits, at::kLong, 1, "seed");
  check_vec(step, logits, at::kInt, 1, "step");
  check_gpu_or_pinned(out_tokens, logits, at::kInt, "out_tokens");
  TORCH_CHECK(out_tokens.is_contiguous() && out_tokens.numel() >= a.rows, "out_tokens must be contiguous [>= rows]");
  if (fail_word.has_value()) check_vec(*fail_word, logits, at::kLong, 1, "fail_word");
  a.fail = ptr_opt<int64_t>(fail_word);
  return a;
}

void sample(Tensor logits, OptTensor mask, OptTensor temperature, Tensor seed, Tensor step, Tensor out_tokens,
            Tensor part_val, Tensor part_idx, OptTensor fail_word, int64_t v_offset) {
  c10::DeviceGuard g(logits.device());
  const SampleArgs a = check_sample(logits, mask, temperature, seed, step, out_tokens, fail_word, v_offset);
  check_vec(part_val, logits, at::kFloat, a.rows, "part_val");
  const int n_chunks = (int)(part_val.numel() / a.rows);
  check_vec(part_idx, logits, at::kInt, (int64_t)a.rows * n_chunks, "part_idx");
  hipStream_t st = cur_stream(logits);
  check_rc(vwa_sample_partial(logits.data_ptr<float>(), (int)logits.stride(0), a.rows, a.V, (int)v_offset, a.mask,
                              a.mask_words, a.temperature, reinterpret_cast<const uint64_t*>(seed.data_ptr<int64_t>()),
                              step.data_ptr<int>(), part_val.data_ptr<float>(), part_idx.data_ptr<int>(), n_chunks, st),
           "sample (partial)");
  check_rc(vwa_sample_final(part_val.data_ptr<float>(), part_idx.data_ptr<int>(), n_chunks, 1, 0,
                            out_tokens.data_ptr<int>(), step.data_ptr<int>(), a.rows, a.fail, st),
           "sample (final)");
}

// Vocab-parallel sampling (SURVEY.md §2.8 C4 as [B, 2] per rank): partial maxima over this rank's
// logits shard (global ids from v_offset) into xin = [val f32 | idx i32] x [rows][n_chunks], the
// one-shot IPC all-gather of xin over the TP group, then every rank merges all ranks' partials in
// rank order -- bit-identical tokens on every rank, and the same token a TP=1 sampler draws
// (the Gumbel noise and the tie-break use global token ids).  Three launches, no host sync.
void sample_tp(Tensor logits, OptTensor mask, OptTensor temperature, Tensor seed, Tensor step, Tensor out_tokens,
               Tensor xin, Tensor xout, int64_t n_chunks, OptTensor fail_word, int64_t v_offset, int64_t ar_state,
               int64_t world) {
  c10::DeviceGuard g(logits.device());
  const SampleArgs a = check_sample(logits, mask, temperature, seed, step, out_tokens, fail_word, v_offset);
  const int64_t words = 2 * (int64_t)a.rows * n_chunks;
  TORCH_CHECK(n_chunks >= 1 && n_chunks <= 1024, "n_chunks");
  TORCH_CHECK(world >= 1 && world <= 8 && ar_state != 0, "TP group state");
  TORCH_CHECK(words <= vwa_ar_gather_max_words(), "sampler partials exceed the all-gather region");
  check_vec(xin, logits, at::kInt, words, "xin");  // [>= 2 * rows * n_chunks]
  check_vec(xout, logits, at::kInt, world * words, "xout");
  hipStream_t st = cur_stream(logits);
  int* in = xin.data_ptr<int>();
  check_rc(vwa_sample_partial(logits.data_ptr<float>(), (int)logits.stride(0), a.rows, a.V, (int)v_offset, a.mask,
                              a.mask_words, a.temperature, reinterpret_cast<const uint64_t*>(seed.data_ptr<int64_t>()),
                              step.data_ptr<int>(), reinterpret_cast<float*>(in), in + a.rows * n_chunks,
                              (int)n_chunks, st),
           "sample_tp (partial)");
  int* out = xout.data_ptr<int>();
  check_rc(vwa_ar_gather(reinterpret_cast<void*>(ar_state), in, out, words, st), "sample_tp (all-gather)");
  check_rc(vwa_sample_final(reinterpret_cast<const float*>(out), out + a.rows * n_chunks, (int)n_chunks, (int)world,
                            words, out_tokens.data_ptr<int>(), step.data_ptr<int>(), a.rows, a.fail, st),
           "sample_tp (merge)");
}

// ---- audio
void pcm16_to_f32(Tensor pcm, Tensor out, double ratio) {
  c10::DeviceGuard g(pcm.device());
  check_vec(pcm, pcm, at::kShort, 0, "pcm");
  check_vec(out, pcm, at::kFloat, 0, "out");
  const int n_in = (int)pcm.numel(), n_out = (int)out.numel();
  TORCH_CHECK((int64_t)((n_out - 1) * ratio) < (int64_t)n_in + 1, "resample ratio overruns input");
  check_rc(vwa_pcm16_to_f32(pcm.data_ptr<int16_t>(), out.data_ptr<float>(), n_in, n_out, ratio, cur_stream(pcm)),
           "pcm16_to_f32");
}

// basis: DFT fragments [26][25][64][4] f32, fb_frag: mel filterbank fragments [n_mels/16][13][64][4] f32
// (ops.logmel_tables); window: n_fft = 400
void log_mel(Tensor audio, int64_t n_frames, Tensor window, Tensor basis, Tensor fb_frag, int64_t n_mels,
             Tensor mel_scratch, Tensor max_buf, Tensor out) {
  c10::DeviceGuard g(audio.device());
  TORCH_CHECK(n_mels >= 1 && n_mels <= 128, "n_mels <= 128");
  check_vec(audio, audio, at::kFloat, 201, "audio");
  check_vec(window, audio, at::kFloat, 400, "window", true);
  check_vec(basis, audio, at::kFloat, 26 * 25 * 64 * 4, "basis", true);
  check_vec(fb_frag, audio, at::kFloat, (n_mels + 15) / 16 * 13 * 64 * 4, "fb_frag", true);
  check_vec(mel_scratch, audio, at::kFloat, n_frames * n_mels, "mel_scratch");
  check_vec(max_buf, audio, at::kFloat, 1, "max_buf");
  check_gpu(out, audio, kBF16, "out");
  check_rows_weak(out, "out");
  TORCH_CHECK(out.size(0) >= n_frames && out.size(1) == n_mels, "out must be bf16 [>= frames, n_mels]");
  check_rc(vwa_log_mel(audio.data_ptr<float>(), (int)audio.numel(), (int)n_frames, window.data_ptr<float>(),
                       basis.data_ptr<float>(), fb_frag.data_ptr<float>(), (int)n_mels, mel_scratch.data_ptr<float>(),
                       max_buf.data_ptr<float>(), bfp_mut(out), (int)out.stride(0), cur_stream(audio)),
           "log_mel");
}

// ---- one-shot all-reduce (opaque state handle as int64)
// TP preflight (parallel/custom_ar.py): may device `dev` map device `peer`'s memory (xGMI P2P)?
// -1 when either index is not visible to this process
int64_t can_access_peer(int64_t dev, int64_t peer) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || dev < 0 || peer < 0 || dev >= n || peer >= n) return -1;
  if (dev == peer) return 1;
  int ok = 0;
  if (hipDeviceCanAccessPeer(&ok, (int)dev, (int)peer) != hipSuccess) return -1;
  return ok;
}

// PCI location "domain:bus:device" of a visible device (a stable id across processes' masks)
std::string pci_id(int64_t dev) {
  char buf[64] = {0};
  if (hipDeviceGetPCIBusId(buf, (int)sizeof(buf), (int)dev) != hipSuccess) return "";
  return std::string(buf);
}

int64_t ar_create(int64_t rank, int64_t world, int64_t max_elems) {
  void* st = vwa_ar_create((int)rank, (int)world, max_elems);
  TORCH_CHECK(st, "all-reduce buffer allocation failed (world <= 8, max_elems % 512 == 0)");
  return reinterpret_cast<int64_t>(st);
}
Tensor ar_handles(int64_t st) {
  Tensor t = torch::empty({vwa_ar_handle_bytes()}, torch::dtype(torch::kUInt8));
  check_rc(vwa_ar_handles(reinterpret_cast<void*>(st), t.data_ptr()), "hipIpcGetMemHandle");
  return t;
}
void ar_open_peer(int64_t st, int64_t p, Tensor h) {
  TORCH_CHECK(h.scalar_type() == at::kByte && h.numel() == vwa_ar_handle_bytes() && !h.is_cuda(), "ipc handle bytes");
  check_rc(vwa_ar_open_peer(reinterpret_cast<void*>(st), (int)p, h.contiguous().data_ptr()), "hipIpcOpenMemHandle");
}
void ar_allreduce(int64_t st, Tensor in, Tensor out) {
  c10::DeviceGuard g(in.device());
  check_vec(in, in, kBF16, 0, "in");
  check_vec(out, in, kBF16, in.numel(), "out", true);
  check_rc(vwa_ar_allreduce(reinterpret_cast<void*>(st), bfp(in), bfp_mut(out), in.numel(), cur_stream(in)),
           "one-shot all-reduce");
}
void ar_gather(int64_t st, Tensor in, Tensor out) {
  c10::DeviceGuard g(in.device());
  check_vec(in, in, at::kInt, 1, "in");
  check_vec(out, in, at::kInt, in.numel(), "out");
  TORCH_CHECK(out.numel() % in.numel() == 0 && in.numel() <= vwa_ar_gather_max_words(),
              "ar_gather: int32 in [n], out [world * n] on the GPU");
  check_rc(vwa_ar_gather(reinterpret_cast<void*>(st), in.data_ptr<int>(), out.data_ptr<int>(), in.numel(),
                         cur_stream(in)),
           "one-shot all-gather");
}
int64_t ar_error(int64_t st) { return vwa_ar_error(reinterpret_cast<void*>(st)); }
void ar_destroy(int64_t st) { vwa_ar_destroy(reinterpret_cast<void*>(st)); }

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quant_fp8_rows", &quant_fp8_rows, py::arg("x"), py::arg("q"), py::arg("scale"),
        py::arg("rstd") = py::none(), py::arg("eps") = 1e-5);
  m.def("can_access_peer", &can_access_peer);
  m.def("pci_id", &pci_id);
  m.def("ar_create", &ar_create);
  m.def("ar_handles", &ar_handles);
  m.def("ar_open_peer", &ar_open_peer);
  m.def("ar_allreduce", &ar_allreduce);
  m.def("ar_gather", &ar_gather);
  m.def("ar_error", &ar_error);
  m.def("ar_destroy", &ar_destroy);
  m.doc() = "MI355X (gfx950) HIP kernels for the voice-web-agent inference engine";
  m.def("skinny_gemm", &skinny_gemm, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("epi"),
        py::arg("fuse_rms"), py::arg("eps"), py::arg("residual"), py::arg("w_scale") = py::none(),
        py::arg("ln_c") = py::none(), py::arg("w_tiled") = false, py::arg("col_mask") = py::none(),
        py::arg("col_mask_off") = 0, py::arg("mask_rows") = 1, py::arg("w_nt") = false);
  m.def("skinny_gemm_swiglu", &skinny_gemm_swiglu, py::arg("x"), py::arg("w_gu"), py::arg("bias"), py::arg("h"),
        py::arg("fuse_rms"), py::arg("eps"), py::arg("w_scale") = py::none(), py::arg("w_tiled") = false,
        py::arg("w_nt") = false);
  m.def("skinny_gemm_qkv", &skinny_gemm_qkv, py::arg("x"), py::arg("w_qkv"), py::arg("bias"), py::arg("fuse_rms"),
        py::arg("eps"), py::arg("n_q_heads"), py::arg("n_kv_heads"), py::arg("head_dim"), py::arg("use_rope"),
        py::arg("positions"), py::arg("slots"), py::arg("rope"), py::arg("q_out"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("w_scale") = py::none(), py::arg("ln_c") = py::none(),
        py::arg("w_tiled") = false, py::arg("w_nt") = false);
  m.def("chain_make", &chain_make, py::arg("h"), py::arg("att"), py::arg("act"), py::arg("w_o"), py::arg("w_gu"),
        py::arg("w_down"), py::arg("eps"), py::arg("w_qkv"), py::arg("n_q_heads"), py::arg("n_kv_heads"),
        py::arg("head_dim"), py::arg("positions"), py::arg("slots"), py::arg("rope"), py::arg("q_out"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("bar"), py::arg("work"), py::arg("ts") = py::none(), py::arg("bar_mode") = 1,
        py::arg("a_q") = py::none(), py::arg("a_k") = py::none(), py::arg("a_v") = py::none(),
        py::arg("a_table") = py::none(), py::arg("a_block_size") = 0, py::arg("a_sb") = 0, py::arg("a_sh") = 0,
        py::arg("a_st") = 0, py::arg("a_ctx") = py::none(), py::arg("a_seq") = py::none(), py::arg("a_scale") = 0.0,
        py::arg("a_n_splits") = 0, py::arg("a_part_o") = py::none(), py::arg("a_part_ml") = py::none(),
        py::arg("a_counters") = py::none(), py::arg("w_tiled") = false, py::arg("a_row_table") = py::none(),
        py::arg("s_o") = py::none(), py::arg("s_gu") = py::none(), py::arg("s_down") = py::none(),
        py::arg("s_qkv") = py::none(), py::arg("tp_ar") = 0, py::arg("a_plan") = py::none(), py::arg("a_plan_mode") = 0,
        py::arg("p_o") = py::none(), py::arg("p_gu") = py::none(), py::arg("p_down") = py::none(),
        py::arg("p_qkv") = py::none(), py::arg("p_base") = std::vector<int64_t>{}, py::arg("w_nt") = false);
  m.def("set_small_gemm_bytes", &set_small_gemm_bytes);
  m.def("gemm_set_p8", [](int64_t mode) { vwa_gemm_set_p8((int)mode); });
  m.def("skinny_set_x_skew", [](int64_t skew) { vwa_skinny_set_x_skew((int)skew); });
  m.def("gemm_set_split_fill", [](int64_t pct) { vwa_gemm_set_split_fill((int)pct); });
  m.def("chain_make_seq", &chain_make_seq, py::arg("seq"), py::arg("X"), py::arg("W"), py::arg("bias"),
        py::arg("ln_c"), py::arg("Y"), py::arg("epi"), py::arg("eps"), py::arg("n_heads"), py::arg("head_dim"),
        py::arg("positions"), py::arg("slots"), py::arg("k_cache"), py::arg("v_cache"), py::arg("bar"),
        py::arg("work"), py::arg("bar_mode") = 1, py::arg("w_tiled") = false);
  m.def("chain_run", &chain_run, py::arg("desc"), py::arg("n_phases"), py::arg("lds"), py::arg("like"),
        py::arg("attn_g") = 0, py::arg("seq") = 0, py::arg("n_layers") = 1);
  m.def("alloc_uncached_i32", &alloc_uncached_i32);
  m.def("device_cus", [](Tensor like) {
    check_anchor(like, "like");
    return (int64_t)device_cus(like);
  });
  m.def("wdec_layers", &wdec_layers, py::arg("flat"), py::arg("n_layers"), py::arg("like"));
  m.def("wdec_run", &wdec_run, py::arg("layers"), py::arg("roles"), py::arg("bufs"), py::arg("ints"), py::arg("eps"),
        py::arg("scale"), py::arg("n_prod"), py::arg("ts") = py::none(), py::arg("opt") = 0, py::arg("lm") = py::none(),
        py::arg("emb") = py::none(), py::arg("smp") = py::none(), py::arg("loop_base_block") = 0);
  m.def("decode_advance", &decode_advance);
  m.def("gemm", &gemm, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("epi"),
        py::arg("rstd") = py::none(), py::arg("residual") = py::none(), py::arg("w_tiled") = false,
        py::arg("ws") = py::none(), py::arg("ss_out") = py::none(), py::arg("ss_zero") = py::none(),
        py::arg("ss_in") = py::none(), py::arg("ss_eps") = 1e-5);
  m.def("row_rstd", &row_rstd);
  m.def("gemm_qkv", &gemm_qkv, py::arg("x"), py::arg("sx"), py::arg("w"), py::arg("sw"), py::arg("bias"),
        py::arg("rstd"), py::arg("w_tiled"), py::arg("ws"), py::arg("n_q_heads"), py::arg("n_kv_heads"),
        py::arg("head_dim"), py::arg("use_rope"), py::arg("positions"), py::arg("slots"), py::arg("rope"),
        py::arg("q_out"), py::arg("k_cache"), py::arg("v_cache"), py::arg("ss_in") = py::none(),
        py::arg("ss_eps") = 1e-5);
  m.def("gemm_fp8", &gemm_fp8, py::arg("x8"), py::arg("sx"), py::arg("w8"), py::arg("sw"), py::arg("bias"),
        py::arg("y"), py::arg("epi"), py::arg("rstd") = py::none(), py::arg("residual") = py::none(),
        py::arg("ws") = py::none(), py::arg("ss_out") = py::none(), py::arg("ss_zero") = py::none(),
        py::arg("ss_in") = py::none(), py::arg("ss_eps") = 1e-5);
  m.def("rmsnorm", &rmsnorm);
  m.def("layernorm", &layernorm);
  m.def("rope_kv_write", &rope_kv_write);
  m.def("swiglu", &swiglu);
  m.def("bias_act", &bias_act);
  m.def("decode_attention", &decode_attention);
  m.def("flash_attention", &flash_attention);
  m.def("embedding", &embedding);
  m.def("sample", &sample, py::arg("logits"), py::arg("mask"), py::arg("temperature"), py::arg("seed"), py::arg("step"),
        py::arg("out_tokens"), py::arg("part_val"), py::arg("part_idx"), py::arg("fail_word") = py::none(),
        py::arg("v_offset") = 0);
  m.def("sample_tp", &sample_tp);
  m.def("pcm16_to_f32", &pcm16_to_f32);
  m.def("log_mel", &log_mel);
  m.def("conv1d_gelu", &conv1d_gelu);
  m.def("set_skinny_mode", &set_skinny_mode, py::arg("mode"), py::arg("grid_cap") = 256, py::arg("ks") = 0,
        py::arg("w_first") = 2);
  m.def("attention_split_tokens", []() { return vwa_attention_split_tokens(); });
  m.def("set_attention_impl", [](int64_t impl) { vwa_set_attention_impl((int)impl); });
}

// Word-alignment kernels for gfx950 (_vwa_align.so): cross-attention probabilities of the
// alignment heads, the token x frame alignment cost, dynamic time warping over it and the
// log-probability of each emitted token.  Every launcher validates its geometry again (the
// bindings are the first line), returns 0 or a negative code and launches on `st`.
//
// No kernel here waits on another workgroup and none uses atomics; every loop is bounded by an
// argument the launcher checked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kAlignHeadDim = 64;     // every model of this project
constexpr int kDtwMaxRows = 448;      // Whisper's text context: one lane per token row
constexpr int kDtwLdsTrace = 48 * 1024;  // bytes of step trace kept in LDS (one byte per cell)

extern "C" {

// out[s][t][j] = softmax_j(scale * q[t, heads[s]] . k[j, heads[s]]) over j < n_keys; columns
// >= n_keys are not written.  q: bf16 rows of H*64 (row stride ldq elements); k: bf16
// [S_max][H][64] contiguous; out strides in elements (unit key stride).  heads[] entries are
// clamped to [0, H) on the device.
int vwa_attn_probs(const uint16_t* q, int64_t ldq, const uint16_t* k, const int* heads, int n_sel, int H, int T,
                   int n_keys, float scale, float* out, int64_t out_stride_head, int64_t out_stride_row,
                   hipStream_t st);

// out[t][j] = -mean_h median7_j((p[h][t][j] - mean_t) / sqrt(var_t + 1e-12)), t < n_tokens,
// j < n_keys (reflect padding; n_keys <= 3: no filter).  probs strides in elements.
int vwa_align_cost(const float* probs, int64_t stride_head, int64_t stride_row, int n_heads, int n_tokens,
                   int n_keys, float* out, int64_t out_stride_row, hipStream_t st);

// DTW over cost[n_tokens][n_keys] (row stride ldc) and its backtrack: first_frame[i] /
// last_frame[i] = smallest / largest frame of the path in row i.  trace: n_tokens * n_keys bytes
// of workspace, required when that exceeds kDtwLdsTrace (else may be null).
int vwa_dtw_path(const float* cost, int64_t ldc, int n_tokens, int n_keys, int* first_frame, int* last_frame,
                 uint8_t* trace, hipStream_t st);

// out[n] = logits[n][t_n] - logsumexp over ids v < vocab whose mask bit is set (mask null: all);
// t_n = targets[n] clamped to [0, vocab); never above 0, -inf for a target the mask forbids.  mask
// rows are mask_stride words apart (0: one row shared by all).
int vwa_token_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* targets,
                      const uint32_t* mask, int64_t mask_stride, float* out, hipStream_t st);

}  // extern "C"

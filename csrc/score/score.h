// Running transcript scores for gfx950 (_vwa_score.so): one launch per decode step, after the
// sampler, that adds to every row's sum the log-probability of the token the sampler just chose,
// under the distribution it was drawn from -- the logits as the boost and the timestamp rules left
// them, restricted to the ids the sampler's mask allows.  Same conventions as csrc/tsrules/tsrules.h:
// the launcher validates its geometry again (the bindings are the first line), returns 0 or a
// negative code, never launches on a rejected call, and launches on `st`.
//
// The kernel does not wait on another workgroup and uses no atomics and no scratch; every loop is
// bounded by an argument the launcher checked, and the one value read from device memory that
// becomes an index (a row's token) is range-tested before it addresses anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kScoreMaxRows = 64;        // rows per launch (one workgroup each)
constexpr int kScoreMaxVocab = 1 << 20;

extern "C" {

// logits f32 [rows, ld], ld >= vocab: read only.  0 <= eot < vocab.
// mask: the sampler's packed allow-bits (int32 words, little bit order); row r reads mask + r * mask_ld,
// mask_ld == 0: one shared row (mask_ld > 0: >= ceil(vocab / 32)).
// State: sum f32 [rows] and cnt int32 [rows, 2] = (n, done): the sum of the log-probabilities of the
// n tokens counted so far; done != 0 once the row's EOT has been counted.
//
// Per row r < rows (x = logits + r * ld, t = tokens[r]):
//   enable[r] <= 0, or done != 0, or t outside [0, vocab): sum_out[r] = sum_in[r] and cnt_out[r] =
//     cnt_in[r] (verbatim), step_lp[r] = 0.
//   otherwise: L = log-sum-exp of x[v] over the ids v < vocab whose mask bit is set (a column at -inf
//     adds nothing); lp = x[t] - L, never above 0, and -inf when the mask forbids t or x[t] is -inf;
//     sum_out[r] = sum_in[r] + lp, cnt_out[r] = (n + 1, t == eot), step_lp[r] = lp.
//   So the first EOT's own log-probability is counted and nothing after it (Whisper's sum_logprobs).
// Columns >= vocab are never read, nor is any row >= rows; nothing but sum_out, cnt_out and step_lp
// (which may be null) is written.  The reduction runs in a fixed order: the same input gives the
// same bits.
//
// sum_out may be sum_in itself and cnt_out may be cnt_in itself (each row reads and writes its own
// cells); any other overlap among sum_in, sum_out, cnt_in, cnt_out and step_lp is rejected.
// rows in [1, 64], vocab <= 2^20.
int vwa_score_step(const float* logits, int64_t ld, int rows, int vocab, int eot, const int* mask, int64_t mask_ld,
                   const int* enable, const int* tokens, const float* sum_in, float* sum_out, const int* cnt_in,
                   int* cnt_out, float* step_lp, hipStream_t st);

}  // extern "C"

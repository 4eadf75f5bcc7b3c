// Log-probability of a set of token ids for gfx950 (_vwa_turn.so): one launch that gives, for every
// row of f32 logits, the probability mass the row's softmax puts on a SET of ids -- the brain's
// turn-completion probe asks it for the ids that close a JSON string.  Same conventions as
// csrc/score/score.h: the launcher validates its geometry again (the bindings are the first line),
// returns 0 or a negative code, never launches on a rejected call, and launches on `st`.
//
// The kernel does not wait on another workgroup and uses no atomics and no scratch; every loop is
// bounded by an argument the launcher checked, and no value read from device memory becomes an
// index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kTurnMaxRows = 64;        // rows per launch (one workgroup each)
constexpr int kTurnMaxVocab = 1 << 20;

extern "C" {

// logits f32 [rows, ld], ld >= vocab: read only.
// set: packed allow-bits in the sampler's mask format (int32 words, little bit order); row r reads
// set + r * set_ld, set_ld == 0: one shared row (set_ld > 0: >= ceil(vocab / 32)).
// out f32 [rows, 2].
//
// Per row r < rows (x = logits + r * ld):
//   A = log-sum-exp of x[v] over v < vocab; S = the same over the ids v < vocab whose set bit is on.
//   A column at -inf (or NaN) adds nothing to either.
//   out[r] = (min(S - A, 0), A).
//   An empty set, a set whose columns are all -inf, and a row that is all -inf (A = -inf) give
//   out[r, 0] = -inf; the result is never NaN.
// Columns >= vocab are never read, nor is any row >= rows, nor a set bit >= 32 ceil(vocab / 32);
// nothing but out[0 .. 2 rows) is written.  One sweep of the row feeds both sums, and the reduction
// runs in a fixed order: the same input gives the same bits.
//
// Any overlap of out with the logits or the set is rejected.  rows in [1, 64], vocab <= 2^20.
int vwa_set_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* set, int64_t set_ld, float* out,
                    hipStream_t st);

}  // extern "C"

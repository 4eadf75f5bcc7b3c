// Whisper's timestamp rules for gfx950 (_vwa_tsrules.so): one launch per decode step that moves every
// row's small decoding state on by the row's last token and writes -inf over the logits the rules
// forbid at that state, before the sampler reads them.  Same conventions as csrc/boost/boost.h: the
// launcher validates its geometry again (the bindings are the first line), returns 0 or a negative
// code, never launches on a rejected call, and launches on `st`.
//
// The kernel does not wait on another workgroup and uses no atomics and no scratch; every loop is
// bounded by an argument the launcher checked, and every value read from device memory that becomes
// an index (a token, a state's last_ts) is range-tested before it addresses anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kTsMaxRows = 64;        // rows per launch (one workgroup each)
constexpr int kTsMaxVocab = 1 << 20;

extern "C" {

// logits f32 [rows, ld], ld >= vocab.  eot < ts_begin < vocab; ts_begin is the id of <|0.00|>
// (<|notimestamps|> + 1) and n_ts = vocab - ts_begin.
// mask: the sampler's packed allow-bits (int32 words, little bit order); row r reads mask + r * mask_ld,
// mask_ld == 0: one shared row (mask_ld > 0: >= ceil(vocab / 32)).  An id whose bit is clear counts
// as banned in rule 5; the mask itself causes no write.
// State: int32 [rows, 4] = (n, last, prev, last_ts): tokens sampled so far (saturating at 2), the
// last and penultimate sampled ids (-1: none), the index of the most recent timestamp token (-1:
// none).  n outside [0, 2] or last_ts outside [-1, n_ts): the state reads as (0, -1, -1, -1).
//
// Per row r < rows (x = logits + r * ld):
//   enable[r] <= 0: the logits are untouched, state_out[r] = state_in[r] (verbatim).
//   tokens given: t = tokens[r] outside [0, vocab) leaves the logits untouched and
//     state_out[r] = state_in[r]; otherwise the state moves first:
//       prev = last; last = t; n = min(n + 1, 2); t >= ts_begin: last_ts = t - ts_begin.
//   tokens null: apply only.
//   state_out[r] = the state, then ("ban [a, b)": f32 -inf over those columns)
//   1. ban ts_begin - 1.
//   2. last_was = n >= 1 && last >= ts_begin; pen_was = n < 2 || prev >= ts_begin.
//      last_was && pen_was: ban [ts_begin, vocab).  last_was && !pen_was: ban [0, eot).
//   3. last_ts >= 0: ban [ts_begin, ts_begin + lim), lim = last_ts when last_was && !pen_was,
//      last_ts + 1 otherwise.
//   4. n == 0: ban [0, ts_begin), and with max_initial >= 0 also [ts_begin + max_initial + 1, vocab).
//   5. over the ids the mask allows and 1-4 left: T = log-sum-exp of the columns >= ts_begin, M = max
//      of the columns < ts_begin (empty: -inf).  T > M: ban [0, ts_begin).
// Every other column keeps its bits; columns >= vocab are never read or written, nor is any row >= rows.
//
// state_out may be state_in itself (each row reads and writes its own four cells); any other
// overlap is rejected.  rows in [1, 64], vocab <= 2^20.
int vwa_ts_rules_step(float* logits, int64_t ld, int rows, int vocab, int eot, int ts_begin, int max_initial,
                      const int* mask, int64_t mask_ld, const int* enable, const int* state_in, int* state_out,
                      const int* tokens, hipStream_t st);

}  // extern "C"

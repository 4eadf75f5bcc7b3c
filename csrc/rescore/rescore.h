// Per-sequence log-probabilities of given continuations for gfx950 (_vwa_rescore.so): one call
// turns "these f32 logits rows, these target ids" into one log-probability per row and their running
// sums per sequence -- the brain's n-best rescoring asks it for the tokens that tell the recogniser's
// alternatives apart.  Same conventions as csrc/turn/turn.h and csrc/score/score.h: the launcher
// validates its geometry again (the bindings are the first line), returns 0 or a negative code,
// never launches on a rejected call, and launches on `st`.
//
// Why not ops.set_logprob with one-hot sets, or ops.token_logprob?  A one-hot set is 16 KB of set
// per row (a 128256-id vocabulary), built and uploaded per request, where a target id is 4 bytes;
// set_logprob takes 64 rows per launch, a rescored n-best of 8 alternatives has more; token_logprob
// lives in the recogniser's alignment library and takes the sampler's masks, not an end set; and
// either route leaves the sums to the host, one readback per piece, where here they stay on the
// device until the request's last row.
//
// Two kernels on the stream inside the one call: the row pass (one workgroup per row), then one
// small workgroup with a lane per sequence that walks the rows in order.  Neither waits on another
// workgroup, neither uses atomics or scratch; every loop is bounded by an argument the launcher
// checked, and no value read from device memory is used as an index without a range check (target
// is checked against [0, vocab); seq is only compared).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kRescoreMaxRows = 256;  // rows per call (one workgroup each)
constexpr int kRescoreMaxSeq = 64;    // running sums per call (one lane each)
constexpr int kRescoreMaxVocab = 1 << 20;

extern "C" {

// logits f32 [rows, ld], ld >= vocab: read only.
// target int32 [rows]: an id in [0, vocab), or -1 = "the end set".
// end_set int32 [ceil(vocab / 32)]: packed allow-bits in the sampler's mask format.
// seq int32 [rows]: which running sum row r belongs to.
// acc_in f32 [n_seq] or null (= zeros); lp f32 [rows]; acc_out f32 [n_seq].
//
// Per row r < rows (x = logits + r * ld, t = target[r]):
//   A = log-sum-exp of x[v] over v < vocab; a column at -inf (or NaN) adds nothing.
//   t in [0, vocab):  lp[r] = min(x[t] - A, 0)
//   t == -1:          lp[r] = min(S - A, 0), S the log-sum-exp over the ids v < vocab whose bit in
//                     end_set is on -- turn.h's rule, fed by the same sweep.
//   lp[r] = -inf for a row that is all -inf, a target column at -inf or NaN, an empty set or one
//   whose columns are all -inf, and a target outside [-1, vocab) (such a row reads nothing outside
//   itself).  lp[r] is never NaN and never above 0.
// Per sequence s < n_seq:
//   acc_out[s] = acc_in[s] + lp[r0] + lp[r1] + ... over the rows with seq[r] == s, in ascending r, as
//   sequential f32 additions in that order.  A seq[r] outside [0, n_seq) adds to nothing; a sequence
//   with no rows copies acc_in[s].
// The sums are out of place on purpose: a step whose chained launch timed out is run again and
// scored again from the same acc_in, so nothing counts twice.
//
// Columns >= vocab are never read, nor is any row >= rows, nor a set bit >= 32 ceil(vocab / 32);
// nothing but lp[0 .. rows) and acc_out[0 .. n_seq) is written.  Every reduction runs in a fixed
// order: the same input gives the same bits.
//
// rows in [1, 256], n_seq in [1, 64], vocab <= 2^20.  Any overlap of lp or acc_out with an input, or
// of lp with acc_out, is rejected.
int vwa_seq_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* target, const int* end_set,
                    const int* seq, int n_seq, const float* acc_in, float* lp, float* acc_out, hipStream_t st);

}  // extern "C"

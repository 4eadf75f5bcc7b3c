// Repetition penalty, top-k and nucleus (top-p) narrowing of the sampler's allow-mask for gfx950
// (_vwa_nucleus.so): one launch per decode step, one workgroup per logits row, in front of the
// sampler on the same stream.  Free-text generation (the brain's summaries) needs it; grammar-forced
// JSON at temperature 0.1 never did.  Same conventions as csrc/turn/turn.h: the launcher validates
// its geometry again (the bindings are the first line), returns 0 or a negative code, never launches
// on a rejected call, and launches on `st`; there is no host synchronisation.
//
// The kernel does not wait on another workgroup and uses no floating-point atomics and no scratch;
// every loop is bounded by an argument the launcher checked.  The only values read from device
// memory that become an index are the history's ids, each range-checked against [0, vocab) first,
// and the per-row top_k, clamped to [0, kNucleusMaxTopK] first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kNucleusMaxRows = 64;         // rows per launch (one workgroup each)
constexpr int kNucleusMaxVocab = 128256;    // the Llama-3 vocabulary: the staged mask row is 4008 words of LDS
constexpr int kNucleusMaxTopK = 1024;       // candidates sorted in LDS
constexpr int kNucleusMaxHistory = 256;     // ids penalised per row

extern "C" {

// Layout (all row-major, row r of an array with row stride s at base + r * s):
//   logits      f32 [rows, ld], ld >= vocab.  Columns [0, vocab) of row r are MODIFIED IN PLACE by the
//               penalty (step 1) and by nothing else; columns [vocab, ld) are neither read nor written.
//   mask_in     packed allow-bits in the sampler's format (int32 words, bit c of a row = word c >> 5,
//               bit c & 31), row stride mask_ld words (0: one shared row; else >= ceil(vocab / 32)).
//               May be pinned host memory: each word in [0, ceil(vocab / 32)) is read exactly once,
//               into LDS.  Null: every column is allowed.
//   mask_out    int32 [rows, out_words] with row stride out_ld >= out_words >= ceil(vocab / 32),
//               device memory: the narrowed allow-bits.  All out_words words of a row are written;
//               bits at or beyond vocab, and so all trailing words, are zero.
//   n_kept      int32 [rows]: the number of bits set in mask_out[r].
//   temperature, top_p, penalty   f32 [rows];  top_k  int32 [rows]: four separate arrays.
//   history     int32 [rows, H] with row stride hist_ld >= H, 0 <= H <= 256: ids to penalise.  An id
//               that is negative (-1 is the padding) or >= vocab is ignored.
//
// Per row r (l = the row's logits, T = temperature[r], p = top_p[r], k = top_k[r], th = penalty[r]):
//  1. Penalty (the HF RepetitionPenaltyLogitsProcessor rule), once per DISTINCT valid id t of
//     history[r], whether or not t is allowed:  l_t <- l_t / th if l_t > 0, else l_t * th.  Each is one
//     correctly rounded f32 operation.  th == 1 writes nothing: the row keeps its bits.
//  2. Pass-through: if !(T > 0), or if k == 0 and !(p < 1), mask_out[r] is mask_in[r] bit for bit with
//     the bits >= vocab cleared, and n_kept[r] its popcount.  (What a grammar row riding in the same
//     launch gets.)  Otherwise:
//  3. Candidates.  A = the ids whose mask_in bit is on and whose penalised logit is > -inf (a NaN is
//     not).  Order A by (logit descending, id ascending); -0 and +0 compare equal.  K = the first
//     min(k, |A|) ids of that order.  Compares and integer counts only: exact, ties go to the lowest id.
//     An empty A gives an all-zero row and n_kept = 0.
//  4. Nucleus.  w_i = expf((l_i - l_0) / T) over K in that order (one f32 subtraction, one correctly
//     rounded f32 division, expf), c_j = sum_{i <= j} w_i in f32, C = c_{|K| - 1}.  Keep ids 0 .. j*,
//     j* = the smallest j with c_j >= p * C (one f32 product); !(p < 1) keeps all of K.  At least one
//     id is kept.  Summation order of c_j (fixed, so a launch repeats its bits): the ranks are dealt
//     to lanes in order, 64 per wave; within a wave a Kogge-Stone scan (steps 1, 2, 4, .. 32, lane i
//     adds the running value of lane i - step); then c_j = (the totals of the waves before j's, added
//     left to right from 0) + (j's in-wave value).
//  Ranges: k is clamped to [0, 1024].  p < 1 with k == 0 is taken over the top 1024 (k = 1024): the
//  nucleus is always a cut of the renormalised top-k, as HF's warper order (top-k, then top-p) makes
//  it -- a documented limit, not full-vocabulary top-p.
//
// mask_out and n_kept must overlap neither each other nor any input.  rows in [1, 64],
// vocab in [1, 128256], H in [0, 256].
int vwa_nucleus_step(float* logits, int64_t ld, int rows, int vocab, const int* mask_in, int64_t mask_ld,
                     int* mask_out, int64_t out_ld, int out_words, int* n_kept, const float* temperature,
                     const float* top_p, const int* top_k, const float* penalty, const int* history, int64_t hist_ld,
                     int H, hipStream_t st);

}  // extern "C"

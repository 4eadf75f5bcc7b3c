// Start-of-transcript analysis for gfx950 (_vwa_sot.so): what Whisper reads from the logits at the
// SOT position -- the probability that the window holds no speech and the distribution over the
// language tokens -- in one launch.  The launcher validates its geometry again (the bindings are
// the first line), returns 0 or a negative code and launches on `st`.
//
// The kernel never waits on another workgroup, uses no atomics and no scratch; every loop is bounded
// by an argument the launcher checked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kSotMaxLangs = 128;  // one lane per language: two of the workgroup's four waves

extern "C" {

// For row r < rows with x = logits + r * ld:
//   no_speech[r]     = softmax over v < vocab of x, at no_speech_id (the row maximum subtracted;
//                      columns >= vocab are never read);
//   A                = the ids lang0 + i with i < n_lang and bit i of allow[] set (bit i of the
//                      128-bit set is bit i % 32 of allow[i / 32]);
//   lang_probs[r][i] = softmax over A (A's own maximum subtracted), exactly 0 for a disallowed i;
//                      columns >= n_lang are not written (row stride ldp);
//   lang_tok[r]      = the lowest id of A whose logit equals the maximum over A -- always an id of
//                      A: when no logit of A compares equal to it (every one NaN) the lowest id of
//                      A.  All of A at -inf: the lowest id of A, NaN probabilities;
//   lang_conf[r]     = lang_probs[r][lang_tok[r] - lang0];
//   tok_dst[dst_rows[r]] = lang_tok[r] where tok_dst is given and 0 <= dst_rows[r] < n_dst (the
//                      next decoder step's staged token rows; any other entry is left alone).
// tok_dst and dst_rows are given together or both null.
int vwa_sot_probe(const float* logits, int64_t ld, int rows, int vocab, int lang0, int n_lang,
                  const uint32_t allow[4], int no_speech_id, float* lang_probs, int64_t ldp, int* lang_tok,
                  float* lang_conf, float* no_speech, int* tok_dst, const int* dst_rows, int n_dst,
                  hipStream_t st);

}  // extern "C"

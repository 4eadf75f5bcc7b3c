// Beam search steps for gfx950 (_vwa_beam.so): choosing the best continuations over a group of
// beams' logits, and moving the beams' self-attention K/V to follow their new parents.  The
// launchers validate their geometry again (the bindings are the first line), return 0 or a negative
// code, never launch on a rejected call, and launch on `st`.
//
// No kernel waits on another workgroup or uses atomics or scratch; every loop is bounded by an
// argument the launcher checked, and every index read from device memory is clamped or tested
// before it addresses anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kBeamMaxWidth = 8;         // beams per group (W)
constexpr int kBeamMaxRows = 64;         // rows (groups x beams) per launch
constexpr int kBeamTile = 8192;          // logit columns one workgroup of the row stage holds in registers
constexpr int kBeamMaxVocab = 1 << 20;   // <= 128 tiles per row

extern "C" {

// Bytes of workspace vwa_beam_select needs for `rows` rows of `vocab` columns (0: rejected).
int64_t vwa_beam_select_workspace(int rows, int vocab);

// Rows are G groups of W consecutive rows (2 <= W <= 8, G * W <= 64); row r = g * W + b has
// x = logits + r * ld, the allow-mask row mask + r * mask_stride (bit v % 32 of word v / 32 admits
// id v; mask_stride 0: one row for all; null: every id) and the running score cum[r].
//   lse[r]        = m + logf(sum of expf(x[v] - m)) over the allowed v < vocab, m their maximum;
//   score(r, v)   = cum[r] + (x[v] - lse[r]) in f32, in that association;
// a candidate exists for every allowed v < vocab of a row whose score is finite (so a row with
// cum = -inf, a -inf logit, a masked id and an id >= vocab never give one).  Per group the
// K = 2 W best candidates, by descending score and -- among equal f32 scores -- ascending
// b * vocab + v, go to cand_score / cand_beam (b) / cand_tok (v) [g * ldc + k], k < K; ranks past
// the group's candidates hold (-inf, -1, -1).  Nothing else of the outputs is written, and
// columns >= vocab of the logits are never read.
//
// Three launches: per (row, tile of kBeamTile columns) the maximum and the sum of exponentials;
// per (row, tile) the tile's K best under the row's lse (the tiles' partial sums combined in tile
// order); per group the K best of its rows' tile lists, read in a fixed order.  The result does
// not depend on the order workgroups run in.
int vwa_beam_select(const float* logits, int64_t ld, int G, int W, int vocab, const uint32_t* mask,
                    int64_t mask_stride, const float* cum, float* cand_score, int* cand_beam, int* cand_tok,
                    int64_t ldc, void* workspace, int64_t workspace_bytes, hipStream_t st);

// In-place permutation of the beams' self-attention K/V.  k_cache / v_cache: bf16
// [L, n_blocks, H, bs, hd] contiguous and 16-byte aligned, bs * hd * 2 a multiple of 16 (else the
// launch is rejected); block_table int32 [sessions, ldbt >= bps]; slots, parents
// int32 [G, W]; n_ctx int32 [G].  For group g, beam w with p = parents[g][w] != w, every layer and
// every block j < min(ceil(n_ctx[g] / bs), max_blocks): the block block_table[slots[g][w]][j] of
// both caches receives the old content of block block_table[slots[g][p]][j].  Each thread owns the
// same 16 bytes of all W beams' blocks and reads all of them before it writes any, so parents may
// repeat or form cycles; the slots of one launch must be distinct.  A slot outside [0, sessions),
// a parent outside [0, W) or a block outside [1, n_blocks) is never dereferenced: that beam is
// left alone.  Block 0 and blocks past the context are never written.
int vwa_kv_beam_gather(void* k_cache, void* v_cache, int L, int n_blocks, int H, int bs, int hd,
                       const int* block_table, int sessions, int64_t ldbt, int bps, const int* slots,
                       const int* parents, const int* n_ctx, int G, int W, int max_blocks, hipStream_t st);

}  // extern "C"

// Keyterm boosting for gfx950 (_vwa_boost.so): one launch per decode step that moves every row's
// keyterm automaton on by the row's last token and adds the automaton state's biases to the row's
// logits.  Same conventions as csrc/beam/beam.h: the launcher validates its geometry again (the
// bindings are the first line), returns 0 or a negative code, never launches on a rejected call,
// and launches on `st`.
//
// The kernel does not wait on another workgroup and uses no atomics and no scratch; every loop is
// bounded by an argument the launcher checked, and every index read from device memory (a root, a
// state, a parent, an edge offset, an edge's token and next state) is range-tested before it
// addresses anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kBoostMaxRows = 64;          // rows per launch (one workgroup each)
constexpr int kBoostMaxStates = 1 << 20;   // S: states of all automata of a launch
constexpr int kBoostMaxEdges = 1 << 24;    // E: resolved edges of all automata of a launch
constexpr int kBoostMaxVocab = 1 << 20;

extern "C" {

// Tables of S states and E edges (several automata concatenated):
//   edge_off int32 [S + 1]   state s owns the edges [edge_off[s], edge_off[s + 1]), its list L(s);
//   edge_tok / edge_next int32 [E], edge_bias f32 [E]   tokens strictly ascending within a list;
//   state_root int32 [S]     the root of the automaton the state belongs to (a root: itself).
// A root's list holds its children.  A non-root state's list holds the children of itself and of
// the non-root nodes on its failure chain, `next` from the deepest of them and `bias` the largest
// over the whole chain, the root included.
//   delta(s, v) = next of v in L(s), else next of v in L(root(s)), else root(s)   (binary searches)
//
// Per row r < rows (x = logits + r * ld):
//   1. root = roots[r]; negative, >= S or not a root: the row's logits are untouched and
//      state_out[r] = state_in[r].
//   2. src = r (parents null) or (r / W) * W + parents[r]; a parent outside [0, W): s = root.
//   3. s = state_in[src]; outside [0, S) or of another automaton: s = root.
//   4. tokens given: a negative tokens[r] leaves the logits untouched and sets state_out[r] = s;
//      otherwise s = delta(s, tokens[r]).  tokens null: apply only.
//   5. state_out[r] = s.
//   6. every edge of L(s) with tok < vocab: x[tok] += bias.
//   7. s not the root: every edge of L(root) with tok < vocab and tok not in L(s): x[tok] += bias.
// One f32 add per boosted id; columns >= vocab are never read or written, nor is any row >= rows.
//
// state_out may be state_in only when parents is null (each row then reads and writes its own
// element); with parents any overlap of the two is rejected.  rows in [1, 64]; with parents,
// W in [1, rows] and rows a multiple of W.
int vwa_boost_step(float* logits, int64_t ld, int rows, int vocab, const int* edge_off, const int* edge_tok,
                   const int* edge_next, const float* edge_bias, const int* state_root, int S, int E,
                   const int* roots, const int* state_in, int* state_out, const int* tokens, const int* parents,
                   int W, hipStream_t st);

}  // extern "C"

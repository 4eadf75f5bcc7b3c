// The keyterm boosting step (see boost.h for the contract): one workgroup of one wave per row.
//
// Every lane works out the row's new state by itself from the same loads (a few dependent reads and
// two binary searches: cheaper than a broadcast through LDS and a barrier), lane 0 stores it, and
// the lanes then share the edges of the state's list and of the root's list.  Tokens ascend
// strictly within a list, and a root edge is skipped when the state's list holds its token, so no
// two lanes add to one column.
#include "boost/boost.h"
#include "kernels/common.h"

namespace {

constexpr int kThreads = 64;
constexpr int kSearchSteps = 25;  // > log2(kBoostMaxEdges): the binary search's bound

struct List {
  int lo, hi;  // edges [lo, hi)
};

// State s's edge list, its offsets range-tested: anything inconsistent is the empty list.
__device__ __forceinline__ List list_of(const int* __restrict__ edge_off, int s, int E) {
  const int lo = edge_off[s], hi = edge_off[s + 1];
  if (lo < 0 || hi > E || lo > hi) return List{0, 0};
  return List{lo, hi};
}

// The edge of `l` with token v, or -1.
__device__ __forceinline__ int find(const int* __restrict__ edge_tok, List l, int v) {
  int lo = l.lo, hi = l.hi;
  for (int it = 0; it < kSearchSteps && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    const int t = edge_tok[mid];
    if (t == v) return mid;
    if (t < v) lo = mid + 1; else hi = mid;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void boost_step_kernel(
    float* __restrict__ logits, int64_t ld, int vocab, const int* __restrict__ edge_off,
    const int* __restrict__ edge_tok, const int* __restrict__ edge_next, const float* __restrict__ edge_bias,
    const int* __restrict__ state_root, int S, int E, const int* __restrict__ roots, const int* state_in,
    int* state_out, const int* __restrict__ tokens, const int* __restrict__ parents, int W, int rows) {
  const int r = blockIdx.x;
  const int lane = threadIdx.x;
  const int root = roots[r];
  if (root < 0 || root >= S || state_root[root] != root) {  // not boosted
    if (lane == 0) state_out[r] = state_in[r];
    return;
  }
  int s = root;
  int src = r;
  if (parents) {
    const int p = parents[r];
    src = (p >= 0 && p < W) ? (r / W) * W + p : -1;
  }
  if (src >= 0 && src < rows) {
    s = state_in[src];
    if (s < 0 || s >= S || state_root[s] != root) s = root;
  }
  const List lroot = list_of(edge_off, root, E);
  if (tokens) {
    const int t = tokens[r];
    if (t < 0) {
      if (lane == 0) state_out[r] = s;
      return;
    }
    int e = find(edge_tok, list_of(edge_off, s, E), t);
    if (e < 0 && s != root) e = find(edge_tok, lroot, t);
    int nx = root;
    if (e >= 0) {
      nx = edge_next[e];
      if (nx < 0 || nx >= S || state_root[nx] != root) nx = root;
    }
    s = nx;
  }
  // (with state_out == state_in -- parents null -- this row's element is the only one it read)
  if (lane == 0) state_out[r] = s;
  float* x = logits + (int64_t)r * ld;
  const List ls = list_of(edge_off, s, E);
  for (int e = ls.lo + lane; e < ls.hi; e += kThreads) {
    const int t = edge_tok[e];
    if (t >= 0 && t < vocab) x[t] += edge_bias[e];
  }
  if (s == root) return;
  for (int e = lroot.lo + lane; e < lroot.hi; e += kThreads) {
    const int t = edge_tok[e];
    if (t >= 0 && t < vocab && find(edge_tok, ls, t) < 0) x[t] += edge_bias[e];
  }
}

}  // namespace

extern "C" int vwa_boost_step(float* logits, int64_t ld, int rows, int vocab, const int* edge_off, const int* edge_tok,
                              const int* edge_next, const float* edge_bias, const int* state_root, int S, int E,
                              const int* roots, const int* state_in, int* state_out, const int* tokens,
                              const int* parents, int W, hipStream_t st) {
  if (!logits || !edge_off || !edge_tok || !edge_next || !edge_bias || !state_root || !roots || !state_in || !state_out)
    return -1;
  if (rows < 1 || rows > kBoostMaxRows) return -2;
  if (vocab < 1 || vocab > kBoostMaxVocab || ld < vocab) return -3;
  if (S < 1 || S > kBoostMaxStates || E < 1 || E > kBoostMaxEdges) return -4;
  if (parents) {
    if (W < 1 || W > rows || rows % W) return -5;
    if (vwa::overlap(state_in, 4 * (int64_t)rows, state_out, 4 * (int64_t)rows)) return -6;
  } else if (state_in != state_out && vwa::overlap(state_in, 4 * (int64_t)rows, state_out, 4 * (int64_t)rows)) {
    return -6;  // (the same buffer steps in place; a shifted overlap would read other rows' new states)
  }
  hipLaunchKernelGGL(boost_step_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, edge_off, edge_tok,
                     edge_next, edge_bias, state_root, S, E, roots, state_in, state_out, tokens, parents, W, rows);
  return (int)hipGetLastError();
}

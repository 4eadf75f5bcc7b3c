// Dynamic time warping over a token x frame cost matrix and its backtrack, in one launch by one
// workgroup (step 4 of the method).
//
//   D[i][j] = cost[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]),  D[0][0] = cost[0][0]
//
// Anti-diagonal wavefront: lane i owns token row i and on diagonal d computes cell (i, d - i).
// Its left neighbour is its own previous value, the cell above is row i-1's previous value and the
// diagonal one is what it read as "above" a step earlier.  Up to 64 rows are one wave: the value
// above comes by a lane shift, no barrier.  More rows (up to 448, 7 waves) pass it through a
// double-buffered LDS row with one __syncthreads per diagonal.  Each cell's step (0 diagonal,
// 1 vertical, 2 horizontal) is one byte of trace, in LDS when the matrix has at most 48 K cells,
// else in the caller's workspace; thread 0 then walks it back from (T-1, n_keys-1) to (0, 0).
//
// Tie rule: the diagonal only if strictly smaller than both others, else the vertical step only
// if strictly smaller than both others, else the horizontal step.
#include "kernels/common.h"
#include "align/align.h"

using namespace vwa;

namespace {

template <bool ONE_WAVE>
__global__ __launch_bounds__(kDtwMaxRows) void dtw_kernel(const float* __restrict__ cost, int64_t ldc, int T, int N,
                                                          int* __restrict__ first_frame,
                                                          int* __restrict__ last_frame, uint8_t* ws) {
  __shared__ uint8_t lds_trace[kDtwLdsTrace];
  __shared__ float above[2][kDtwMaxRows];
  uint8_t* const trace = (int64_t)T * N <= kDtwLdsTrace ? lds_trace : ws;
  const int i = threadIdx.x;
  const bool row = i < T;
  const float* crow = cost + (int64_t)(row ? i : 0) * ldc;
  float left = INFINITY, diag = INFINITY, mine = INFINITY;
  // the cost of this lane's next cell is loaded a diagonal ahead
  float c_next = (row && i == 0) ? crow[0] : 0.f;
  const int n_diag = T + N - 1;
  for (int d = 0; d < n_diag; ++d) {
    const int j = d - i;
    const bool active = row && j >= 0 && j < N;
    const float c = c_next;
    const int jn = j + 1;
    if (row && jn >= 0 && jn < N) c_next = crow[jn];
    float up;
    if (ONE_WAVE) {
      up = __shfl_up(mine, 1, 64);
    } else {
      up = i > 0 ? above[(d + 1) & 1][i - 1] : INFINITY;
    }
    if (active) {
      const float c0 = (i > 0 && j > 0) ? diag : INFINITY;
      const float c1 = i > 0 ? up : INFINITY;
      const float c2 = j > 0 ? left : INFINITY;
      uint8_t step;
      float best;
      if (c0 < c1 && c0 < c2) {
        best = c0;
        step = 0;
      } else if (c1 < c0 && c1 < c2) {
        best = c1;
        step = 1;
      } else {
        best = c2;
        step = 2;
      }
      if (d == 0) best = 0.f;  // (0, 0): no predecessor
      mine = c + best;
      left = mine;
      trace[(int64_t)i * N + j] = step;
    }
    diag = up;
    if (!ONE_WAVE) {
      if (row) above[d & 1][i] = mine;
      __syncthreads();
    }
  }
  __syncthreads();  // the trace (LDS or this workgroup's global stores) before thread 0 reads it
  if (i == 0) {
    int r = T - 1, j = N - 1;
    last_frame[r] = j;
    // at most T + N - 2 steps: every step lowers r + j... or r or j, never below (0, 0)
    for (int n = 0; n < T + N && (r > 0 || j > 0); ++n) {
      const int step = r == 0 ? 2 : j == 0 ? 1 : trace[(int64_t)r * N + j];
      if (step != 2) {
        first_frame[r] = j;
        --r;
        if (step == 0) --j;
        last_frame[r] = j;
      } else {
        --j;
      }
    }
    first_frame[0] = 0;
  }
}

}  // namespace

extern "C" int vwa_dtw_path(const float* cost, int64_t ldc, int n_tokens, int n_keys, int* first_frame,
                            int* last_frame, uint8_t* trace, hipStream_t st) {
  if (n_tokens < 1 || n_tokens > kDtwMaxRows || n_keys < 1 || ldc < n_keys) return -1;
  if ((int64_t)n_tokens * n_keys > kDtwLdsTrace && trace == nullptr) return -2;
  if (n_tokens <= 64)
    hipLaunchKernelGGL(dtw_kernel<true>, dim3(1), dim3(64), 0, st, cost, ldc, n_tokens, n_keys, first_frame,
                       last_frame, trace);
  else
    hipLaunchKernelGGL(dtw_kernel<false>, dim3(1), dim3((n_tokens + 63) / 64 * 64), 0, st, cost, ldc, n_tokens, n_keys,
                       first_frame, last_frame, trace);
  return (int)hipGetLastError();
}

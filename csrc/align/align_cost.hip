// Token x frame alignment cost from the alignment heads' probabilities (step 3 of the method):
// per head and frame column a z-score over the token rows, a median of 7 along the frames
// (reflect padding), the mean over heads, negated.
//
// One workgroup per tile of 58 output columns (64 with the filter's 3-column halo on each side).
// Per head: the 64 columns' mean and 1/sqrt(var + 1e-12) over the token rows (two passes: mean,
// then the variance about it; 4 row groups x 64 columns, tree-added in LDS), then 16 rows at a
// time the z-scores go through LDS and each output cell takes the median of its 7.  The running
// head sum of a cell lives in `out` itself, always read and written by the same thread; the last
// head's visit turns it into -sum / heads.
#include "kernels/common.h"
#include "align/align.h"

using namespace vwa;

namespace {

constexpr int kCols = 64, kHalo = 3, kOutCols = kCols - 2 * kHalo, kRowsPerIter = 16;

VWA_DEVICE void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// median of 7: the 4th smallest (a full 7-element sort, unrolled)
VWA_DEVICE float median7(float* v) {
#pragma unroll
  for (int n = 6; n >= 3; --n)  // bubble passes until position 3 is final
#pragma unroll
    for (int i = 0; i < n; ++i) cswap(v[i], v[i + 1]);
  return v[3];
}

__global__ __launch_bounds__(256) void align_cost_kernel(const float* __restrict__ probs, int64_t sh, int64_t sr,
                                                         int n_heads, int n_tokens, int n_keys,
                                                         float* __restrict__ out, int64_t osr) {
  __shared__ float part[4][kCols];
  __shared__ float mean[kCols], rstd[kCols];
  __shared__ float zs[kRowsPerIter][kCols];
  const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j0 = blockIdx.x * kOutCols;
  // this thread's source column: j0 - 3 + c reflected into [0, n_keys) (index -1 -> 1; the edge is
  // not repeated).  n_keys <= 3: no filter, the halo is never read -- clamped to stay in bounds.
  int col = j0 - kHalo + c;
  if (col < 0) col = -col;
  if (col >= n_keys) col = 2 * (n_keys - 1) - col;
  col = min(max(col, 0), n_keys - 1);
  const bool filter = n_keys > 3;
  const int jo = j0 + c;  // the output column of a thread with c < kOutCols
  const bool writes = c < kOutCols && jo < n_keys;
  const float inv_n = 1.f / (float)n_tokens;

  for (int h = 0; h < n_heads; ++h) {
    const float* p = probs + (int64_t)h * sh + col;
    float acc = 0.f;
    for (int t = rg; t < n_tokens; t += 4) acc += p[(int64_t)t * sr];
    part[rg][c] = acc;
    __syncthreads();
    if (rg == 0) mean[c] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) * inv_n;
    __syncthreads();
    const float mu = mean[c];
    acc = 0.f;
    for (int t = rg; t < n_tokens; t += 4) {
      const float d = p[(int64_t)t * sr] - mu;
      acc += d * d;
    }
    part[rg][c] = acc;
    __syncthreads();
    if (rg == 0) rstd[c] = 1.f / sqrtf(((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) * inv_n + 1e-12f);
    __syncthreads();
    const float rs = rstd[c];
    for (int t0 = 0; t0 < n_tokens; t0 += kRowsPerIter) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + 4 * i + rg;
        zs[4 * i + rg][c] = t < n_tokens ? (p[(int64_t)t * sr] - mu) * rs : 0.f;
      }
      __syncthreads();
      if (writes) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = t0 + 4 * i + rg;
          if (t >= n_tokens) continue;
          float med = zs[4 * i + rg][c + kHalo];
          if (filter) {
            float v[7];
#pragma unroll
            for (int e = 0; e < 7; ++e) v[e] = zs[4 * i + rg][c + e];
            med = median7(v);
          }
          float* o = out + (int64_t)t * osr + jo;
          const float sum = (h ? *o : 0.f) + med;
          *o = h == n_heads - 1 ? -sum / (float)n_heads : sum;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int vwa_align_cost(const float* probs, int64_t stride_head, int64_t stride_row, int n_heads, int n_tokens,
                              int n_keys, float* out, int64_t out_stride_row, hipStream_t st) {
  if (n_heads < 1 || n_tokens < 1 || n_keys < 1 || stride_row < n_keys || out_stride_row < n_keys) return -1;
  hipLaunchKernelGGL(align_cost_kernel, dim3((n_keys + kOutCols - 1) / kOutCols), dim3(256), 0, st, probs, stride_head,
                     stride_row, n_heads, n_tokens, n_keys, out, out_stride_row);
  return (int)hipGetLastError();
}

// Log-probability of each emitted token under the distribution the sampler drew from: the row's
// logits restricted to ids below `vocab` whose bit is set in the sampler's packed allow-mask.
//
// One workgroup per row, two sweeps of the (L2-resident) row: the maximum, then the sum of
// exp(x - max); out = (x_target - max) - log(sum).  A row whose only allowed id is the target
// gives exactly 0 (sum = exp(0) = 1).  A row with no allowed id gives NaN.
#include "kernels/logit_row.h"
#include "align/align.h"

using namespace vwa;

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void token_logprob_kernel(const float* __restrict__ logits, int64_t ld,
                                                                 int vocab, const int* __restrict__ targets,
                                                                 const uint32_t* __restrict__ mask,
                                                                 int64_t mask_stride, float* __restrict__ out) {
  __shared__ float red[kThreads / 64];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (int64_t)row * ld;
  const uint32_t* mk = mask ? mask + (int64_t)row * mask_stride : nullptr;
  float m = -INFINITY;
  for (int v = threadIdx.x; v < vocab; v += kThreads)
    if (allowed(mk, v)) m = fmaxf(m, x[v]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = wg_max(red);
  __syncthreads();
  float s = 0.f;
  for (int v = threadIdx.x; v < vocab; v += kThreads)
    if (allowed(mk, v)) s += expf(x[v] - m);
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    s = (red[0] + red[1]) + (red[2] + red[3]);  // (wg_sum4's order, written out: see the comment there)
    const int t = min(max(targets[row], 0), vocab - 1);
    // (a log-probability: rounding may not lift it above 0; a masked-out target stays -inf)
    out[row] = allowed(mk, t) ? fminf((x[t] - m) - logf(s), 0.f) : -INFINITY;
  }
}

}  // namespace

extern "C" int vwa_token_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* targets,
                                 const uint32_t* mask, int64_t mask_stride, float* out, hipStream_t st) {
  if (rows < 1 || vocab < 1 || ld < vocab || mask_stride < 0) return -1;
  hipLaunchKernelGGL(token_logprob_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, targets, mask,
                     mask_stride, out);
  return (int)hipGetLastError();
}

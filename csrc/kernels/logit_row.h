// A row of f32 logits read through the sampler's packed allow-mask: the device helpers shared by
// the step kernels that do so (score_step, ts_rules, token_logprob, sot_probe, beam_select).
//
// Everything here is force-inlined and holds no barrier: a kernel's loads, __syncthreads() and
// stores stay where its own header comment argues from.
#pragma once
#include "kernels/common.h"

namespace vwa {

VWA_DEVICE float neg_inf() { return -__builtin_huge_valf(); }

// Bit c of the packed allow-mask (word c >> 5, bit c & 31).  A null mask allows every column;
// allowed<true> is for a kernel whose launcher rejects a null mask (no test for it is compiled).
template <bool kRequired = false>
VWA_DEVICE bool allowed(const uint32_t* mask, int c) {
  return (!kRequired && !mask) || ((mask[c >> 5] >> (c & 31)) & 1u);
}

// the allow-bits of columns c .. c + 3 (mask not null, c + 3 < vocab)
VWA_DEVICE uint32_t allowed4(const uint32_t* mask, int c) {
  const int w = c >> 5, w3 = (c + 3) >> 5;
  uint64_t bits = mask[w];
  if (w3 != w) bits |= (uint64_t)mask[w3] << 32;
  return (uint32_t)(bits >> (c & 31)) & 0xFu;
}

// Columns [lo, hi) of row x shared among a workgroup's kThreads threads: one(c) for the columns
// before the first 16-byte aligned address and after the last whole float4, four(c) for the float4
// at c between.  An empty range (lo >= hi) calls neither.
template <int kThreads, class F1, class F4>
VWA_DEVICE void sweep(const float* x, int lo, int hi, int tid, F1 one, F4 four) {
  int head = (int)(((16u - (unsigned)((uintptr_t)(x + lo) & 15u)) & 15u) >> 2);
  if (head > hi - lo) head = hi - lo;
  const int body = lo + head;
  const int nvec = (hi - body) >> 2;
  const int tail = body + (nvec << 2);
  if (tid < head) one(lo + tid);
  for (int i = tid; i < nvec; i += kThreads) four(body + (i << 2));
  if (tid < hi - tail) one(tail + tid);
}

// Online log-sum-exp, one read of each value: log(sum exp(v)) = m + log(s) over the values added
// so far; -inf values (and NaNs) add nothing.  It works on the kernel's own locals -- the running
// maximum m (from -inf), the sum s (from 0) and its -inf constant -- by reference, as the lambdas it
// replaces captured them, so the kernels compile to the code they had.
struct OnlineLse {
  float& m;
  float& s;
  const float& ninf;
  VWA_DEVICE void add(float v) {
    if (v > m) {
      s = s * expf(m - v) + 1.f;
      m = v;
    } else if (v > ninf) {
      s += expf(v - m);
    }
  }
  // the components of v whose bit in k (allowed4) is set
  VWA_DEVICE void add4(float4 v, uint32_t k) {
    if (k & 1u) add(v.x);
    if (k & 2u) add(v.y);
    if (k & 4u) add(v.z);
    if (k & 8u) add(v.w);
  }
  // s scaled to the workgroup's maximum bm >= m: this lane's summand of the workgroup's sum
  VWA_DEVICE float scaled(float bm) const { return s > 0.f ? s * expf(m - bm) : 0.f; }
};

// Workgroup reductions of the waves' partials in LDS, read after the caller's own __syncthreads()
// (lane 0 of wave w stored sh[w] before it); every thread gets the result.
// The maximum is exact in any order: four waves pair up, any other count folds from -inf.
template <int kWaves>
VWA_DEVICE float wg_max(const float (&sh)[kWaves]) {
  if constexpr (kWaves == 4) {
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  } else {
    float v = neg_inf();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) v = fmaxf(v, sh[w]);
    return v;
  }
}
// The sum of four waves' partials, in the order (0 + 1) + (2 + 3), which is part of the contract: it
// decides the rounding.  (The eight-wave kernels add theirs left to right, in place; token_logprob
// writes this sum out, because through a call the compiler pairs its LDS loads another way.)
VWA_DEVICE float wg_sum4(const float* sh) { return (sh[0] + sh[1]) + (sh[2] + sh[3]); }

}  // namespace vwa

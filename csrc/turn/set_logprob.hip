// The set log-probability (see turn.h for the contract): one workgroup of eight waves per row.
//
// The lanes share the row's columns [0, vocab) exactly as logit_row.h's sweep() deals them -- 16
// bytes per lane wherever the address allows, scalar head and tail, lane t taking the float4s t,
// t + 512, ... in that order -- but the body issues kBatch of a lane's loads before it uses the
// first, so four 16-byte loads are in flight per lane (the row was just written by the LM head and
// mostly sits in L2 / MALL: the sweep is latency-bound, not bandwidth-bound).  Every value feeds
// two online log-sum-exps in that one read: all columns (A), and the columns whose set bit is on
// (S).  Two workgroup reductions per sum follow, as in score_step.hip (wave shuffles, then eight
// values through LDS): the maxima first, which are exact in any order, then the sums, each lane's
// scaled once to the common maximum and the eight waves' added left to right.  Every order is
// fixed, so a launch repeats its bits.  Thread 0 alone writes, and only out[2 r], out[2 r + 1].
#include "kernels/logit_row.h"
#include "turn/turn.h"

#include <math.h>

using namespace vwa;

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kBatch = 4;  // float4 loads a lane has in flight

// sweep() of logit_row.h -- the same split of [0, hi) into head, float4 body and tail, the same
// columns per thread in the same order -- with the body's loads issued kBatch at a time; four(c, v)
// gets the float4 at c already loaded.
template <class F1, class F4>
VWA_DEVICE void sweep_loaded(const float* x, int hi, int tid, F1 one, F4 four) {
  int head = (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2);
  if (head > hi) head = hi;
  const int nvec = (hi - head) >> 2;
  const int tail = head + (nvec << 2);
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  if (tid < head) one(tid);
  int i = tid;
  for (; i + (kBatch - 1) * kThreads < nvec; i += kBatch * kThreads) {
    float4 v[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) v[k] = xv[i + k * kThreads];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) four(head + ((i + k * kThreads) << 2), v[k]);
  }
  for (; i < nvec; i += kThreads) four(head + (i << 2), xv[i]);
  if (tid < hi - tail) one(tail + tid);
}

__global__ __launch_bounds__(kThreads) void set_logprob_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                               const int* __restrict__ set, int64_t set_ld,
                                                               float* __restrict__ out) {
  __shared__ float sh_ma[kWaves], sh_ms[kWaves], sh_sa[kWaves], sh_ss[kWaves];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const float* x = logits + (int64_t)r * ld;
  const uint32_t* srow = reinterpret_cast<const uint32_t*>(set) + (int64_t)r * set_ld;
  const float ninf = neg_inf();
  float ma = ninf, sa = 0.f, ms = ninf, ss = 0.f;
  OnlineLse all{ma, sa, ninf}, in_set{ms, ss, ninf};
  sweep_loaded(
      x, vocab, tid,
      [&](int c) {
        const float v = x[c];
        all.add(v);
        if (allowed<true>(srow, c)) in_set.add(v);
      },
      [&](int c, float4 v) {
        all.add4(v, 0xFu);
        in_set.add4(v, allowed4(srow, c));
      });

  const int wave = tid >> 6, lane = tid & 63;
  const float wma = wave_max(ma), wms = wave_max(ms);
  if (lane == 0) {
    sh_ma[wave] = wma;
    sh_ms[wave] = wms;
  }
  __syncthreads();
  const float bma = wg_max(sh_ma), bms = wg_max(sh_ms);
  const float wsa = wave_sum(all.scaled(bma)), wss = wave_sum(in_set.scaled(bms));
  if (lane == 0) {
    sh_sa[wave] = wsa;
    sh_ss[wave] = wss;
  }
  __syncthreads();
  if (tid != 0) return;
  float SA = 0.f, SS = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    SA += sh_sa[w];
    SS += sh_ss[w];
  }
  const float A = SA > 0.f ? bma + logf(SA) : ninf;
  float lp = ninf;
  if (SS > 0.f && SA > 0.f) lp = fminf((bms + logf(SS)) - A, 0.f);
  out[2 * r] = lp;
  out[2 * r + 1] = A;
}

}  // namespace

extern "C" int vwa_set_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* set, int64_t set_ld,
                               float* out, hipStream_t st) {
  if (!logits || !set || !out) return -1;
  if (rows < 1 || rows > kTurnMaxRows) return -2;
  if (vocab < 1 || vocab > kTurnMaxVocab || ld < vocab) return -3;
  const int64_t words = (vocab + 31) / 32;
  if (set_ld != 0 && set_ld < words) return -5;
  const int64_t out_b = 8 * (int64_t)rows;
  if (overlap(out, out_b, logits, 4 * ((int64_t)(rows - 1) * ld + vocab))) return -6;
  if (overlap(out, out_b, set, 4 * ((int64_t)(rows - 1) * set_ld + words))) return -6;
  hipLaunchKernelGGL(set_logprob_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, set, set_ld, out);
  return (int)hipGetLastError();
}

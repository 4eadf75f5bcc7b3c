// The per-sequence log-probabilities (see rescore.h for the contract): two kernels on one stream.
//
// Row pass: one workgroup of eight waves per row, the sweep of csrc/turn/set_logprob.hip.  The lanes
// share the row's columns [0, vocab) exactly as logit_row.h's sweep() deals them -- 16 bytes per lane
// wherever the address allows, scalar head and tail, lane t taking the float4s t, t + 512, ... in
// that order -- with kBatch of a lane's loads issued before the first is used (the row was just
// written by the LM head and mostly sits in L2 / MALL: the sweep is latency-bound).  Every value
// feeds the online log-sum-exp of all columns (A); in a row whose target is -1 it also feeds the one
// of the end set's columns (S).  The target is the same for the whole workgroup, so that branch does
// not diverge.  Two workgroup reductions per sum follow (wave shuffles, then eight values through
// LDS): the maxima first, exact in any order, then the sums, each lane's scaled once to the common
// maximum and the eight waves' added left to right.  Thread 0 alone writes, and only lp[r].  An id
// target is range-checked before x[target] is read; a target outside [-1, vocab) leaves before any
// load or barrier.
//
// Sum pass: one wave, lane s < n_seq walks seq[0 .. rows) in order and adds lp[r] where seq[r] == s
// (seq is compared, never used as an index).  It reads what the row pass wrote: stream order is the
// only hand-off.
#include "kernels/logit_row.h"
#include "rescore/rescore.h"

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

__global__ __launch_bounds__(kThreads) void row_logprob_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                               const int* __restrict__ target,
                                                               const int* __restrict__ end_set,
                                                               float* __restrict__ lp) {
  __shared__ float sh_ma[kWaves], sh_ms[kWaves], sh_sa[kWaves], sh_ss[kWaves];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const float ninf = neg_inf();
  const int t = target[r];
  if (t < -1 || t >= vocab) {  // (the whole workgroup: no barrier has been reached)
    if (tid == 0) lp[r] = ninf;
    return;
  }
  const bool set = t == -1;
  const float* x = logits + (int64_t)r * ld;
  const uint32_t* srow = reinterpret_cast<const uint32_t*>(end_set);
  float ma = ninf, sa = 0.f, ms = ninf, ss = 0.f;
  OnlineLse all{ma, sa, ninf}, in_set{ms, ss, ninf};
  sweep_loaded(
      x, vocab, tid,
      [&](int c) {
        const float v = x[c];
        all.add(v);
        if (set && allowed<true>(srow, c)) in_set.add(v);
      },
      [&](int c, float4 v) {
        all.add4(v, 0xFu);
        if (set) in_set.add4(v, allowed4(srow, c));
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
  float out = ninf;
  if (SA > 0.f) {
    const float A = bma + logf(SA);
    if (set) {
      if (SS > 0.f) out = fminf((bms + logf(SS)) - A, 0.f);
    } else {
      const float xt = x[t];  // 0 <= t < vocab, checked above
      if (xt > ninf) out = fminf(xt - A, 0.f);  // (false for a NaN)
    }
  }
  lp[r] = out;
}

__global__ __launch_bounds__(64) void seq_sum_kernel(const float* __restrict__ lp, const int* __restrict__ seq, int rows,
                                                     int n_seq, const float* __restrict__ acc_in,
                                                     float* __restrict__ acc_out) {
  const int s = threadIdx.x;
  if (s >= n_seq) return;
  float acc = acc_in ? acc_in[s] : 0.f;
  for (int r = 0; r < rows; ++r)
    if (seq[r] == s) acc += lp[r];
  acc_out[s] = acc;
}

}  // namespace

extern "C" int vwa_seq_logprob(const float* logits, int64_t ld, int rows, int vocab, const int* target,
                               const int* end_set, const int* seq, int n_seq, const float* acc_in, float* lp,
                               float* acc_out, hipStream_t st) {
  if (!logits || !target || !end_set || !seq || !lp || !acc_out) return -1;
  if (rows < 1 || rows > kRescoreMaxRows) return -2;
  if (vocab < 1 || vocab > kRescoreMaxVocab || ld < vocab) return -3;
  if (n_seq < 1 || n_seq > kRescoreMaxSeq) return -4;
  const int64_t words = (vocab + 31) / 32;
  const int64_t rows_b = 4 * (int64_t)rows, seq_b = 4 * (int64_t)n_seq;
  const struct {
    const void* p;
    int64_t n;
  } ins[] = {{logits, 4 * ((int64_t)(rows - 1) * ld + vocab)}, {target, rows_b}, {end_set, 4 * words},
             {seq, rows_b}, {acc_in, acc_in ? seq_b : 0}};
  for (const auto& in : ins) {
    if (!in.n) continue;
    if (overlap(lp, rows_b, in.p, in.n) || overlap(acc_out, seq_b, in.p, in.n)) return -6;
  }
  if (overlap(lp, rows_b, acc_out, seq_b)) return -6;
  hipLaunchKernelGGL(row_logprob_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, target, end_set, lp);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  // lp is __restrict__ const in the second kernel only: the two never run as one
  hipLaunchKernelGGL(seq_sum_kernel, dim3(1), dim3(64), 0, st, lp, seq, rows, n_seq, acc_in, acc_out);
  return (int)hipGetLastError();
}

// The timestamp rules step (see tsrules.h for the contract): one workgroup of eight waves per row.
//
// Rules 1-4 leave the allowed text a range [tx_lo, ts_begin - 1) and the allowed timestamps a range
// [a, b) of indices, all worked out by every lane from the same few loads.  The lanes then share
// the two ranges -- 16 bytes per lane wherever the address allows, scalar head and tail -- for the
// text's maximum and the timestamps' online log-sum-exp (running max and sum, one read).  Two
// workgroup reductions follow (wave shuffles, then eight values through LDS): the maxima first,
// which are exact in any order, then the sums, each lane's scaled once to the common maximum.
// Nothing is written before the second reduction's barrier, so no lane reads a column another has
// banned, and the state goes out after the first barrier: with state_out == state_in every wave has
// read the row's cells by then.
#include "kernels/logit_row.h"
#include "tsrules/tsrules.h"

#include <math.h>

using namespace vwa;

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;

// sweep() of [lo, hi); the rules often leave a range empty, which then costs one uniform branch
template <class F1, class F4>
VWA_DEVICE void sweep_range(const float* x, int lo, int hi, int tid, F1 one, F4 four) {
  if (lo < hi) sweep<kThreads>(x, lo, hi, tid, one, four);
}

VWA_DEVICE void ban(float* x, int lo, int hi, int tid) {
  const float ninf = neg_inf();
  sweep_range(x, lo, hi, tid, [&](int c) { x[c] = ninf; },
              [&](int c) { *reinterpret_cast<float4*>(x + c) = make_float4(ninf, ninf, ninf, ninf); });
}

__global__ __launch_bounds__(kThreads) void ts_rules_kernel(
    float* logits, int64_t ld, int vocab, int eot, int ts_begin, int max_initial, const int* __restrict__ mask,
    int64_t mask_ld, const int* __restrict__ enable, const int* state_in, int* state_out,
    const int* __restrict__ tokens) {
  __shared__ float sh_M[kWaves], sh_m[kWaves], sh_s[kWaves];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int n_ts = vocab - ts_begin;
  const int* si = state_in + 4 * r;
  int* so = state_out + 4 * r;
  const int s0 = si[0], s1 = si[1], s2 = si[2], s3 = si[3];
  int tok = 0;
  bool skip = enable[r] <= 0;
  if (!skip && tokens) {
    tok = tokens[r];
    skip = tok < 0 || tok >= vocab;
  }
  if (skip) {  // (the same values the row's cells hold: in place, a wave that reads late reads them too)
    if (tid == 0) { so[0] = s0; so[1] = s1; so[2] = s2; so[3] = s3; }
    return;
  }
  int n = s0, last = s1, prev = s2, last_ts = s3;
  if (n < 0 || n > 2 || last_ts < -1 || last_ts >= n_ts) { n = 0; last = -1; prev = -1; last_ts = -1; }
  if (tokens) {
    prev = last;
    last = tok;
    n = n < 2 ? n + 1 : 2;
    if (tok >= ts_begin) last_ts = tok - ts_begin;  // (tok < vocab: below n_ts)
  }
  const bool last_was = n >= 1 && last >= ts_begin;
  const bool pen_was = n < 2 || prev >= ts_begin;
  const bool closing = last_was && !pen_was;
  // the timestamps rules 2-4 leave: indices [a, b)
  int a = 0, b = n_ts;
  if (last_was && pen_was) a = n_ts;
  if (last_ts >= 0) {
    const int lim = closing ? last_ts : last_ts + 1;
    if (lim > a) a = lim;
  }
  if (n == 0 && max_initial >= 0 && max_initial < n_ts) b = max_initial + 1;
  if (a > b) a = b;
  // the text they leave: [tx_lo, ts_begin - 1)
  const int tx_hi = ts_begin - 1;
  const int tx_lo = n == 0 ? tx_hi : (closing ? (eot < tx_hi ? eot : tx_hi) : 0);

  float* x = logits + (int64_t)r * ld;
  const uint32_t* mrow = reinterpret_cast<const uint32_t*>(mask) + (int64_t)r * mask_ld;
  const float ninf = neg_inf();
  float M = ninf;
  sweep_range(x, tx_lo, tx_hi, tid, [&](int c) { if (allowed<true>(mrow, c)) M = fmaxf(M, x[c]); },
              [&](int c) {
                const float4 v = *reinterpret_cast<const float4*>(x + c);
                const uint32_t k = allowed4(mrow, c);
                if (k & 1u) M = fmaxf(M, v.x);
                if (k & 2u) M = fmaxf(M, v.y);
                if (k & 4u) M = fmaxf(M, v.z);
                if (k & 8u) M = fmaxf(M, v.w);
              });
  float m = ninf, s = 0.f;
  OnlineLse acc{m, s, ninf};
  sweep_range(x, ts_begin + a, ts_begin + b, tid, [&](int c) { if (allowed<true>(mrow, c)) acc.add(x[c]); },
              [&](int c) { acc.add4(*reinterpret_cast<const float4*>(x + c), allowed4(mrow, c)); });

  const int wave = tid >> 6, lane = tid & 63;
  const float wM = wave_max(M), wm = wave_max(m);
  if (lane == 0) { sh_M[wave] = wM; sh_m[wave] = wm; }
  __syncthreads();
  if (tid == 0) { so[0] = n; so[1] = last; so[2] = prev; so[3] = last_ts; }
  const float bM = wg_max(sh_M), bm = wg_max(sh_m);
  const float ws = wave_sum(acc.scaled(bm));
  if (lane == 0) sh_s[wave] = ws;
  __syncthreads();
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) S += sh_s[w];
  const float T = S > 0.f ? bm + logf(S) : ninf;

  // the bans, now that every read is done
  if (n == 0 || T > bM) {
    ban(x, 0, ts_begin, tid);
  } else {
    if (closing) ban(x, 0, eot, tid);
    if (tid == 0) x[ts_begin - 1] = ninf;
  }
  ban(x, ts_begin, ts_begin + a, tid);
  ban(x, ts_begin + b, vocab, tid);
}

}  // namespace

extern "C" int vwa_ts_rules_step(float* logits, int64_t ld, int rows, int vocab, int eot, int ts_begin,
                                 int max_initial, const int* mask, int64_t mask_ld, const int* enable,
                                 const int* state_in, int* state_out, const int* tokens, hipStream_t st) {
  if (!logits || !mask || !enable || !state_in || !state_out) return -1;
  if (rows < 1 || rows > kTsMaxRows) return -2;
  if (vocab < 1 || vocab > kTsMaxVocab || ld < vocab) return -3;
  if (eot < 0 || eot >= ts_begin || ts_begin >= vocab) return -4;
  if (mask_ld != 0 && mask_ld < (vocab + 31) / 32) return -5;
  if (state_in != state_out && overlap(state_in, 16 * (int64_t)rows, state_out, 16 * (int64_t)rows)) return -6;
  hipLaunchKernelGGL(ts_rules_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, eot, ts_begin, max_initial,
                     mask, mask_ld, enable, state_in, state_out, tokens);
  return (int)hipGetLastError();
}

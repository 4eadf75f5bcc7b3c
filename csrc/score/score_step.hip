// The score step (see score.h for the contract): one workgroup of eight waves per row.
//
// The lanes share the row's columns [0, vocab) -- 16 bytes per lane wherever the address allows,
// scalar head and tail -- for an online log-sum-exp over the ids the mask allows (running max and
// sum, one read).  Two workgroup reductions follow, as in ts_rules.hip rule 5 (wave shuffles, then
// eight values through LDS): the maxima first, which are exact in any order, then the sums, each
// lane's scaled once to the common maximum.  Every order is fixed, so a launch repeats its bits.
// Every thread reads the row's state cells before the first barrier and thread 0 writes them after
// the second: with sum_out == sum_in and cnt_out == cnt_in no wave reads a cell already written.
#include "kernels/logit_row.h"
#include "score/score.h"

#include <math.h>

using namespace vwa;

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void score_step_kernel(
    const float* __restrict__ logits, int64_t ld, int vocab, int eot, const int* __restrict__ mask, int64_t mask_ld,
    const int* __restrict__ enable, const int* __restrict__ tokens, const float* sum_in, float* sum_out,
    const int* cnt_in, int* cnt_out, float* step_lp) {
  __shared__ float sh_m[kWaves], sh_s[kWaves];
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const float sum0 = sum_in[r];
  const int n0 = cnt_in[2 * r], done0 = cnt_in[2 * r + 1];
  int tok = 0;
  bool skip = enable[r] <= 0 || done0 != 0;
  if (!skip) {
    tok = tokens[r];
    skip = tok < 0 || tok >= vocab;
  }
  if (skip) {  // (the same values the row's cells hold: in place, a wave that reads late reads them too)
    if (tid == 0) {
      sum_out[r] = sum0;
      cnt_out[2 * r] = n0;
      cnt_out[2 * r + 1] = done0;
      if (step_lp) step_lp[r] = 0.f;
    }
    return;
  }
  const float* x = logits + (int64_t)r * ld;
  const uint32_t* mrow = reinterpret_cast<const uint32_t*>(mask) + (int64_t)r * mask_ld;
  const float ninf = neg_inf();
  float m = ninf, s = 0.f;
  OnlineLse acc{m, s, ninf};
  sweep<kThreads>(x, 0, vocab, tid, [&](int c) { if (allowed<true>(mrow, c)) acc.add(x[c]); },
                  [&](int c) { acc.add4(*reinterpret_cast<const float4*>(x + c), allowed4(mrow, c)); });

  const int wave = tid >> 6, lane = tid & 63;
  const float wm = wave_max(m);
  if (lane == 0) sh_m[wave] = wm;
  __syncthreads();
  const float bm = wg_max(sh_m);
  const float ws = wave_sum(acc.scaled(bm));
  if (lane == 0) sh_s[wave] = ws;
  __syncthreads();
  if (tid != 0) return;
  float S = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) S += sh_s[w];
  const float xt = allowed<true>(mrow, tok) ? x[tok] : ninf;  // (tok < vocab: tested above)
  float lp = ninf;
  if (xt > ninf && S > 0.f) lp = fminf(xt - (bm + logf(S)), 0.f);
  sum_out[r] = sum0 + lp;
  cnt_out[2 * r] = n0 + 1;
  cnt_out[2 * r + 1] = tok == eot ? 1 : 0;
  if (step_lp) step_lp[r] = lp;
}

}  // namespace

extern "C" int vwa_score_step(const float* logits, int64_t ld, int rows, int vocab, int eot, const int* mask,
                              int64_t mask_ld, const int* enable, const int* tokens, const float* sum_in,
                              float* sum_out, const int* cnt_in, int* cnt_out, float* step_lp, hipStream_t st) {
  if (!logits || !mask || !enable || !tokens || !sum_in || !sum_out || !cnt_in || !cnt_out) return -1;
  if (rows < 1 || rows > kScoreMaxRows) return -2;
  if (vocab < 1 || vocab > kScoreMaxVocab || ld < vocab) return -3;
  if (eot < 0 || eot >= vocab) return -4;
  if (mask_ld != 0 && mask_ld < (vocab + 31) / 32) return -5;
  // the state tensors and step_lp: the two in-place pairs may coincide exactly, nothing else may overlap
  const void* p[5] = {sum_in, sum_out, cnt_in, cnt_out, step_lp};
  const int64_t nb[5] = {4 * (int64_t)rows, 4 * (int64_t)rows, 8 * (int64_t)rows, 8 * (int64_t)rows, 4 * (int64_t)rows};
  for (int i = 0; i < 5; ++i)
    for (int j = i + 1; j < 5; ++j) {
      if (!p[i] || !p[j]) continue;
      if (p[i] == p[j] && ((i == 0 && j == 1) || (i == 2 && j == 3))) continue;
      if (overlap(p[i], nb[i], p[j], nb[j])) return -6;
    }
  hipLaunchKernelGGL(score_step_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, eot, mask, mask_ld,
                     enable, tokens, sum_in, sum_out, cnt_in, cnt_out, step_lp);
  return (int)hipGetLastError();
}

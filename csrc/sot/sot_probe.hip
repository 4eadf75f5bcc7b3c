// The start-of-transcript probe: no-speech probability and language distribution of each row's
// logits (see sot.h for the contract).
//
// One 256-thread workgroup per row.  Two sweeps of the (L2-resident) row give the softmax
// denominator over the vocabulary -- the maximum, then the sum of exp(x - max) -- as token_logprob
// does.  The language part is one lane per language (n_lang <= 128): the maximum over the allowed
// ids, the lowest lane holding it (compared on the raw logits, so ties resolve exactly), the sum of
// exp(x - max) and each lane's own probability.
#include "kernels/logit_row.h"
#include "sot/sot.h"

using namespace vwa;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kNone = 1 << 30;

struct Allow {
  uint32_t w[4];
};

VWA_DEVICE int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(kThreads) void sot_probe_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                             int lang0, int n_lang, Allow allow, int no_speech_id,
                                                             float* __restrict__ lang_probs, int64_t ldp,
                                                             int* __restrict__ lang_tok, float* __restrict__ lang_conf,
                                                             float* __restrict__ no_speech, int* __restrict__ tok_dst,
                                                             const int* __restrict__ dst_rows, int n_dst) {
  __shared__ float red[4][kWaves];
  __shared__ int redi[2][kWaves];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)row * ld;

  // this lane's language (tid < n_lang <= 128; the launcher checked lang0 + n_lang <= vocab)
  const bool mine = tid < n_lang && ((allow.w[(tid >> 5) & 3] >> (tid & 31)) & 1u);
  const float xl = mine ? x[lang0 + tid] : -INFINITY;

  float m = -INFINITY;
  for (int v = tid; v < vocab; v += kThreads) m = fmaxf(m, x[v]);
  m = wave_max(m);
  const float ml_w = wave_max(xl);  // (fmaxf drops a NaN operand)
  const int low_w = wave_min_int(mine ? tid : kNone);
  if (lane == 0) {
    red[0][wave] = m;
    red[1][wave] = ml_w;
    redi[0][wave] = low_w;
  }
  __syncthreads();
  m = wg_max(red[0]);
  const float ml = wg_max(red[1]);
  const int low = min(min(redi[0][0], redi[0][1]), min(redi[0][2], redi[0][3]));  // lowest allowed language

  float s = 0.f;
  for (int v = tid; v < vocab; v += kThreads) s += expf(x[v] - m);
  s = wave_sum(s);
  // (all of A at -inf: -inf - -inf = NaN, as the contract says)
  const float el = mine ? expf(xl - ml) : 0.f;
  const float sl_w = wave_sum(el);
  const int best_w = wave_min_int(mine && xl == ml ? tid : kNone);
  if (lane == 0) {
    red[2][wave] = s;
    red[3][wave] = sl_w;
    redi[1][wave] = best_w;
  }
  __syncthreads();
  s = wg_sum4(red[2]);
  const float sl = wg_sum4(red[3]);
  int best = min(min(redi[1][0], redi[1][1]), min(redi[1][2], redi[1][3]));
  if (best == kNone) best = low;  // no logit of A equals the maximum (all NaN): still an id of A

  const float p = mine ? el / sl : 0.f;
  if (tid < n_lang) lang_probs[(int64_t)row * ldp + tid] = p;
  if (tid == best) {
    lang_conf[row] = p;
    lang_tok[row] = lang0 + best;
    if (tok_dst) {
      const int d = dst_rows[row];
      if (d >= 0 && d < n_dst) tok_dst[d] = lang0 + best;
    }
  }
  if (tid == 0) no_speech[row] = expf(x[no_speech_id] - m) / s;
}

}  // namespace

extern "C" int vwa_sot_probe(const float* logits, int64_t ld, int rows, int vocab, int lang0, int n_lang,
                             const uint32_t allow[4], int no_speech_id, float* lang_probs, int64_t ldp, int* lang_tok,
                             float* lang_conf, float* no_speech, int* tok_dst, const int* dst_rows, int n_dst,
                             hipStream_t st) {
  if (!logits || !allow || !lang_probs || !lang_tok || !lang_conf || !no_speech) return -1;
  if (rows < 1 || n_lang < 1 || n_lang > kSotMaxLangs || lang0 < 0 || vocab < 1) return -2;
  if ((int64_t)lang0 + n_lang > vocab || vocab > ld || no_speech_id < 0 || no_speech_id >= vocab || ldp < n_lang)
    return -3;
  if ((tok_dst == nullptr) != (dst_rows == nullptr) || (tok_dst && n_dst < 1)) return -4;
  Allow a;
  bool any = false;
  for (int i = 0; i < 4; ++i) {
    const int bits = n_lang - 32 * i;  // bits of word i below n_lang
    const uint32_t keep = bits >= 32 ? 0xffffffffu : bits <= 0 ? 0u : ((1u << bits) - 1u);
    a.w[i] = allow[i] & keep;
    any = any || a.w[i] != 0;
  }
  if (!any) return -5;
  hipLaunchKernelGGL(sot_probe_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, lang0, n_lang, a,
                     no_speech_id, lang_probs, ldp, lang_tok, lang_conf, no_speech, tok_dst, dst_rows, n_dst);
  return (int)hipGetLastError();
}

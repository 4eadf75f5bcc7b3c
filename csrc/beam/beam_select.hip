// The beam step's selection: per group of W beams the 2 W best (beam, token) continuations by
// cumulative log-probability (see beam.h for the contract).
//
// A row (207 KB of f32 for Whisper's vocabulary) is cut into tiles of kBeamTile columns; a
// 256-thread workgroup holds its tile in registers, 32 columns a lane.
//   1. lse_part:  per (row, tile) the maximum m_t over the allowed columns and s_t = sum exp(x - m_t).
//   2. row_topk:  per (row, tile) lse = M + logf(sum_t s_t exp(m_t - M)), the tiles taken in order
//                 (M = max_t m_t; every lane runs the same loop, so every workgroup of a row holds
//                 the same lse); the scores cum + (x - lse) of the tile; K rounds of a block-wide
//                 arg-best over the registers, the winner struck out after each round.
//   3. group_merge: per group, K rounds over its rows' tile lists: the best entry strictly after the
//                 previous round's in the total order (score descending, beam * vocab + token
//                 ascending).  The lists are only read, in index order.
// A row can give the group no more than its own K best and a tile the row no more than its own K
// best, so nothing is lost.  Ties are compared on the f32 scores themselves: two logits whose
// scores round to the same f32 are ordered by their ids, as the contract says.
#include "kernels/logit_row.h"
#include "beam/beam.h"

using namespace vwa;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = kBeamTile / kThreads;  // columns a lane holds
constexpr int kList = 2 * kBeamMaxWidth;    // entries of a (row, tile) list
constexpr int kNoKey = 0x7fffffff;

VWA_DEVICE bool finite(float v) { return fabsf(v) < INFINITY; }  // (false for a NaN)

// (score, key) pairs: the better one has the higher score, among equal scores the lower key
VWA_DEVICE bool better(float s, int k, float s0, int k0) { return s > s0 || (s == s0 && k < k0); }

VWA_DEVICE void wave_best(float& s, int& k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(s, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    if (better(os, ok, s, k)) {
      s = os;
      k = ok;
    }
  }
}

// the block's best pair in every lane (red_*: one buffer per round parity, so one barrier a round)
VWA_DEVICE void block_best(float& s, int& k, float* red_s, int* red_k) {
  wave_best(s, k);
  if ((threadIdx.x & 63) == 0) {
    red_s[threadIdx.x >> 6] = s;
    red_k[threadIdx.x >> 6] = k;
  }
  __syncthreads();
  s = red_s[0];
  k = red_k[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (better(red_s[w], red_k[w], s, k)) {
      s = red_s[w];
      k = red_k[w];
    }
}

// the tile's allowed logits, -inf elsewhere (columns >= vocab are not read)
VWA_DEVICE void load_tile(const float* x, const uint32_t* mk, int c0, int vocab, float (&xv)[kPer]) {
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const int c = c0 + e * kThreads + (int)threadIdx.x;
    xv[e] = (c < vocab && allowed(mk, c)) ? x[c] : -INFINITY;
  }
}

__global__ __launch_bounds__(kThreads) void lse_part_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                            const uint32_t* __restrict__ mask, int64_t mask_stride,
                                                            float* __restrict__ part_m, float* __restrict__ part_s) {
  __shared__ float red[2][kWaves];
  const int tile = blockIdx.x, row = blockIdx.y, T = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (int64_t)row * ld;
  const uint32_t* mk = mask ? mask + (int64_t)row * mask_stride : nullptr;
  float xv[kPer];
  load_tile(x, mk, tile * kBeamTile, vocab, xv);
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < kPer; ++e) m = fmaxf(m, xv[e]);
  m = wave_max(m);
  if (lane == 0) red[0][wave] = m;
  __syncthreads();
  m = wg_max(red[0]);
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int e = 0; e < kPer; ++e) s += expf(xv[e] - m);  // (expf(-inf) = 0: a column that is not allowed)
  }
  s = wave_sum(s);
  if (lane == 0) red[1][wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    part_m[row * T + tile] = m;
    part_s[row * T + tile] = wg_sum4(red[1]);
  }
}

__global__ __launch_bounds__(kThreads) void row_topk_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                            const uint32_t* __restrict__ mask, int64_t mask_stride,
                                                            const float* __restrict__ cum,
                                                            const float* __restrict__ part_m,
                                                            const float* __restrict__ part_s, int K,
                                                            float* __restrict__ list_s, int* __restrict__ list_c) {
  __shared__ float red_s[2][kWaves];
  __shared__ int red_k[2][kWaves];
  const int tile = blockIdx.x, row = blockIdx.y, T = gridDim.x;
  const int c0 = tile * kBeamTile;
  float* out_s = list_s + (int64_t)(row * T + tile) * kList;
  int* out_c = list_c + (int64_t)(row * T + tile) * kList;
  const float base = cum[row];
  float M = -INFINITY;
  for (int t = 0; t < T; ++t) M = fmaxf(M, part_m[row * T + t]);
  float S = 0.f;
  for (int t = 0; t < T; ++t) {
    const float mt = part_m[row * T + t];
    if (mt > -INFINITY) S += part_s[row * T + t] * expf(mt - M);
  }
  const float lse = M + logf(S);
  float sc[kPer];
  if (base > -INFINITY && finite(lse)) {  // (uniform: a dead row, or one with nothing allowed, gives no candidate)
    const uint32_t* mk = mask ? mask + (int64_t)row * mask_stride : nullptr;
    load_tile(logits + (int64_t)row * ld, mk, c0, vocab, sc);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const float s = base + (sc[e] - lse);
      sc[e] = finite(s) ? s : -INFINITY;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e) sc[e] = -INFINITY;
  }
  for (int k = 0; k < K; ++k) {
    float bs = -INFINITY;
    int bc = kNoKey;
#pragma unroll
    for (int e = 0; e < kPer; ++e)  // (columns ascend with e: a strict > keeps the lowest of equals)
      if (sc[e] > bs) {
        bs = sc[e];
        bc = c0 + e * kThreads + (int)threadIdx.x;
      }
    block_best(bs, bc, red_s[k & 1], red_k[k & 1]);
    if (!(bs > -INFINITY)) {  // (uniform) the tile is exhausted
      if (threadIdx.x == 0)
        for (int j = k; j < K; ++j) {
          out_s[j] = -INFINITY;
          out_c[j] = -1;
        }
      break;
    }
    if (threadIdx.x == 0) {
      out_s[k] = bs;
      out_c[k] = bc;
    }
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (c0 + e * kThreads + (int)threadIdx.x == bc) sc[e] = -INFINITY;
  }
}

__global__ __launch_bounds__(kThreads) void group_merge_kernel(const float* __restrict__ list_s,
                                                               const int* __restrict__ list_c, int W, int T, int K,
                                                               int vocab, float* __restrict__ cand_score,
                                                               int* __restrict__ cand_beam, int* __restrict__ cand_tok,
                                                               int64_t ldc) {
  __shared__ float red_s[2][kWaves];
  __shared__ int red_k[2][kWaves];
  const int g = blockIdx.x;
  const int per_beam = T * K, n = W * per_beam;
  float prev_s = INFINITY;
  int prev_k = -1;
  for (int r = 0; r < K; ++r) {
    float bs = -INFINITY;
    int bk = kNoKey;
    for (int i = threadIdx.x; i < n; i += kThreads) {
      const int b = i / per_beam, rem = i - b * per_beam, t = rem / K, k = rem - t * K;
      const int64_t at = (int64_t)((g * W + b) * T + t) * kList + k;
      const int c = list_c[at];
      if (c < 0 || c >= vocab) continue;
      const float s = list_s[at];
      const int key = b * vocab + c;
      // strictly after the previous round's entry in the total order, and the best such
      if ((s < prev_s || (s == prev_s && key > prev_k)) && better(s, key, bs, bk)) {
        bs = s;
        bk = key;
      }
    }
    block_best(bs, bk, red_s[r & 1], red_k[r & 1]);
    const bool any = bs > -INFINITY;
    if (threadIdx.x == 0) {
      cand_score[g * ldc + r] = any ? bs : -INFINITY;
      cand_beam[g * ldc + r] = any ? bk / vocab : -1;
      cand_tok[g * ldc + r] = any ? bk % vocab : -1;
    }
    if (!any) {  // (uniform) the rest is the tail
      if (threadIdx.x == 0)
        for (int j = r + 1; j < K; ++j) {
          cand_score[g * ldc + j] = -INFINITY;
          cand_beam[g * ldc + j] = -1;
          cand_tok[g * ldc + j] = -1;
        }
      break;
    }
    prev_s = bs;
    prev_k = bk;
  }
}

int tiles_of(int vocab) { return (vocab + kBeamTile - 1) / kBeamTile; }

}  // namespace

extern "C" int64_t vwa_beam_select_workspace(int rows, int vocab) {
  if (rows < 1 || rows > kBeamMaxRows || vocab < 1 || vocab > kBeamMaxVocab) return 0;
  // per (row, tile): the maximum, the sum, and a list of kList (score, column) entries
  return (int64_t)rows * tiles_of(vocab) * (2 + 2 * kList) * 4;
}

extern "C" int vwa_beam_select(const float* logits, int64_t ld, int G, int W, int vocab, const uint32_t* mask,
                               int64_t mask_stride, const float* cum, float* cand_score, int* cand_beam,
                               int* cand_tok, int64_t ldc, void* workspace, int64_t workspace_bytes,
                               hipStream_t st) {
  if (!logits || !cum || !cand_score || !cand_beam || !cand_tok || !workspace) return -1;
  if (W < 2 || W > kBeamMaxWidth || G < 1 || G * W > kBeamMaxRows) return -2;
  if (vocab < 1 || vocab > kBeamMaxVocab || vocab > ld || mask_stride < 0 || ldc < 2 * W) return -3;
  const int rows = G * W, T = tiles_of(vocab), K = 2 * W;
  if (workspace_bytes < vwa_beam_select_workspace(rows, vocab) || ((uintptr_t)workspace & 3)) return -4;
  float* part_m = (float*)workspace;
  float* part_s = part_m + rows * T;
  float* list_s = part_s + rows * T;
  int* list_c = (int*)(list_s + (int64_t)rows * T * kList);
  hipLaunchKernelGGL(lse_part_kernel, dim3(T, rows), dim3(kThreads), 0, st, logits, ld, vocab, mask, mask_stride,
                     part_m, part_s);
  hipLaunchKernelGGL(row_topk_kernel, dim3(T, rows), dim3(kThreads), 0, st, logits, ld, vocab, mask, mask_stride, cum,
                     part_m, part_s, K, list_s, list_c);
  hipLaunchKernelGGL(group_merge_kernel, dim3(G), dim3(kThreads), 0, st, list_s, list_c, W, T, K, vocab, cand_score,
                     cand_beam, cand_tok, ldc);
  return (int)hipGetLastError();
}

// Cross-attention probabilities of selected heads (word alignment, step 2 of the method).
//
// One workgroup per (16-row token tile, selected head), 4 waves.  Two passes over that head's K
// (192 KB for 1500 frames: L2-resident): pass 1 computes the 16 x 16 score tiles on the bf16 MFMA
// (f32 accumulation; wave w takes key tiles w, w + 4, ...) and keeps an online (max, sum) per row;
// pass 2 recomputes the same tiles -- the same instructions on the same operands, so the same
// scores -- and stores exp(x - max) / sum.  Nothing but the [16] row statistics crosses waves.
#include "kernels/common.h"
#include "align/align.h"

using namespace vwa;

namespace {

constexpr int kWaves = 4;

// (m, s) <- the statistics of the union of two key sets (m: max, s: sum of exp(x - m))
VWA_DEVICE void merge_stats(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = nm == -INFINITY ? 0.f : s * expf(m - nm) + os * expf(om - nm);
  m = nm;
}

__global__ __launch_bounds__(64 * kWaves) void attn_probs_kernel(const u16* __restrict__ q, int64_t ldq,
                                                                 const u16* __restrict__ k,
                                                                 const int* __restrict__ heads, int H, int T,
                                                                 int n_keys, float scale, float* __restrict__ out,
                                                                 int64_t osh, int64_t osr) {
  __shared__ float sm[kWaves][16], ss[kWaves][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * 16;
  const int h = min(max(heads[blockIdx.y], 0), H - 1);
  const int n_tiles = (n_keys + 15) >> 4;

  // A operand: q[row0 + r][h * 64 + 32 s + 8 g .. + 8), s = 0, 1 (rows >= T: zeros)
  uint4 qa0 = make_uint4(0, 0, 0, 0), qa1 = qa0;
  if (row0 + r < T) {
    const u16* qp = q + (int64_t)(row0 + r) * ldq + h * kAlignHeadDim + 8 * g;
    qa0 = *reinterpret_cast<const uint4*>(qp);
    qa1 = *reinterpret_cast<const uint4*>(qp + 32);
  }
  // lane's C values: token rows row0 + 4 g + i, key j0 + r
  auto scores = [&](int j0, float* x) {
    const int key = j0 + r;
    uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0;
    if (key < n_keys) {
      const u16* kp = k + ((int64_t)key * H + h) * kAlignHeadDim + 8 * g;
      b0 = *reinterpret_cast<const uint4*>(kp);
      b1 = *reinterpret_cast<const uint4*>(kp + 32);
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = mfma16(as_bf16x8(qa0), as_bf16x8(b0), c);
    c = mfma16(as_bf16x8(qa1), as_bf16x8(b1), c);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = __fmul_rn(c[i], scale);  // (no contraction: both passes see this value)
  };

  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int jt = wave; jt < n_tiles; jt += kWaves) {
    float x[4];
    scores(jt * 16, x);
    if (jt * 16 + r < n_keys) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (x[i] > m[i]) {
          s[i] = s[i] * expf(m[i] - x[i]) + 1.f;
          m[i] = x[i];
        } else {
          s[i] += expf(x[i] - m[i]);
        }
      }
    }
  }
  // the 16 lanes of a group hold the 16 keys of a tile column-wise: butterfly over lane bits 0..3
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) merge_stats(m[i], s[i], __shfl_xor(m[i], o, 64), __shfl_xor(s[i], o, 64));
    if (r == 0) {
      sm[wave][4 * g + i] = m[i];
      ss[wave][4 * g + i] = s[i];
    }
  }
  __syncthreads();
  float inv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float M = sm[0][4 * g + i], S = ss[0][4 * g + i];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) merge_stats(M, S, sm[w][4 * g + i], ss[w][4 * g + i]);
    m[i] = M;
    inv[i] = 1.f / S;  // (n_keys >= 1: wave 0 saw a key, S >= 1)
  }
  float* o = out + (int64_t)blockIdx.y * osh;
  for (int jt = wave; jt < n_tiles; jt += kWaves) {
    float x[4];
    scores(jt * 16, x);
    const int key = jt * 16 + r;
    if (key >= n_keys) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 4 * g + i;
      if (row < T) o[(int64_t)row * osr + key] = expf(x[i] - m[i]) * inv[i];
    }
  }
}

}  // namespace

extern "C" int vwa_attn_probs(const uint16_t* q, int64_t ldq, const uint16_t* k, const int* heads, int n_sel, int H,
                              int T, int n_keys, float scale, float* out, int64_t out_stride_head,
                              int64_t out_stride_row, hipStream_t st) {
  if (n_sel < 1 || n_sel > 65535 || H < 1 || T < 1 || n_keys < 1 || ldq < (int64_t)H * kAlignHeadDim || (ldq & 7) ||
      out_stride_row < n_keys)
    return -1;
  hipLaunchKernelGGL(attn_probs_kernel, dim3((T + 15) / 16, n_sel), dim3(64 * kWaves), 0, st, q, ldq, k, heads, H, T,
                     n_keys, scale, out, out_stride_head, out_stride_row);
  return (int)hipGetLastError();
}

// Wire audio ingest (ingest.h has the contract): decode, downmix and polyphase windowed-sinc
// resampling to 16 kHz in one launch.
//
// LDS layout of the span: plain, sample j of the span at dword j.  Lane t of a wave reads dword
// d_t + k at tap k, d_t = pos(i0 + t) - pos(i0), which advances by M / L per lane: 3 dwords at
// 48 kHz (coprime with the 32 banks of a 32-lane ds_read_b32 group: conflict-free), 2 at 32 kHz
// (2-way), between 1 and 3 at the other downsampling rates (at most ceil(M / L)-way) and 1/2 at 8 kHz
// (neighbours share an address: a broadcast).  The table reads, one row of 2H floats per lane from
// L2, cost more than the worst of these; a skewed layout was not worth its index arithmetic.
#include "ingest/ingest.h"

namespace {

__device__ __forceinline__ int mulaw_value(int code) {
  const int u = ~code & 0xff;
  const int t = (((u & 0x0f) << 3) + 0x84) << ((u >> 4) & 7);
  return (u & 0x80) ? 0x84 - t : t - 0x84;
}

__device__ __forceinline__ int alaw_value(int code) {
  const int a = code ^ 0x55;
  const int seg = (a >> 4) & 7;
  int t = (a & 0x0f) << 4;
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg - 1);
  return (a & 0x80) ? t : -t;
}

// frame f of the window, decoded and mixed (ingest.h Decode, Mix); f in [0, n_in)
__device__ __forceinline__ float frame_value(const uint8_t* __restrict__ raw, int64_t f, int enc, int C, int channel) {
  const int c0 = channel < 0 ? 0 : channel;
  const int c1 = channel < 0 ? C : channel + 1;
  float sum = 0.f;
  for (int c = c0; c < c1; ++c) {
    const int64_t s = f * C + c;
    int v;
    if (enc == kIngestLinear16) {
      v = reinterpret_cast<const int16_t*>(raw)[s];
    } else if (enc == kIngestMulaw) {
      v = mulaw_value(raw[s]);
    } else {
      v = alaw_value(raw[s]);
    }
    const float x = (float)v * (1.f / 32768.f);
    sum = c == c0 ? x : sum + x;
  }
  return (channel < 0 && C > 1) ? sum / (float)C : sum;
}

__global__ __launch_bounds__(kIngestBlock) void ingest_copy_kernel(const uint8_t* __restrict__ raw, int64_t n_out,
                                                                   int enc, int C, int channel,
                                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kIngestBlock + threadIdx.x;
  if (i < n_out) out[i] = frame_value(raw, i, enc, C, channel);
}

__global__ __launch_bounds__(kIngestBlock) void ingest_resample_kernel(const uint8_t* __restrict__ raw, int64_t n_in,
                                                                       int64_t n_out, int enc, int C, int channel,
                                                                       int L, int M, int H,
                                                                       const float* __restrict__ table,
                                                                       float* __restrict__ out) {
  __shared__ float span[kIngestMaxSpan];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kIngestBlock;
  const int64_t i1 = min(i0 + kIngestBlock, n_out) - 1;  // the workgroup's last output (i0 < n_out: the grid)
  const int64_t first = (i0 * M) / L - H + 1;            // the input sample at span[0]
  const int n_span = (int)((i1 * M) / L + H - first) + 1;  // <= 255 * M / L + 1 + 2H <= kIngestMaxSpan (launcher)
  for (int j = t; j < n_span; j += kIngestBlock) {
    const int64_t f = first + j;
    span[j] = (f >= 0 && f < n_in) ? frame_value(raw, f, enc, C, channel) : 0.f;
  }
  __syncthreads();
  const int64_t i = i0 + t;
  if (i >= n_out) return;
  const int64_t q = i * M;
  const int64_t pos = q / L;
  const int ph = (int)(q - pos * L);
  const float* __restrict__ h = table + (int64_t)ph * (2 * H);
  const float* x = span + (int)(pos - H + 1 - first);  // in [0, n_span - 2H]
  float acc = 0.f;
  for (int k = 0; k < 2 * H; ++k) acc = __fmaf_rn(h[k], x[k], acc);
  out[i] = acc;
}

}  // namespace

extern "C" int vwa_ingest_geometry(int rate, int* L, int* M, int* H) {
  int l, m;
  switch (rate) {
    case 8000: l = 2, m = 1; break;
    case 11025: l = 640, m = 441; break;
    case 12000: l = 4, m = 3; break;
    case 16000: l = 1, m = 1; break;
    case 22050: l = 320, m = 441; break;
    case 24000: l = 2, m = 3; break;
    case 32000: l = 1, m = 2; break;
    case 44100: l = 160, m = 441; break;
    case 48000: l = 1, m = 3; break;
    default: return -1;
  }
  *L = l;
  *M = m;
  *H = l >= m ? 16 : (16 * m + l - 1) / l;
  return 0;
}

extern "C" int vwa_ingest(const uint8_t* raw, int64_t n_in, int encoding, int channels, int channel, int rate,
                          const float* table, float* out, int64_t out_len, hipStream_t st) {
  int L, M, H;
  if (vwa_ingest_geometry(rate, &L, &M, &H) != 0) return -2;
  if (encoding != kIngestLinear16 && encoding != kIngestMulaw && encoding != kIngestAlaw) return -3;
  if (channels < 1 || channels > kIngestMaxChannels || channel >= channels) return -4;
  if (n_in < 0 || n_in > kIngestMaxFrames) return -5;
  const int64_t n_out = n_in * L / M;
  if (out_len < n_out) return -6;
  if (n_out == 0) return 0;
  if (!raw || !out || (L != M && !table)) return -1;
  if (encoding == kIngestLinear16 && (reinterpret_cast<uintptr_t>(raw) & 1)) return -7;
  if (L > kIngestMaxL || H > kIngestMaxH || (int64_t)(kIngestBlock - 1) * M / L + 1 + 2 * H > kIngestMaxSpan) return -8;
  const unsigned blocks = (unsigned)((n_out + kIngestBlock - 1) / kIngestBlock);
  if (L == M) {
    hipLaunchKernelGGL(ingest_copy_kernel, dim3(blocks), dim3(kIngestBlock), 0, st, raw, n_out, encoding, channels,
                       channel, out);
  } else {
    hipLaunchKernelGGL(ingest_resample_kernel, dim3(blocks), dim3(kIngestBlock), 0, st, raw, n_in, n_out, encoding,
                       channels, channel, L, M, H, table, out);
  }
  return (int)hipGetLastError();
}

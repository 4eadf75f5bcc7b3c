// Wire audio ingest for gfx950 (_vwa_ingest.so): one launch turns a window of wire bytes -- s16le,
// G.711 mu-law or A-law, 1..8 interleaved channels, 8..48 kHz -- into the 16 kHz f32 mono samples
// the log-mel kernel reads.  Same conventions as csrc/nucleus/nucleus.h: the launcher validates its
// geometry again (the bindings are the first line), returns 0 or a negative code, never launches on
// a rejected call, and launches on `st`; there is no host synchronisation.
//
// The kernel does not wait on another workgroup and uses no atomics and no scratch; every loop is
// bounded by an argument the launcher checked, and no value read from device memory becomes an
// index.  A launch repeats its bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kIngestLinear16 = 0, kIngestMulaw = 1, kIngestAlaw = 2;
constexpr int kIngestMaxChannels = 8;
constexpr int kIngestMaxL = 640;       // 16000 / 11025 = 640 / 441
constexpr int kIngestMaxH = 48;        // 48 kHz: ceil(16 * 3)
constexpr int kIngestBlock = 256;      // outputs per workgroup
constexpr int kIngestMaxSpan = 896;    // >= 255 * 3 + 1 + 2 * 48: the widest input span of a workgroup
constexpr int64_t kIngestMaxFrames = (int64_t)1 << 30;

extern "C" {

// The rate's resampling ratio 16000 / rate = L / M in lowest terms and the filter's half length
// H = ceil(16 / min(1, L / M)).  Returns 0, or -1 for a rate that is not one of 8000, 11025, 12000,
// 16000, 22050, 24000, 32000, 44100, 48000.
int vwa_ingest_geometry(int rate, int* L, int* M, int* H);

// raw     n_in frames of C interleaved samples: 2 bytes each (little endian, 2-byte aligned) for
//         linear16, 1 byte each for the two G.711 laws.
// Decode: linear16 is the s16 value; mu-law and A-law the standard's 16-bit value (of 14 and 13
//         significant bits).  v = (float)value * (1 / 32768): exact.
// Mix:    channel < 0: x = (((v_0 + v_1) + v_2) + ...) / (float)C in f32 (C == 1: x = v_0);
//         else x = v_channel.
// Out:    n_out = n_in * L / M (integer division) samples.  L == M (16 kHz): out[i] = x[i], no filter.
//         Else, with pos = (i * M) / L and ph = (i * M) % L in 64-bit integers,
//           out[i] = sum_{k = 0}^{2H - 1} table[ph][k] * x[pos - H + 1 + k],   x[j] = 0 outside [0, n_in),
//         accumulated in f32 from 0 in ascending k, one fused multiply-add per tap.
// table   f32 [L][2H] (ops.ingest_tables), unused when L == M.
// A workgroup of 256 threads owns 256 consecutive outputs: it decodes and mixes its input span
// (<= 255 * M / L + 1 + 2H <= 896 samples) once into LDS, then every thread reads its 2H taps there.
int vwa_ingest(const uint8_t* raw, int64_t n_in, int encoding, int channels, int channel, int rate,
               const float* table, float* out, int64_t out_len, hipStream_t st);

}  // extern "C"

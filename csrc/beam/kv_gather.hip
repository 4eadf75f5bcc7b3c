// The beam step's K/V move: every beam's self-attention cache blocks take the content of its new
// parent's, in place (see beam.h for the contract).
//
// A thread owns the same 16 bytes of one (layer, block index, cache) unit in all W beams of a group.
// It loads the W parents' 16 bytes into registers, then stores the beams that changed parent:
// every source is read before any destination of the same bytes is written, by the same thread,
// so repeated parents and cycles (a swap) need no second buffer.  Distinct beams hold distinct
// blocks (the slots of a launch are distinct), so no other thread touches these bytes.
#include "kernels/common.h"
#include "beam/beam.h"

namespace {

constexpr int kThreads = 256;

// (no __restrict__ on the caches: sources and destinations are the same memory)
__global__ __launch_bounds__(kThreads) void kv_beam_gather_kernel(uint4* k_cache, uint4* v_cache, int n_blocks,
                                                                  int unit_vecs, int bs,
                                                                  const int* __restrict__ block_table, int sessions,
                                                                  int64_t ldbt, int bps,
                                                                  const int* __restrict__ slots,
                                                                  const int* __restrict__ parents,
                                                                  const int* __restrict__ n_ctx, int W,
                                                                  int max_blocks) {
  const int off = blockIdx.x * kThreads + threadIdx.x;
  const int layer = blockIdx.y / max_blocks, j = blockIdx.y - layer * max_blocks;
  const int g = blockIdx.z >> 1;
  uint4* cache = (blockIdx.z & 1) ? v_cache : k_cache;
  const int ctx = min(max(n_ctx[g], 0), bps * bs);
  if (off >= unit_vecs || j >= (ctx + bs - 1) / bs) return;  // (j < bps: the launcher bounds max_blocks)
  uint4 val[kBeamMaxWidth];
  int64_t dst[kBeamMaxWidth];  // the beam's own 16 bytes, or -1: not written
#pragma unroll
  for (int w = 0; w < kBeamMaxWidth; ++w) {
    dst[w] = -1;
    val[w] = make_uint4(0, 0, 0, 0);
    if (w >= W) continue;
    const int p = parents[g * W + w];
    if (p == w || p < 0 || p >= W) continue;
    const int sd = slots[g * W + w], ss = slots[g * W + p];
    if (sd < 0 || sd >= sessions || ss < 0 || ss >= sessions) continue;
    const int bd = block_table[sd * ldbt + j], bsrc = block_table[ss * ldbt + j];
    if (bd < 1 || bd >= n_blocks || bsrc < 1 || bsrc >= n_blocks) continue;
    val[w] = cache[((int64_t)layer * n_blocks + bsrc) * unit_vecs + off];
    dst[w] = ((int64_t)layer * n_blocks + bd) * unit_vecs + off;
  }
#pragma unroll
  for (int w = 0; w < kBeamMaxWidth; ++w)
    if (dst[w] >= 0) cache[dst[w]] = val[w];
}

}  // namespace

extern "C" int vwa_kv_beam_gather(void* k_cache, void* v_cache, int L, int n_blocks, int H, int bs, int hd,
                                  const int* block_table, int sessions, int64_t ldbt, int bps, const int* slots,
                                  const int* parents, const int* n_ctx, int G, int W, int max_blocks,
                                  hipStream_t st) {
  if (!k_cache || !v_cache || !block_table || !slots || !parents || !n_ctx) return -1;
  if (W < 2 || W > kBeamMaxWidth || G < 1 || G * W > kBeamMaxRows) return -2;
  if (L < 1 || n_blocks < 2 || H < 1 || bs < 1 || hd < 1 || ((int64_t)bs * hd * 2) % 16) return -3;
  const int64_t unit_bytes = (int64_t)H * bs * hd * 2;  // one layer's block: [H, bs, hd] bf16
  if (unit_bytes / 16 > (1 << 24)) return -3;
  if (sessions < 1 || bps < 1 || ldbt < bps || max_blocks < 0 || max_blocks > bps) return -4;
  if (((uintptr_t)k_cache | (uintptr_t)v_cache) & 15) return -5;
  if ((int64_t)L * max_blocks > 65535) return -6;
  if (max_blocks == 0) return 0;  // nothing in context: nothing to move
  const int unit_vecs = (int)(unit_bytes / 16);
  hipLaunchKernelGGL(kv_beam_gather_kernel, dim3((unit_vecs + kThreads - 1) / kThreads, L * max_blocks, 2 * G),
                     dim3(kThreads), 0, st, (uint4*)k_cache, (uint4*)v_cache, n_blocks, unit_vecs, bs, block_table,
                     sessions, ldbt, bps, slots, parents, n_ctx, W, max_blocks);
  return (int)hipGetLastError();
}

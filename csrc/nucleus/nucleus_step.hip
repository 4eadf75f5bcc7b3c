// The nucleus step (see nucleus.h for the contract): one workgroup of sixteen waves per row.
//
// Shape.  The row's allow-mask is staged once into LDS (it may be pinned host memory), the history
// too.  Every candidate column gets a 49-bit composite  key << 17 | (0x1FFFF - id),  key the
// order-preserving u32 image of its f32 logit: composites are distinct, and descending composite IS
// the contract's order (logit descending, id ascending).  The k-th largest composite is found by
// radix select, one coalesced sweep of the row per digit (12, 10, 10 bits of the key, then 9 and 8 of
// the id) into an integer LDS histogram; the select ends early as soon as every column under the
// current prefix is needed, which without a tie at the k-th key is after the key's digits.  The ids
// digits are what fills the remainder from a tie run in id order -- an all-equal row included.
// One more sweep gathers the k composites >= the threshold into LDS (slot by an integer LDS counter:
// the slots' order varies, the bitonic sort that follows makes it the contract's).  Weights, the
// fixed-order scan of nucleus.h, the cut, and the output row built in LDS with atomicOr and stored
// whole.  Integer LDS atomics only; no floating-point atomics: a launch repeats its bits.
//
// Barrier and visibility of the penalty.  The <= 256 threads that hold a distinct valid history id
// each load one column of the row and store it back (distinct ids: no two threads touch one
// column).  Every other access to the row's logits is a load AFTER the __syncthreads() that follows
// those stores.  __syncthreads() is a workgroup-scope release/acquire fence plus s_barrier: the
// compiler puts s_waitcnt vmcnt(0) in front of the barrier, so every penalty store has been
// performed at the CU's vector L1 (write-through; the line is updated, and all waves of a workgroup
// run on one CU and share that L1) before any wave passes it.  The readers are in the same
// workgroup, so workgroup scope is sufficient: no other workgroup reads this row during the launch,
// and the kernel boundary publishes it to the sampler.  The logits pointer is neither const nor
// __restrict__, so the compiler may not move a load of the row over the stores or use a
// non-coherent load.
//
// Control flow.  Every branch that encloses a barrier is on a value all threads of the workgroup
// read from the same address (the row's parameters) or from LDS after a barrier: it is uniform.
#include "kernels/logit_row.h"
#include "nucleus/nucleus.h"

#include <math.h>

using namespace vwa;

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxWords = (kNucleusMaxVocab + 31) / 32;
constexpr int kIdBits = 17;
constexpr uint32_t kIdMask = (1u << kIdBits) - 1;
static_assert(kNucleusMaxVocab <= (1 << kIdBits), "ids must fit the composite's low bits");
constexpr int kHistBins = 4096;
// the composite's digits, most significant first: 32 key bits, then 17 id bits
constexpr int kPasses = 5;
__constant__ const int kShift[kPasses] = {37, 27, 17, 8, 0};
__constant__ const int kBits[kPasses] = {12, 10, 10, 9, 8};

// order-preserving u32 image of an f32 (larger float <=> larger key); -0 maps with +0
VWA_DEVICE uint32_t key_of(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
VWA_DEVICE float float_of(uint32_t key) { return __uint_as_float((key >> 31) ? (key & 0x7FFFFFFFu) : ~key); }
VWA_DEVICE uint64_t composite(float v, int c) { return ((uint64_t)key_of(v) << kIdBits) | (uint64_t)(kIdMask - (uint32_t)c); }

// Exclusive prefix of v over the workgroup's threads in thread order; total = the sum over all.
// Two barriers: the first frees sh (a previous call's readers are done), the second publishes it.
VWA_DEVICE int wg_scan(int v, int* sh, int tid, int& total) {
  const int lane = tid & 63, wave = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int s = sh[w];
    if (w < wave) before += s;
    tot += s;
  }
  total = tot;
  return before + inc - v;
}

// The f32 scan of nucleus.h, inclusive: in-wave Kogge-Stone, then the earlier waves' totals added
// left to right from 0 and that sum added to the lane's in-wave value.
VWA_DEVICE float wg_scan_f32(float v, float* sh, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  float inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  __syncthreads();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  float before = 0.f;
  for (int w = 0; w < wave; ++w) before += sh[w];
  return before + inc;
}

// f(c, v) for every candidate column c of the row: allowed by the staged mask and v = x[c] > -inf
template <class F>
VWA_DEVICE void for_candidates(const float* x, int vocab, const uint32_t* smask, int tid, F f) {
  const float ninf = neg_inf();
  sweep<kThreads>(
      x, 0, vocab, tid,
      [&](int c) {
        const float v = x[c];
        if (allowed<true>(smask, c) && v > ninf) f(c, v);
      },
      [&](int c) {
        const float4 v = *reinterpret_cast<const float4*>(x + c);
        const uint32_t k = allowed4(smask, c);
        if ((k & 1u) && v.x > ninf) f(c, v.x);
        if ((k & 2u) && v.y > ninf) f(c + 1, v.y);
        if ((k & 4u) && v.z > ninf) f(c + 2, v.z);
        if ((k & 8u) && v.w > ninf) f(c + 3, v.w);
      });
}

// the staged row (words [0, words), the rest zero) to mask_out's row, all out_words words
VWA_DEVICE void store_row(const uint32_t* smask, int words, int* out, int out_words, int tid) {
  for (int i = tid; i < out_words; i += kThreads) out[i] = i < words ? (int)smask[i] : 0;
}

__global__ __launch_bounds__(kThreads) void nucleus_step_kernel(float* logits, int64_t ld, int vocab,
                                                                const int* mask_in, int64_t mask_ld, int* mask_out,
                                                                int64_t out_ld, int out_words, int* n_kept,
                                                                const float* temperature, const float* top_p,
                                                                const int* top_k, const float* penalty,
                                                                const int* history, int64_t hist_ld, int H) {
  __shared__ uint32_t smask[kMaxWords];
  __shared__ int hist[kHistBins];
  __shared__ unsigned long long pairs[kNucleusMaxTopK];
  __shared__ int shist[kNucleusMaxHistory];
  __shared__ int sh_scan[kWaves];
  __shared__ float sh_fscan[kWaves];
  __shared__ int sh_sel[3];
  __shared__ int sh_cnt, sh_jstar;
  __shared__ float sh_C;

  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  float* x = logits + (int64_t)r * ld;
  int* orow = mask_out + (int64_t)r * out_ld;
  const int words = (vocab + 31) >> 5;

  // stage the mask (bits >= vocab cleared) and the history
  for (int i = tid; i < words; i += kThreads) {
    uint32_t w = mask_in ? (uint32_t)mask_in[(int64_t)r * mask_ld + i] : 0xFFFFFFFFu;
    if (i == words - 1 && (vocab & 31)) w &= (1u << (vocab & 31)) - 1u;
    smask[i] = w;
  }
  if (tid < H) shist[tid] = history[(int64_t)r * hist_ld + tid];
  if (tid == 0) {
    sh_cnt = 0;
    sh_sel[0] = sh_sel[1] = sh_sel[2] = 0;
  }
  __syncthreads();

  // 1. penalty, once per distinct valid id: the first occurrence in the history owns it
  const float theta = penalty[r];
  if (theta != 1.f && tid < H) {
    const int id = shist[tid];
    bool own = id >= 0 && id < vocab;
    for (int j = 0; own && j < tid; ++j) own = shist[j] != id;
    if (own) {
      const float l = x[id];
      x[id] = l > 0.f ? __fdiv_rn(l, theta) : l * theta;
    }
  }
  __syncthreads();  // the penalty stores are performed before any load of the row below (header)

  const float T = temperature[r];
  const float p = top_p[r];
  int k0 = top_k[r];
  k0 = k0 < 0 ? 0 : (k0 > kNucleusMaxTopK ? kNucleusMaxTopK : k0);
  const bool keep_all = !(p < 1.f);

  // 2. pass-through
  if (!(T > 0.f) || (k0 == 0 && keep_all)) {
    int pc = 0;
    for (int i = tid; i < words; i += kThreads) pc += __popc(smask[i]);
    int total;
    wg_scan(pc, sh_scan, tid, total);
    store_row(smask, words, orow, out_words, tid);
    if (tid == 0) n_kept[r] = total;
    return;
  }
  if (k0 == 0) k0 = kNucleusMaxTopK;

  // 3. radix select of the k-th largest composite
  uint64_t prefix = 0;  // the digits chosen so far
  int k = 0, kk = k0;   // kk: rank of the wanted composite among those under the prefix
  int low = 0;          // bits of the composite below the prefix
  for (int pass = 0; pass < kPasses; ++pass) {
    const int shift = kShift[pass], nb = 1 << kBits[pass];
    const int hi = shift + kBits[pass];
    for (int i = tid; i < nb; i += kThreads) hist[i] = 0;
    __syncthreads();
    for_candidates(x, vocab, smask, tid, [&](int c, float v) {
      const uint64_t cmp = composite(v, c);
      if ((cmp >> hi) == prefix) atomicAdd(&hist[(int)(cmp >> shift) & (nb - 1)], 1);
    });
    __syncthreads();
    // thread t owns the bins nb - 1 - (t per .. t per + per - 1): counted from the top
    const int per = nb > kThreads ? nb / kThreads : 1;
    const int rb0 = tid * per;
    int s = 0;
    for (int q = 0; q < per; ++q)
      if (rb0 + q < nb) s += hist[nb - 1 - (rb0 + q)];
    int total;
    const int e = wg_scan(s, sh_scan, tid, total);
    if (pass == 0) {  // total = |A|
      k = k0 < total ? k0 : total;
      kk = k;
      if (k == 0) {
        for (int i = tid; i < out_words; i += kThreads) orow[i] = 0;
        if (tid == 0) n_kept[r] = 0;
        return;
      }
    }
    if (e < kk && kk <= e + s) {  // exactly one thread: the wanted composite is in its bins
      int acc = e;
      for (int q = 0; q < per; ++q) {
        const int b = nb - 1 - (rb0 + q);
        const int cnt = hist[b];
        if (acc + cnt >= kk) {
          sh_sel[0] = b;
          sh_sel[1] = acc;
          sh_sel[2] = cnt;
          break;
        }
        acc += cnt;
      }
    }
    __syncthreads();
    prefix = (prefix << kBits[pass]) | (uint64_t)sh_sel[0];
    kk -= sh_sel[1];
    low = shift;
    if (sh_sel[2] == kk) break;  // every composite under the prefix is wanted
  }
  const uint64_t thr = prefix << low;  // exactly k candidates have composite >= thr

  // gather them, then sort descending: (logit descending, id ascending)
  int P = 1;
  while (P < k) P <<= 1;
  for (int i = tid; i < P; i += kThreads) pairs[i] = 0ull;  // below every candidate's composite
  __syncthreads();
  for_candidates(x, vocab, smask, tid, [&](int c, float v) {
    const uint64_t cmp = composite(v, c);
    if (cmp >= thr) {
      const int pos = atomicAdd(&sh_cnt, 1);
      if (pos < P) pairs[pos] = cmp;
    }
  });
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < (P >> 1)) {
        const int i = 2 * tid - (tid & (stride - 1));
        const int j = i + stride;
        const bool desc = (i & size) == 0;
        const unsigned long long a = pairs[i], b = pairs[j];
        if ((a < b) == desc) {
          pairs[i] = b;
          pairs[j] = a;
        }
      }
      __syncthreads();
    }
  }

  // 4. weights, scan, cut
  int id = 0;
  float w = 0.f;
  if (tid < k) {
    const unsigned long long cmp = pairs[tid];
    id = (int)(kIdMask - (uint32_t)(cmp & kIdMask));
    const float l0 = float_of((uint32_t)(pairs[0] >> kIdBits));
    w = expf(__fdiv_rn(float_of((uint32_t)(cmp >> kIdBits)) - l0, T));
  }
  const float c = wg_scan_f32(w, sh_fscan, tid);
  if (tid == k - 1) {
    sh_C = c;
    sh_jstar = k - 1;
  }
  for (int i = tid; i < words; i += kThreads) smask[i] = 0u;
  __syncthreads();
  if (!keep_all && tid < k && c >= p * sh_C) atomicMin(&sh_jstar, tid);
  __syncthreads();
  const int jstar = sh_jstar;
  if (tid <= jstar && tid < k) atomicOr(&smask[id >> 5], 1u << (id & 31));
  __syncthreads();
  store_row(smask, words, orow, out_words, tid);
  if (tid == 0) n_kept[r] = jstar + 1;
}

}  // namespace

extern "C" int vwa_nucleus_step(float* logits, int64_t ld, int rows, int vocab, const int* mask_in, int64_t mask_ld,
                                int* mask_out, int64_t out_ld, int out_words, int* n_kept, const float* temperature,
                                const float* top_p, const int* top_k, const float* penalty, const int* history,
                                int64_t hist_ld, int H, hipStream_t st) {
  if (!logits || !mask_out || !n_kept || !temperature || !top_p || !top_k || !penalty) return -1;
  if (rows < 1 || rows > kNucleusMaxRows) return -2;
  if (vocab < 1 || vocab > kNucleusMaxVocab || ld < vocab) return -3;
  if (H < 0 || H > kNucleusMaxHistory || (H > 0 && (!history || hist_ld < H))) return -4;
  const int64_t words = (vocab + 31) / 32;
  if (mask_in && mask_ld != 0 && mask_ld < words) return -5;
  if (out_words < words || out_ld < out_words) return -5;
  const int64_t n1 = rows - 1;
  const struct {
    const void* p;
    int64_t bytes;
  } out[2] = {{mask_out, 4 * (n1 * out_ld + out_words)}, {n_kept, 4 * (int64_t)rows}},
    in[7] = {{logits, 4 * (n1 * ld + vocab)},
             {mask_in, mask_in ? 4 * (n1 * mask_ld + words) : 0},
             {temperature, 4 * (int64_t)rows},
             {top_p, 4 * (int64_t)rows},
             {top_k, 4 * (int64_t)rows},
             {penalty, 4 * (int64_t)rows},
             {history, H > 0 ? 4 * (n1 * hist_ld + H) : 0}};
  if (overlap(out[0].p, out[0].bytes, out[1].p, out[1].bytes)) return -6;
  for (const auto& o : out)
    for (const auto& i : in)
      if (i.bytes > 0 && overlap(o.p, o.bytes, i.p, i.bytes)) return -6;
  hipLaunchKernelGGL(nucleus_step_kernel, dim3(rows), dim3(kThreads), 0, st, logits, ld, vocab, mask_in, mask_ld,
                     mask_out, out_ld, out_words, n_kept, temperature, top_p, top_k, penalty, history, hist_ld, H);
  return (int)hipGetLastError();
}

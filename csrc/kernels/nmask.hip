// Neurotoxin attacker (config poison_neurotoxin_ratio; Zhang et al., ICML 2022): the server-side
// coordinate mask, built once per round from the update the server just applied.
//   u[j]    = fl32(w_new[j] - w_old[j]), one IEEE fp32 subtraction, j < P
//   key[j]  = the bits of u[j] with the sign bit cleared, as uint32 (|u| ordered as integers: -0 and
//             +0 are 0, denormals order, inf above every finite value, a NaN above inf by payload)
//   T       = the k-th SMALLEST key; coordinate j is kept iff key[j] <= T (m >= k kept, more only on
//             ties at T)
// * select  topk.hip's most-significant-digit-first radix select on 32-bit keys, 4 passes of 8 bits,
//           with the bin scan run from the bottom.  A pass histograms the current digit of the keys
//           that match the prefix found so far (LDS integer adds, then one integer global add per
//           non-empty bin and block: exact, so every count is the same run to run); a one-block launch
//           scans the 256 bins, picks the digit at which the running count reaches what is left of k
//           and updates {prefix, left} in device memory.  Nothing is read by the host between the
//           passes.  The last scan leaves (T, m).  u is recomputed in every pass (two coalesced fp32
//           reads; no [P] key buffer).
// * words   one pass: a wave takes 64 consecutive coordinates, every lane recomputes key <= T for its
//           own and the wave's 64-lane ballot IS the mask word; lane 0 writes it.  Lanes at and past
//           P vote 0, so the last word's tail bits are 0.  No atomics.
#include "common.hpp"
#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kDigitBits = 8, kBins = 1 << kDigitBits, kPasses = 4;   // 4 x 8 bits over the 31-bit keys
constexpr int kThreads = 256;
// every launch but the scans: x 256 threads x 1 coordinate = 262144 per sweep of the grid.  Four
// blocks per CU: a histogram block ends with up to 256 global integer adds on the same 256 words
constexpr int kBlocksMax = 1024;
constexpr unsigned kAbsMask = 0x7FFFFFFFu;
// workspace, in int64 words: the passes' histograms, then {prefix, left}
constexpr int kStateAt = kPasses * kBins, kWsWords = kStateAt + 2;

__device__ __forceinline__ unsigned key_of(const float* __restrict__ wn, const float* __restrict__ wo, long long j) {
  return __float_as_uint(__fsub_rn(wn[j], wo[j])) & kAbsMask;
}

// hist [256] += the counts of digit (key >> shift) & 255 over the keys whose bits above the digit
// equal the prefix's (FIRST: shift = 24, every key matches)
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void nmask_hist_kernel(const float* __restrict__ wn,
                                                              const float* __restrict__ wo, long long P, int shift,
                                                              const u64* __restrict__ state, u64* __restrict__ hist) {
  __shared__ unsigned bins[kBins];      // (a block takes fewer than 2^32 coordinates for any P < 2^41)
  bins[threadIdx.x] = 0;
  __syncthreads();
  const unsigned want = FIRST ? 0u : ((unsigned)state[0] >> shift) >> kDigitBits;   // (shift <= 16 here)
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long j = blockIdx.x * (long long)kThreads + threadIdx.x; j < P; j += stride) {
    const unsigned d = key_of(wn, wo, j) >> shift;
    if (FIRST || (d >> kDigitBits) == want) atomicAdd(&bins[d & (kBins - 1)], 1u);
  }
  __syncthreads();
  const unsigned c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], (u64)c);
}

// One block, thread b = bin b.  below[b + 1] = the count of the bins 0 .. b (an inclusive prefix sum
// in LDS, below[0] = 0); the digit is the one bin with below[b + 1] >= left > below[b].  state =
// {prefix | digit << shift, left - below[digit]}.  FIRST: the prefix is empty and left = k.  LAST:
// sel = (T, m) with m = (the keys below T) + (the keys equal to T) = (k - left') + hist[digit]
__global__ __launch_bounds__(kBins) void nmask_scan_kernel(const u64* __restrict__ hist, u64* __restrict__ state,
                                                           int shift, long long k, int first, int last,
                                                           long long* __restrict__ sel) {
  __shared__ u64 below[kBins + 1];
  const int b = threadIdx.x;
  const u64 mine = hist[b];
  below[b + 1] = mine;
  if (b == 0) below[0] = 0;
  __syncthreads();
  for (int o = 1; o < kBins; o <<= 1) {
    const u64 add = b + 1 - o >= 1 ? below[b + 1 - o] : 0;
    __syncthreads();
    below[b + 1] += add;
    __syncthreads();
  }
  const u64 prefix = first ? 0 : state[0], left = first ? (u64)k : state[1];
  __syncthreads();                      // (every thread has read the state before one rewrites it)
  if (below[b + 1] >= left && below[b] < left) {
    const u64 p = prefix | ((u64)b << shift), l = left - below[b];
    state[0] = p;
    state[1] = l;
    if (last) {
      sel[0] = (long long)p;
      sel[1] = (long long)((u64)k - l + mine);
    }
  }
}

// words [ceil(P / 64)]: bit j % 64 of word j / 64 = (key[j] <= T) for j < P, 0 at and past P.  The
// loop is wave-uniform (every lane of a wave has the same word index), so all 64 lanes vote
__global__ __launch_bounds__(kThreads) void nmask_words_kernel(const float* __restrict__ wn,
                                                               const float* __restrict__ wo, long long P,
                                                               const long long* __restrict__ sel,
                                                               u64* __restrict__ words) {
  const unsigned T = (unsigned)sel[0];
  const int lane = threadIdx.x & (kWave - 1);
  const long long nwords = (P + kWave - 1) / kWave;
  const long long wstride = (long long)gridDim.x * (kThreads / kWave);
  for (long long wd = blockIdx.x * (long long)(kThreads / kWave) + (threadIdx.x >> 6); wd < nwords; wd += wstride) {
    const long long j = wd * kWave + lane;
    const bool keep = j < P && key_of(wn, wo, j) <= T;
    const u64 vote = __builtin_amdgcn_ballot_w64(keep);
    if (lane == 0) words[wd] = vote;
  }
}

}  // namespace

// blocks of a histogram pass and of the word pass over P coordinates
DBA_EXPORT int dba_nmask_blocks(long long P) {
  return (int)std::max(1LL, std::min((long long)kBlocksMax, (P + kThreads - 1) / kThreads));
}

// coordinates one block takes per sweep of the grid, and the most blocks a launch has
DBA_EXPORT int dba_nmask_block_sweep() { return kThreads; }
DBA_EXPORT int dba_nmask_blocks_max() { return kBlocksMax; }

// int64 words of the select workspace
DBA_EXPORT int dba_nmask_ws_words() { return kWsWords; }

// words [ceil(P / 64)] int64 = the keep mask of the k smallest |w_new - w_old| over the first P
// entries (ties at the threshold all kept, tail bits 0); sel [2] int64 = (T, m): the k-th smallest
// key as its integer value and the number of keys <= T.  ws: [dba_nmask_ws_words()] int64 workspace
// (no initialisation needed: the call clears what it counts into, and reads nothing an earlier call
// left).  1 <= k <= P (hipErrorInvalidValue otherwise)
DBA_EXPORT int dba_neurotoxin_mask(const float* w_new, const float* w_old, long long P, long long k,
                                   long long* words, long long* sel, long long* ws, void* stream) {
  if (P < 1 || k < 1 || k > P) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  u64* hist = (u64*)ws;
  u64* state = hist + kStateAt;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(u64) * kPasses * kBins, s);
  if (e != hipSuccess) return (int)e;
  const int bx = dba_nmask_blocks(P);
  for (int p = 0; p < kPasses; ++p) {
    const int shift = kDigitBits * (kPasses - 1 - p);
    u64* h = hist + p * kBins;
    if (p == 0)
      hipLaunchKernelGGL(nmask_hist_kernel<true>, dim3(bx), dim3(kThreads), 0, s, w_new, w_old, P, shift, state, h);
    else
      hipLaunchKernelGGL(nmask_hist_kernel<false>, dim3(bx), dim3(kThreads), 0, s, w_new, w_old, P, shift, state, h);
    hipLaunchKernelGGL(nmask_scan_kernel, dim3(1), dim3(kBins), 0, s, h, state, shift, k, (int)(p == 0),
                       (int)(p == kPasses - 1), sel);
  }
  hipLaunchKernelGGL(nmask_words_kernel, dim3(bx), dim3(kThreads), 0, s, w_new, w_old, P, sel, (u64*)words);
  DBA_LAUNCH_CHECK();
}

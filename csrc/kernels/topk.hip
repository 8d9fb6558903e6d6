// SparseFed (config sparse_topk; Panda et al., AISTATS 2022): the server adds the round's aggregate
// into an fp64 error-feedback residual R, applies only the k largest-magnitude coordinates of R to
// the model and keeps the rest in R for later rounds.
//   key[j]  = the bits of R[j] with the sign bit cleared, as uint64 (|R| ordered as integers: -0 and
//             +0 are 0, denormals order, inf above every finite value, a NaN above inf by payload)
//   T       = the k-th largest key; coordinate j is kept iff key[j] >= T (m >= k kept, more only on
//             ties at T)
// * select  a most-significant-digit-first radix select over the keys, 8 passes of 8 bits.  A pass
//           histograms the current digit of the keys that match the prefix found so far (LDS integer
//           adds, then one integer global add per non-empty bin and block: exact, so every count is
//           the same run to run); a one-block launch scans the 256 bins from the top, picks the digit
//           at which the running count reaches what is left of k and updates {prefix, left} in
//           device memory.  The first pass also does R += total, so the aggregate is read once.
//           Nothing is read by the host between the passes.  The last scan leaves (T, m).
// * apply   one pass: the mask is recomputed from R and T (no [L] mask is stored); a kept coordinate
//           gets w[j] += (float)(R[j] * (double)coef) (noise.hpp, noise off: the bits of
//           dba_add_noise_scaled) and R[j] = +0.0; a dropped coordinate's w[j] is not written and its
//           R[j] stays.  The kept coordinates are counted through block_sum, per-block int64
//           partials and count_finalize (countfin.hpp), as rlr.hip counts.
// The fp64 vectors are read 16 bytes per lane where their start allows (scalar otherwise, and for
// the tail); which elements a thread takes never depends on the alignment.
#include "common.hpp"
#include "countfin.hpp"
#include "noise.hpp"
#include "rowquad.hpp"
#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kDigitBits = 8, kBins = 1 << kDigitBits, kPasses = 8;   // 8 x 8 bits over the 63-bit keys
constexpr int kPair = 2;               // fp64 elements per lane per step of a histogram pass
// histogram passes: x 256 threads x 2 coordinates = 262144 per sweep.  Two blocks per CU: each ends
// with up to 256 global integer adds on the same 256 words, and those serialise per word
constexpr int kSelectBlocksMax = 512;
constexpr int kApplyBlocksMax = 2048;  // apply: x 256 threads x 4 coordinates = 2097152 per sweep
constexpr u64 kAbsMask = 0x7FFFFFFFFFFFFFFFull;
// workspace, in int64 words: the passes' histograms, then {prefix, left}
constexpr int kStateAt = kPasses * kBins, kWsWords = kStateAt + 2;

__device__ __forceinline__ u64 key_of(double r) { return (u64)__double_as_longlong(r) & kAbsMask; }

// p[0], p[1] (16 bytes where ``vec``: p is 16-byte aligned)
__device__ __forceinline__ void ld_pair(const double* __restrict__ p, bool vec, double (&v)[kPair]) {
  if (vec) {
    const double2 x = *(const double2*)p;
    v[0] = x.x; v[1] = x.y;
  } else {
    v[0] = p[0]; v[1] = p[1];
  }
}

__device__ __forceinline__ void st_pair(double* __restrict__ p, bool vec, const double (&v)[kPair]) {
  if (vec) {
    *(double2*)p = make_double2(v[0], v[1]);
  } else {
    p[0] = v[0]; p[1] = v[1];
  }
}

// ------------------------------------------------------------------------ histogram pass
// hist [256] += the counts of digit (key >> shift) & 255 over the keys whose bits above the digit
// equal the prefix's (FIRST: shift = 56, every key matches, and R += total on the way)
template <bool FIRST>
__global__ __launch_bounds__(256) void topk_hist_kernel(double* __restrict__ resid, const double* __restrict__ total,
                                                        long long L, int shift, const u64* __restrict__ state,
                                                        u64* __restrict__ hist) {
  __shared__ unsigned bins[kBins];      // (a block takes fewer than 2^32 coordinates for any L < 2^41)
  bins[threadIdx.x] = 0;
  __syncthreads();
  const bool vr = aligned16_dev(resid), vt = FIRST ? aligned16_dev(total) : false;
  const u64 want = FIRST ? 0 : (state[0] >> shift) >> kDigitBits;
  const long long npair = L / kPair;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (; q < npair; q += stride) {
    double r[kPair];
    ld_pair(resid + q * kPair, vr, r);
    if (FIRST) {
      double t[kPair];
      ld_pair(total + q * kPair, vt, t);
      r[0] += t[0]; r[1] += t[1];
      st_pair(resid + q * kPair, vr, r);
    }
#pragma unroll
    for (int j = 0; j < kPair; ++j) {
      const u64 d = key_of(r[j]) >> shift;
      if (FIRST || (d >> kDigitBits) == want) atomicAdd(&bins[d & (kBins - 1)], 1u);
    }
  }
  if (q == npair && L % kPair) {        // the odd last coordinate (one thread of the launch)
    double r = resid[L - 1];
    if (FIRST) {
      r += total[L - 1];
      resid[L - 1] = r;
    }
    const u64 d = key_of(r) >> shift;
    if (FIRST || (d >> kDigitBits) == want) atomicAdd(&bins[d & (kBins - 1)], 1u);
  }
  __syncthreads();
  const unsigned c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], (u64)c);
}

// ---------------------------------------------------------------------------- bin scan
// One block, thread b = bin b.  above[b] = the count of the bins b .. 255 (an inclusive suffix sum
// in LDS); the digit is the one bin with above[b] >= left > above[b + 1].  state = {prefix | digit <<
// shift, left - above[digit + 1]}.  FIRST: the prefix is empty and left = k.  LAST: sel = (T, m) with
// m = (the keys above T) + (the keys equal to T) = (k - left') + hist[digit]
__global__ __launch_bounds__(256) void topk_scan_kernel(const u64* __restrict__ hist, u64* __restrict__ state,
                                                        int shift, long long k, int first, int last,
                                                        long long* __restrict__ sel) {
  __shared__ u64 above[kBins + 1];
  const int b = threadIdx.x;
  const u64 mine = hist[b];
  above[b] = mine;
  if (b == 0) above[kBins] = 0;
  __syncthreads();
  for (int o = 1; o < kBins; o <<= 1) {
    const u64 add = b + o < kBins ? above[b + o] : 0;
    __syncthreads();
    above[b] += add;
    __syncthreads();
  }
  const u64 prefix = first ? 0 : state[0], left = first ? (u64)k : state[1];
  __syncthreads();                      // (every thread has read the state before one rewrites it)
  if (above[b] >= left && above[b + 1] < left) {
    const u64 p = prefix | ((u64)b << shift), l = left - above[b + 1];
    state[0] = p;
    state[1] = l;
    if (last) {
      sel[0] = (long long)p;
      sel[1] = (long long)((u64)k - l + mine);
    }
  }
}

// ------------------------------------------------------------------------------- apply
// one step: coordinates c .. c + cnt; returns how many were kept
template <bool FULL>
__device__ __forceinline__ int apply_step(float* __restrict__ dst, bool vd, double* __restrict__ resid, bool vr,
                                          u64 T, long long c, int cnt, float coef) {
  double r[kQuad];
  if (FULL) {
    double a[kPair], b[kPair];
    ld_pair(resid + c, vr, a);
    ld_pair(resid + c + kPair, vr, b);
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1];
  } else {
#pragma unroll
    for (int j = 0; j < kQuad; ++j) r[j] = j < cnt ? resid[c + j] : 0.0;
  }
  bool kept[kQuad];
  int n = 0;
#pragma unroll
  for (int j = 0; j < kQuad; ++j) {
    kept[j] = (FULL || j < cnt) && key_of(r[j]) >= T;
    n += kept[j] ? 1 : 0;
  }
  if (n == 0) return 0;                 // nothing kept: neither vector is written
  if (FULL && n == kQuad) {
    float d[kQuad];
    ld_quad<true>(dst + c, vd, kQuad, d);
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
      d[j] += noise_scaled_update<double>(r[j], coef, 0.f, 0u, 0, c + j);
      r[j] = 0.0;
    }
    st_quad<true>(dst + c, vd, kQuad, d);
    st_quad<true>(resid + c, vr, kQuad, r);
    return n;
  }
#pragma unroll
  for (int j = 0; j < kQuad; ++j)
    if (kept[j]) {
      dst[c + j] += noise_scaled_update<double>(r[j], coef, 0.f, 0u, 0, c + j);
      resid[c + j] = 0.0;
    }
  return n;
}

// part [gridDim.x] int64: this block's kept coordinates
__global__ __launch_bounds__(256) void topk_apply_kernel(float* __restrict__ dst, double* __restrict__ resid,
                                                         const long long* __restrict__ sel, long long L, float coef,
                                                         long long* __restrict__ part) {
  __shared__ long long red[4];
  const u64 T = (u64)sel[0];
  const bool vd = aligned16_dev(dst), vr = aligned16_dev(resid);
  const long long nq = (L + kQuad - 1) / kQuad, nfull = L / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  int kept = 0;                         // (a thread takes fewer than 2^31 coordinates for any L < 2^50)
  for (; q < nfull; q += stride) kept += apply_step<true>(dst, vd, resid, vr, T, q * kQuad, kQuad, coef);
  if (q < nq) kept += apply_step<false>(dst, vd, resid, vr, T, q * kQuad, (int)(L - q * kQuad), coef);
  const long long s = block_sum<long long>(kept, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

}  // namespace

// blocks of a histogram pass over L coordinates
DBA_EXPORT int dba_topk_select_blocks(long long L) {
  const long long np = (L + kPair - 1) / kPair;
  return (int)std::max(1LL, std::min((long long)kSelectBlocksMax, (np + 255) / 256));
}

// blocks of the apply pass over L coordinates: its workspace is as many int64
DBA_EXPORT int dba_topk_apply_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kApplyBlocksMax, (nq + 255) / 256));
}

// int64 words of the select workspace
DBA_EXPORT int dba_topk_ws_words() { return kWsWords; }

// resid [L] fp64 += total [L] in place, then sel [2] int64 = (T, m): the k-th largest key of resid as
// its integer value and the number of keys >= T.  ws: [dba_topk_ws_words()] int64 workspace (no
// initialisation needed: the call clears what it counts into, and reads nothing an earlier call
// left).  1 <= k <= L (hipErrorInvalidValue otherwise)
DBA_EXPORT int dba_topk_select(double* resid, const double* total, long long L, long long k, long long* sel,
                               long long* ws, void* stream) {
  if (L < 1 || k < 1 || k > L) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  u64* hist = (u64*)ws;
  u64* state = hist + kStateAt;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(u64) * kPasses * kBins, s);
  if (e != hipSuccess) return (int)e;
  const int bx = dba_topk_select_blocks(L);
  for (int p = 0; p < kPasses; ++p) {
    const int shift = kDigitBits * (kPasses - 1 - p);
    u64* h = hist + p * kBins;
    if (p == 0)
      hipLaunchKernelGGL(topk_hist_kernel<true>, dim3(bx), dim3(256), 0, s, resid, total, L, shift, state, h);
    else
      hipLaunchKernelGGL(topk_hist_kernel<false>, dim3(bx), dim3(256), 0, s, resid, total, L, shift, state, h);
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(256), 0, s, h, state, shift, k, (int)(p == 0),
                       (int)(p == kPasses - 1), sel);
  }
  DBA_LAUNCH_CHECK();
}

// where key(resid[j]) >= sel[0]: dst[j] += (float)(resid[j] * (double)coef) (the bits of
// dba_add_noise_scaled, noise off), resid[j] = +0.0; elsewhere neither is written.  sel[1] = the
// number of coordinates applied.  part: [dba_topk_apply_blocks(L)] int64 workspace (no
// initialisation needed).  L >= 1
DBA_EXPORT int dba_topk_apply(float* dst, double* resid, long long* sel, long long L, float coef, long long* part,
                              void* stream) {
  if (L < 1) return (int)hipErrorInvalidValue;
  const int bx = dba_topk_apply_blocks(L);
  hipLaunchKernelGGL(topk_apply_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, dst, resid, sel, L, coef, part);
  hipLaunchKernelGGL(count_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, part, bx, sel + 1);
  DBA_LAUNCH_CHECK();
}

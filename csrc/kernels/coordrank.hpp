// Coordinate-wise rank rules over client rows (trim.hip: the symmetric trim; bulyan.hip: the
// median window): one fused pass over n strided fp32 rows of length L (the clients' final states,
// read where they lie: rows are picked by an optional index list; no [n, L] copy and no delta
// temporary).  Per coordinate c the n values are sorted, the rule picks a run of ranks lo .. hi and
//     total[c] = ((d_lo + d_{lo+1}) + ...) + d_hi,   d_r = (double)s_r - (double)base[c]
// is added in ascending rank with one fp64 rounding per operation; per client, the coordinates at
// which its value was kept (s_lo <= v <= s_hi) and at which it was cut as high (v > s_hi, or v NaN
// and s_hi not) are counted.  This header is the pass; a rule is a tag type whose
//     template <int N, int CPT, bool FULL> static void step(buf, rstride, row_idx, vecmask, n, base,
//                                                           base_vec, arg, c, cnt, total, count)
// does one step (coordinates c .. c + cnt of every row: load, sort, total, counts) and whose ``arg``
// is the rule's one integer (trim's k, Bulyan's f).  The rule is a template argument of the kernel:
// nothing is switched at run time.  A step's load, count and store loops stay written out in each
// rule: as helpers they compile to other code (more registers in the larger instantiations;
// profiles/coordrank/README.md has the figures).
//   * a thread owns whole coordinates, CPT of them per step: every row element is fetched once
//     and stays in registers, and the sort is a fully unrolled compare-exchange network
//     (sortnet.hpp) with no cross-lane traffic
//   * a float becomes an unsigned key whose integer order is the sort order: -0 joins +0 (x + 0),
//     the sign-flip transform, every NaN to 0xFFFFFFFF (after +inf, as numpy and torch sort).  A
//     comparator is an integer min and max; ranks are decoded back to floats for the total; the
//     counts compare keys (a NaN threshold compares false against everything, as floats do)
//   * n <= 16: the network of exactly n inputs, four coordinates per thread.  17 .. 64 rows run the
//     network of 24 / 32 / 48 / 64 inputs with the unused top inputs holding the top key (they
//     never move; the ranks below n are the rows'), two coordinates per thread up to 32 rows and
//     one beyond: the keys, their unsorted copy and the counters stay in registers
//   * which coordinates a thread takes depends only on L, CPT and the launch grid; a coordinate's
//     total depends on nothing else in the call.  Counts are integers: a thread's per-client
//     counters (kept in the low half of an int, high in the upper half; a thread takes fewer than
//     2^16 coordinates for any L < 2^31) go through lanes in a butterfly, the four waves in order,
//     per-block int64 partials and a finalize launch: no atomics, bitwise run to run
// Rows are read CPT floats per lane: as in rowquad.hpp for CPT = 4 (ld_group below is this
// family's own form of that load: through the shared one the kernels compile to other code),
// scalar loads for CPT < 4; the last, partial step reads only the row's remaining floats and
// stores only their results.
#pragma once
#include "common.hpp"
#include "rowquad.hpp"
#include "sortnet.hpp"
#include <algorithm>

// sums only: nothing to contract, and nothing is to be (this holds for the including file too)
#pragma clang fp contract(off)

namespace {

constexpr int kMaxRows = 64;
constexpr int kBlocksMax = 512;     // x 256 threads x 4 floats = 524288 elements per sweep of the grid
constexpr uint32_t kNanKey = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t to_key(float x) {
  const float z = x + 0.0f;                                 // -0 -> +0 (and nothing else changes its value)
  const uint32_t b = __float_as_uint(z);
  const uint32_t key = b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
  return z != z ? kNanKey : key;
}

__device__ __forceinline__ float from_key(uint32_t key) {
  const uint32_t b = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
  return __uint_as_float(b);                                // (kNanKey -> 0x7FFFFFFF, a NaN)
}

// floats p[0 .. CPT) (FULL) or p[0 .. cnt), zero-filled; ``vec``: p is 16-byte aligned (CPT = 4)
template <int CPT, bool FULL>
__device__ __forceinline__ void ld_group(const float* __restrict__ p, bool vec, int cnt, float (&v)[CPT]) {
  if constexpr (FULL) {
    if constexpr (CPT == kQuad) {
      if (vec) {
        const float4 x = *(const float4*)p;
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        return;
      }
    }
#pragma unroll
    for (int j = 0; j < CPT; ++j) v[j] = p[j];
  } else {
#pragma unroll
    for (int j = 0; j < CPT; ++j) v[j] = j < cnt ? p[j] : 0.f;
  }
}

__device__ __forceinline__ const float* row_start(const float* __restrict__ buf, long long rstride,
                                                  const int* __restrict__ row_idx, int r) {
  return buf + (long long)(row_idx ? row_idx[r] : r) * rstride;
}

// N: inputs of the network; EXACT: n == N (else n <= N, the rest sentinels); CPT coordinates per step.
// part [n][2][gridDim.x] int64: per-block kept and high counts
template <class Rule, int N, int CPT, bool EXACT>
__global__ __launch_bounds__(256) void coord_rank_kernel(const float* __restrict__ buf, long long rstride,
                                                         const int* __restrict__ row_idx, int n_arg,
                                                         const float* __restrict__ base, int arg, long long L,
                                                         double* __restrict__ total, long long* __restrict__ part) {
  __shared__ int red[4][2 * N];
  const int n = EXACT ? N : n_arg;
  unsigned long long vecmask = 0;
  if constexpr (CPT == kQuad) {
    for (int r = 0; r < n; ++r)
      vecmask |= (unsigned long long)aligned16_dev(row_start(buf, rstride, row_idx, r)) << r;
  }
  const bool base_vec = aligned16_dev(base);
  int count[N];
#pragma unroll
  for (int r = 0; r < N; ++r) count[r] = 0;

  // whole steps in ascending order, then the rows' last, partial one (one thread of the launch)
  const long long ng = (L + CPT - 1) / CPT, nfull = L / CPT;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (; g < nfull; g += stride)
    Rule::template step<N, CPT, true>(buf, rstride, row_idx, vecmask, n, base, base_vec, arg, g * CPT, CPT, total,
                                      count);
  if (g < ng)
    Rule::template step<N, CPT, false>(buf, rstride, row_idx, vecmask, n, base, base_vec, arg, g * CPT,
                                       (int)(L - g * CPT), total, count);

  // lanes in a fixed butterfly, then the four waves in order
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r < n) {
      int kept = count[r] & 0xFFFF, high = (int)((unsigned)count[r] >> 16);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        kept += __shfl_xor(kept, o, kWave);
        high += __shfl_xor(high, o, kWave);
      }
      if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][2 * r] = kept;
        red[threadIdx.x >> 6][2 * r + 1] = high;
      }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 2 * n)
    part[(long long)t * gridDim.x + blockIdx.x] =
        (((long long)red[0][t] + (long long)red[1][t]) + (long long)red[2][t]) + (long long)red[3][t];
}

// one wave per (client, kept | high): lane l takes the partials of blocks l, l + 64, ..., then the
// lanes combine in a fixed butterfly
__global__ __launch_bounds__(64) void coord_rank_finalize(const long long* __restrict__ part, int nblk,
                                                         long long* __restrict__ counts) {
  const long long slot = blockIdx.x;
  long long s = 0;
  for (int b = threadIdx.x; b < nblk; b += kWave) s += part[slot * nblk + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if (threadIdx.x == 0) counts[slot] = s;
}

// blocks of a call over rows of length L: the workspace is 2 n times as many int64
inline int coord_rank_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kBlocksMax, (nq + 255) / 256));
}

// what every rule's entry point refuses (hipErrorInvalidValue: the caller composes those)
inline bool coord_rank_valid(int n, long long L, const double* total) {
  return n >= 1 && n <= kMaxRows && L >= 1 && L < (1LL << 31) && aligned16(total);
}

// total [L] fp64 (16-byte aligned) = the rule's sum of (row - base) over rows row_idx[r] (r if
// row_idx is null) of buf, each of L floats, rstride floats apart; counts [n][2] int64 = (kept,
// high) coordinates per row; part: [2 n][coord_rank_blocks(L)] int64 workspace (no initialisation
// needed).  The arguments are valid (coord_rank_valid, and ``arg`` by the rule's own bounds)
template <class Rule>
int coord_rank(const float* buf, long long rstride, const int* row_idx, int n, const float* base, int arg,
               long long L, double* total, long long* counts, long long* part, void* stream) {
  const int bx = coord_rank_blocks(L);
  hipStream_t s = (hipStream_t)stream;
#define COORD_RANK_LAUNCH(N, CPT, EXACT)                                                                             \
  hipLaunchKernelGGL((coord_rank_kernel<Rule, N, CPT, EXACT>), dim3(bx), dim3(256), 0, s, buf, rstride, row_idx, n, \
                     base, arg, L, total, part)
#define COORD_RANK_EXACT(N) \
  case N: COORD_RANK_LAUNCH(N, kQuad, true); break;
  switch (n) {
    COORD_RANK_EXACT(1) COORD_RANK_EXACT(2) COORD_RANK_EXACT(3) COORD_RANK_EXACT(4) COORD_RANK_EXACT(5)
    COORD_RANK_EXACT(6) COORD_RANK_EXACT(7) COORD_RANK_EXACT(8) COORD_RANK_EXACT(9) COORD_RANK_EXACT(10)
    COORD_RANK_EXACT(11) COORD_RANK_EXACT(12) COORD_RANK_EXACT(13) COORD_RANK_EXACT(14) COORD_RANK_EXACT(15)
    COORD_RANK_EXACT(16)
    default:
      if (n <= 24) COORD_RANK_LAUNCH(24, 2, false);
      else if (n <= 32) COORD_RANK_LAUNCH(32, 2, false);
      else if (n <= 48) COORD_RANK_LAUNCH(48, 1, false);
      else COORD_RANK_LAUNCH(64, 1, false);
  }
#undef COORD_RANK_EXACT
#undef COORD_RANK_LAUNCH
  hipLaunchKernelGGL(coord_rank_finalize, dim3(2 * n), dim3(kWave), 0, s, part, bx, counts);
  DBA_LAUNCH_CHECK();
}

}  // namespace

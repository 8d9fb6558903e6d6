// Bulyan's second stage (config krum_f with krum_bulyan; El Mhamdi, Guerraoui and Rouault, ICML
// 2018): the coordinate-wise median window over the t rows that iterated Krum selected, one fused
// pass in the shape of trim.hip.  Per coordinate c the t values are sorted (s_0 <= ... <= s_{t-1},
// trim's order: -0 == +0, every NaN after +inf); with beta = t - 2 f, m = (t - 1) / 2 and
// med = (double)s_m the window is the ranks a .. a + beta - 1, where
//     a = #{ j in 0 .. 2 f - 1 : (double)s_{j+beta} - med < med - (double)s_j }
// (fp64 on both sides, an ordered comparison: false when a side is NaN), and
//     total[c] = ((d_a + d_{a+1}) + ...) + d_{a+beta-1},   d_r = (double)s_r - (double)base[c]
// is added in ascending rank with one fp64 rounding per operation.  Per row, the coordinates at
// which its value was kept (lo <= v <= hi, lo = s_a, hi = s_{a+beta-1}) and at which it was cut as
// high (v > hi, or v NaN and hi not) are counted, as trim.hip counts them.
//   * loads, keys, the sorting network, the instantiations and the count reduction are trim.hip's
//     (this file carries its own copies of the small helpers: trim.hip is left as it is)
//   * beta is uniform, a differs per lane.  s_{j+beta} comes from a copy of the sorted keys moved
//     down by beta in log2 N conditional stages (a uniform branch around moves between constant
//     register indices); lo, hi and the summands are picked by per-lane selects over constant
//     indices: nothing is indexed dynamically, so nothing goes to scratch
//   * only the window's ranks are added (a select between tot and tot + d_r, never tot + 0)
//   * a thread's coordinates are sorted and windowed one after the other, so one moved copy of the
//     keys is live at a time: up to 32 inputs every instantiation needs fewer registers than
//     trim.hip's of the same N, the 48- and 64-input ones 8 and 10 more at the same waves per SIMD
#include "common.hpp"
#include "rowquad.hpp"
#include "sortnet.hpp"
#include <algorithm>

// sums only: nothing to contract, and nothing is to be
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

// the window of one coordinate from its sorted keys: the total over its ranks and the two
// threshold keys.  n, f (and beta, m) are uniform; a is not
template <int N>
__device__ __forceinline__ void median_window(const uint32_t (&key)[N], int n, int f, float base, double& tot_out,
                                              uint32_t& lo_out, uint32_t& hi_out) {
  const int beta = n - 2 * f, m = (n - 1) / 2;
  uint32_t mk = 0u;
#pragma unroll
  for (int r = 0; r < N; ++r)
    if (r == m) mk = key[r];
  const double med = (double)from_key(mk);

  // up[r] = key[r + beta] wherever r + beta < N (all that is read: r < 2 f, r + beta < n)
  uint32_t up[N];
#pragma unroll
  for (int r = 0; r < N; ++r) up[r] = key[r];
#pragma unroll
  for (int s = 1; s < N; s <<= 1) {
    if (beta & s) {
#pragma unroll
      for (int r = 0; r + s < N; ++r) up[r] = up[r + s];
    }
  }
  int a = 0;
#pragma unroll
  for (int r = 0; r < N - 1; ++r) {
    if (r < 2 * f) {
      const double above = (double)from_key(up[r]) - med, below = med - (double)from_key(key[r]);
      a += above < below ? 1 : 0;
    }
  }

  // ranks a .. a + beta - 1 in ascending order
  const int top = a + beta - 1;
  const double b = (double)base;
  double tot = 0.0;                 // (0 + d_a = d_a but for the sign of a zero)
  uint32_t lo = 0u, hi = 0u;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r < n) {
      const double with = tot + ((double)from_key(key[r]) - b);
      tot = (r >= a && r <= top) ? with : tot;
      lo = r == a ? key[r] : lo;
      hi = r == top ? key[r] : hi;
    }
  }
  tot_out = tot;
  lo_out = lo;
  hi_out = hi;
}

// one step: coordinates c .. c + cnt of every row
template <int N, int CPT, bool FULL>
__device__ __forceinline__ void bulyan_step(const float* __restrict__ buf, long long rstride,
                                            const int* __restrict__ row_idx, unsigned long long vecmask, int n,
                                            const float* __restrict__ base, bool base_vec, int f, long long c, int cnt,
                                            double* __restrict__ total, int (&count)[N]) {
  uint32_t key[CPT][N], own[CPT][N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r < n) {
      float v[CPT];
      ld_group<CPT, FULL>(row_start(buf, rstride, row_idx, r) + c, (vecmask >> r) & 1, cnt, v);
#pragma unroll
      for (int j = 0; j < CPT; ++j) key[j][r] = own[j][r] = to_key(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < CPT; ++j) key[j][r] = own[j][r] = kNanKey;
    }
  }
  float b[CPT];
  ld_group<CPT, FULL>(base + c, base_vec, cnt, b);

  double tot[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    sortnet_apply<N>(key[j]);
    uint32_t lo, hi;
    median_window<N>(key[j], n, f, b[j], tot[j], lo, hi);
    // a NaN lower threshold: nothing is below it
    const uint32_t lo_j = lo == kNanKey ? 0u : lo;
    const bool live = FULL || j < cnt;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (r < n) {
        const int add = own[j][r] > hi ? 0x10000 : (own[j][r] >= lo_j ? 1 : 0);
        count[r] += live ? add : 0;
      }
    }
  }
  if constexpr (FULL && CPT % 2 == 0) {
#pragma unroll
    for (int j = 0; j < CPT; j += 2) *(double2*)(total + c + j) = make_double2(tot[j], tot[j + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (FULL || j < cnt) total[c + j] = tot[j];
  }
}

// N: inputs of the network; EXACT: n == N (else n <= N, the rest sentinels); CPT coordinates per step.
// part [n][2][gridDim.x] int64: per-block kept and high counts
template <int N, int CPT, bool EXACT>
__global__ __launch_bounds__(256) void coord_bulyan_kernel(const float* __restrict__ buf, long long rstride,
                                                           const int* __restrict__ row_idx, int n_arg,
                                                           const float* __restrict__ base, int f, long long L,
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
    bulyan_step<N, CPT, true>(buf, rstride, row_idx, vecmask, n, base, base_vec, f, g * CPT, CPT, total, count);
  if (g < ng)
    bulyan_step<N, CPT, false>(buf, rstride, row_idx, vecmask, n, base, base_vec, f, g * CPT, (int)(L - g * CPT),
                               total, count);

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

// one wave per (row, kept | high): lane l takes the partials of blocks l, l + 64, ..., then the
// lanes combine in a fixed butterfly
__global__ __launch_bounds__(64) void coord_bulyan_finalize(const long long* __restrict__ part, int nblk,
                                                           long long* __restrict__ counts) {
  const long long slot = blockIdx.x;
  long long s = 0;
  for (int b = threadIdx.x; b < nblk; b += kWave) s += part[slot * nblk + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if (threadIdx.x == 0) counts[slot] = s;
}

template <int N, int CPT, bool EXACT>
void launch(int bx, hipStream_t stream, const float* buf, long long rstride, const int* row_idx, int n,
            const float* base, int f, long long L, double* total, long long* part) {
  hipLaunchKernelGGL((coord_bulyan_kernel<N, CPT, EXACT>), dim3(bx), dim3(256), 0, stream, buf, rstride, row_idx, n,
                     base, f, L, total, part);
}

}  // namespace

// blocks of a call over rows of length L: the workspace is 2 t times as many int64
DBA_EXPORT int dba_coord_bulyan_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kBlocksMax, (nq + 255) / 256));
}

// total [L] fp64 (16-byte aligned) = the median-window sum of (row - base) over rows row_idx[r] (r
// if row_idx is null) of buf, each of L floats, rstride floats apart: per coordinate the n - 2 f
// values closest to the lower median; counts [n][2] int64 = (kept, high) coordinates per row.
// 1 <= n <= 64, 0 <= f, 2 f + 1 <= n, 1 <= L < 2^31 (hipErrorInvalidValue beyond: the caller
// composes those).  part: [2 n][dba_coord_bulyan_blocks(L)] int64 workspace (no initialisation
// needed).
DBA_EXPORT int dba_coord_bulyan(const float* buf, long long rstride, const int* row_idx, int n, const float* base,
                                int f, long long L, double* total, long long* counts, long long* part, void* stream) {
  if (n < 1 || n > kMaxRows || f < 0 || f > kMaxRows || 2 * f + 1 > n || L < 1 || L >= (1LL << 31) ||
      !aligned16(total))
    return (int)hipErrorInvalidValue;
  const int bx = dba_coord_bulyan_blocks(L);
  hipStream_t s = (hipStream_t)stream;
#define BULYAN_EXACT(N) \
  case N: launch<N, kQuad, true>(bx, s, buf, rstride, row_idx, n, base, f, L, total, part); break;
  switch (n) {
    BULYAN_EXACT(1) BULYAN_EXACT(2) BULYAN_EXACT(3) BULYAN_EXACT(4) BULYAN_EXACT(5) BULYAN_EXACT(6)
    BULYAN_EXACT(7) BULYAN_EXACT(8) BULYAN_EXACT(9) BULYAN_EXACT(10) BULYAN_EXACT(11) BULYAN_EXACT(12)
    BULYAN_EXACT(13) BULYAN_EXACT(14) BULYAN_EXACT(15) BULYAN_EXACT(16)
    default:
      if (n <= 24) launch<24, 2, false>(bx, s, buf, rstride, row_idx, n, base, f, L, total, part);
      else if (n <= 32) launch<32, 2, false>(bx, s, buf, rstride, row_idx, n, base, f, L, total, part);
      else if (n <= 48) launch<48, 1, false>(bx, s, buf, rstride, row_idx, n, base, f, L, total, part);
      else launch<64, 1, false>(bx, s, buf, rstride, row_idx, n, base, f, L, total, part);
  }
#undef BULYAN_EXACT
  hipLaunchKernelGGL(coord_bulyan_finalize, dim3(2 * n), dim3(kWave), 0, s, part, bx, counts);
  DBA_LAUNCH_CHECK();
}

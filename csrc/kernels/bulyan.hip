// Bulyan's second stage (config krum_f with krum_bulyan; El Mhamdi, Guerraoui and Rouault, ICML
// 2018) as a rule of the coordinate-rank pass (coordrank.hpp, which describes the pass): the
// coordinate-wise median window over the t rows that iterated Krum selected.  Per coordinate c the
// t values are sorted (s_0 <= ... <= s_{t-1}); with beta = t - 2 f, m = (t - 1) / 2 and
// med = (double)s_m the window is the ranks a .. a + beta - 1, where
//     a = #{ j in 0 .. 2 f - 1 : (double)s_{j+beta} - med < med - (double)s_j }
// (fp64 on both sides, an ordered comparison: false when a side is NaN), with lo = s_a and
// hi = s_{a+beta-1}.
//   * beta is uniform, a differs per lane.  s_{j+beta} comes from a copy of the sorted keys moved
//     down by beta in log2 N conditional stages (a uniform branch around moves between constant
//     register indices); lo, hi and the summands are picked by per-lane selects over constant
//     indices: nothing is indexed dynamically, so nothing goes to scratch
//   * only the window's ranks are added (a select between tot and tot + d_r, never tot + 0)
//   * a thread's coordinates are sorted and windowed one after the other, so one moved copy of the
//     keys is live at a time: up to 32 inputs every instantiation needs fewer registers than
//     trim.hip's of the same N, the 48- and 64-input ones 8 and 10 more at the same waves per SIMD
#include "coordrank.hpp"

namespace {

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

struct Bulyan {
// one step: coordinates c .. c + cnt of every row
template <int N, int CPT, bool FULL>
static __device__ __forceinline__ void step(const float* __restrict__ buf, long long rstride,
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
};

}  // namespace

// blocks of a call over rows of length L: the workspace is 2 t times as many int64
DBA_EXPORT int dba_coord_bulyan_blocks(long long L) { return coord_rank_blocks(L); }

// total [L] fp64 (16-byte aligned) = the median-window sum of (row - base) over rows row_idx[r] (r
// if row_idx is null) of buf, each of L floats, rstride floats apart: per coordinate the n - 2 f
// values closest to the lower median; counts [n][2] int64 = (kept, high) coordinates per row.
// 1 <= n <= 64, 0 <= f, 2 f + 1 <= n, 1 <= L < 2^31 (hipErrorInvalidValue beyond: the caller
// composes those).  part: [2 n][dba_coord_bulyan_blocks(L)] int64 workspace (no initialisation
// needed).
DBA_EXPORT int dba_coord_bulyan(const float* buf, long long rstride, const int* row_idx, int n, const float* base,
                                int f, long long L, double* total, long long* counts, long long* part, void* stream) {
  if (!coord_rank_valid(n, L, total) || f < 0 || f > kMaxRows || 2 * f + 1 > n) return (int)hipErrorInvalidValue;
  return coord_rank<Bulyan>(buf, rstride, row_idx, n, base, f, L, total, counts, part, stream);
}

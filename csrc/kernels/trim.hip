// Coordinate-wise trimmed mean / median (config trim_k; Yin et al., ICML 2018) as a rule of the
// coordinate-rank pass (coordrank.hpp, which describes the pass): per coordinate the k smallest and
// k largest of the n sorted values are dropped, that is the ranks k .. n - 1 - k are added, with
// lo = s_k and hi = s_{n-1-k}.
#include "coordrank.hpp"

namespace {

struct Trim {
// one step: coordinates c .. c + cnt of every row
template <int N, int CPT, bool FULL>
static __device__ __forceinline__ void step(const float* __restrict__ buf, long long rstride,
                                          const int* __restrict__ row_idx, unsigned long long vecmask, int n,
                                          const float* __restrict__ base, bool base_vec, int k, long long c, int cnt,
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
#pragma unroll
  for (int j = 0; j < CPT; ++j) sortnet_apply<N>(key[j]);

  // ranks k .. n - 1 - k in ascending order (k is uniform: scalar branches around constant indices)
  const int top = n - 1 - k;
  double tot[CPT];
  uint32_t lo[CPT], hi[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    tot[j] = 0.0;                   // (0 + d_k = d_k but for the sign of a zero)
    lo[j] = hi[j] = 0u;
  }
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (r >= k && r <= top) {
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        tot[j] = tot[j] + ((double)from_key(key[j][r]) - (double)b[j]);
        if (r == k) lo[j] = key[j][r];
        if (r == top) hi[j] = key[j][r];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    // a NaN lower threshold: nothing is below it
    const uint32_t lo_j = lo[j] == kNanKey ? 0u : lo[j];
    const bool live = FULL || j < cnt;
#pragma unroll
    for (int r = 0; r < N; ++r) {
      if (r < n) {
        const int add = own[j][r] > hi[j] ? 0x10000 : (own[j][r] >= lo_j ? 1 : 0);
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

// blocks of a call over rows of length L: the workspace is 2 n times as many int64
DBA_EXPORT int dba_coord_trim_blocks(long long L) { return coord_rank_blocks(L); }

// total [L] fp64 (16-byte aligned) = the trimmed sum of (row - base) over rows row_idx[r] (r if
// row_idx is null) of buf, each of L floats, rstride floats apart, dropping the k smallest and k
// largest per coordinate; counts [n][2] int64 = (kept, high) coordinates per row.  1 <= n <= 64,
// 0 <= k <= (n - 1) / 2, 1 <= L < 2^31 (hipErrorInvalidValue beyond: the caller composes those).
// part: [2 n][dba_coord_trim_blocks(L)] int64 workspace (no initialisation needed).
DBA_EXPORT int dba_coord_trim(const float* buf, long long rstride, const int* row_idx, int n, const float* base, int k,
                              long long L, double* total, long long* counts, long long* part, void* stream) {
  if (!coord_rank_valid(n, L, total) || k < 0 || 2 * k + 1 > n) return (int)hipErrorInvalidValue;
  return coord_rank<Trim>(buf, rstride, row_idx, n, base, k, L, total, counts, part, stream);
}

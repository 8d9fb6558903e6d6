// FLAME's hot path: G[i][j] = sum_k d_i[k] d_j[k] in fp64, d_i = x_i - base, over n strided fp32
// rows of length L (the clients' final states, read where they lie: rows are picked by an optional
// index list, and there is no [n, L] delta or fp64 temporary) and one fp32 base row (the global
// model).  The layout of krum.hip's pairwise distances, with a base operand and the diagonal kept:
//   * blockIdx.x walks the row length, blockIdx.y the tile pairs (ti <= tj) of the rows.  A block
//     keeps its tile pair's fp64 accumulators in registers, at most 64 of them (128 VGPRs), and
//     loads each of its rows, and the base, once per quad:
//       - up to kLone = 10 rows are ONE triangular tile (55 pairs i <= j; 11 rows would need 66):
//         every row and the base are fetched once, so the n = 10 round case moves (n + 1) L 4 bytes
//       - more rows are cut into tiles of kTile = 8: a diagonal tile pair holds its tile's
//         36 pairs a <= b, an off-diagonal one 8 x 8; each row is fetched once per tile pair it is in
//   * d = (double)x - (double)base is exact; it is formed once per row and element, then one fma
//     per product.  The diagonal is a pair (i, i) like any other: the same code, the same order, so
//     two identical rows give G[a][b] == G[a][a] == G[b][b] bit for bit
//   * every unordered pair is accumulated once, in exactly one tile pair; the finalize launch sums
//     its per-block partials in one fixed order (no atomics: bitwise run to run) and writes
//     G[i][j] and G[j][i] from the same value
//   * which elements a thread takes and the order it adds them in depend only on L and the
//     launch grid (quad q of every row goes to thread q mod the grid, in ascending q), not on the
//     rows' alignment, on the tile a pair falls into or on the other rows of the call: the same
//     bits from an aligned copy and a misaligned view, and from any subset of the rows
// Rows are read four floats per lane (rowquad.hpp).
#include "common.hpp"
#include "rowquad.hpp"
#include <algorithm>
#include <math.h>

// the accumulation below is written with explicit fma(): nothing else is to be contracted
#pragma clang fp contract(off)

namespace {

constexpr int kTile = 8;            // rows per tile: kTile x kTile fp64 accumulators per thread
constexpr int kLone = 10;           // most rows of a lone triangular tile: 10 * 11 / 2 = 55 accumulators
constexpr int kAcc = kTile * kTile;
constexpr int kMaxRows = 64;
constexpr int kBlocksMax = 512;     // x 256 threads x 4 floats = 524288 elements per sweep of the grid

static_assert(kLone * (kLone + 1) / 2 <= kAcc && kLone >= kTile, "a triangular tile's pairs fit the accumulators");
static_assert((kLone + 1) * (kLone + 2) / 2 > kAcc, "kLone is the largest lone tile");

// the accumulator of local rows (a, b): a triangular (DIAG) tile holds its pairs a <= b column by
// column, an off-diagonal tile pair all kTile x kTile
template <bool DIAG>
__device__ __forceinline__ constexpr int acc_slot(int a, int b) {
  return DIAG ? b * (b + 1) / 2 + a : a * kTile + b;
}

// the rows of one side of a tile pair: row starts and their alignment
template <int R>
struct Rows {
  const float* p[R];
  bool vec[R];
  int n;                            // rows in use (the others repeat the last one and are never loaded)
};

template <int R>
__device__ __forceinline__ void rows_init(Rows<R>& t, const float* __restrict__ buf, long long rstride,
                                          const int* __restrict__ row_idx, int r0, int cnt) {
  t.n = cnt;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = r0 + min(r, cnt - 1);
    t.p[r] = buf + (long long)(row_idx ? row_idx[row] : row) * rstride;
    t.vec[r] = aligned16_dev(t.p[r]);
  }
}

// the quad at float k of every row in use (zeros for the others: their products are never kept)
template <bool FULL, int R>
__device__ __forceinline__ void load_rows(const Rows<R>& t, long long k, int cnt, float (&x)[R][kQuad]) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < t.n) {
      ld_quad_f4<FULL>(t.p[r] + k, t.vec[r], cnt, x[r]);
    } else {
#pragma unroll
      for (int j = 0; j < kQuad; ++j) x[r][j] = 0.f;
    }
  }
}

// one quad (floats k .. k + cnt of every row of the tile pair and of the base) into the
// accumulators, element by element: the deltas of the element (exact in fp64), then one fma, one
// rounding, per pair.  The zero fill of the last quad makes d = 0 - 0 and adds 0.
template <bool DIAG, int RA, int RB>
__device__ __forceinline__ void pair_acc(const float (&xa)[RA][kQuad], const float (&xb)[RB][kQuad],
                                         const float (&bs)[kQuad], int na, int nb, double (&acc)[kAcc]) {
#pragma unroll
  for (int j = 0; j < kQuad; ++j) {
    const double bj = (double)bs[j];
    double da[RA], db[RB];
#pragma unroll
    for (int a = 0; a < RA; ++a) da[a] = (double)xa[a][j] - bj;
#pragma unroll
    for (int b = 0; b < RB; ++b) db[b] = DIAG ? da[b] : (double)xb[b][j] - bj;
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      if (b < nb) {
#pragma unroll
        for (int a = 0; a < RA; ++a)
          if (DIAG ? a <= b : a < na) acc[acc_slot<DIAG>(a, b)] = fma(da[a], db[b], acc[acc_slot<DIAG>(a, b)]);
      }
    }
  }
}

template <bool DIAG, bool FULL, int RA, int RB>
__device__ __forceinline__ void pair_step(const Rows<RA>& ta, const Rows<RB>& tb, const float* __restrict__ base,
                                          bool bvec, long long k, int cnt, double (&acc)[kAcc]) {
  float xa[RA][kQuad], bs[kQuad];
  load_rows<FULL>(ta, k, cnt, xa);
  ld_quad_f4<FULL>(base + k, bvec, cnt, bs);
  if constexpr (DIAG) {
    pair_acc<true, RA, RA>(xa, xa, bs, ta.n, ta.n, acc);
  } else {
    float xb[RB][kQuad];
    load_rows<FULL>(tb, k, cnt, xb);
    pair_acc<false, RA, RB>(xa, xb, bs, ta.n, tb.n, acc);
  }
}

// pair (i <= j) -> its slot in the partials: row-major order of the upper triangle with its diagonal
__device__ __forceinline__ long long pair_slot(int i, int j, int n) {
  return (long long)i * (2 * n - i + 1) / 2 + (j - i);
}

// a block's share of one tile pair: rows a0 .. a0 + na against rows b0 .. b0 + nb (DIAG: the same
// tile, pairs a <= b), partials to part[pair_slot][blockIdx.x]
template <bool DIAG, int RA, int RB>
__device__ __forceinline__ void tile_pair_body(const float* __restrict__ buf, long long rstride,
                                               const int* __restrict__ row_idx, int n,
                                               const float* __restrict__ base, long long L, int a0, int na, int b0,
                                               int nb, double* __restrict__ part, double (&red)[4][kAcc]) {
  Rows<RA> ta;
  Rows<RB> tb;
  rows_init(ta, buf, rstride, row_idx, a0, na);
  rows_init(tb, buf, rstride, row_idx, b0, nb);
  const bool bvec = aligned16_dev(base);
  double acc[kAcc];
#pragma unroll
  for (int s = 0; s < kAcc; ++s) acc[s] = 0.0;

  // whole quads in ascending order, then the row's last, partial quad (one thread of the launch)
  const long long nq = (L + kQuad - 1) / kQuad, nfull = L / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if constexpr (DIAG) {
    // a triangular tile has the registers to issue the next quad's loads before this quad's
    // arithmetic (the same quads in the same order)
    if (q < nfull) {
      float xa[RA][kQuad], bs[kQuad];
      load_rows<true>(ta, q * kQuad, kQuad, xa);
      ld_quad_f4<true>(base + q * kQuad, bvec, kQuad, bs);
      for (;;) {
        const long long qn = q + stride;
        if (qn >= nfull) break;
        float xn[RA][kQuad], bn[kQuad];
        load_rows<true>(ta, qn * kQuad, kQuad, xn);
        ld_quad_f4<true>(base + qn * kQuad, bvec, kQuad, bn);
        pair_acc<true, RA, RA>(xa, xa, bs, na, na, acc);
#pragma unroll
        for (int r = 0; r < RA; ++r)
#pragma unroll
          for (int j = 0; j < kQuad; ++j) xa[r][j] = xn[r][j];
#pragma unroll
        for (int j = 0; j < kQuad; ++j) bs[j] = bn[j];
        q = qn;
      }
      pair_acc<true, RA, RA>(xa, xa, bs, na, na, acc);
      q += stride;
    }
  } else {
    for (; q < nfull; q += stride) pair_step<DIAG, true>(ta, tb, base, bvec, q * kQuad, kQuad, acc);
  }
  if (q < nq) pair_step<DIAG, false>(ta, tb, base, bvec, q * kQuad, (int)(L - q * kQuad), acc);

  // lanes in a fixed butterfly, then the four waves in order
#pragma unroll
  for (int b = 0; b < (DIAG ? RA : RB); ++b) {
#pragma unroll
    for (int a = 0; a < RA; ++a) {
      if (b < nb && (DIAG ? a <= b : a < na)) {
        double s = acc[acc_slot<DIAG>(a, b)];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][acc_slot<DIAG>(a, b)] = s;
      }
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kAcc) {
    int a, b;
    if (DIAG) {                    // t = b (b + 1) / 2 + a, a <= b
      b = 0;
      a = t;
      while (a > b) {
        a -= b + 1;
        ++b;
      }
    } else {
      a = t / kTile;
      b = t % kTile;
    }
    if (a < na && b < nb)
      part[pair_slot(a0 + a, b0 + b, n) * gridDim.x + blockIdx.x] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  }
}

// n <= kLone rows as one triangular tile (a kernel of its own: its registers are not the tiled one's)
__global__ __launch_bounds__(256) void delta_gram_lone_kernel(const float* __restrict__ buf, long long rstride,
                                                              const int* __restrict__ row_idx, int n,
                                                              const float* __restrict__ base, long long L,
                                                              double* __restrict__ part) {
  __shared__ double red[4][kAcc];
  tile_pair_body<true, kLone, kLone>(buf, rstride, row_idx, n, base, L, 0, n, 0, n, part, red);
}

// n > kLone rows in tiles of kTile
__global__ __launch_bounds__(256) void delta_gram_kernel(const float* __restrict__ buf, long long rstride,
                                                         const int* __restrict__ row_idx, int n,
                                                         const float* __restrict__ base, long long L,
                                                         double* __restrict__ part) {
  __shared__ double red[4][kAcc];
  // tile pair blockIdx.y in row-major order of the upper triangle of nt x nt tiles
  const int nt = (n + kTile - 1) / kTile;
  int ti = 0, tj = blockIdx.y;
  while (tj >= nt - ti) {
    tj -= nt - ti;
    ++ti;
  }
  tj += ti;
  const int a0 = ti * kTile, b0 = tj * kTile;
  const int na = min(kTile, n - a0), nb = min(kTile, n - b0);
  if (ti == tj)                    // (a last tile of one row still holds that row's diagonal)
    tile_pair_body<true, kTile, kTile>(buf, rstride, row_idx, n, base, L, a0, na, a0, na, part, red);
  else
    tile_pair_body<false, kTile, kTile>(buf, rstride, row_idx, n, base, L, a0, na, b0, nb, part, red);
}

// one wave per pair (i <= j): lane l takes the partials of blocks l, l + 64, ... in that order, then
// the lanes combine in a fixed butterfly (krum.hip's finalize order)
__global__ __launch_bounds__(64) void delta_gram_finalize(const double* __restrict__ part, int nblk, int n,
                                                         double* __restrict__ out) {
  int t = blockIdx.x;
  const long long slot = t;
  int i = 0;
  while (t >= n - i) {
    t -= n - i;
    ++i;
  }
  const int j = i + t;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kWave) s += part[slot * nblk + b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if (threadIdx.x == 0) {
    out[(long long)i * n + j] = s;
    out[(long long)j * n + i] = s;
  }
}

}  // namespace

// per-pair partials of a call over rows of length L: the workspace is n (n + 1) / 2 times as many doubles
DBA_EXPORT int dba_delta_gram_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kBlocksMax, (nq + 255) / 256));
}

// out [n][n] fp64 = Gram matrix of the deltas (row - base) of rows row_idx[r] (r if row_idx is null)
// of buf, each of L floats, rstride floats apart, against base [L]; 1 <= n <= 64
// (hipErrorInvalidValue beyond: the caller composes larger sets).  part: [n (n + 1) / 2]
// [dba_delta_gram_blocks(L)] fp64 workspace (no initialisation needed).  n = 0: nothing is
// launched; L = 0: zeros, without a pass over the rows.
DBA_EXPORT int dba_delta_gram(const float* buf, long long rstride, const int* row_idx, int n, const float* base,
                              long long L, double* out, double* part, void* stream) {
  if (n <= 0) return 0;
  if (n > kMaxRows) return (int)hipErrorInvalidValue;
  if (L <= 0) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * n * n, (hipStream_t)stream);
    return (int)e;
  }
  const int bx = dba_delta_gram_blocks(L);
  if (n <= kLone) {
    hipLaunchKernelGGL(delta_gram_lone_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, buf, rstride, row_idx, n,
                       base, L, part);
  } else {
    const int nt = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(delta_gram_kernel, dim3(bx, nt * (nt + 1) / 2), dim3(256), 0, (hipStream_t)stream, buf, rstride,
                       row_idx, n, base, L, part);
  }
  hipLaunchKernelGGL(delta_gram_finalize, dim3(n * (n + 1) / 2), dim3(kWave), 0, (hipStream_t)stream, part, bx, n,
                     out);
  DBA_LAUNCH_CHECK();
}

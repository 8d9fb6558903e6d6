// Robust-learning-rate FedAvg (config rlr_threshold; Ozdayi, Kantarcioglu and Gel, AAAI 2021): the
// server takes a sign vote per coordinate over the clients' updates and applies the averaged
// update with a NEGATIVE rate wherever fewer than theta clients' worth of signs agree.  Three
// passes over the strided client rows (the final states, read where they lie: no [n, L] delta or
// sign temporary):
//   * delta sum + votes   total[c] = sum_i ((double)x_i[c] - (double)w[c]) in row order (the bits of
//                         flat.hip delta_sum_kernel) and V[c] = sum_i sign(x_i[c] - w[c]) as int32,
//                         the sign from fp32 comparisons (a NaN on either side, -0 against +0: 0)
//   * vote agreement      per client, over the KEPT coordinates (|V| >= theta): at how many its
//                         non-zero sign equals sign(V) (agree) and -sign(V) (dissent)
//   * apply               w[c] += (float)(total[c] * (double)(kept ? coef : -coef)) (+ noise): the
//                         update of flat.hip noise_add_kernel (noise.hpp), so a kept / flipped
//                         coordinate gets the bits of dba_add_noise_scaled with +coef / -coef; and
//                         the number of flipped coordinates
// Sums over clients decompose, so each rank runs the first two passes on its own rows and the
// fp64 totals, int32 votes and int64 counts are all-reduced (fl/aggregate.py fedavg_rlr).
// No atomics: the counts go through lanes in a fixed butterfly, the four waves in order, per-block
// int64 partials and a finalize launch (countfin.hpp), so they are bitwise run to run; every other output
// depends on its own coordinate alone, never on the launch grid.
// Rows are read four floats per lane (rowquad.hpp); outputs take 16-byte stores where their own
// start allows.
#include "common.hpp"
#include "countfin.hpp"
#include "noise.hpp"
#include "rowquad.hpp"
#include <algorithm>

namespace {

constexpr int kBlocksMax = 4096;   // sum + votes, apply: x 256 threads x 4 coordinates = 4194304 per sweep
constexpr int kRowBatch = 4;       // rows whose loads are in flight together in the sum + votes pass
constexpr int kAgreeBatch = 4;     // quads in flight per lane in the agreement pass
constexpr int kAgreeBlocksMax = 1024;   // x 256 threads x kAgreeBatch x 4 coordinates = the same sweep
constexpr int kMaxGridY = 65535;

// +1 / -1 / 0: fp32 comparisons (NaN on either side and -0 against +0 give 0)
__device__ __forceinline__ int sign_of(float x, float b) { return (int)(x > b) - (int)(x < b); }

// ---------------------------------------------------------------------------------- apply
// (compiled under the translation unit's default fp contraction, as flat.hip is: the update is
// noise.hpp's, contracted as there)

// one step: coordinates c .. c + cnt
template <bool FULL>
__device__ __forceinline__ int apply_step(float* __restrict__ dst, bool vd, const double* __restrict__ total, bool vt,
                                          const int* __restrict__ votes, bool vv, int theta, long long c, int cnt,
                                          float coef, float sigma, uint32_t seed, int noise) {
  float d[kQuad];
  int V[kQuad];
  double t[kQuad];
  ld_quad<FULL>(dst + c, vd, cnt, d);
  ld_quad<FULL>(votes + c, vv, cnt, V);
  if (FULL && vt) {
    const double2 a = ((const double2*)(total + c))[0], b = ((const double2*)(total + c))[1];
    t[0] = a.x; t[1] = a.y; t[2] = b.x; t[3] = b.y;
  } else {
#pragma unroll
    for (int j = 0; j < kQuad; ++j) t[j] = (FULL || j < cnt) ? total[c + j] : 0.0;
  }
  int flipped = 0;
#pragma unroll
  for (int j = 0; j < kQuad; ++j) {
    const bool kept = (V[j] < 0 ? -(long long)V[j] : (long long)V[j]) >= (long long)theta;
    const float u = noise_scaled_update<double>(t[j], kept ? coef : -coef, sigma, seed, noise, c + j);
    d[j] += u;
    flipped += ((FULL || j < cnt) && !kept) ? 1 : 0;
  }
  st_quad<FULL>(dst + c, vd, cnt, d);
  return flipped;
}

// part [gridDim.x] int64: this block's flipped coordinates
__global__ __launch_bounds__(256) void rlr_apply_kernel(float* __restrict__ dst, const double* __restrict__ total,
                                                        const int* __restrict__ votes, int theta, long long L,
                                                        float coef, float sigma, uint32_t seed, int noise,
                                                        long long* __restrict__ part) {
  __shared__ long long red[4];
  const bool vd = aligned16_dev(dst), vt = aligned16_dev(total), vv = aligned16_dev(votes);
  const long long nq = (L + kQuad - 1) / kQuad, nfull = L / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  int flipped = 0;
  for (; q < nfull; q += stride)
    flipped += apply_step<true>(dst, vd, total, vt, votes, vv, theta, q * kQuad, kQuad, coef, sigma, seed, noise);
  if (q < nq)
    flipped += apply_step<false>(dst, vd, total, vt, votes, vv, theta, q * kQuad, (int)(L - q * kQuad), coef, sigma,
                                 seed, noise);
  const long long s = block_sum<long long>(flipped, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// sums only from here on: nothing to contract, and nothing is to be
#pragma clang fp contract(off)

// ---------------------------------------------------------------------- delta sum + votes
// one row's quad into the running fp64 sums and int32 votes of its four coordinates
__device__ __forceinline__ void vote_acc(const float (&x)[kQuad], const float (&b)[kQuad], double (&acc)[kQuad],
                                         int (&V)[kQuad]) {
#pragma unroll
  for (int j = 0; j < kQuad; ++j) {
    acc[j] += (double)x[j] - (double)b[j];
    V[j] += sign_of(x[j], b[j]);
  }
}

// one step: coordinates c .. c + cnt of every row, the rows in order, kRowBatch rows' loads issued
// before the first use
template <bool FULL>
__device__ __forceinline__ void votes_step(const float* __restrict__ rows, long long rstride, int nrows,
                                           const float* __restrict__ base, bool vb, long long c, int cnt,
                                           double* __restrict__ total, bool vt, int* __restrict__ votes, bool vv) {
  float b[kQuad];
  ld_quad<FULL>(base + c, vb, cnt, b);
  double acc[kQuad] = {0.0, 0.0, 0.0, 0.0};
  int V[kQuad] = {0, 0, 0, 0};
  int r = 0;
  for (; r + kRowBatch <= nrows; r += kRowBatch) {
    float x[kRowBatch][kQuad];
#pragma unroll
    for (int u = 0; u < kRowBatch; ++u) {
      const float* p = rows + (long long)(r + u) * rstride;
      ld_quad<FULL>(p + c, aligned16_dev(p), cnt, x[u]);
    }
#pragma unroll
    for (int u = 0; u < kRowBatch; ++u) vote_acc(x[u], b, acc, V);
  }
  for (; r < nrows; ++r) {
    float x[kQuad];
    const float* p = rows + (long long)r * rstride;
    ld_quad<FULL>(p + c, aligned16_dev(p), cnt, x);
    vote_acc(x, b, acc, V);
  }
  st_quad<FULL>(total + c, vt, cnt, acc);
  st_quad<FULL>(votes + c, vv, cnt, V);
}

__global__ __launch_bounds__(256) void delta_sum_votes_kernel(const float* __restrict__ rows, long long rstride,
                                                              int nrows, const float* __restrict__ base, long long L,
                                                              double* __restrict__ total, int* __restrict__ votes) {
  const bool vb = aligned16_dev(base), vt = aligned16_dev(total), vv = aligned16_dev(votes);
  // whole steps, then the rows' last, partial one (one thread of the launch)
  const long long nq = (L + kQuad - 1) / kQuad, nfull = L / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  for (; q < nfull; q += stride)
    votes_step<true>(rows, rstride, nrows, base, vb, q * kQuad, kQuad, total, vt, votes, vv);
  if (q < nq)
    votes_step<false>(rows, rstride, nrows, base, vb, q * kQuad, (int)(L - q * kQuad), total, vt, votes, vv);
}

// ------------------------------------------------------------------------- vote agreement
// one quad of client i against the reduced votes (the zero fill of a partial quad has sign 0)
__device__ __forceinline__ void agree_acc(const float (&x)[kQuad], const float (&b)[kQuad], const int (&V)[kQuad],
                                          int theta, int& agree, int& dissent) {
#pragma unroll
  for (int j = 0; j < kQuad; ++j) {
    const int s = sign_of(x[j], b[j]);
    const int m = (int)(V[j] > 0) - (int)(V[j] < 0);
    const bool kept = (V[j] < 0 ? -(long long)V[j] : (long long)V[j]) >= (long long)theta;
    agree += (kept && s != 0 && s == m) ? 1 : 0;
    dissent += (kept && s != 0 && s == -m) ? 1 : 0;
  }
}

// part [n][2][gridDim.x] int64: block (x, i)'s agree and dissent counts of client i
__global__ __launch_bounds__(256) void vote_agreement_kernel(const float* __restrict__ rows, long long rstride,
                                                             const float* __restrict__ base,
                                                             const int* __restrict__ votes, int theta, long long L,
                                                             long long* __restrict__ part) {
  __shared__ long long red_a[4], red_d[4];
  const int i = blockIdx.y;
  const float* p = rows + (long long)i * rstride;
  const bool vp = aligned16_dev(p), vb = aligned16_dev(base), vv = aligned16_dev(votes);
  const long long nq = (L + kQuad - 1) / kQuad, nfull = L / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int agree = 0, dissent = 0;      // (a thread takes fewer than 2^31 coordinates for any L < 2^51)
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  // batches of kAgreeBatch whole quads, every load issued before the first use, then what is left
  for (; q + (kAgreeBatch - 1) * stride < nfull; q += kAgreeBatch * stride) {
    float x[kAgreeBatch][kQuad], b[kAgreeBatch][kQuad];
    int V[kAgreeBatch][kQuad];
#pragma unroll
    for (int u = 0; u < kAgreeBatch; ++u) {
      const long long c = (q + u * stride) * kQuad;
      ld_quad<true>(p + c, vp, kQuad, x[u]);
      ld_quad<true>(base + c, vb, kQuad, b[u]);
      ld_quad<true>(votes + c, vv, kQuad, V[u]);
    }
#pragma unroll
    for (int u = 0; u < kAgreeBatch; ++u) agree_acc(x[u], b[u], V[u], theta, agree, dissent);
  }
  for (; q < nq; q += stride) {
    const long long c = q * kQuad;
    float x[kQuad], b[kQuad];
    int V[kQuad];
    if (q < nfull) {
      ld_quad<true>(p + c, vp, kQuad, x);
      ld_quad<true>(base + c, vb, kQuad, b);
      ld_quad<true>(votes + c, vv, kQuad, V);
    } else {
      const int cnt = (int)(L - c);
      ld_quad<false>(p + c, vp, cnt, x);
      ld_quad<false>(base + c, vb, cnt, b);
      ld_quad<false>(votes + c, vv, cnt, V);
    }
    agree_acc(x, b, V, theta, agree, dissent);
  }
  const long long a = block_sum<long long>(agree, red_a), d = block_sum<long long>(dissent, red_d);
  if (threadIdx.x == 0) {
    part[((long long)i * 2 + 0) * gridDim.x + blockIdx.x] = a;
    part[((long long)i * 2 + 1) * gridDim.x + blockIdx.x] = d;
  }
}

}  // namespace

// blocks per client of the agreement pass over rows of length L (a thread takes kAgreeBatch quads
// at a time): its workspace is 2 n times as many int64
DBA_EXPORT int dba_vote_agreement_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad, per = 256 * kAgreeBatch;
  return (int)std::max(1LL, std::min((long long)kAgreeBlocksMax, (nq + per - 1) / per));
}

// blocks of the sum + votes and the apply pass over L coordinates: the apply workspace is as many int64
DBA_EXPORT int dba_rlr_apply_blocks(long long L) {
  const long long nq = (L + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kBlocksMax, (nq + 255) / 256));
}

// total [L] fp64 = sum_r (rows[r] - base) in row order (the bits of dba_delta_sum), votes [L] int32 =
// sum_r sign(rows[r] - base); rows: nrows rows of L floats, rstride floats apart
DBA_EXPORT int dba_delta_sum_votes(const float* rows, long long rstride, int nrows, const float* base, long long L,
                                   double* total, int* votes, void* stream) {
  if (nrows < 0 || L < 0) return (int)hipErrorInvalidValue;
  if (L == 0) return 0;
  hipLaunchKernelGGL(delta_sum_votes_kernel, dim3(dba_rlr_apply_blocks(L)), dim3(256), 0, (hipStream_t)stream,
                     rows, rstride, nrows, base, L, total, votes);
  DBA_LAUNCH_CHECK();
}

// counts [nrows][2] int64 = (agree, dissent) of each row against the reduced votes [L] at threshold
// theta.  part: [2 nrows][dba_vote_agreement_blocks(L)] int64 workspace (no initialisation needed).
// 1 <= nrows <= 65535 (hipErrorInvalidValue beyond), L >= 1
DBA_EXPORT int dba_vote_agreement(const float* rows, long long rstride, int nrows, const float* base, const int* votes,
                                  int theta, long long L, long long* counts, long long* part, void* stream) {
  if (nrows < 1 || nrows > kMaxGridY || L < 1) return (int)hipErrorInvalidValue;
  const int bx = dba_vote_agreement_blocks(L);
  hipLaunchKernelGGL(vote_agreement_kernel, dim3(bx, nrows), dim3(256), 0, (hipStream_t)stream, rows, rstride, base,
                     votes, theta, L, part);
  hipLaunchKernelGGL(count_finalize, dim3(2 * nrows), dim3(256), 0, (hipStream_t)stream, part, bx, counts);
  DBA_LAUNCH_CHECK();
}

// dst[c] += (float)(total[c] * (double)(|votes[c]| >= theta ? coef : -coef)) (+ N(0, sigma), the hash
// RNG and counters of dba_add_noise_scaled); flipped [1] int64 = the coordinates with |votes[c]| <
// theta.  part: [dba_rlr_apply_blocks(L)] int64 workspace (no initialisation needed).  L >= 1
DBA_EXPORT int dba_rlr_apply(float* dst, const double* total, const int* votes, int theta, long long L, float coef,
                             float sigma, unsigned seed, int noise, long long* flipped, long long* part,
                             void* stream) {
  if (L < 1) return (int)hipErrorInvalidValue;
  const int bx = dba_rlr_apply_blocks(L);
  hipLaunchKernelGGL(rlr_apply_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, dst, total, votes, theta, L, coef,
                     sigma, (uint32_t)seed, noise, part);
  hipLaunchKernelGGL(count_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, part, bx, flipped);
  DBA_LAUNCH_CHECK();
}

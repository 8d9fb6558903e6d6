// Norm-clipped FedAvg over the strided client rows (no [n, L] delta temporary; no atomics: every
// cross-block reduction writes per-block partials summed in a fixed order, as in flat.hip).
//   * delta stats        ||rows_i - base||^2 (fp64) and max |rows_i - base| (fp32) for ALL clients in
//                        one pass: the update norms the clip factors come from, and the bound the
//                        fixed grid's exponent comes from
//   * clipped delta sum  sum_i s_i (rows_i - base) as two-limb fixed-point int64 sums (the grid of
//                        flat.hip wsum_fixed_kernel: exact and order-free, so rank partials
//                        all-reduce to world-invariant bits), or in plain fp64 when the grid cannot
//                        hold the sum (a non-finite delta, more than 512 clients)
// Rows are read four floats per lane (rowquad.hpp; where a row start is not 16-byte aligned the
// compiler is free to serve the four scalar loads as one dword-aligned wide load, which gfx950 allows).
#include "common.hpp"
#include "rowquad.hpp"
#include <algorithm>
#include <math.h>

// every fp64 operation below is evaluated exactly as written (no fused multiply-add): the limbs
// must equal ops/reference.py's bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int kStatBlocksMax = 512;
constexpr int kStatBatch = 4;      // quads in flight per lane in the stats pass
constexpr int kSumBlocksMax = 4096;   // x 256 threads x 4 floats = 16384 * 256 elements per sweep

// floats p[0 .. cnt) (cnt = 4 except at the end of a row, tested at run time), zero-filled
__device__ __forceinline__ void ld_row_quad(const float* __restrict__ p, bool vec, int cnt, float (&v)[kQuad]) {
  if (cnt == kQuad) ld_quad_f4<true>(p, vec, kQuad, v);
  else ld_quad_f4<false>(p, vec, cnt, v);
}

// one element of a client's delta into its thread's running sum of squares and max |.|
__device__ __forceinline__ void stat_acc(float x, float b, double& s, float& m) {
  const double d = (double)x - (double)b;
  s += d * d;
  const float a = fabsf((float)d);
  if (!(a <= m)) m = (a != a) ? INFINITY : a;
}

// part_sq[i][blk] / part_mx[i][blk] = this block's fp64 sum of squares / fp32 max |.| of client
// i's delta; a NaN delta makes the sum NaN and the max +inf (the max itself is never NaN, so no
// later max can swallow it).  Element -> thread assignment and summation order do not depend on
// the rows' alignment: the same bits from an aligned copy and a misaligned view.
__global__ __launch_bounds__(256) void delta_stats_kernel(const float* __restrict__ rows, long long rstride,
                                                          const float* __restrict__ base, long long n,
                                                          double* __restrict__ part_sq,
                                                          float* __restrict__ part_mx) {
  __shared__ double red_s[4];
  __shared__ float red_m[4];
  const int i = blockIdx.y;
  const float* p = rows + (long long)i * rstride;
  const long long nq = (n + kQuad - 1) / kQuad, nfull = n / kQuad;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const bool vp = aligned16_dev(p), vb = aligned16_dev(base);
  double s = 0.0;
  float m = 0.f;
  long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  // batches of kStatBatch whole quads, every load issued before the first use (the same quads in
  // the same order as the one-at-a-time loop below, which takes what is left)
  for (; q + (kStatBatch - 1) * stride < nfull; q += kStatBatch * stride) {
    float x[kStatBatch][kQuad], b[kStatBatch][kQuad];
#pragma unroll
    for (int u = 0; u < kStatBatch; ++u) {
      ld_quad_f4<true>(p + (q + u * stride) * kQuad, vp, kQuad, x[u]);
      ld_quad_f4<true>(base + (q + u * stride) * kQuad, vb, kQuad, b[u]);
    }
#pragma unroll
    for (int u = 0; u < kStatBatch; ++u)
#pragma unroll
      for (int j = 0; j < kQuad; ++j) stat_acc(x[u][j], b[u][j], s, m);
  }
  for (; q < nq; q += stride) {
    const long long k = q * kQuad;
    const int cnt = n - k < kQuad ? (int)(n - k) : kQuad;
    float x[kQuad], b[kQuad];
    ld_row_quad(p + k, vp, cnt, x);
    ld_row_quad(base + k, vb, cnt, b);
#pragma unroll
    for (int j = 0; j < kQuad; ++j) stat_acc(x[j], b[j], s, m);   // (the zero fill adds 0 and leaves the max)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, kWave);
    m = fmaxf(m, __shfl_xor(m, o, kWave));
  }
  if ((threadIdx.x & 63) == 0) {
    red_s[threadIdx.x >> 6] = s;
    red_m[threadIdx.x >> 6] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_sq[(long long)i * gridDim.x + blockIdx.x] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
    part_mx[(long long)i * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
  }
}

// one wave per client: lane l takes the partials of blocks l, l + 64, ... in that order, then the
// lanes combine in a fixed butterfly — one fixed order, so bitwise run to run (a lone thread
// walking up to 512 partials is a chain of as many dependent L2 round trips: it took longer than
// the pass over the rows)
__global__ __launch_bounds__(64) void delta_stats_finalize(const double* __restrict__ part_sq,
                                                          const float* __restrict__ part_mx, int nblk,
                                                          double* __restrict__ sqnorm, float* __restrict__ maxabs) {
  const int i = blockIdx.x;
  double s = 0.0;
  float m = 0.f;
  for (int b = threadIdx.x; b < nblk; b += kWave) {
    s += part_sq[(long long)i * nblk + b];
    m = fmaxf(m, part_mx[(long long)i * nblk + b]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, kWave);
    m = fmaxf(m, __shfl_xor(m, o, kWave));
  }
  if (threadIdx.x == 0) {
    sqnorm[i] = s;
    maxabs[i] = m;
  }
}

// FIXED: out [2][n] int64 limb sums over r of q = scale[r] * (rows[r][k] - base[k]) * 2^E, hi =
// floor(q), lo = floor((q - hi) * 2^53) (each product quantised ON ITS OWN, then summed exactly);
// E is chosen by the caller so |q| <= 2^52 / nrows.  Otherwise: out [n] fp64, the products summed
// in row order (a NaN / Inf delta is carried into the sum).
template <bool FIXED>
__global__ __launch_bounds__(256) void clipped_sum_kernel(const float* __restrict__ rows, long long rstride, int nrows,
                                                          const float* __restrict__ base,
                                                          const float* __restrict__ scale, void* __restrict__ outp,
                                                          long long n, double scale2E) {
  const long long nq = (n + kQuad - 1) / kQuad;
  const bool vb = aligned16_dev(base);
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    const long long k = q * kQuad;
    const int cnt = n - k < kQuad ? (int)(n - k) : kQuad;
    float b[kQuad];
    ld_row_quad(base + k, vb, cnt, b);
    long long hs[kQuad] = {0, 0, 0, 0}, ls[kQuad] = {0, 0, 0, 0};
    double fs[kQuad] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < nrows; ++r) {
      float x[kQuad];
      const float* p = rows + (long long)r * rstride;
      ld_row_quad(p + k, aligned16_dev(p), cnt, x);
      const double s = (double)scale[r];
#pragma unroll
      for (int j = 0; j < kQuad; ++j) {
        const double d = (double)x[j] - (double)b[j];
        if constexpr (FIXED) {
          const double qv = s * d * scale2E;
          const double hi = floor(qv);
          hs[j] += (long long)hi;
          ls[j] += (long long)floor((qv - hi) * 0x1p53);
        } else {
          fs[j] += s * d;
        }
      }
    }
    if constexpr (FIXED) {
      long long* out = (long long*)outp;
      // 16-byte stores where both limb planes allow them (n even: out + n keeps the alignment)
      if (cnt == kQuad && ((uintptr_t)out & 15) == 0 && (n & 1) == 0) {
        ((longlong2*)(out + k))[0] = make_longlong2(hs[0], hs[1]);
        ((longlong2*)(out + k))[1] = make_longlong2(hs[2], hs[3]);
        ((longlong2*)(out + n + k))[0] = make_longlong2(ls[0], ls[1]);
        ((longlong2*)(out + n + k))[1] = make_longlong2(ls[2], ls[3]);
      } else {
#pragma unroll
        for (int j = 0; j < kQuad; ++j)
          if (j < cnt) {
            out[k + j] = hs[j];
            out[n + k + j] = ls[j];
          }
      }
    } else {
      double* out = (double*)outp;
#pragma unroll
      for (int j = 0; j < kQuad; ++j)
        if (j < cnt) out[k + j] = fs[j];
    }
  }
}

int sum_grid(long long n) {
  const long long nq = (n + kQuad - 1) / kQuad;
  return (int)std::max(1LL, std::min((long long)kSumBlocksMax, (nq + 255) / 256));
}

}  // namespace

DBA_EXPORT int dba_delta_stats_blocks(long long n) {
  return (int)std::max(1LL, std::min((long long)kStatBlocksMax, (n + 4095) / 4096));
}

// part_sq / part_mx: [nrows][dba_delta_stats_blocks(n)] fp64 / fp32 workspaces (no initialisation needed)
DBA_EXPORT int dba_delta_stats(const float* rows, long long rstride, int nrows, const float* base, long long n,
                               double* sqnorm, float* maxabs, double* part_sq, float* part_mx, void* stream) {
  if (nrows <= 0) return 0;
  const int bx = dba_delta_stats_blocks(n);
  hipLaunchKernelGGL(delta_stats_kernel, dim3(bx, nrows), dim3(256), 0, (hipStream_t)stream, rows, rstride, base, n,
                     part_sq, part_mx);
  hipLaunchKernelGGL(delta_stats_finalize, dim3(nrows), dim3(kWave), 0, (hipStream_t)stream, part_sq, part_mx, bx,
                     sqnorm, maxabs);
  DBA_LAUNCH_CHECK();
}

// out [2][n] int64: the fixed-point limb sums of sum_r scale[r] * (rows[r] - base); scale2E = 2^E
DBA_EXPORT int dba_clipped_delta_sum_fixed(const float* rows, long long rstride, int nrows, const float* base,
                                           const float* scale, long long* out, long long n, double scale2E,
                                           void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(clipped_sum_kernel<true>, dim3(sum_grid(n)), dim3(256), 0, (hipStream_t)stream, rows, rstride,
                     nrows, base, scale, (void*)out, n, scale2E);
  DBA_LAUNCH_CHECK();
}

// out [n] fp64: sum_r scale[r] * (rows[r] - base), the fallback when the fixed grid cannot hold it
DBA_EXPORT int dba_clipped_delta_sum(const float* rows, long long rstride, int nrows, const float* base,
                                     const float* scale, double* out, long long n, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(clipped_sum_kernel<false>, dim3(sum_grid(n)), dim3(256), 0, (hipStream_t)stream, rows, rstride,
                     nrows, base, scale, (void*)out, n, 1.0);
  DBA_LAUNCH_CHECK();
}

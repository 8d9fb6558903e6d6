// Flat-buffer server-side kernels over whole model states.  No atomics:
// every cross-block reduction writes per-block partials summed in a fixed order, so results
// are bitwise reproducible.
//   * model-replacement scaling  w' = base + gamma (w - base)             (image_train.py:166-171)
//   * FedAvg delta sum (fp64) + apply + DP noise  dst += coef*sum_i(w_i - g) + N(0, sigma)
//                                 (hash RNG)  (helper.py:218-257)
//   * batched squared distances   ||p_i - m||^2 for ALL clients in one pass (RFA, helper.py:376-381)
//   * weighted sum                sum_i w_i p_i                            (Weiszfeld / FoolsGold)
//   * Gram matrix F F^T on the f32-input MFMA (v_mfma_f32_16x16x4_f32)     (FoolsGold cosine)
//   * anomaly-evasion distance loss  a*CE + (1-a)*||w - w_g||  on the grouped replicas
//     (helper.py:111-123, image_train.py:87-90, loan_train.py:114-117)
#include "common.hpp"
#include "rowquad.hpp"
#include "noise.hpp"
#include <algorithm>

namespace {

int egrid(long long n) { return (int)std::max(1LL, std::min(16384LL, (n + 255) / 256)); }

__global__ void scale_kernel(const float* __restrict__ w, const float* __restrict__ base, float gamma,
                             float* __restrict__ out, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = base[i] + (w[i] - base[i]) * gamma;
}

// dst += coef*upd (+ N(0, sigma)); upd fp32 or fp64 (the FedAvg delta sum is kept in fp64)
template <typename U>
__global__ void noise_add_kernel(float* __restrict__ dst, const U* __restrict__ upd, long long n, float coef,
                                 float sigma, uint32_t seed, int noise) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float u = noise_scaled_update<U>(upd[i], coef, sigma, seed, noise, i);
    dst[i] += u;
  }
}

// out[i] = sum_r (rows[r][i] - base[i]) in fp64, rows in order (FedAvg's per-rank delta sum:
// fp32 deltas summed in fp64 are exact, so the all-reduced total does not depend on how the
// clients are split over ranks)
__global__ void delta_sum_kernel(const float* __restrict__ rows, long long rstride, int nrows,
                                 const float* __restrict__ base, long long n, double* __restrict__ out) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double b = base[i];
    double acc = 0.0;
    for (int r = 0; r < nrows; ++r) acc += (double)rows[(long long)r * rstride + i] - b;
    out[i] = acc;
  }
}

// deterministic two-pass squared distances: part[i][blk] = this block's sum (fp64), then
// sqdist_finalize sums the blocks of point i in block order
__global__ __launch_bounds__(256) void sqdist_kernel(const float* __restrict__ pts, long long p_rstride,
                                                     const float* __restrict__ m, long long n,
                                                     double* __restrict__ part) {
  __shared__ double red[4];
  const int i = blockIdx.y;
  const float* p = pts + (long long)i * p_rstride;
  double s = 0.0;
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    const double d = (double)p[k] - (double)m[k];
    s += d * d;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[(long long)i * gridDim.x + blockIdx.x] = s;
}

__global__ void sqdist_finalize(const double* __restrict__ part, int nblk, int npts, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npts) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(long long)i * nblk + b];
  out[i] = s;
}

template <typename O>
__global__ void wsum_kernel(const float* __restrict__ pts, long long p_rstride, const float* __restrict__ w, int npts,
                            O* __restrict__ out, long long n) {
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    O s = 0;
    for (int i = 0; i < npts; ++i) s += (O)w[i] * (O)pts[(long long)i * p_rstride + k];
    out[k] = s;
  }
}

// Reproducible weighted sum (RFA's Weiszfeld average, FoolsGold's weighted gradient): every
// product q = w_i * p_ik * 2^E is exact in fp64 (two fp32 factors, a power-of-two scale) and is
// quantised ON ITS OWN onto a fixed two-limb grid, hi = floor(q), lo = floor((q - hi) * 2^53);
// the limbs are summed as int64 — over the rank's clients here, then over ranks by an int64
// all-reduce — which is exact and order-free, so the sum does not depend on which rank holds
// which client (world-1 == world-N bits).  E is chosen by the caller so |q| <= 2^52 / n (no
// overflow of either limb sum for n <= 512).  out: [2][n] int64 (hi sums, lo sums).
__global__ void wsum_fixed_kernel(const float* __restrict__ pts, long long p_rstride, const float* __restrict__ w,
                                  int npts, long long* __restrict__ out, long long n, double scale) {
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    long long hs = 0, ls = 0;
    for (int i = 0; i < npts; ++i) {
      const double q = (double)w[i] * (double)pts[(long long)i * p_rstride + k] * scale;
      const double hi = floor(q);
      hs += (long long)hi;
      ls += (long long)floor((q - hi) * 0x1p53);
    }
    out[k] = hs;
    out[n + k] = ls;
  }
}

// slab[z][i][j] = sum over k-chunk z of F[i][k] F[j][k]; one wave per 16x16 tile (f32 MFMA),
// summed over z in order by gram_finalize (no atomics)
__global__ __launch_bounds__(64) void gram_kernel(const float* __restrict__ F, long long f_rstride, int n, int d,
                                                  int kchunk, float* __restrict__ slab) {
  const int ti = blockIdx.x, tj = blockIdx.y;
  const int k0 = blockIdx.z * kchunk, k1 = min(d, k0 + kchunk);
  const int lane = threadIdx.x;
  const int r = lane & 15, kk = lane >> 4;
  const int ia = ti * 16 + r, ib = tj * 16 + r;
  const float* fa = F + (long long)ia * f_rstride;
  const float* fb = F + (long long)ib * f_rstride;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = k0; k < k1; k += 4) {
    const int kx = k + kk;
    const float a = (ia < n && kx < k1) ? fa[kx] : 0.f;
    const float b = (ib < n && kx < k1) ? fb[kx] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  const int j = tj * 16 + (lane & 15);
  float* out = slab + (long long)blockIdx.z * n * n;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = ti * 16 + (lane >> 4) * 4 + q;
    if (i < n && j < n) out[(long long)i * n + j] = acc[q];
  }
}

__global__ void gram_finalize(const float* __restrict__ slab, int nz, int nn, double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nn) return;
  double s = 0.0;
  for (int z = 0; z < nz; ++z) s += (double)slab[(long long)z * nn + e];
  out[e] = s;
}

// part[g][blk] = this block's sum of (w_g - base_g)^2 over the parameter region (replicas in
// their poison phase only); distgrad_kernel sums a replica's parts in block order
__global__ __launch_bounds__(256) void distnorm_kernel(const float* __restrict__ w, long long ws,
                                                       const float* __restrict__ base, long long bs,
                                                       const int* __restrict__ trig, const int* __restrict__ active,
                                                       long long n, float* __restrict__ part) {
  __shared__ float red[4];
  const int g = blockIdx.y;
  if (trig[g] < 0 || active[g] == 0) return;
  const float* wg = w + (long long)g * ws;
  const float* bg = base + (long long)g * bs;
  float s = 0.f;
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
    const float d = wg[k] - bg[k];
    s = fmaf(d, d, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(long long)g * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// d/dw [a*CE + (1-a)*||w-b||] = a*g + (1-a)(w-b)/||w-b||  (0 at w == b, torch's norm subgradient);
// block (0, g) also publishes ||w-b||^2 into nrm2[g]
__global__ void distgrad_kernel(const float* __restrict__ w, long long ws, const float* __restrict__ base,
                                long long bs, float* __restrict__ grads, long long n, const int* __restrict__ trig,
                                const int* __restrict__ active, float alpha, const float* __restrict__ part,
                                float* __restrict__ nrm2) {
  const int g = blockIdx.y;
  if (trig[g] < 0 || active[g] == 0) return;
  float n2 = 0.f;
  for (int b = 0; b < (int)gridDim.x; ++b) n2 += part[(long long)g * gridDim.x + b];
  if (blockIdx.x == 0 && threadIdx.x == 0) nrm2[g] = n2;
  const float nr = sqrtf(n2);
  const float c = nr > 0.f ? (1.f - alpha) / nr : 0.f;
  const float* wg = w + (long long)g * ws;
  const float* bg = base + (long long)g * bs;
  float* gg = grads + (long long)g * n;
  for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
    gg[k] = fmaf(alpha, gg[k], c * (wg[k] - bg[k]));
}

// How the blocks of one replica row walk its n entries: entries [h, h + 4 nv) as nv float4 (both
// row pointers 16-byte aligned from entry h on), the other h + (n - h - 4 nv) <= 6 entries one
// by one.  Rows whose two pointers are misaligned differently have nv = 0 (all entries one by
// one).  Nothing at or past n is touched.
struct BallSpan {
  long long h, nv;
  __device__ BallSpan(const float* wg, const float* bg, long long n) {
    const unsigned mw = ((unsigned)(uintptr_t)wg & 15u) >> 2, mb = ((unsigned)(uintptr_t)bg & 15u) >> 2;
    if (mw != mb) {
      h = 0;
      nv = 0;
    } else {
      h = std::min<long long>((4 - mw) & 3, n);
      nv = (n - h) >> 2;
    }
  }
  // the k-th entry outside the float4 body, k in [0, n - 4 nv)
  __device__ long long edge(long long k) const { return k < h ? k : k + 4 * nv; }
};

// PGD attacker, launch 1: part[g][blk] = this block's fp64 sum of (w_g - base_g)^2 over the first
// n entries (replicas training with a trigger only).  The difference of two floats is exact in
// fp64; one fma per entry, then a wave and a block reduction in a fixed order
__global__ __launch_bounds__(256) void ballnorm_kernel(const float* __restrict__ w, long long ws,
                                                       const float* __restrict__ base, long long bs,
                                                       const int* __restrict__ trig, const int* __restrict__ active,
                                                       long long n, double* __restrict__ part) {
  __shared__ double red[4];
  const int g = blockIdx.y;
  if (trig[g] < 0 || active[g] == 0) return;
  const float* wg = w + (long long)g * ws;
  const float* bg = base + (long long)g * bs;
  const BallSpan sp(wg, bg, n);
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x, dt = (long long)gridDim.x * blockDim.x;
  double s = 0.0;
  for (long long i = t0; i < sp.nv; i += dt) {
    const float4 a = *reinterpret_cast<const float4*>(wg + sp.h + 4 * i);
    const float4 b = *reinterpret_cast<const float4*>(bg + sp.h + 4 * i);
    const double d0 = (double)a.x - (double)b.x, d1 = (double)a.y - (double)b.y;
    const double d2 = (double)a.z - (double)b.z, d3 = (double)a.w - (double)b.w;
    s = fma(d0, d0, s);
    s = fma(d1, d1, s);
    s = fma(d2, d2, s);
    s = fma(d3, d3, s);
  }
  for (long long k = t0; k < n - 4 * sp.nv; k += dt) {
    const long long e = sp.edge(k);
    const double d = (double)wg[e] - (double)bg[e];
    s = fma(d, d, s);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[(long long)g * gridDim.x + blockIdx.x] = s;
}

__device__ __forceinline__ float ball_pull(float w, float b, double s) {
  return (float)__dadd_rn((double)b, __dmul_rn(s, (double)w - (double)b));
}

// launch 2: norm = sqrt(sum of the replica's parts, in block order); a finite norm > radius pulls
// w_g onto the sphere, w = base + (radius / norm)(w - base) in fp64 rounded once, anything else
// writes nothing to w.  Thread (0, g) publishes the norm and counts the projection
__global__ __launch_bounds__(256) void ballproj_kernel(float* __restrict__ w, long long ws,
                                                       const float* __restrict__ base, long long bs,
                                                       const int* __restrict__ trig, const int* __restrict__ active,
                                                       long long n, double radius, const double* __restrict__ part,
                                                       double* __restrict__ norm_out, int* __restrict__ count) {
  const int g = blockIdx.y;
  if (trig[g] < 0 || active[g] == 0) return;
  double n2 = 0.0;
  for (int b = 0; b < (int)gridDim.x; ++b) n2 += part[(long long)g * gridDim.x + b];
  const double nr = sqrt(n2);
  const bool pull = isfinite(nr) && nr > radius;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    norm_out[g] = nr;
    if (pull) count[g] = count[g] + 1;
  }
  if (!pull) return;
  const double s = radius / nr;
  float* wg = w + (long long)g * ws;
  const float* bg = base + (long long)g * bs;
  const BallSpan sp(wg, bg, n);
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x, dt = (long long)gridDim.x * blockDim.x;
  for (long long i = t0; i < sp.nv; i += dt) {
    float4 a = *reinterpret_cast<const float4*>(wg + sp.h + 4 * i);
    const float4 b = *reinterpret_cast<const float4*>(bg + sp.h + 4 * i);
    a.x = ball_pull(a.x, b.x, s);
    a.y = ball_pull(a.y, b.y, s);
    a.z = ball_pull(a.z, b.z, s);
    a.w = ball_pull(a.w, b.w, s);
    *reinterpret_cast<float4*>(wg + sp.h + 4 * i) = a;
  }
  for (long long k = t0; k < n - 4 * sp.nv; k += dt) {
    const long long e = sp.edge(k);
    wg[e] = ball_pull(wg[e], bg[e], s);
  }
}

// Neurotoxin attacker's per-step restore (replicas training with a trigger only): every one of the
// first n entries whose bit in the keep mask is 0 goes back to its phase-start value, w = base, a
// copy; a kept entry is neither read nor written.  mask: bit j % 64 of word j / 64 belongs to entry
// j (nmask.hip).  A lane reads the four bits of its float4 first: all kept costs nothing more, all
// dropped is one 16-byte load and store, a mix copies entry by entry.  w is never read.  Thread
// (0, g) counts the step
__global__ __launch_bounds__(256) void maskrestore_kernel(float* __restrict__ w, long long ws,
                                                          const float* __restrict__ base, long long bs,
                                                          const int* __restrict__ trig, const int* __restrict__ active,
                                                          long long n, const unsigned long long* __restrict__ mask,
                                                          int* __restrict__ count) {
  const int g = blockIdx.y;
  if (trig[g] < 0 || active[g] == 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) count[g] = count[g] + 1;
  float* wg = w + (long long)g * ws;
  const float* bg = base + (long long)g * bs;
  const BallSpan sp(wg, bg, n);
  const long long t0 = blockIdx.x * (long long)blockDim.x + threadIdx.x, dt = (long long)gridDim.x * blockDim.x;
  for (long long i = t0; i < sp.nv; i += dt) {
    const long long j = sp.h + 4 * i;       // entries j .. j + 3 < n: the word of j + 3 exists
    const int sh = (int)(j & 63);
    unsigned long long m = mask[j >> 6] >> sh;
    if (sh > 60) m |= mask[(j >> 6) + 1] << (64 - sh);
    const unsigned keep = (unsigned)m & 15u;
    if (keep == 15u) continue;
    if (keep == 0u) {
      *reinterpret_cast<float4*>(wg + j) = *reinterpret_cast<const float4*>(bg + j);
      continue;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (!((keep >> c) & 1u)) wg[j + c] = bg[j + c];
  }
  for (long long k = t0; k < n - 4 * sp.nv; k += dt) {
    const long long e = sp.edge(k);
    if (!((mask[e >> 6] >> (e & 63)) & 1ull)) wg[e] = bg[e];
  }
}

}  // namespace

// PGD attacker's per-step projection of the replicas training with a trigger onto the L2 ball of
// `radius` around base, over the first n entries of each row.  part: [G][256] fp64 workspace (no
// initialisation needed); norm_out [G] fp64, count [G] int32 (+1 per projection)
DBA_EXPORT int dba_project_to_ball(float* w, long long ws, const float* base, long long bs, long long n, int G,
                                   const int* trig, const int* active, double radius, double* norm_out, int* count,
                                   double* part, void* stream) {
  const int bx = (int)std::max(1LL, std::min(256LL, (n + 2047) / 2048));
  hipLaunchKernelGGL(ballnorm_kernel, dim3(bx, G), dim3(256), 0, (hipStream_t)stream, w, ws, base, bs, trig, active, n,
                     part);
  hipLaunchKernelGGL(ballproj_kernel, dim3(bx, G), dim3(256), 0, (hipStream_t)stream, w, ws, base, bs, trig, active, n,
                     radius, part, norm_out, count);
  DBA_LAUNCH_CHECK();
}

// Neurotoxin attacker's per-step restore of the replicas training with a trigger: over the first n
// entries of each row, w = base where the keep mask's bit is 0.  mask [ceil(n / 64)] int64 words
// (dba_neurotoxin_mask's); count [G] int32 (+1 per gated-in replica)
DBA_EXPORT int dba_mask_restore(float* w, long long ws, const float* base, long long bs, long long n, int G,
                                const int* trig, const int* active, const long long* mask, int* count,
                                void* stream) {
  const int bx = (int)std::max(1LL, std::min(256LL, (n + 2047) / 2048));
  hipLaunchKernelGGL(maskrestore_kernel, dim3(bx, G), dim3(256), 0, (hipStream_t)stream, w, ws, base, bs, trig, active,
                     n, (const unsigned long long*)mask, count);
  DBA_LAUNCH_CHECK();
}

// part: [G][256] fp32 workspace (no initialisation needed)
DBA_EXPORT int dba_dist_loss_grad(const float* w, long long ws, const float* base, long long bs, float* grads,
                                  long long n, int G, const int* trig, const int* active, float alpha, float* nrm2,
                                  float* part, void* stream) {
  const int bx = (int)std::max(1LL, std::min(256LL, (n + 2047) / 2048));
  hipLaunchKernelGGL(distnorm_kernel, dim3(bx, G), dim3(256), 0, (hipStream_t)stream, w, ws, base, bs, trig, active,
                     n, part);
  hipLaunchKernelGGL(distgrad_kernel, dim3(bx, G), dim3(256), 0, (hipStream_t)stream, w, ws, base, bs, grads, n, trig,
                     active, alpha, part, nrm2);
  DBA_LAUNCH_CHECK();
}

DBA_EXPORT int dba_scale_from_base(const float* w, const float* base, float gamma, float* out, long long n,
                                   void* stream) {
  hipLaunchKernelGGL(scale_kernel, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, w, base, gamma, out, n);
  DBA_LAUNCH_CHECK();
}

// upd fp64 (upd_f64) or fp32
DBA_EXPORT int dba_add_noise_scaled(float* dst, const void* upd, long long n, float coef, float sigma,
                                    unsigned seed, int noise, int upd_f64, void* stream) {
  if (upd_f64)
    hipLaunchKernelGGL(noise_add_kernel<double>, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, dst,
                       (const double*)upd, n, coef, sigma, seed, noise);
  else
    hipLaunchKernelGGL(noise_add_kernel<float>, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, dst,
                       (const float*)upd, n, coef, sigma, seed, noise);
  DBA_LAUNCH_CHECK();
}

DBA_EXPORT int dba_delta_sum(const float* rows, long long rstride, int nrows, const float* base, long long n,
                             double* out, void* stream) {
  hipLaunchKernelGGL(delta_sum_kernel, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, rows, rstride, nrows, base,
                     n, out);
  DBA_LAUNCH_CHECK();
}

DBA_EXPORT int dba_sqdist_blocks(long long n) { return (int)std::max(1LL, std::min(512LL, (n + 1023) / 1024)); }

// part: [npts][dba_sqdist_blocks(n)] fp64 workspace
DBA_EXPORT int dba_sq_dists(const float* pts, long long p_rstride, const float* m, int npts, long long n, double* out,
                            double* part, void* stream) {
  const int bx = dba_sqdist_blocks(n);
  hipLaunchKernelGGL(sqdist_kernel, dim3(bx, npts), dim3(256), 0, (hipStream_t)stream, pts, p_rstride, m, n, part);
  hipLaunchKernelGGL(sqdist_finalize, dim3((npts + 63) / 64), dim3(64), 0, (hipStream_t)stream, part, bx, npts, out);
  DBA_LAUNCH_CHECK();
}

// out fp64 (out_f64) or fp32
DBA_EXPORT int dba_weighted_sum(const float* pts, long long p_rstride, const float* w, int npts, void* out,
                                long long n, int out_f64, void* stream) {
  if (out_f64)
    hipLaunchKernelGGL(wsum_kernel<double>, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, pts, p_rstride, w, npts,
                       (double*)out, n);
  else
    hipLaunchKernelGGL(wsum_kernel<float>, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, pts, p_rstride, w, npts,
                       (float*)out, n);
  DBA_LAUNCH_CHECK();
}

// out [2][n] int64: the fixed-point limb sums of sum_i w[i] * pts[i] (wsum_fixed_kernel); scale = 2^E
DBA_EXPORT int dba_weighted_sum_fixed(const float* pts, long long p_rstride, const float* w, int npts, long long* out,
                                      long long n, double scale, void* stream) {
  hipLaunchKernelGGL(wsum_fixed_kernel, dim3(egrid(n)), dim3(256), 0, (hipStream_t)stream, pts, p_rstride, w, npts, out,
                     n, scale);
  DBA_LAUNCH_CHECK();
}

DBA_EXPORT int dba_gram_chunks(int d) { return std::max(1, (d + 1023) / 1024); }

// slab: [dba_gram_chunks(d)][n][n] fp32 workspace; out [n][n] fp64
DBA_EXPORT int dba_gram(const float* F, long long f_rstride, int n, int d, double* out, float* slab, void* stream) {
  const int t = (n + 15) / 16;
  const int kchunk = 1024;
  const int nz = dba_gram_chunks(d);
  dim3 grid(t, t, nz);
  hipLaunchKernelGGL(gram_kernel, grid, dim3(64), 0, (hipStream_t)stream, F, f_rstride, n, d, kchunk, slab);
  hipLaunchKernelGGL(gram_finalize, dim3((n * n + 255) / 256), dim3(256), 0, (hipStream_t)stream, slab, nz, n * n, out);
  DBA_LAUNCH_CHECK();
}

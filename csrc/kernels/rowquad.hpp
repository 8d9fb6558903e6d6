// Row helpers shared by the aggregation kernels over strided client rows (clip.hip, krum.hip,
// coordrank.hpp with its rules trim.hip and bulyan.hip, rlr.hip): a lane takes four consecutive 4-byte elements of a row per step, as one
// 16-byte access where the row start is 16-byte aligned and as four scalar ones otherwise
// (finals[:, :n_upd] is a strided view whose rows may start anywhere); the last, partial step
// touches only the row's remaining elements.  Which elements a thread takes never depends on the
// alignment, so the bits are the same from an aligned copy and a misaligned view.  And the block
// sum of their (and flat.hip's) fixed-order cross-block reductions.
#pragma once
#include "common.hpp"

constexpr int kQuad = 4;           // elements per lane per step

__device__ __forceinline__ bool aligned16_dev(const void* p) { return ((uintptr_t)p & 15) == 0; }

// T p[0 .. 4) (FULL) or p[0 .. cnt), zero-filled; ``vec``: p is 16-byte aligned.  A quad's offset
// from its row start is a multiple of 16 bytes, so ``vec`` is the row start's alignment
template <bool FULL, typename T>
__device__ __forceinline__ void ld_quad(const T* __restrict__ p, bool vec, int cnt, T (&v)[kQuad]) {
  static_assert(sizeof(T) == 4, "four 4-byte elements per 16-byte load");
  if constexpr (FULL) {
    if (vec) {
      const uint4 x = *(const uint4*)p;
      __builtin_memcpy(v, &x, sizeof(x));
    } else {
      v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kQuad; ++j) v[j] = j < cnt ? p[j] : T(0);
  }
}

// the same for floats through a float4: krum.hip and clip.hip were written with this form and
// rlr.hip with the one above, and each compiles to other device code with the other's
template <bool FULL>
__device__ __forceinline__ void ld_quad_f4(const float* __restrict__ p, bool vec, int cnt, float (&v)[kQuad]) {
  if constexpr (FULL) {
    if (vec) {
      const float4 x = *(const float4*)p;
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kQuad; ++j) v[j] = j < cnt ? p[j] : 0.f;
  }
}

// p[0 .. 4) (FULL) or p[0 .. cnt) = v
template <bool FULL>
__device__ __forceinline__ void st_quad(float* __restrict__ p, bool vec, int cnt, const float (&v)[kQuad]) {
  if constexpr (FULL) {
    if (vec) {
      *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < kQuad; ++j)
    if (FULL || j < cnt) p[j] = v[j];
}
template <bool FULL>
__device__ __forceinline__ void st_quad(int* __restrict__ p, bool vec, int cnt, const int (&v)[kQuad]) {
  if constexpr (FULL) {
    if (vec) {
      *(int4*)p = make_int4(v[0], v[1], v[2], v[3]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < kQuad; ++j)
    if (FULL || j < cnt) p[j] = v[j];
}
template <bool FULL>
__device__ __forceinline__ void st_quad(double* __restrict__ p, bool vec, int cnt, const double (&v)[kQuad]) {
  if constexpr (FULL) {
    if (vec) {
      ((double2*)p)[0] = make_double2(v[0], v[1]);
      ((double2*)p)[1] = make_double2(v[2], v[3]);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < kQuad; ++j)
    if (FULL || j < cnt) p[j] = v[j];
}

// a 256-thread block's sum in one fixed order: lanes in a butterfly, then the four waves in order
// (every thread calls it, every thread gets the sum).  With per-block partials and a finalize
// launch that adds them in a fixed order, a cross-block sum needs no atomics and is bitwise run to run
template <typename T>
__device__ __forceinline__ T block_sum(T v, T (&red)[4]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

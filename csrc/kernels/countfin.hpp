// The finalize launch of the fixed-order integer counts shared by rlr.hip (agree / dissent / flipped)
// and topk.hip (kept): a pass leaves one int64 partial per block (rowquad.hpp block_sum), this
// launch adds them in one fixed order.  No atomics, so a count is bitwise run to run.
#pragma once
#include "rowquad.hpp"

constexpr int kFinalBatch = 4;     // partials in flight per thread in the finalize launch

// one block per output slot: thread t takes the partials of blocks t, t + 256, ... (kFinalBatch
// loads in flight: a chain of dependent L2 round trips over thousands of partials would take
// longer than the pass over the rows), then the block combines in the fixed order of block_sum
static __global__ __launch_bounds__(256) void count_finalize(const long long* __restrict__ part, int nblk,
                                                            long long* __restrict__ counts) {
  __shared__ long long red[4];
  const long long* p = part + (long long)blockIdx.x * nblk;
  long long s = 0;
  int b = threadIdx.x;
  for (; b + (kFinalBatch - 1) * 256 < nblk; b += kFinalBatch * 256) {
    long long v[kFinalBatch];
#pragma unroll
    for (int u = 0; u < kFinalBatch; ++u) v[u] = p[b + u * 256];
#pragma unroll
    for (int u = 0; u < kFinalBatch; ++u) s += v[u];
  }
  for (; b < nblk; b += 256) s += p[b];
  s = block_sum<long long>(s, red);
  if (threadIdx.x == 0) counts[blockIdx.x] = s;
}

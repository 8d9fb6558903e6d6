// Host check of the compile-time sorting networks of csrc/kernels/sortnet.hpp, the ones trim.hip
// instantiates: every N <= 16 against the 0-1 principle exhaustively (a comparator network sorts
// every input iff it sorts every 0-1 input), the padded sizes 24 / 32 / 48 / 64 on random 0-1
// inputs, random keys with many ties and sorted / reversed runs, through sortnet_apply itself.
#include "../kernels/sortnet.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>

static int failures = 0;

template <int N>
static bool apply_and_check(const uint32_t (&in)[N]) {
  uint32_t v[N], want[N];
  for (int i = 0; i < N; ++i) v[i] = want[i] = in[i];
  sortnet_apply<N>(v);
  std::sort(want, want + N);
  for (int i = 0; i < N; ++i)
    if (v[i] != want[i]) return false;
  return true;
}

template <int N>
static void check(std::mt19937& rng) {
  constexpr SortNet net = kSortNet<N>;
  bool ok = true;
  for (int c = 0; c < net.cnt; ++c) ok = ok && 0 <= net.lo[c] && net.lo[c] < net.hi[c] && net.hi[c] < N;
  uint32_t x[N];
  if (N <= 16) {
    ok = ok && sortnet_sorts(net, N);
    for (uint32_t m = 0; ok && m < (1u << (N <= 16 ? N : 0)); ++m) {
      for (int i = 0; i < N; ++i) x[i] = (m >> i) & 1u;
      ok = apply_and_check<N>(x);
    }
  }
  for (int t = 0; ok && t < 20000; ++t) {
    const int mode = t % 4;
    for (int i = 0; i < N; ++i) {
      if (mode == 0) x[i] = rng() & 1u;                         // 0-1
      else if (mode == 1) x[i] = rng() % 5u;                    // many ties
      else if (mode == 2) x[i] = rng();                         // distinct
      else x[i] = (t & 4) ? (uint32_t)(N - i) : 0xFFFFFFFFu - (rng() % 3u);   // reversed / top-valued ties
    }
    ok = apply_and_check<N>(x);
  }
  std::printf("N = %2d: %3d comparators %s\n", N, net.cnt, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

int main() {
  std::mt19937 rng(12345);
  check<1>(rng); check<2>(rng); check<3>(rng); check<4>(rng); check<5>(rng); check<6>(rng); check<7>(rng);
  check<8>(rng); check<9>(rng); check<10>(rng); check<11>(rng); check<12>(rng); check<13>(rng); check<14>(rng);
  check<15>(rng); check<16>(rng); check<24>(rng); check<32>(rng); check<48>(rng); check<64>(rng);
  if (kSortNet<10>.cnt != 29 || kSortNet<16>.cnt != 63 || kSortNet<64>.cnt != 543) {
    std::printf("unexpected comparator counts\n");
    ++failures;
  }
  std::printf(failures ? "sortnet check FAILED\n" : "sortnet check OK\n");
  return failures ? 1 : 0;
}

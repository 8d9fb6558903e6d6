// Compile-time sorting networks for register-resident keys (coordrank.hpp: trim.hip, bulyan.hip).
//   * kSortNet<N> is the comparator list of an N-input network: Batcher's odd-even merge sort on
//     the next power of two P >= N with every comparator that touches an input >= N dropped.  The
//     inputs N .. P - 1 would hold top-valued sentinels in the top positions; a comparator whose
//     upper input is one of them cannot move anything, and none has a sentinel as its lower input
//     only, so the pruned list sorts N inputs.  N = 10, a round's client count in every recipe,
//     takes a 29-comparator network instead (Batcher's pruned one has 32).
//   * sortnet_apply<N>(v) runs the list on v[0 .. N) with every index a compile-time constant, so
//     v stays in registers.
// Host and device code may both include this file (the network check of csrc/tests compiles it
// with the host compiler).
#pragma once
#include <utility>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SORTNET_HD __host__ __device__ __forceinline__
#else
#define SORTNET_HD inline
#endif

constexpr int kSortNetMaxInputs = 64;
constexpr int kSortNetMaxCmp = 543;   // Batcher's count at 64 inputs

struct SortNet {
  short lo[kSortNetMaxCmp + 1];
  short hi[kSortNetMaxCmp + 1];
  int cnt;
};

constexpr SortNet sortnet_batcher(int n) {
  SortNet s{};
  int P = 1;
  while (P < n) P *= 2;
  for (int p = 1; p < P; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < P; j += 2 * k)
        for (int i = 0; i < k && i + j + k < P; ++i) {
          const int a = i + j, b = i + j + k;
          if (a / (2 * p) == b / (2 * p) && b < n) {
            s.lo[s.cnt] = (short)a;
            s.hi[s.cnt] = (short)b;
            ++s.cnt;
          }
        }
  return s;
}

// 10 inputs in 29 comparators, 8 layers
constexpr SortNet sortnet_ten() {
  constexpr int c[29][2] = {{0, 8}, {1, 9}, {2, 7}, {3, 5}, {4, 6}, {0, 2}, {1, 4}, {5, 8}, {7, 9}, {0, 3},
                            {2, 4}, {5, 7}, {6, 9}, {0, 1}, {3, 6}, {8, 9}, {1, 5}, {2, 3}, {4, 8}, {6, 7},
                            {1, 2}, {3, 5}, {4, 6}, {7, 8}, {2, 3}, {4, 5}, {6, 7}, {3, 4}, {5, 6}};
  SortNet s{};
  for (int i = 0; i < 29; ++i) {
    s.lo[i] = (short)c[i][0];
    s.hi[i] = (short)c[i][1];
  }
  s.cnt = 29;
  return s;
}

// the 0-1 principle: a comparator network sorts every input iff it sorts every 0-1 input
constexpr bool sortnet_sorts(const SortNet& s, int n) {
  for (unsigned m = 0; m < (1u << n); ++m) {
    unsigned x = m;
    for (int c = 0; c < s.cnt; ++c) {
      const unsigned a = (x >> s.lo[c]) & 1u, b = (x >> s.hi[c]) & 1u;
      if (a > b) x ^= (1u << s.lo[c]) | (1u << s.hi[c]);
    }
    // sorted ascending: the ones fill the top positions, so x + its lowest set bit is a power of two
    const unsigned y = x + (x & (~x + 1u));
    if (x != 0 && (y & (y - 1u)) != 0) return false;
  }
  return true;
}

template <int N>
inline constexpr SortNet kSortNet = N == 10 ? sortnet_ten() : sortnet_batcher(N);

static_assert(sortnet_sorts(kSortNet<10>, 10), "the 10-input network sorts");
static_assert(sortnet_sorts(kSortNet<7>, 7) && sortnet_sorts(kSortNet<9>, 9), "pruned Batcher networks sort");
static_assert(sortnet_batcher(16).cnt == 63 && sortnet_batcher(64).cnt == kSortNetMaxCmp, "Batcher's counts");

template <int N, int I, typename T>
SORTNET_HD void sortnet_step(T (&v)[N]) {
  constexpr int a = kSortNet<N>.lo[I], b = kSortNet<N>.hi[I];
  static_assert(a < b && b < N, "comparator inside the inputs");
  const T x = v[a], y = v[b];
  v[a] = x < y ? x : y;
  v[b] = x < y ? y : x;
}

template <int N, typename T, int... I>
SORTNET_HD void sortnet_run(T (&v)[N], std::integer_sequence<int, I...>) {
  // (an initializer list, not a fold expression: no nesting limit at 543 comparators)
  const int done[] = {0, (sortnet_step<N, I>(v), 0)...};
  (void)done;
}

// ascending, in place
template <int N, typename T>
SORTNET_HD void sortnet_apply(T (&v)[N]) {
  static_assert(N >= 1 && N <= kSortNetMaxInputs, "network size");
  sortnet_run<N>(v, std::make_integer_sequence<int, kSortNet<N>.cnt>{});
}

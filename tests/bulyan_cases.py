"""Shared inputs and oracle of the Bulyan second-stage tests (CPU reference op in
test_bulyan_aggregation.py, HIP kernel in test_gpu_bulyan.py): the generator of trim_cases.py and
one numpy fp64 oracle that does literally what the op is defined to do.  Every value is fixed by
IEEE arithmetic in a stated order, so the tests compare bits: there is no tolerance."""
import numpy as np

import trim_cases as tc

# the launch grid of the kernel is trim's (csrc/kernels/coordrank.hpp); the GPU test sizes the wrap
# case from the kernel's own dba_coord_bulyan_blocks
GRID_THREADS, GRID_QUAD = tc.GRID_THREADS, tc.GRID_QUAD

# (t, L, rstride, column offset of the view, f): the smallest input; three rows down to their
# median; f = 0 (the plain sum); the recipe's 8 selected rows of 10 clients at f = 1; even t down to
# beta = 2; an odd stride; every row misaligned over several blocks; 16 rows; a padded network down
# to beta = 1; 33 rows; the kernel's maximum t at its largest and smallest f
RECIPE_CASE = (8, 257, 257, 0, 1)
SMALL_CASES = [(1, 1, 1, 0, 0), (3, 1, 1, 0, 1), (3, 5, 5, 0, 0), RECIPE_CASE, (8, 257, 257, 0, 3),
               (7, 1029, 1031, 2, 2), (9, 4099, 5000, 1, 3), (16, 130, 130, 0, 5), (17, 130, 131, 0, 8),
               (33, 70, 70, 0, 4), (64, 130, 130, 0, 31), (64, 130, 130, 0, 0)]
NINE_ROWS = SMALL_CASES[6]
# every instantiation of the kernel: each exact size at its largest f and at f = 0; either side of
# each padded network size with an odd L (a partial step of the two-per-thread kernels), the sizes
# themselves at their largest f, the next ones at a middle f
SMALL_CASES += [tc.exact_case(t, (t - 1) // 2) for t in range(1, 17)]
SMALL_CASES += [tc.exact_case(t, 0) for t in range(3, 17)]         # (one and two rows: 0 is the largest f)
SMALL_CASES += [(t, 71, 71, 0, (t - 1) // 2 if t % 2 == 0 else t // 4) for t in (24, 25, 32, 33, 48, 49)]
FALLBACK_CASE = (65, 33, 33, 0, 2)        # t > 64: the composition on the device

case_id = tc.case_id
make_case = tc.make_case


def wrap_case(sweep):
    """Three rows, f = 1, three elements past one sweep of the launch grid (``sweep`` elements)."""
    return (3, sweep + 3, sweep + 3, 0, 1)


def window_start(s, f):
    """a [L] of the sorted fp32 values s [t, L]: the number of j in 0 .. 2 f - 1 with
    (double)s[j + beta] - med < med - (double)s[j], med = (double)s[(t - 1) // 2] (NaN compares
    false)."""
    t, L = s.shape
    beta = t - 2 * f
    med = s[(t - 1) // 2].astype(np.float64)
    a = np.zeros(L, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(t - beta):
            a += (s[j + beta].astype(np.float64) - med) < (med - s[j].astype(np.float64))
    return a


def oracle(rows, base, f):
    """(total fp64 [L], kept int64 [t], high int64 [t]) in numpy: ``np.sort`` along the rows (NaN
    last), the window start by the counting rule, a Python loop of fp64 additions over the ranks
    a .. a + beta - 1 in ascending order, then the comparisons of the definition."""
    x = np.asarray(rows, dtype=np.float32)
    b = np.asarray(base, dtype=np.float32).astype(np.float64)
    t, L = x.shape
    if t == 0:
        return np.zeros(L), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    beta = t - 2 * f
    s = np.sort(x, axis=0)
    a = window_start(s, f)
    cols = np.arange(L)
    with np.errstate(invalid="ignore"):
        total = s[a, cols].astype(np.float64) - b
        for r in range(1, beta):
            total = total + (s[a + r, cols].astype(np.float64) - b)
        lo, hi = s[a, cols][None], s[a + beta - 1, cols][None]
        low = x < lo
        high = (x > hi) | (np.isnan(x) & ~np.isnan(hi))
    kept = ~low & ~high
    return total, kept.sum(1).astype(np.int64), high.sum(1).astype(np.int64)


def greedy_window(col, f):
    """The sorted values of one coordinate's window by the procedure the counting rule stands for:
    start at the lower median and grow to beta values, each time towards the neighbour nearer to
    the median (fp64 distances), ties to the lower one."""
    s = np.sort(np.asarray(col, dtype=np.float32))
    t = s.size
    beta, m = t - 2 * f, (t - 1) // 2
    med = np.float64(s[m])
    lo = hi = m
    while hi - lo + 1 < beta:
        if lo == 0:
            hi += 1
        elif hi == t - 1:
            lo -= 1
        elif np.float64(s[hi + 1]) - med < med - np.float64(s[lo - 1]):
            hi += 1
        else:
            lo -= 1
    return s[lo:hi + 1]


def check(out, rows, base, f, tag=""):
    """The op's (total, kept, high) against the oracle, as trim_cases.check compares them."""
    tc.check(out, rows, base, f, tag, oracle)

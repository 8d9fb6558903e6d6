"""Shared inputs, oracle and bound of the Multi-Krum pairwise-distance tests (CPU reference op in
test_krum_aggregation.py, HIP kernel in test_gpu_krum.py): one generator, one numpy fp64 oracle,
one tolerance."""
import numpy as np
import torch

# the launch grid of csrc/kernels/krum.hip: at most 512 blocks x 256 threads x 4 floats per step,
# so one sweep of the grid covers 524288 elements and a longer row wraps the grid-stride loop
GRID_BLOCKS_MAX, GRID_THREADS, GRID_QUAD = 512, 256, 4
SWEEP = GRID_BLOCKS_MAX * GRID_THREADS * GRID_QUAD

# (n, L, rstride, column offset of the view): the smallest input; a padded stride; an odd stride
# (alternate rows misaligned); every row misaligned over several blocks; one row past 8 over many
# blocks; three tiles of 8 (the last of one row); the kernel's maximum n.  The kernel takes up to
# 11 rows as one triangular tile and cuts more into tiles of 8, so two more: the largest lone
# tile; and 12 rows, the fewest that are cut (8 + 4), misaligned over several blocks
SMALL_CASES = [(2, 1, 1, 0), (3, 255, 300, 0), (10, 257, 257, 0), (5, 4099, 5000, 1), (9, 70001, 70004, 0),
               (17, 1031, 1040, 3), (64, 130, 130, 0), (11, 1029, 1031, 2), (12, 4099, 5000, 1)]
NINE_ROWS, TWELVE_ROWS, MISALIGNED = SMALL_CASES[4], SMALL_CASES[8], SMALL_CASES[3]
WRAP_CASE = (2, SWEEP + 3, SWEEP + 3, 0)
CASES = SMALL_CASES + [WRAP_CASE]
FALLBACK_CASE = (65, 33, 33, 0)          # n > 64: the composition on the device


def case_id(c):
    return "x".join(map(str, c))


def make_case(n, L, rstride, off, seed=0):
    """The [n, L] view big[:, off:off + L] of a [n, rstride] fp32 buffer: client states around a
    common model with deltas whose magnitudes span 1e-8 .. 1e2, both signs, exact zeros (half of
    the model is exactly zero, so the small deltas survive the fp32 rows), and the last row a
    copy of the first (n >= 3; the two rows of n = 2 stay distinct)."""
    g = torch.Generator().manual_seed(seed + 1000 * n + L)
    base = torch.randn(L, generator=g)
    base[torch.rand(L, generator=g) < 0.5] = 0.0
    mag = 10.0 ** (torch.rand(n, L, generator=g, dtype=torch.float64) * 10.0 - 8.0)
    sign = torch.where(torch.rand(n, L, generator=g) < 0.5, -1.0, 1.0).double()
    delta = mag * sign
    delta[torch.rand(n, L, generator=g) < 0.1] = 0.0
    big = torch.zeros(n, rstride)
    big[:, off:off + L] = (base.double()[None] + delta).float()
    if n >= 3:
        big[n - 1] = big[0]
    return big[:, off:off + L]


def twins(n):
    """The pair of identical rows of :func:`make_case`, or None."""
    return (0, n - 1) if n >= 3 else None


_ORACLE = {}


def oracle(rows):
    """numpy fp64 [n, n]: sum_k (x_i[k] - x_j[k])^2 pair by pair (no [n, n, L] temporary); computed
    once per input (the input is kept alive with the result)."""
    key = (rows.data_ptr(), tuple(rows.shape))
    if key not in _ORACLE:
        x = rows.numpy().astype(np.float64)
        n = x.shape[0]
        D = np.zeros((n, n))
        for i in range(n):
            for j in range(i + 1, n):
                d = x[i] - x[j]
                D[i, j] = D[j, i] = np.dot(d, d)
        _ORACLE[key] = (D, rows)
    return _ORACLE[key][0]


def check(D, rows, tag=""):
    """fp64 [n, n], exactly zero diagonal, bitwise symmetric, identical rows exactly 0, and
    |D - oracle| <= (L + 2) 2^-52 oracle elementwise: each side makes one rounding for the square
    (the fp64 difference of two fp32 values is exact, counted all the same) and at most L - 1
    roundings of 2^-53 in a sum of non-negative terms, in any order; the factor 2 covers the
    kernel's side and the oracle's."""
    n, L = rows.shape
    assert D.dtype == torch.float64 and tuple(D.shape) == (n, n)
    D = D.cpu()
    assert torch.equal(torch.diagonal(D), torch.zeros(n, dtype=torch.float64))
    assert torch.equal(D, D.t())
    tw = twins(n)
    if tw is not None:
        assert float(D[tw[0], tw[1]]) == 0.0
    o = oracle(rows)
    err = np.abs(D.numpy() - o)
    bound = (L + 2) * 2.0 ** -52
    rel = float(np.max(err / np.maximum(o, 1e-300))) if n else 0.0
    print(f"  {tag}pairwise max rel err {rel:.3e} (bound {bound:.3e})")
    assert np.all(err <= bound * o), (err, o)

"""Shared inputs and oracle of the coordinate-wise trimmed-mean tests (CPU reference op in
test_trim_aggregation.py, HIP kernel in test_gpu_trim.py): one generator and one numpy fp64 oracle
that does literally what the op is defined to do.  Every value is fixed by IEEE arithmetic in a
stated order, so the tests compare bits: there is no tolerance.  And what the GPU tests of the
coordinate-rank kernels (test_gpu_trim.py, test_gpu_bulyan.py) share: a case's rows made once, its
strided view on the device, the comparison of two results' bits."""
import functools

import numpy as np
import torch

# the launch grid of csrc/kernels/coordrank.hpp: at most 512 blocks x 256 threads x 4 floats per
# step; the GPU test sizes the wrap case from the kernel's own dba_coord_trim_blocks
GRID_THREADS, GRID_QUAD = 256, 4


def exact_case(n, arg):
    """n <= 16 rows, the kernel instantiated for exactly n: two full quads and a partial step of one,
    every row misaligned."""
    return (n, 9, 12, 1, arg)


# (n, L, rstride, column offset of the view, k): the smallest input; the median of two; an odd
# stride at k = 1, 2 and 4 (the even-n median); the odd-n median with every row misaligned over
# several blocks; 11 rows; either side of a padded network size; 33 rows; the kernel's maximum n
SMALL_CASES = [(3, 1, 1, 0, 1), (2, 5, 5, 0, 0), (10, 257, 257, 0, 1), (10, 257, 257, 0, 2), (10, 257, 257, 0, 4),
               (9, 4099, 5000, 1, 4), (11, 1029, 1031, 2, 3), (16, 130, 130, 0, 5), (17, 130, 131, 0, 8),
               (33, 70, 70, 0, 1), (64, 130, 130, 0, 31)]
NINE_ROWS = SMALL_CASES[5]
# every instantiation of the kernel: each exact size at its largest k; either side of each padded
# network size with an odd L (a partial step of the two-per-thread kernels), the sizes themselves at
# their largest k, the next ones at a middle k
SMALL_CASES += [exact_case(n, (n - 1) // 2) for n in range(1, 17)]
SMALL_CASES += [(n, 71, 71, 0, (n - 1) // 2 if n % 2 == 0 else n // 4) for n in (24, 25, 32, 33, 48, 49)]
FALLBACK_CASE = (65, 33, 33, 0, 2)        # n > 64: the composition on the device


def wrap_case(sweep):
    """Three rows, three elements past one sweep of the launch grid (``sweep`` elements)."""
    return (3, sweep + 3, sweep + 3, 0, 1)


def case_id(c):
    return "x".join(map(str, c))


def make_case(n, L, rstride, off, k=None, seed=0):
    """(view, base): the [n, L] view big[:, off:off + L] of a [n, rstride] fp32 buffer and the
    common model ``base`` [L] the clients' states lie around.  Half of the model is exactly zero
    (so the small deltas survive the fp32 rows), the deltas' magnitudes span 1e-8 .. 1e2 with
    both signs, 10 % of them are exactly zero (many cross-client ties at a coordinate), and a few
    entries are -0.0."""
    g = torch.Generator().manual_seed(seed + 1000 * n + L)
    base = torch.randn(L, generator=g)
    base[torch.rand(L, generator=g) < 0.5] = 0.0
    mag = 10.0 ** (torch.rand(n, L, generator=g, dtype=torch.float64) * 10.0 - 8.0)
    sign = torch.where(torch.rand(n, L, generator=g) < 0.5, -1.0, 1.0).double()
    delta = mag * sign
    delta[torch.rand(n, L, generator=g) < 0.1] = 0.0
    rows = (base.double()[None] + delta).float()
    neg0 = (torch.rand(n, L, generator=g) < 0.02) & (rows == 0)
    rows[neg0] = -0.0
    big = torch.zeros(n, rstride)
    big[:, off:off + L] = rows
    return big[:, off:off + L], base


def oracle(rows, base, k):
    """(total fp64 [L], kept int64 [n], high int64 [n]) in numpy: ``np.sort`` along the clients
    (NaN last), a Python loop of fp64 additions over the ranks k .. n - 1 - k in ascending order,
    then the comparisons of the definition (NaN compares false)."""
    x = np.asarray(rows, dtype=np.float32)
    b = np.asarray(base, dtype=np.float32).astype(np.float64)
    n, L = x.shape
    if n == 0:
        return np.zeros(L), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    s = np.sort(x, axis=0)
    with np.errstate(invalid="ignore"):
        total = s[k].astype(np.float64) - b
        for r in range(k + 1, n - k):
            total = total + (s[r].astype(np.float64) - b)
        lo, hi = s[k][None], s[n - 1 - k][None]
        low = x < lo
        high = (x > hi) | (np.isnan(x) & ~np.isnan(hi))
    kept = ~low & ~high
    return total, kept.sum(1).astype(np.int64), high.sum(1).astype(np.int64)


def check(out, rows, base, k, tag="", oracle=oracle):
    """The op's (total, kept, high) against the oracle (another rule's: ``oracle``): dtypes and
    shapes, ``total`` equal (``==``, which ignores the sign of a zero) wherever the oracle is not
    NaN and NaN exactly where it is, the counts equal integers."""
    total, kept, high = out
    n, L = rows.shape
    assert total.dtype == torch.float64 and tuple(total.shape) == (L,)
    assert kept.dtype == torch.int64 and tuple(kept.shape) == (n,)
    assert high.dtype == torch.int64 and tuple(high.shape) == (n,)
    want_t, want_k, want_h = oracle(rows.numpy(), base.numpy(), k)
    total, kept, high = total.cpu(), kept.cpu(), high.cpu()
    want = torch.from_numpy(want_t)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(total), nan), f"{tag}NaN positions differ"
    bad = (total != want) & ~nan
    assert torch.equal(total[~nan], want[~nan]), (tag, int(bad.sum()), total[bad][:4], want[bad][:4])
    assert kept.tolist() == want_k.tolist(), (tag, kept.tolist(), want_k.tolist())
    assert high.tolist() == want_h.tolist(), (tag, high.tolist(), want_h.tolist())


@functools.lru_cache(maxsize=None)
def case_rows(case):
    """(rows, base) of a case on the host, made once."""
    return make_case(*case)


def on_device(case, dev):
    """The same strided view on the device (big[:, off:off + L] of a [n, rstride] buffer) and the base."""
    n, L, rstride, off, _ = case
    rows, base = case_rows(case)
    big = torch.zeros(n, rstride, device=dev)
    big[:, off:off + L] = rows.to(dev)
    view = big[:, off:off + L]
    assert view.stride(0) == rstride or n == 1
    return view, base.to(dev)


def same_bits(a, b):
    """Two (total, kept, high) results with the same bits."""
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(a, b))

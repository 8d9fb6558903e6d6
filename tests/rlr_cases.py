"""Shared inputs and oracle of the robust-learning-rate tests (CPU reference ops in
test_rlr_aggregation.py, HIP kernels in test_gpu_rlr.py): one generator and one numpy oracle that
does literally what the definition says — fp32 comparisons for the signs, a Python loop of fp64
additions in row order, integer counts.  Every value is an integer or fixed by IEEE arithmetic in
a stated order, so the tests compare bits: there is no tolerance."""
import numpy as np
import torch

import trim_cases as tc

# the launch grids of csrc/kernels/rlr.hip: the sum + votes and the apply pass take at most 4096
# blocks x 256 threads x 4 coordinates per step, the agreement pass at most 1024 blocks x 256
# threads x a batch of 4 steps x 4 coordinates: the same sweep.  The GPU test sizes the wrap case
# from the kernels' own dba_vote_agreement_blocks / dba_rlr_apply_blocks
SUM_BLOCKS, AGREE_BLOCKS, AGREE_BATCH, GRID_THREADS, GRID_QUAD = 4096, 1024, 4, 256, 4
SWEEP = SUM_BLOCKS * GRID_THREADS * GRID_QUAD
assert SWEEP == AGREE_BLOCKS * GRID_THREADS * AGREE_BATCH * GRID_QUAD

# (n, L, rstride, column offset of the view): the smallest input; a few odd coordinates; an odd
# stride (rows misaligned); several blocks with every row misaligned; a two-float offset; more
# rows than any unroll factor; and one more: 5 blocks per client of the agreement pass, in which
# some threads take a whole batch of steps and the others single steps, the last one partial
SMALL_CASES = [(1, 1, 1, 0), (3, 5, 5, 0), (10, 257, 257, 0), (9, 4099, 5000, 1), (2, 1029, 1031, 2),
               (65, 130, 131, 0), (3, 20001, 20004, 1)]
TEN_ROWS = SMALL_CASES[2]
THETA = 4


def wrap_case(sweep):
    """Two rows, three elements past one sweep of the launch grid (``sweep`` elements)."""
    return (2, sweep + 3, sweep + 3, 0)


def case_id(c):
    return "x".join(map(str, c))


def make_case(n, L, rstride, off, seed=0):
    """(view, base) of trim_cases.make_case: 10 % exact-zero deltas (sign 0), -0.0 entries (sign 0
    against a +0 base), magnitudes from 1e-8 to 1e2 with both signs."""
    return tc.make_case(n, L, rstride, off, seed=seed)


def thetas(n):
    """The thresholds a case is checked at: 1, the recipe's 4 and n (those within 1 .. n)."""
    return sorted({t for t in (1, THETA, n) if 1 <= t <= n})


def signs(rows, base):
    """int32 [n, L]: +1 / -1 / 0 from fp32 comparisons (NaN and -0 against +0 give 0)."""
    x = np.asarray(rows, dtype=np.float32)
    b = np.asarray(base, dtype=np.float32)[None]
    with np.errstate(invalid="ignore"):
        return (x > b).astype(np.int32) - (x < b).astype(np.int32)


def oracle_votes(rows, base):
    """(total fp64 [L], votes int32 [L]): a Python loop over the rows, one fp64 addition each."""
    x = np.asarray(rows, dtype=np.float32)
    b = np.asarray(base, dtype=np.float32).astype(np.float64)
    n, L = x.shape
    total = np.zeros(L, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            total = total + (x[i].astype(np.float64) - b)
    votes = signs(x, base).sum(0, dtype=np.int32) if n else np.zeros(L, dtype=np.int32)
    return total, votes


def oracle_agreement(rows, base, votes, theta):
    """int64 [n, 2]: per row the kept coordinates (|V| >= theta) at which its non-zero sign equals
    sign(V) (agree) / -sign(V) (dissent)."""
    s = signs(rows, base)
    V = np.asarray(votes, dtype=np.int64)
    kept = np.abs(V) >= theta
    m = np.sign(V)[None]
    live = kept[None] & (s != 0)
    agree = (live & (s == m)).sum(1).astype(np.int64)
    dissent = (live & (s == -m)).sum(1).astype(np.int64)
    return np.stack([agree, dissent], axis=1).reshape(s.shape[0], 2)


def oracle_flipped(votes, theta):
    return int((np.abs(np.asarray(votes, dtype=np.int64)) < theta).sum())


def same_f64(got, want, tag=""):
    """``got`` (a tensor) equals ``want`` (numpy fp64) wherever the oracle is not NaN, and is NaN
    exactly where it is (``==`` ignores the sign of a zero)."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.asarray(want, dtype=np.float64))
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape), (tag, got.dtype, got.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{tag}NaN positions differ"
    bad = (got != want) & ~nan
    assert not bool(bad.any()), (tag, int(bad.sum()), got[bad][:4], want[bad][:4])


def check_votes(out, rows, base, tag=""):
    """``delta_sum_votes``'s (total, votes) against the oracle; returns the oracle's votes."""
    total, votes = out
    n, L = rows.shape
    want_t, want_v = oracle_votes(rows.numpy(), base.numpy())
    same_f64(total, want_t, tag)
    assert votes.dtype == torch.int32 and tuple(votes.shape) == (L,)
    assert torch.equal(votes.cpu(), torch.from_numpy(want_v)), (tag, "votes")
    return want_v


def check_agreement(counts, rows, base, votes, theta, tag=""):
    n = rows.shape[0]
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (n, 2)
    want = oracle_agreement(rows.numpy(), base.numpy(), votes, theta)
    assert counts.cpu().tolist() == want.tolist(), (tag, theta, counts.cpu().tolist(), want.tolist())


def bits(t):
    """The tensor's bits as integers (so NaNs and signed zeros compare)."""
    t = t.detach().cpu().contiguous()
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def check_apply(ops, dst0, total, votes, theta, coef, sigma, seed, noise, tag=""):
    """``ops.rlr_apply`` on a copy of ``dst0`` against ``ops.add_noise_scaled`` on the same device:
    the bits of the ``+coef`` result at the kept coordinates, of the ``-coef`` result at the flipped
    ones, and the flipped count the oracle's."""
    got, pos, neg = dst0.clone(), dst0.clone(), dst0.clone()
    flipped = ops.rlr_apply(got, total, votes, theta, coef, sigma, seed, noise)
    ops.add_noise_scaled(pos, total, coef, sigma, seed, noise)
    ops.add_noise_scaled(neg, total, -coef, sigma, seed, noise)
    kept = (votes.to(torch.int64).abs() >= theta).cpu()
    want = torch.where(kept, bits(pos), bits(neg))
    assert torch.equal(bits(got), want), (tag, theta, noise, int((bits(got) != want).sum()))
    assert int(flipped) == oracle_flipped(votes.cpu().numpy(), theta) == int((~kept).sum()), (tag, theta)
    return got

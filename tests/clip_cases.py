"""Shared inputs, oracle and bounds of the norm-clipped FedAvg kernel tests (CPU reference ops in
test_clip_aggregation.py, HIP kernels in test_gpu_clip.py): one generator, one numpy fp64 oracle,
one set of tolerances."""
import numpy as np
import torch

from dba_mod_amd.fl import aggregate as agg

# (n, L, rstride, column offset of the view): one element; rows shorter than a block with a padded
# stride; an odd length equal to the stride (every other row misaligned); a view big[:, 1:1+L]
# (every row misaligned, several blocks); one more quad than a launch of the sum kernel sweeps
# (4096 blocks x 256 threads x 4 floats = 16384 * 256 elements: the grid-stride loop wraps)
SMALL_CASES = [(1, 1, 1, 0), (3, 255, 300, 0), (10, 257, 257, 0), (4, 4099, 5000, 1)]
WRAP_CASE = (2, 16384 * 256 + 3, 16384 * 256 + 3, 0)


def make_case(n, L, rstride, off, seed=0):
    """(rows view [n, L] of a [n, rstride] buffer, base [L], scale [n]) with deltas whose
    magnitudes span 1e-8 .. 1e2, both signs, exact zeros, and (n >= 2) one client equal to base.
    Half of base is exactly zero, so the small deltas survive the fp32 rows."""
    g = torch.Generator().manual_seed(seed + 1000 * n + L)
    base = torch.randn(L, generator=g)
    base[torch.rand(L, generator=g) < 0.5] = 0.0
    mag = 10.0 ** (torch.rand(n, L, generator=g, dtype=torch.float64) * 10.0 - 8.0)
    sign = torch.where(torch.rand(n, L, generator=g) < 0.5, -1.0, 1.0).double()
    delta = mag * sign
    delta[torch.rand(n, L, generator=g) < 0.1] = 0.0
    if n >= 2:
        delta[n - 1] = 0.0
    big = torch.zeros(n, rstride)
    big[:, off:off + L] = (base.double()[None] + delta).float()
    scale = torch.rand(n, generator=g).float()
    scale[0] = 1.0
    return big[:, off:off + L], base, scale


_ORACLE = {}


def oracle(rows, base, scale):
    """numpy fp64: (squared norms [n], fp32 max |delta| [n], sum_i s_i delta_i [L], sum_i |s_i delta_i| [L]);
    computed once per input (the inputs are kept alive with the result)."""
    key = (rows.data_ptr(), base.data_ptr(), scale.data_ptr(), tuple(rows.shape))
    if key not in _ORACLE:
        d = rows.numpy().astype(np.float64) - base.numpy().astype(np.float64)[None]
        prod = scale.numpy().astype(np.float64)[:, None] * d
        _ORACLE[key] = ((d * d).sum(1), np.abs(d.astype(np.float32)).max(1), prod.sum(0), np.abs(prod).sum(0),
                        (rows, base, scale))
    return _ORACLE[key][:4]


def exponent(maxabs, n):
    return agg.fixed_exponent(float(np.max(maxabs)), n)


def check_stats(sq, mx, rows, base, scale):
    """sqnorm within relative L * 2^-53 of the oracle (the two differ only in summation order);
    maxabs exactly equal."""
    L = base.numel()
    o_sq, o_mx, _, _ = oracle(rows, base, scale)
    sq, mx = sq.cpu().numpy(), mx.cpu().numpy()
    assert sq.dtype == np.float64 and mx.dtype == np.float32
    err = np.abs(sq - o_sq)
    print(f"  sqnorm max rel err {np.max(err / np.maximum(o_sq, 1e-300)):.3e} (bound {L * 2.0 ** -53:.3e})")
    assert np.all(err <= L * 2.0 ** -53 * o_sq), (err, o_sq)
    assert np.array_equal(mx, o_mx), (mx, o_mx)


def check_decoded(limbs, E, rows, base, scale):
    """decoded limb sum within n * maxabs * 2^-50 of the fp64 oracle (one fp64 rounding per
    product plus the quantisation of the grid)."""
    n = rows.shape[0]
    _, o_mx, o_sum, _ = oracle(rows, base, scale)
    dec = agg.fixed_decode(limbs.cpu(), E).numpy()
    bound = n * float(np.max(o_mx)) * 2.0 ** -50
    err = float(np.max(np.abs(dec - o_sum)))
    print(f"  decoded max abs err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


def check_fp64(out, rows, base, scale):
    """fp64 fallback within n * 2^-52 * sum_i |s_i delta_i| of the oracle per element: n products
    and n - 1 additions of one fp64 rounding (2^-53 relative) each, every partial sum bounded by
    the sum of magnitudes — twice that worst case, for the oracle's own summation."""
    n = rows.shape[0]
    _, _, o_sum, o_abs = oracle(rows, base, scale)
    err = np.abs(out.cpu().numpy() - o_sum)
    print(f"  fp64 max rel err {np.max(err / np.maximum(o_abs, 1e-300)):.3e} (bound {n * 2.0 ** -52:.3e})")
    assert np.all(err <= n * 2.0 ** -52 * o_abs)

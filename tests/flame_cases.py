"""Shared inputs, oracles and bounds of the FLAME tests (CPU reference op and rule in
test_flame_aggregation.py, HIP kernel in test_gpu_flame.py): one generator and one numpy fp64 oracle
for the Gram matrix of the updates, one tolerance; and the planted round with a numpy oracle of the
whole rule."""
import numpy as np
import torch

# the launch grid of csrc/kernels/dgram.hip: at most 512 blocks x 256 threads x 4 floats per step,
# so one sweep of the grid covers 524288 elements and a longer row wraps the grid-stride loop
GRID_BLOCKS_MAX, GRID_THREADS, GRID_QUAD = 512, 256, 4
SWEEP = GRID_BLOCKS_MAX * GRID_THREADS * GRID_QUAD
LONE_ROWS, TILE_ROWS, MAX_ROWS = 10, 8, 64       # dgram.hip kLone, kTile, kMaxRows

# (n, L, rstride, column offset of the view): the diagonal alone; the smallest pair; a padded
# stride; an odd stride (alternate rows misaligned) with n = 10, the largest lone tile; every row
# misaligned over several blocks; nine rows over many blocks (the subset test's); n = 10 misaligned;
# n = 11, the fewest rows that are cut (8 + 3); three tiles of 8, the last of one row; the
# kernel's maximum n
SMALL_CASES = [(1, 1, 1, 0), (2, 1, 1, 0), (3, 255, 300, 0), (10, 257, 257, 0), (5, 4099, 5000, 1),
               (9, 70001, 70004, 0), (10, 1029, 1031, 2), (11, 1029, 1031, 2), (17, 1031, 1040, 3), (64, 130, 130, 0)]
MISALIGNED, NINE_ROWS, ELEVEN_ROWS = SMALL_CASES[4], SMALL_CASES[5], SMALL_CASES[7]
WRAP_CASE = (2, SWEEP + 3, SWEEP + 3, 0)         # three elements past a full sweep of the grid
CASES = SMALL_CASES + [WRAP_CASE]
FALLBACK_CASE = (65, 33, 33, 0)                  # n > 64: the composition on the device


def case_id(c):
    return "x".join(map(str, c))


def make_case(n, L, rstride, off, seed=0):
    """(the [n, L] view big[:, off:off + L] of a [n, rstride] fp32 buffer, base [L] fp32): client
    states around a common model with deltas whose magnitudes span 1e-8 .. 1e2, both signs, exact
    zeros (half of the model is exactly zero, so the small deltas survive the fp32 rows), and the
    last row a copy of the first (n >= 3; the two rows of n = 2 stay distinct)."""
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
    return big[:, off:off + L], base


def twins(n):
    """The pair of identical rows of :func:`make_case`, or None."""
    return (0, n - 1) if n >= 3 else None


_ORACLE = {}


def oracle(rows, base):
    """numpy fp64 ([n, n] G[i][j] = sum_k d_i[k] d_j[k], [n, n] A[i][j] = sum_k |d_i[k] d_j[k]|) with
    d = rows - base, pair by pair (no [n, n, L] temporary); computed once per input (the inputs
    are kept alive with the result)."""
    key = (rows.data_ptr(), base.data_ptr(), tuple(rows.shape))
    if key not in _ORACLE:
        d = rows.numpy().astype(np.float64) - base.numpy().astype(np.float64)[None]
        a = np.abs(d)
        n = d.shape[0]
        G, A = np.zeros((n, n)), np.zeros((n, n))
        for i in range(n):
            for j in range(i, n):
                G[i, j] = G[j, i] = np.dot(d[i], d[j])
                A[i, j] = A[j, i] = np.dot(a[i], a[j])
        _ORACLE[key] = (G, A, (rows, base))
    return _ORACLE[key][:2]


def bound(L):
    """|G - oracle| <= (L + 2) 2^-52 A elementwise: each side makes at most one rounding per product
    (the fp64 delta of two fp32 values is exact and the kernel's fma does not round the product on
    its own: counted all the same) and at most L - 1 roundings of 2^-53 in the sum, in any order,
    every partial sum bounded by the sum of magnitudes A; the factor 2 covers the side under test
    and the oracle's.  Relative to A and not to G: the terms have both signs."""
    return (L + 2) * 2.0 ** -52


def check(G, rows, base, tag=""):
    """fp64 [n, n], bitwise symmetric, identical rows bitwise interchangeable (G[a][b] == G[a][a]
    == G[b][b] and equal rows), and within :func:`bound` of the oracle."""
    n, L = rows.shape
    assert G.dtype == torch.float64 and tuple(G.shape) == (n, n)
    G = G.cpu()
    assert torch.equal(G, G.t())
    tw = twins(n)
    if tw is not None:
        a, b = tw
        assert float(G[a, b]) == float(G[a, a]) == float(G[b, b])
        assert torch.equal(G[a], G[b])
    o, A = oracle(rows, base)
    err = np.abs(G.numpy() - o)
    rel = float(np.max(err / np.maximum(A, 1e-300))) if n else 0.0
    print(f"  {tag}gram max err / A {rel:.3e} (bound {bound(L):.3e})")
    assert np.all(err <= bound(L) * A), (err, A)


# ------------------------------------------------------------------ the planted round
PLANT_N, PLANT_L = 10, 257
PLANT_M = PLANT_N // 2 + 1
PLANT_CROWD = [0, 2, 3, 5, 6, 8, 9]              # m + 1 clients; the rest are the outsiders


def planted(seed=3):
    """(finals [n, L] fp32, base [L] fp32): the crowd's updates are ``u + 0.2 noise_i`` (cosine
    distances near 0.04 among them), the others' independent directions at 50 times the norm
    (distances near 1 to everyone, 1 / sqrt(L) = 0.06 wide): no rounding can move the admitted set."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(PLANT_L, generator=g)
    u = torch.randn(PLANT_L, generator=g, dtype=torch.float64)
    delta = 50.0 * torch.randn(PLANT_N, PLANT_L, generator=g, dtype=torch.float64)
    for i in PLANT_CROWD:
        delta[i] = u + 0.2 * torch.randn(PLANT_L, generator=g, dtype=torch.float64)
    return (base.double()[None] + delta).float(), base


def rule_oracle(finals, base, eta):
    """numpy fp64 oracle of the whole rule without noise, written independently of the code under
    test: (admitted, norms [n], S, gamma [n], clipped mean update [L] = (eta / |A|) sum_{i in A}
    gamma_i d_i, sum_{i in A} |gamma_i d_i| [L], max |d| over A).  The admission grows a threshold
    graph (edges of distance <= t, t ascending over the distinct distances) until a connected
    component holds m clients, which equals Kruskal's order where no two distances tie.  Rows with
    a non-finite update are unusable and rank as +inf for the median."""
    d = finals.numpy().astype(np.float64) - base.numpy().astype(np.float64)[None]
    n = d.shape[0]
    m = n // 2 + 1
    with np.errstate(invalid="ignore", over="ignore"):
        sq = np.array([np.dot(d[i], d[i]) for i in range(n)])
    usable = [i for i in range(n) if np.isfinite(sq[i])]
    D = np.ones((n, n))
    for i in usable:
        for j in usable:
            if i != j and sq[i] > 0 and sq[j] > 0:
                D[i, j] = 1.0 - min(1.0, max(-1.0, np.dot(d[i], d[j]) / np.sqrt(sq[i] * sq[j])))
    admitted = None
    for t in sorted({D[i, j] for i in usable for j in usable if i < j}):
        comp = {i: i for i in usable}
        for _ in range(n):
            for i in usable:
                for j in usable:
                    if i != j and D[i, j] <= t:
                        comp[i] = comp[j] = min(comp[i], comp[j])
        groups = {}
        for i in usable:
            groups.setdefault(comp[i], []).append(i)
        big = [v for v in groups.values() if len(v) >= m]
        if big:
            assert len(big) == 1
            admitted = sorted(big[0])
            break
    assert admitted is not None
    norms = np.where(np.isfinite(sq), np.sqrt(np.where(np.isfinite(sq), sq, 0.0)), np.inf)
    S = float(np.sort(norms)[(n - 1) // 2])
    gamma = np.array([1.0 if norms[i] <= S else S / norms[i] for i in range(n)])
    prod = np.stack([gamma[i] * d[i] for i in admitted])
    upd = (eta / len(admitted)) * prod.sum(0)
    return admitted, norms, S, gamma, upd, np.abs(prod).sum(0), float(np.abs(d[admitted]).max())


def check_rule(factors, norms, admitted, before, after, finals, base, eta):
    """The outputs of ``fedavg_flame`` (lambda = 0) against :func:`rule_oracle`: the admitted set
    exactly; norms within (L + 4) 2^-53 relative (G[i][i] within (L + 2) 2^-52 of the oracle's, A
    being G on the diagonal; the square root halves that and rounds once); a factor exactly 1 or
    0 where the oracle's is, else within (2 L + 10) 2^-53 relative (the two norms' errors and the
    division's rounding); the model within: the clipped sum's bound of clip_cases.check_decoded,
    |A| max|d| 2^-50, plus 2^-24 sum_i |gamma_i d_i| for the factors reaching the kernel as fp32,
    both times eta / |A|; plus one fp32 ulp of the larger of |update| and |after| for the two fp32
    roundings of the apply (the bound of the Krum round test)."""
    adm, o_norms, S, gamma, upd, absum, maxabs = rule_oracle(finals, base, eta)
    n, L = finals.shape
    assert list(admitted) == adm, (admitted, adm)
    norms, factors = np.array(norms), np.array(factors)
    fin = np.isfinite(o_norms)
    assert np.all(norms[~fin] == np.inf)
    rel_n = np.abs(norms[fin] - o_norms[fin]) / np.maximum(o_norms[fin], 1e-300)
    print(f"  norms max rel err {rel_n.max():.3e} (bound {(L + 4) * 2.0 ** -53:.3e})")
    assert np.all(rel_n <= (L + 4) * 2.0 ** -53)
    want = np.where(np.isin(np.arange(n), adm), gamma, 0.0)
    for i in range(n):
        if want[i] in (0.0, 1.0):
            assert factors[i] == want[i], (i, factors[i], want[i])
        else:
            assert abs(factors[i] - want[i]) <= (2 * L + 10) * 2.0 ** -53 * want[i], (i, factors[i], want[i])
    target = before.double().numpy() + upd
    err = np.abs(after.double().numpy() - target)
    big = np.maximum(np.abs(after.numpy()), np.abs(target)).astype(np.float32)
    ulp = np.maximum(np.spacing(big), np.spacing(np.abs(upd).astype(np.float32))).astype(np.float64)
    tol = ulp + (eta / len(adm)) * (len(adm) * maxabs * 2.0 ** -50 + 2.0 ** -24 * absum)
    print(f"  model max err / tol {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    return adm, S

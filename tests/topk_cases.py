"""Cases and the numpy oracle of SparseFed's select and sparse apply (``ops.topk_threshold``,
``ops.topk_apply``), shared by test_sparse_aggregation.py (CPU, ``ops.reference``) and
test_gpu_sparse.py (csrc/kernels/topk.hip).  Every comparison is of bits; there is no tolerance.

A case is ``(resid0 fp64 [L], total fp64 [L], dst0 fp32 [L], ks)``: the residual before the round,
the round's aggregate, the model before the round and the k values to select with.  The cases are
the smallest at which a most-significant-digit-first radix select can still go wrong (whatever its
digit width): one element, keys on both sides of every bit boundary, keys that differ only in
their lowest bits, heavy ties, a wide range with denormals and zeros, non-finite values, and one
sweep of the launch grid plus three."""
import functools

import numpy as np
import torch

ABS_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
COEF = 0.1 / 3                       # (a coefficient that fp32 does not hold exactly)
# one sweep of the widest launch grid of csrc/kernels/topk.hip: the apply pass, 2048 blocks x 256
# threads x 4 coordinates (test_gpu_sparse.py checks it against the kernels' own)
GRID_THREADS, APPLY_QUAD, SELECT_PAIR = 256, 4, 2
APPLY_BLOCKS, SELECT_BLOCKS = 2048, 512
SWEEP = APPLY_BLOCKS * GRID_THREADS * APPLY_QUAD


# ------------------------------------------------------------------------------- oracle
def keys_of(r):
    return np.ascontiguousarray(r, dtype=np.float64).view(np.uint64) & ABS_MASK


def oracle(resid0, total, dst0, k, coef=COEF):
    """(resid, dst, T, m) after one SparseFed round, by the definition: R += total; key = the bits
    of R with the sign cleared; T = the k-th largest key; kept = key >= T; at a kept coordinate dst
    += float32(R * float64(float32(coef))) and R = +0; a dropped coordinate is untouched."""
    with np.errstate(all="ignore"):
        R = resid0.astype(np.float64) + total.astype(np.float64)
        keys = keys_of(R)
        L = R.size
        assert 1 <= k <= L
        T = np.sort(keys)[L - k]
        kept = keys >= T
        upd = (R * np.float64(np.float32(coef))).astype(np.float32)
        dst = dst0.copy()
        dst[kept] = dst0[kept] + upd[kept]
        R[kept] = 0.0
    return R, dst, int(T), int(kept.sum())


def bits(t):
    """A float tensor's bits as integers of the same width (NaNs and signed zeros compare)."""
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}[t.dtype])


def same_bits(got, want, what, nan_any_payload=False):
    """``got`` (a tensor, any device) against the numpy ``want`` bit for bit.  ``nan_any_payload``:
    where ``want`` is a NaN, ``got`` only has to be a NaN (an fp64 NaN narrowed to fp32 and added
    keeps a payload that the arithmetic unit picks)."""
    got = got.detach().cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if nan_any_payload:
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), what
        got, want = torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want)
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:5].flatten().tolist())


# -------------------------------------------------------------------------------- cases
def _from_keys(keys, rng):
    """fp64 values with the given uint64 keys and random signs, shuffled."""
    keys = np.asarray(keys, dtype=np.uint64)
    signs = rng.integers(0, 2, keys.size).astype(np.uint64) << np.uint64(63)
    v = (keys | signs).view(np.float64)
    return v[rng.permutation(keys.size)].copy()


def _dst(L, rng):
    """A model vector with ``-0.0f`` at about a quarter of the coordinates."""
    d = rng.standard_normal(L).astype(np.float32)
    d[rng.random(L) < 0.25] = np.float32(-0.0)
    return d


def _split(r, rng):
    """(resid0, total) with the keys of resid0 + total those of r: half of the coordinates arrive
    with the round's total, half already wait in the residual."""
    at = rng.random(r.size) < 0.5
    return np.where(at, r, 0.0), np.where(at, 0.0, r)


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(sum(name.encode()) * 7919 + len(name))
    if name == "one":
        r, ks = np.array([-3.5]), [1]
    elif name == "five":
        r, ks = np.array([0.5, -2.0, 0.0, 2.0, -1e-310]), [1, 2, 3, 4, 5]      # (a tie at 2, a zero, a denormal)
    elif name == "bit_boundaries":
        # keys 1 << b and (1 << b) - 1 for b = 0 .. 62: every shift and every prefix mask is crossed
        keys = [np.uint64(1) << np.uint64(b) for b in range(63)] + \
               [(np.uint64(1) << np.uint64(b)) - np.uint64(1) for b in range(63)]
        r, ks = _from_keys(keys, rng), list(range(1, 127))
    elif name == "low_digits":
        # the top bits all equal: the answer is decided by the lowest ones
        r = _from_keys(np.uint64(0x3FF0000000000000) + rng.permutation(257).astype(np.uint64), rng)
        ks = [1, 2, 128, 256, 257]
    elif name == "ties":
        L, mags = 4099, np.array([1e-3, 0.5, 1.0, 1.0 + 2.0 ** -52, 7.0, 1e9, 1e300])
        r = mags[rng.integers(0, 7, L)] * rng.choice([-1.0, 1.0], L)
        counts = [(np.abs(r) == m).sum() for m in mags[::-1]]          # group sizes, largest magnitude first
        ks, above = [], 0
        for c in counts:                                                # each group's first, middle, last element
            ks += [above + 1, above + (c + 1) // 2, above + c]
            above += c
        ks = sorted(set(int(k) for k in ks))
    elif name == "misaligned":
        L = 1029
        r, ks = rng.standard_normal(L) * np.exp(rng.uniform(-20, 20, L)), [1, 100, 515, 1029]
    elif name == "wide":
        L = 20001
        r = rng.choice([-1.0, 1.0], L) * 10.0 ** rng.uniform(-300, 300, L)
        den = rng.random(L) < 0.05
        r[den] = 5e-324 * rng.integers(1, 1 << 40, int(den.sum()))    # denormals
        zero = rng.random(L) < 0.10
        r[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)
        nz = int((r != 0).sum())
        ks = [1, L // 100, L // 2, nz, nz + 1, L]                      # the last two: T = 0, everything kept
    elif name == "nonfinite":
        L = 300
        r = rng.standard_normal(L)
        nans = np.array([0x7FF8000000000001, 0xFFF8000000000123, 0x7FFC000000000000, 0xFFF80000DEADBEEF],
                        dtype=np.uint64).view(np.float64)
        r[[3, 77, 150, 299]] = nans
        r[[10, 200]] = [np.inf, -np.inf]
        # 1: the largest-key NaN alone; 4: all NaNs; 5: T is inf's key, both infinities (a tie); 7: one finite value
        ks = [1, 4, 5, 7, L]
    elif name == "wrap":
        # three coordinates past one sweep of the widest grid; the k-th largest is one of those three
        L = SWEEP + 3
        r = rng.standard_normal(L)
        r[-3:] = [40.0, -50.0, 60.0]
        r[:5] = [100.0, -200.0, 300.0, -45.0, 55.0]
        ks = [4, 8]                                                     # T = 60 and T = 40: both in the wrapped tail
    else:
        raise KeyError(name)
    L = r.size
    if name == "nonfinite":      # NaNs arrive through total alone (0 + NaN keeps the payload on every adder)
        resid0, total = np.zeros(L), r
    elif name == "misaligned":   # a sum that rounds at every coordinate
        resid0, total = r, rng.standard_normal(L) * np.exp(rng.uniform(-20, 20, L))
        r = resid0 + total
    else:
        resid0, total = _split(r, rng)
    assert np.array_equal(keys_of(resid0 + total), keys_of(r))
    return resid0, total, _dst(L, rng), ks


SMALL_CASES = ["one", "five", "bit_boundaries", "low_digits", "ties", "misaligned", "wide", "nonfinite"]
WRAP_CASE = "wrap"


# -------------------------------------------------------------------------------- checks
def workspace(ops, dev):
    """The select workspace of the backend that serves ``dev`` (None off the HIP backend)."""
    return ops.hip_module().topk_workspace(dev) if ops.backend_name(torch.device(dev)) == "hip" else None


def run(ops, dev, resid0, total, dst0, k, ws=None, coef=COEF):
    """One round through the two ops on ``dev``: (resid, dst, sel after the select, sel after the apply)."""
    resid = torch.from_numpy(resid0).to(dev).clone()
    dst = torch.from_numpy(dst0).to(dev).clone()
    sel = ops.topk_threshold(resid, torch.from_numpy(total).to(dev), k, ws=ws)
    assert sel.dtype == torch.int64 and tuple(sel.shape) == (2,) and sel.device.type == torch.device(dev).type
    first = sel.clone()
    assert ops.topk_apply(dst, resid, sel, coef) is None
    return resid, dst, first, sel


def check_case(ops, dev, name):
    """Every k of the case against the oracle, then every k again on the same workspace: the second
    sweep follows a select with another k, so anything a call left behind would show."""
    resid0, total, dst0, ks = case(name)
    ws = workspace(ops, dev)
    seen = {}
    for sweep in range(2):
        for k in ks:
            resid, dst, first, sel = run(ops, dev, resid0, total, dst0, k, ws)
            if sweep == 0:
                want_r, want_d, T, m = oracle(resid0, total, dst0, k)
                assert first.tolist() == [T, m], (name, k, first.tolist(), [T, m])
                assert sel.tolist() == [T, m], (name, k, sel.tolist(), [T, m])
                assert m >= k
                same_bits(resid, want_r, (name, k, "resid"))
                same_bits(dst, want_d, (name, k, "dst"), nan_any_payload=True)
                seen[k] = (resid, dst, sel)
            else:
                assert torch.equal(bits(seen[k][0]), bits(resid)) and torch.equal(bits(seen[k][1]), bits(dst)) \
                    and torch.equal(seen[k][2], sel), (name, k, "second sweep")


def check_offsets(ops, dev):
    """The "misaligned" case with ``resid`` / ``total`` starting 8 bytes off a 16-byte boundary and
    ``dst`` at float offsets 0 .. 3: every placement gives the bits of the aligned copy."""
    resid0, total, dst0, ks = case("misaligned")
    L = resid0.size
    for k in ks:
        want = run(ops, dev, resid0, total, dst0, k)
        for roff, toff, doff in [(1, 1, 0), (1, 0, 1), (0, 1, 2), (1, 1, 3), (0, 0, 1)]:
            rbuf = torch.zeros(L + 2, dtype=torch.float64, device=dev)
            tbuf = torch.zeros(L + 2, dtype=torch.float64, device=dev)
            dbuf = torch.zeros(L + 4, dtype=torch.float32, device=dev)
            resid, tot, dst = rbuf[roff:roff + L], tbuf[toff:toff + L], dbuf[doff:doff + L]
            assert resid.data_ptr() % 16 == 8 * roff and tot.data_ptr() % 16 == 8 * toff and dst.data_ptr() % 16 == 4 * doff
            resid.copy_(torch.from_numpy(resid0))
            tot.copy_(torch.from_numpy(total))
            dst.copy_(torch.from_numpy(dst0))
            sel = ops.topk_threshold(resid, tot, k)
            ops.topk_apply(dst, resid, sel, COEF)
            assert torch.equal(bits(resid), bits(want[0])) and torch.equal(bits(dst), bits(want[1])) \
                and torch.equal(sel, want[3]), (k, roff, toff, doff)
            # nothing outside the views was written
            assert not rbuf[:roff].any() and not rbuf[roff + L:].any() and not dbuf[:doff].any() and not dbuf[doff + L:].any()


def check_full_support_is_fedavg(ops, dev, coef):
    """k = L on a zero residual: ``topk_apply`` gives the bits of ``ops.add_noise_scaled`` (noise
    off) on the same total, and the residual stays all zeros.  (On a total without ``-0.0``, which
    no delta sum produces: a sum that starts from +0.0 never ends at -0.0, and R = +0.0 + -0.0 is +0.0.)"""
    _, total, dst0, _ = case("wide")
    total = total + 0.0
    L = total.size
    t = torch.from_numpy(total).to(dev)
    resid = torch.zeros(L, dtype=torch.float64, device=dev)
    got, want = torch.from_numpy(dst0).to(dev).clone(), torch.from_numpy(dst0).to(dev).clone()
    sel = ops.topk_threshold(resid, t, L)
    ops.topk_apply(got, resid, sel, coef)
    ops.add_noise_scaled(want, t, coef, 0.0, 1, False)
    assert torch.equal(bits(got), bits(want))
    assert sel.tolist()[1] == L and not bits(resid).any()


def check_degenerate(o, dev):
    """L = 0 returns (0, 0) and touches nothing; k out of range or not an integer is a ValueError,
    before anything is written."""
    import pytest
    e64, e32 = torch.zeros(0, dtype=torch.float64, device=dev), torch.zeros(0, device=dev)
    for k in (0, 1, 5):
        sel = o.topk_threshold(e64, e64, k)
        assert sel.dtype == torch.int64 and sel.tolist() == [0, 0] and sel.device.type == torch.device(dev).type
    assert o.topk_apply(e32, e64, sel, 0.1) is None and sel.tolist() == [0, 0]
    r = torch.ones(3, dtype=torch.float64, device=dev)
    for k in (0, -1, 4, True, 2.0, "2", None):
        with pytest.raises(ValueError):
            o.topk_threshold(r, r.clone(), k)
    assert r.tolist() == [1.0, 1.0, 1.0]


def check_hand_case(dev):
    """L = 4, n = 3, k = 2, eta = 1.5 (so eta / no_models = 0.5), two rounds on one residual.  Round 1:
    the total is [6, 1, -4, -1]; 6 and -4 are applied (w = [3, 0, -2, 0]) and [0, 1, 0, -1] waits.  Round
    2: the total is [1.5, 1, -4, -1], which alone would select coordinates 2 and 0; with what round 1
    left R = [1.5, 2, -4, -2], so -4 and the tie at 2 are applied (three coordinates for k = 2) and
    coordinate 0 waits with 1.5."""
    from dba_mod_amd.fl import aggregate as agg
    d1 = torch.tensor([[1.0, 0.5, -4.0, 0.0], [2.0, 0.25, 1.0, 0.0], [3.0, 0.25, -1.0, -1.0]], device=dev)
    d2 = torch.tensor([[1.0, 0.5, -4.0, 0.0], [-2.0, 0.25, 1.0, 0.0], [2.5, 0.25, -1.0, -1.0]], device=dev)
    g = torch.zeros(4, device=dev)
    R = torch.zeros(4, dtype=torch.float64, device=dev)
    factors, norms, m, thr = agg.fedavg_sparse(g, g[None] + d1, 2, None, R, 1.5, 3, 4)
    assert g.tolist() == [3.0, 0.0, -2.0, 0.0] and R.tolist() == [0.0, 1.0, 0.0, -1.0]
    assert (m, thr) == (2, 4.0) and factors == [1.0, 1.0, 1.0]
    assert norms == [float(np.sqrt(np.float64(x))) for x in (17.25, 5.0625, 11.0625)]
    factors, norms, m, thr = agg.fedavg_sparse(g, g[None] + d2, 2, None, R, 1.5, 3, 4)
    assert g.tolist() == [3.0, 1.0, -4.0, -1.0] and R.tolist() == [1.5, 0.0, 0.0, 0.0]
    assert (m, thr) == (3, 2.0)
    assert bits(R).tolist() == [bits(torch.tensor([1.5], dtype=torch.float64)).item(), 0, 0, 0]      # (+0.0, not -0.0)

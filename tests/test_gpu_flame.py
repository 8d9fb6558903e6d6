"""FLAME on the GPU: the fused Gram kernel of csrc/kernels/dgram.hip against the numpy fp64 oracle
of flame_cases.py (bound, exact symmetry, twins, bitwise reproducibility, independence of alignment
and of the other rows), the n > 64 composition, the planted round on the device against the CPU
path, and one model-replacement round through ``Server``."""
import functools

import pytest
import torch

import flame_cases as fc
import test_trim_aggregation as trim_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case):
    return fc.make_case(*case)


def _on_device(case, dev):
    """(the same strided view on the device: big[:, off:off + L] of a [n, rstride] buffer, base)."""
    n, L, rstride, off = case
    rows, base = _case(case)
    big = torch.zeros(n, rstride, device=dev)
    big[:, off:off + L] = rows.to(dev)
    view = big[:, off:off + L]
    assert view.stride(0) == rstride or n == 1
    return view, base.to(dev)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_kernel_matches_oracle(dev, case):
    from dba_mod_amd import ops
    view, base = _on_device(case, dev)
    G = ops.delta_gram(view, base)
    assert G.is_cuda
    fc.check(G, *_case(case))
    assert torch.equal(G, ops.delta_gram(view, base))            # bitwise run to run
    assert torch.equal(G, torch.ops.dba.delta_gram(view, base, None))


def test_wrap_case_wraps_the_grid(dev):
    """The wrap case is three elements past one sweep of the kernel's own launch grid."""
    from dba_mod_amd.ops import hip as H
    L = fc.WRAP_CASE[1]
    assert int(H._L.dba_delta_gram_blocks(L)) == fc.GRID_BLOCKS_MAX
    assert int(H._L.dba_delta_gram_blocks(L - 4)) == fc.GRID_BLOCKS_MAX
    assert fc.GRID_BLOCKS_MAX * fc.GRID_THREADS * fc.GRID_QUAD == L - 3
    assert int(H._L.dba_delta_gram_blocks(fc.SWEEP - 4 * fc.GRID_THREADS)) == fc.GRID_BLOCKS_MAX - 1
    assert H.GRAM_MAX_ROWS == fc.MAX_ROWS


def test_row_idx_reads_rows_in_place(dev):
    """Rows taken out of order from a larger buffer, one index repeated: the bits of the gathered
    call, and the repeated pair equal to its diagonal."""
    from dba_mod_amd import ops
    view, base = _on_device(fc.NINE_ROWS, dev)
    idx = [7, 2, 5, 2, 8, 0]
    G = ops.delta_gram(view, base, idx)
    assert tuple(G.shape) == (6, 6)
    assert torch.equal(G, ops.delta_gram(view[idx].contiguous(), base))
    assert float(G[1, 3]) == float(G[1, 1]) == float(G[3, 3])
    assert float(G[4, 5]) == float(G[4, 4]) == float(G[5, 5])      # rows 8 and 0 are the case's twins
    assert torch.equal(G, ops.delta_gram(view, base, torch.tensor(idx, device=dev)))
    with pytest.raises(ValueError):
        ops.delta_gram(view, base, [0, 9])


def test_aligned_copy_and_misaligned_view_agree(dev):
    """The offset-1 view (every row misaligned: scalar loads) and a 16-byte aligned copy of it
    (vector loads) give the same bits; so does a misaligned base."""
    from dba_mod_amd import ops
    view, base = _on_device(fc.MISALIGNED, dev)
    assert view.data_ptr() % 16 != 0
    L = view.shape[1]
    pad = torch.zeros(view.shape[0], (L + 3) // 4 * 4, device=dev)
    pad[:, :L] = view
    copy = pad[:, :L]
    assert copy.data_ptr() % 16 == 0 and copy.stride(0) % 4 == 0
    G = ops.delta_gram(view, base)
    assert torch.equal(G, ops.delta_gram(copy, base))
    shifted = torch.zeros(L + 1, device=dev)
    shifted[1:] = base
    assert shifted[1:].data_ptr() % 16 != 0 and base.data_ptr() % 16 == 0
    assert torch.equal(G, ops.delta_gram(copy, shifted[1:]))


def test_subset_of_rows_keeps_its_bits(dev):
    """G of rows {1, 4, 8} of the 9-row case equals those entries of the full G bit for bit, by
    row_idx and from a gathered copy (whose rows are aligned differently); so do rows
    {1, 3, 9, 10} of the 11-row case, which the full call cuts into two tiles (pairs from two
    diagonal tiles and from an off-diagonal tile pair) and the subset call takes as one."""
    from dba_mod_amd import ops
    for case, sub in ((fc.NINE_ROWS, [1, 4, 8]), (fc.ELEVEN_ROWS, [1, 3, 9, 10])):
        view, base = _on_device(case, dev)
        full = ops.delta_gram(view, base)
        want = full[sub][:, sub]
        assert torch.equal(ops.delta_gram(view, base, sub), want)
        assert torch.equal(ops.delta_gram(view[sub].contiguous(), base), want)


def test_nonfinite_poisons_its_row_only(dev):
    from dba_mod_amd import ops
    for n in (10, 13):                                            # the lone tile and the cut tiles
        g = torch.Generator().manual_seed(n)
        rows = torch.randn(n, 3000, generator=g).to(dev)
        base = torch.randn(3000, generator=g).to(dev)
        off = [j for j in range(n) if j != 8]
        for bad in (float("nan"), float("inf")):
            rows[8, 2047] = bad
            G = ops.delta_gram(rows, base)
            assert not torch.isfinite(G[8]).any() and not torch.isfinite(G[:, 8]).any()
            assert torch.isfinite(G[off][:, off]).all()
        assert float(G[8, 8]) == float("inf")


def test_degenerate_shapes(dev):
    from dba_mod_amd import ops
    for shape in ((0, 37), (5, 0), (0, 0)):
        G = ops.delta_gram(torch.randn(*shape, device=dev), torch.randn(shape[1], device=dev))
        assert G.is_cuda and G.dtype == torch.float64 and tuple(G.shape) == (shape[0], shape[0]) and not G.any()
    x, base = torch.randn(1, 37, device=dev), torch.randn(37, device=dev)
    G = ops.delta_gram(x, base)
    want = ((x[0].double() - base.double()) ** 2).sum()
    assert tuple(G.shape) == (1, 1) and abs(float(G[0, 0]) - float(want)) <= fc.bound(37) * float(want)
    assert tuple(ops.delta_gram(x, base, []).shape) == (0, 0)


def test_more_than_64_rows_take_the_composition(dev):
    from dba_mod_amd import ops
    from dba_mod_amd.ops import hip as H
    view, base = _on_device(fc.FALLBACK_CASE, dev)
    G = ops.delta_gram(view, base)
    assert G.is_cuda
    fc.check(G, *_case(fc.FALLBACK_CASE))
    # the entry point itself declines: hipErrorInvalidValue (1), nothing launched
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    rc = H._L.dba_delta_gram(view.data_ptr(), view.stride(0), None, 65, base.data_ptr(), view.shape[1], out.data_ptr(),
                             out.data_ptr(), H._stream())
    assert rc == 1 and float(out) == 0.0


def test_planted_rule_on_the_device(dev):
    """The planted round on the GPU: the oracle's admitted set, factors, norms and model within its
    bounds, and the admitted set and factors of the CPU path."""
    from dba_mod_amd.fl import aggregate as agg
    finals, base = fc.planted()
    eta = 0.7
    g = base.to(dev)
    factors, norms, admitted = agg.fedavg_flame(g, finals.to(dev), 0.0, eta, 5, fc.PLANT_L)
    fc.check_rule(factors, norms, admitted, base, g.cpu(), finals, base, eta)
    c = base.clone()
    c_factors, c_norms, c_admitted = agg.fedavg_flame(c, finals, 0.0, eta, 5, fc.PLANT_L)
    assert admitted == c_admitted
    assert [f == 0.0 for f in factors] == [f == 0.0 for f in c_factors]
    assert [f == 1.0 for f in factors] == [f == 1.0 for f in c_factors]
    L = fc.PLANT_L
    for a, b in zip(factors, c_factors):          # (each within the oracle's bound: twice that apart)
        assert abs(a - b) <= 2 * (2 * L + 10) * 2.0 ** -53 * max(a, b)
    # in place out of a larger bank with row_idx, with noise: bitwise run to run
    bank = torch.zeros(2 * fc.PLANT_N + 1, L + 3, device=dev)
    slots = list(range(1, 2 * fc.PLANT_N + 1, 2))
    bank[slots, :L] = finals.to(dev)
    outs = []
    for _ in range(2):
        g2 = torch.cat([base, torch.ones(3)]).to(dev)
        res = agg.fedavg_flame(g2, bank, 0.01, eta, 5, L, row_idx=slots)
        assert res == (factors, norms, admitted)
        outs.append(g2)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0][:L], g)
    assert torch.equal(outs[0][L:], torch.ones(3, device=dev))


def test_server_round_on_the_gpu(dev, tmp_path):
    """The CPU test's round (MNIST synthetic, attacker 41 poisons in round 12 with scale 100) on the
    GPU with FLAME, twice: identical bits; the attacker's norm is the largest, its factor 0 or
    S / e_41 below 1; the model moved."""
    from dba_mod_amd.fl import aggregate as agg
    outs = []
    for rep in range(2):
        res = trim_cpu.run_round(tmp_path / f"r{rep}", device=dev, clip_norm="median", clip_flame=True)
        before, after, finals, wr, n_upd, p = res
        outs.append((after, wr))
        if rep == 0:
            names, factors, norms = wr
            print(f"names {names}\nfactors {factors}\nnorms {norms}")
            i = names.index(41)
            assert all(norms[i] > v for j, v in enumerate(norms) if j != i)
            S = agg.clip_bound(norms, "median")
            clipped = float(S / torch.tensor(norms[i], dtype=torch.float64))
            assert factors[i] == 0.0 or (factors[i] == clipped and factors[i] < 1.0)
            assert sum(f > 0.0 for f in factors) >= len(names) // 2 + 1
            assert not torch.equal(after[:n_upd], before[:n_upd]) and torch.equal(after[n_upd:], before[n_upd:])
            g = before.clone()
            dp_seed = (int(p["seed"]) * 7919 + 12) & 0x7FFFFFFF
            want = agg.fedavg_flame(g, finals, p.flame_lambda, float(p["eta"]), dp_seed, n_upd)
            assert (want[0], want[1]) == (factors, norms) and torch.equal(g, after)
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]

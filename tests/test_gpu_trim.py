"""The coordinate-wise trimmed mean on the GPU: the fused kernel of csrc/kernels/trim.hip against
the numpy oracle of trim_cases.py bit for bit (every case, a wrap of the launch grid, row_idx,
non-finite values, degenerate shapes), the n > 64 composition, and one model-replacement round
through ``Server``."""
import pytest
import torch

import test_trim_aggregation as cpu
import trim_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", tc.SMALL_CASES, ids=tc.case_id)
def test_kernel_matches_oracle(dev, case):
    from dba_mod_amd import ops
    view, base = tc.on_device(case, dev)
    out = ops.trimmed_delta_sum(view, base, case[4])
    assert all(t.is_cuda for t in out)
    tc.check(out, *tc.case_rows(case), case[4])
    assert tc.same_bits(out, ops.trimmed_delta_sum(view, base, case[4]))    # bitwise run to run


def test_wrap_case_wraps_the_grid(dev):
    """Three elements past one sweep of the kernel's own launch grid: a thread's second step."""
    from dba_mod_amd import ops
    from dba_mod_amd.ops import hip as H
    blocks = int(H._L.dba_coord_trim_blocks(1 << 40))                       # the grid's maximum
    sweep = blocks * tc.GRID_THREADS * tc.GRID_QUAD
    assert sweep == cpu.SWEEP
    assert int(H._L.dba_coord_trim_blocks(sweep)) == blocks
    assert int(H._L.dba_coord_trim_blocks(sweep - 4 * tc.GRID_THREADS)) == blocks - 1
    assert H.TRIM_MAX_ROWS == 64
    case = tc.wrap_case(sweep)
    assert int(H._L.dba_coord_trim_blocks(case[1])) == blocks
    view, base = tc.on_device(case, dev)
    tc.check(ops.trimmed_delta_sum(view, base, case[4]), *tc.case_rows(case), case[4])


def test_row_idx_reads_rows_in_place(dev):
    """Rows taken out of order from a larger buffer, one index repeated: the bits of the gathered call."""
    from dba_mod_amd import ops
    view, base = tc.on_device(tc.NINE_ROWS, dev)
    idx = [7, 2, 5, 2, 8, 0]
    out = ops.trimmed_delta_sum(view, base, 2, idx)
    assert tuple(out[1].shape) == (6,)
    assert tc.same_bits(out, ops.trimmed_delta_sum(view[idx].contiguous(), base, 2))
    assert tc.same_bits(out, ops.trimmed_delta_sum(view, base, 2, torch.tensor(idx, device=dev)))
    rows, b = tc.case_rows(tc.NINE_ROWS)
    tc.check(out, rows[idx], b, 2)
    with pytest.raises(ValueError):
        ops.trimmed_delta_sum(view, base, 1, [0, 9, 1])


def test_nonfinite_values_follow_ieee(dev):
    from dba_mod_amd import ops
    x, base = cpu.nonfinite_input()
    out = ops.trimmed_delta_sum(x.to(dev), base.to(dev), 1)
    cpu.check_nonfinite(*out)
    tc.check(out, x, base, 1)
    # ... and in the middle of a longer, misaligned row, with negative-signed NaNs
    rows, b = tc.make_case(10, 3001, 3004, 1)
    rows = rows.clone()
    rows[8, 2047] = float("nan")
    rows[3, 2047] = -float("nan")
    rows[2, 2047] = float("inf")
    rows[5, 100] = -float("nan")
    rows[6, 3000] = float("-inf")
    big = torch.zeros(10, 3004, device=dev)
    big[:, 1:3002] = rows.to(dev)
    for k in (1, 2, 3):
        tc.check(ops.trimmed_delta_sum(big[:, 1:3002], b.to(dev), k), rows, b, k, tag=f"k={k} ")


def test_degenerate_shapes_return_zeros(dev):
    from dba_mod_amd import ops
    for (n, L), k in (((0, 37), 0), ((5, 0), 2)):
        total, kept, high = ops.trimmed_delta_sum(torch.randn(n, L, device=dev), torch.randn(L, device=dev), k)
        assert total.is_cuda and total.dtype == torch.float64 and tuple(total.shape) == (L,) and not total.any()
        assert kept.dtype == torch.int64 and tuple(kept.shape) == (n,) and not kept.any()
        assert high.dtype == torch.int64 and tuple(high.shape) == (n,) and not high.any()
    total, kept, high = ops.trimmed_delta_sum(torch.randn(4, 7, device=dev), torch.randn(7, device=dev), 0, [])
    assert tuple(total.shape) == (7,) and not total.any() and kept.numel() == 0 and high.numel() == 0
    # a single row: its delta, kept everywhere
    x, b = torch.randn(1, 37, device=dev), torch.randn(37, device=dev)
    total, kept, high = ops.trimmed_delta_sum(x, b, 0)
    assert torch.equal(total, x[0].double() - b.double()) and kept.tolist() == [37] and high.tolist() == [0]
    with pytest.raises(ValueError):
        ops.trimmed_delta_sum(torch.randn(4, 7, device=dev), torch.randn(7, device=dev), 2)


def test_more_than_64_rows_take_the_composition(dev):
    from dba_mod_amd import ops
    case = tc.FALLBACK_CASE
    view, base = tc.on_device(case, dev)
    out = ops.trimmed_delta_sum(view, base, case[4])
    assert all(t.is_cuda for t in out)
    tc.check(out, *tc.case_rows(case), case[4])


def test_server_round_cuts_the_attacker(dev, tmp_path):
    """The CPU test's round (MNIST synthetic, attacker 41 poisons in round 12 with scale 100) on the
    GPU with trim_k = 2, twice: identical bits, the attacker's kept share the smallest, and the
    state equal to the oracle's total applied with the same op."""
    outs = []
    for rep in range(2):
        res = cpu.run_round(tmp_path / f"r{rep}", device=dev, trim_k=2)
        outs.append((res[1], res[3]))
        if rep == 0:
            cpu.check_round(res, 2)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert outs[0][1] == outs[1][1]

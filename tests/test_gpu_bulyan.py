"""Bulyan's second stage on the GPU: the fused kernel of csrc/kernels/bulyan.hip against the numpy
oracle of bulyan_cases.py bit for bit (every case, a wrap of the launch grid, row_idx, non-finite
values, degenerate shapes), the t > 64 composition, and one model-replacement round through
``Server``."""
import pytest
import torch

import bulyan_cases as bc
import test_bulyan_aggregation as cpu
import test_trim_aggregation as trim_cpu
import trim_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", bc.SMALL_CASES, ids=bc.case_id)
def test_kernel_matches_oracle(dev, case):
    from dba_mod_amd import ops
    view, base = tc.on_device(case, dev)
    out = ops.bulyan_delta_sum(view, base, case[4])
    assert all(t.is_cuda for t in out)
    bc.check(out, *tc.case_rows(case), case[4])
    assert tc.same_bits(out, ops.bulyan_delta_sum(view, base, case[4]))     # bitwise run to run


def test_wrap_case_wraps_the_grid(dev):
    """Three elements past one sweep of the kernel's own launch grid: a thread's second step."""
    from dba_mod_amd import ops
    from dba_mod_amd.ops import hip as H
    blocks = int(H._L.dba_coord_bulyan_blocks(1 << 40))                     # the grid's maximum
    sweep = blocks * bc.GRID_THREADS * bc.GRID_QUAD
    assert sweep == cpu.SWEEP
    assert int(H._L.dba_coord_bulyan_blocks(sweep)) == blocks
    assert int(H._L.dba_coord_bulyan_blocks(sweep - 4 * bc.GRID_THREADS)) == blocks - 1
    assert H.BULYAN_MAX_ROWS == 64
    case = bc.wrap_case(sweep)
    assert int(H._L.dba_coord_bulyan_blocks(case[1])) == blocks
    view, base = tc.on_device(case, dev)
    bc.check(ops.bulyan_delta_sum(view, base, case[4]), *tc.case_rows(case), case[4])


def test_row_idx_reads_rows_in_place(dev):
    """Rows taken out of order from a larger buffer, one index repeated: the bits of the gathered call."""
    from dba_mod_amd import ops
    view, base = tc.on_device(bc.NINE_ROWS, dev)
    idx = [7, 2, 5, 2, 8, 0, 3]
    out = ops.bulyan_delta_sum(view, base, 2, idx)
    assert tuple(out[1].shape) == (7,)
    assert tc.same_bits(out, ops.bulyan_delta_sum(view[idx].contiguous(), base, 2))
    assert tc.same_bits(out, ops.bulyan_delta_sum(view, base, 2, torch.tensor(idx, device=dev)))
    rows, b = tc.case_rows(bc.NINE_ROWS)
    bc.check(out, rows[idx], b, 2)
    with pytest.raises(ValueError):
        ops.bulyan_delta_sum(view, base, 1, [0, 9, 1])


def test_nonfinite_values_follow_the_rule(dev):
    from dba_mod_amd import ops
    x, base = trim_cpu.nonfinite_input()
    for f in (0, 1, 2):
        bc.check(ops.bulyan_delta_sum(x.to(dev), base.to(dev), f), x, base, f, tag=f"f={f} ")
    # ... and in the middle of a longer, misaligned row, with negative-signed NaNs
    rows, b = bc.make_case(10, 3001, 3004, 1)
    rows = rows.clone()
    rows[8, 2047] = float("nan")
    rows[3, 2047] = -float("nan")
    rows[2, 2047] = float("inf")
    rows[5, 100] = -float("nan")
    rows[6, 3000] = float("-inf")
    rows[1, 77] = float("inf")
    rows[4, 77] = float("inf")
    rows[0, 78] = float("-inf")
    rows[9, 78] = float("-inf")
    big = torch.zeros(10, 3004, device=dev)
    big[:, 1:3002] = rows.to(dev)
    for f in (1, 2, 3):
        bc.check(ops.bulyan_delta_sum(big[:, 1:3002], b.to(dev), f), rows, b, f, tag=f"f={f} ")


def test_degenerate_shapes_return_zeros(dev):
    from dba_mod_amd import ops
    for (t, L), f in (((0, 37), 0), ((5, 0), 2)):
        total, kept, high = ops.bulyan_delta_sum(torch.randn(t, L, device=dev), torch.randn(L, device=dev), f)
        assert total.is_cuda and total.dtype == torch.float64 and tuple(total.shape) == (L,) and not total.any()
        assert kept.dtype == torch.int64 and tuple(kept.shape) == (t,) and not kept.any()
        assert high.dtype == torch.int64 and tuple(high.shape) == (t,) and not high.any()
    total, kept, high = ops.bulyan_delta_sum(torch.randn(4, 7, device=dev), torch.randn(7, device=dev), 0, [])
    assert tuple(total.shape) == (7,) and not total.any() and kept.numel() == 0 and high.numel() == 0
    # a single row: its delta, kept everywhere
    x, b = torch.randn(1, 37, device=dev), torch.randn(37, device=dev)
    total, kept, high = ops.bulyan_delta_sum(x, b, 0)
    assert torch.equal(total, x[0].double() - b.double()) and kept.tolist() == [37] and high.tolist() == [0]
    # invalid f: rejected on the host, nothing is launched
    for t, f in ((4, 2), (5, -1), (0, 1)):
        with pytest.raises(ValueError):
            ops.bulyan_delta_sum(torch.randn(t, 7, device=dev), torch.randn(7, device=dev), f)


def test_f0_is_the_plain_trimmed_sum(dev):
    from dba_mod_amd import ops
    view, base = tc.on_device(bc.NINE_ROWS, dev)
    assert tc.same_bits(ops.bulyan_delta_sum(view, base, 0), ops.trimmed_delta_sum(view, base, 0))


def test_more_than_64_rows_take_the_composition(dev):
    from dba_mod_amd import ops
    case = bc.FALLBACK_CASE
    view, base = tc.on_device(case, dev)
    out = ops.bulyan_delta_sum(view, base, case[4])
    assert all(t.is_cuda for t in out)
    bc.check(out, *tc.case_rows(case), case[4])


def test_server_round_drops_the_attacker(dev, tmp_path):
    """The CPU test's round (MNIST synthetic, attacker 41 poisons in round 12 with scale 100) on the
    GPU with krum_f = 1 and krum_bulyan, twice: identical bits, the attacker not selected, and the
    state equal to the oracle's total over the selected rows applied with the same op."""
    outs = []
    for rep in range(2):
        res = trim_cpu.run_round(tmp_path / f"r{rep}", device=dev, krum_f=1, krum_bulyan=True)
        outs.append((res[1], res[3]))
        if rep == 0:
            cpu.check_round(res, 1)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert outs[0][1] == outs[1][1]

"""Robust-learning-rate FedAvg on the GPU: the three kernels of csrc/kernels/rlr.hip against the
numpy oracle of rlr_cases.py bit for bit (every case, a wrap of the launch grid, strided and
misaligned rows, non-finite values, degenerate shapes), ``total`` against ``ops.delta_sum``,
``rlr_apply`` against ``ops.add_noise_scaled`` with noise off and on, run-to-run bit equality, and
one model-replacement round through ``Server``, twice."""
import functools

import pytest
import torch

import rlr_cases as rc
import test_rlr_aggregation as cpu
import test_trim_aggregation as trim_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case):
    """(rows, base, the oracle's total and votes) on the host: computed once per case."""
    rows, base = rc.make_case(*case)
    total, votes = rc.oracle_votes(rows.numpy(), base.numpy())
    return rows, base, total, votes


def _on_device(case, dev):
    """The same strided view on the device (big[:, off:off + L] of a [n, rstride] buffer) and the base."""
    n, L, rstride, off = case
    rows, base = _case(case)[:2]
    big = torch.zeros(n, rstride, device=dev)
    big[:, off:off + L] = rows.to(dev)
    view = big[:, off:off + L]
    assert view.stride(0) == rstride or n == 1
    return view, base.to(dev)


def _same(a, b):
    return all(torch.equal(rc.bits(x), rc.bits(y)) for x, y in zip(a, b))


def _check_case(case, dev):
    """All three kernels on one case against the oracle, ``delta_sum`` and ``add_noise_scaled``."""
    from dba_mod_amd import ops
    n = case[0]
    rows, base, want_t, want_v = _case(case)
    view, b = _on_device(case, dev)
    out = ops.delta_sum_votes(view, b)
    assert all(t.is_cuda for t in out)
    rc.same_f64(out[0], want_t)
    assert out[1].dtype == torch.int32 and torch.equal(out[1].cpu(), torch.from_numpy(want_v))
    assert _same(out, ops.delta_sum_votes(view, b))                          # bitwise run to run
    assert torch.equal(rc.bits(out[0]), rc.bits(ops.delta_sum(view, b)))     # the bits of plain FedAvg's sum
    total, votes = out
    for theta in rc.thetas(n):
        counts = ops.vote_agreement(view, b, votes, theta)
        assert counts.is_cuda
        rc.check_agreement(counts, rows, base, want_v, theta)
        assert torch.equal(counts, ops.vote_agreement(view, b, votes, theta))
        for noise in (False, True):
            got = rc.check_apply(ops, b, total, votes, theta, cpu.COEF, cpu.SIGMA, cpu.SEED, noise)
            again = b.clone()
            ops.rlr_apply(again, total, votes, theta, cpu.COEF, cpu.SIGMA, cpu.SEED, noise)
            assert torch.equal(rc.bits(got), rc.bits(again))


@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=rc.case_id)
def test_kernels_match_oracle(dev, case):
    _check_case(case, dev)


def test_wrap_case_wraps_the_grid(dev):
    """Three elements past one sweep of the kernels' own launch grid: a thread's second step."""
    from dba_mod_amd.ops import hip as H
    blocks = int(H._L.dba_vote_agreement_blocks(1 << 40))                    # the agreement grid's maximum
    per_block = rc.GRID_THREADS * rc.AGREE_BATCH * rc.GRID_QUAD
    sweep = blocks * per_block
    assert blocks == rc.AGREE_BLOCKS and sweep == rc.SWEEP
    assert int(H._L.dba_vote_agreement_blocks(sweep)) == blocks
    assert int(H._L.dba_vote_agreement_blocks(sweep - per_block)) == blocks - 1
    sum_blocks = int(H._L.dba_rlr_apply_blocks(1 << 40))                     # ... the other two passes'
    assert sum_blocks == rc.SUM_BLOCKS and sum_blocks * rc.GRID_THREADS * rc.GRID_QUAD == sweep
    assert int(H._L.dba_rlr_apply_blocks(sweep - rc.GRID_THREADS * rc.GRID_QUAD)) == sum_blocks - 1
    case = rc.wrap_case(sweep)
    assert int(H._L.dba_vote_agreement_blocks(case[1])) == blocks
    assert int(H._L.dba_rlr_apply_blocks(case[1])) == sum_blocks
    _check_case(case, dev)


def test_alignment_does_not_change_the_bits(dev):
    """The same rows at every offset from a 16-byte boundary, and gathered into an aligned copy."""
    from dba_mod_amd import ops
    n, L = 10, 1029
    rows, base = rc.make_case(n, L, L, 0)
    want = None
    for off in range(4):
        big = torch.zeros(n, L + 7, device=dev)
        big[:, off:off + L] = rows.to(dev)
        view = big[:, off:off + L]
        bb = torch.zeros(L + 4, device=dev)
        bb[off:off + L] = base.to(dev)
        b = bb[off:off + L]
        total, votes = ops.delta_sum_votes(view, b)
        counts = ops.vote_agreement(view, b, votes, rc.THETA)
        dst = bb.clone()[off:off + L]                                        # (as misaligned as the base)
        flipped = ops.rlr_apply(dst, total, votes, rc.THETA, cpu.COEF, cpu.SIGMA, cpu.SEED, True)
        got = (total, votes, counts, dst, flipped)
        if want is None:
            want = got
            rc.check_votes((total, votes), rows, base)
            rc.check_agreement(counts, rows, base, votes.cpu().numpy(), rc.THETA)
        assert _same(got, want), off
    # non-unit inner stride: the wrapper gathers the rows
    wide = torch.zeros(n, 2 * L, device=dev)
    wide[:, ::2] = rows.to(dev)
    assert _same(ops.delta_sum_votes(wide[:, ::2], base.to(dev)), want[:2])


def test_nonfinite_values_follow_ieee(dev):
    from dba_mod_amd import ops
    x, base = cpu.nonfinite_input()
    cpu.check_nonfinite(ops, x.to(dev), base.to(dev))
    # ... and in the middle of longer, misaligned rows, with negative-signed NaNs
    rows, b = rc.make_case(10, 3001, 3004, 1)
    rows, b = rows.clone(), b.clone()
    rows[8, 2047] = float("nan")
    rows[3, 2047] = -float("nan")
    rows[2, 2047] = float("inf")
    rows[5, 100] = -float("nan")
    rows[6, 3000] = float("-inf")
    b[7] = float("inf")
    rows[4, 7] = float("inf")
    b[9] = float("nan")
    big = torch.zeros(10, 3004, device=dev)
    big[:, 1:3002] = rows.to(dev)
    view, bd = big[:, 1:3002], b.to(dev)
    out = ops.delta_sum_votes(view, bd)
    want_v = rc.check_votes(out, rows, b)
    assert torch.equal(rc.bits(out[0]), rc.bits(ops.delta_sum(view, bd)))
    for theta in (1, rc.THETA, 10):
        rc.check_agreement(ops.vote_agreement(view, bd, out[1], theta), rows, b, want_v, theta)
        for noise in (False, True):
            rc.check_apply(ops, torch.ones(3001, device=dev), out[0], out[1], theta, cpu.COEF, cpu.SIGMA, cpu.SEED,
                           noise)


def test_degenerate_shapes_return_zeros(dev):
    from dba_mod_amd import ops
    cpu.check_degenerate(ops, dev)


def test_hand_case_fedavg_rlr(dev):
    from dba_mod_amd.fl import aggregate as agg
    finals = torch.tensor([[1.0, 1.0, -1.0, 5.0], [2.0, 2.0, -2.0, -5.0], [-6.0, 3.0, 0.0, 0.0]], device=dev)
    g = torch.zeros(4, device=dev)
    agree, dissent, flipped = agg.fedavg_rlr(g, finals, 2, 3.0, 3, False, 0.0, 1, 4)
    assert g.tolist() == [3.0, 6.0, -3.0, 0.0] and flipped == 2
    assert agree == [0.5, 0.5, 0.25] and dissent == [0.0, 0.0, 0.0]


def test_server_round_votes_against_the_attacker(dev, tmp_path):
    """The CPU test's round (MNIST synthetic, attacker 41 poisons in round 12 with scale 100) on the
    GPU with rlr_threshold = 4, twice: identical bits, the state and the shares equal to the
    oracle's, the attacker's agree share the strictly smallest and its dissent share the strictly
    largest."""
    outs = []
    for rep in range(2):
        res = trim_cpu.run_round(tmp_path / f"r{rep}", device=dev, rlr_threshold=rc.THETA)
        outs.append((res[1], res[3]))
        if rep == 0:
            cpu.check_round(res, rc.THETA)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert outs[0][1] == outs[1][1]

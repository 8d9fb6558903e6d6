"""SparseFed on the GPU: the radix select and the sparse apply of csrc/kernels/topk.hip against
the numpy oracle of topk_cases.py bit for bit (every case, each k twice on one workspace with other
k in between, a wrap of the launch grids, misaligned vectors, non-finite values, degenerate
inputs), ``topk_apply`` at full support against ``ops.add_noise_scaled``, the two-round hand case,
the equivalences with plain and norm-clipped FedAvg, and two rounds through ``Server``, twice."""
import pytest
import torch

import test_sparse_aggregation as cpu
import topk_cases as tk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", tk.SMALL_CASES)
def test_kernels_match_oracle(dev, name):
    from dba_mod_amd import ops
    assert ops.backend_name(dev) == "hip" and tk.workspace(ops, dev) is not None
    tk.check_case(ops, dev, name)


def test_wrap_case_wraps_the_grids(dev):
    """Three elements past one sweep of the apply grid (eight sweeps of the histogram grid): a thread's
    second step, the odd last element of the pairs and the partial last quad."""
    from dba_mod_amd import ops
    from dba_mod_amd.ops import hip as H
    apply_blocks = int(H._L.dba_topk_apply_blocks(1 << 40))               # the grids' maxima
    select_blocks = int(H._L.dba_topk_select_blocks(1 << 40))
    assert (apply_blocks, select_blocks) == (tk.APPLY_BLOCKS, tk.SELECT_BLOCKS)
    per_apply, per_select = tk.GRID_THREADS * tk.APPLY_QUAD, tk.GRID_THREADS * tk.SELECT_PAIR
    assert apply_blocks * per_apply == tk.SWEEP and select_blocks * per_select <= tk.SWEEP
    assert int(H._L.dba_topk_apply_blocks(tk.SWEEP)) == apply_blocks
    assert int(H._L.dba_topk_apply_blocks(tk.SWEEP - per_apply)) == apply_blocks - 1
    assert int(H._L.dba_topk_select_blocks(select_blocks * per_select - per_select)) == select_blocks - 1
    assert int(H._L.dba_topk_apply_blocks(1)) == 1 and int(H._L.dba_topk_select_blocks(1)) == 1
    L = tk.case(tk.WRAP_CASE)[0].size
    assert L == tk.SWEEP + 3 and int(H._L.dba_topk_apply_blocks(L)) == apply_blocks
    tk.check_case(ops, dev, tk.WRAP_CASE)


def test_workspace_needs_no_initialisation(dev):
    """A workspace full of ones, then one a select with another k and another vector has just used."""
    from dba_mod_amd import ops
    from dba_mod_amd.ops import hip as H
    resid0, total, dst0, ks = tk.case("ties")
    other = tk.case("wide")
    ws = H.topk_workspace(dev)
    assert ws.dtype == torch.int64 and ws.numel() == int(H._L.dba_topk_ws_words())
    for k in ks[:4]:
        want = tk.oracle(resid0, total, dst0, k)
        ws.fill_(-1)
        assert tk.run(ops, dev, resid0, total, dst0, k, ws)[3].tolist() == list(want[2:])
        tk.run(ops, dev, other[0], other[1], other[2], other[3][2], ws)
        assert tk.run(ops, dev, resid0, total, dst0, k, ws)[3].tolist() == list(want[2:])


def test_alignment_does_not_change_the_bits(dev):
    from dba_mod_amd import ops
    tk.check_offsets(ops, dev)


def test_degenerate_inputs(dev):
    from dba_mod_amd import ops
    tk.check_degenerate(ops, dev)


def test_matches_the_reference_ops_on_the_device(dev):
    """The torch implementation on the same device gives the same bits (the benchmark's comparison)."""
    from dba_mod_amd import ops
    from dba_mod_amd.ops import reference as R
    resid0, total, dst0, ks = tk.case("wide")
    for k in ks:
        a, b = tk.run(ops, dev, resid0, total, dst0, k), tk.run(R, dev, resid0, total, dst0, k)
        assert torch.equal(tk.bits(a[0]), tk.bits(b[0])) and torch.equal(tk.bits(a[1]), tk.bits(b[1]))
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_full_support_is_add_noise_scaled(dev):
    from dba_mod_amd import ops
    tk.check_full_support_is_fedavg(ops, dev, tk.COEF)
    tk.check_full_support_is_fedavg(ops, dev, 0.125)


def test_hand_case_two_rounds(dev):
    tk.check_hand_case(dev)


def test_full_support_round_is_fedavg_and_clip_norm(dev):
    cpu.check_equivalences(dev, 0.1)               # (eta / n = 0.01: a coefficient fp32 does not hold)


def test_server_rounds_equal_the_oracle(dev, tmp_path):
    """The CPU test's rounds 12 and 13 (MNIST synthetic, attacker 41 poisons in round 12 with scale
    100) on the GPU, twice: identical bits, and the state and the residual equal to the oracle's."""
    outs = []
    for rep in range(2):
        s, rec = cpu.run_rounds(tmp_path / f"r{rep}", device=dev, sparse_topk=cpu.FRAC)
        if rep == 0:
            cpu.check_rounds(s, rec)
        outs.append((tk.bits(s.global_state).clone(), tk.bits(s.sparse_residual).clone(),
                     [list(r) for r in s.csv.weight_result]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]

"""Coordinate-wise trimmed mean / median (config ``trim_k``) on CPU: the config key, the reference
op against the numpy oracle of trim_cases.py bit for bit, a hand case, non-finite client values,
the median against ``numpy.median``, a model-replacement round through ``Server``, the warm
start and world-size invariance."""
import csv
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import trim_cases as tc
from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")
# one sweep of the launch grid of csrc/kernels/coordrank.hpp (test_gpu_trim.py checks it against the kernel's own)
SWEEP = 512 * tc.GRID_THREADS * tc.GRID_QUAD
CASES = tc.SMALL_CASES + [tc.wrap_case(SWEEP), tc.FALLBACK_CASE]


# ------------------------------------------------------------------------------ config
def test_trim_defaults_and_accepts():
    assert C.Params()["trim_k"] is None and C.Params().trim_k is None
    for k in (1, 2, 4):
        assert C.Params({"no_models": 10, "trim_k": k}).trim_k == k
    assert C.Params({"trim_k": "median"}).trim_k == "median"
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")


@pytest.mark.parametrize("bad", [True, False, 0, -1, 1.5, 2.0, "2", "mean", [1]])
def test_trim_rejects_values(bad):
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "trim_k": bad})


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_trim_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({"trim_k": 1, "aggregation_methods": method})
    with pytest.raises(ValueError):
        C.Params({"trim_k": "median", "aggregation_methods": method})
    assert C.Params({"trim_k": None, "aggregation_methods": method}).trim_k is None


def test_trim_excludes_clip_norm_and_krum():
    with pytest.raises(ValueError):
        C.Params({"trim_k": 1, "clip_norm": 1.0})
    with pytest.raises(ValueError):
        C.Params({"trim_k": "median", "clip_norm": "median"})
    with pytest.raises(ValueError):
        C.Params({"trim_k": 1, "krum_f": 1})
    with pytest.raises(ValueError):
        C.Params({"trim_k": "median", "krum_f": 0})


def test_trim_size_inequality():
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "trim_k": 5})             # 10 < 2 * 5 + 1
    assert C.Params({"no_models": 11, "trim_k": 5}).trim_k == 5
    assert C.Params({"no_models": 10, "trim_k": 4}).trim_k == 4
    # ... and again against a round's actual client count
    assert agg.trim_count(10, 4) == 4 and agg.trim_count(9, 4) == 4
    with pytest.raises(ValueError):
        agg.trim_count(8, 4)
    assert [agg.trim_count(n, "median") for n in (1, 2, 9, 10)] == [0, 0, 4, 4]
    with pytest.raises(ValueError):
        agg.trim_count(0, "median")
    with pytest.raises(ValueError):
        agg.trim_count(10, None)


def test_shipped_recipe_loads():
    p = C.load_params(os.path.join(ROOT, "configs", "cifar_trim.yaml"))
    assert p.trim_k == 2 and p["aggregation_methods"] == "mean" and p.krum_f is None and p.clip_norm is None


# ------------------------------------------------------------------ the kernel's networks
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sorting_networks_sort(tmp_path):
    """The compile-time networks of csrc/kernels/sortnet.hpp that trim.hip instantiates, checked on
    the host: exhaustively by the 0-1 principle up to 16 inputs, on random inputs beyond."""
    exe = str(tmp_path / "sortnet_check")
    r = subprocess.run(["g++", "-O0", "-std=c++17", "-o", exe, os.path.join(ROOT, "csrc", "tests", "sortnet_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sortnet check OK" in r.stdout, r.stdout + r.stderr
    assert "N = 10:  29 comparators ok" in r.stdout


# ------------------------------------------------------- reference op vs the numpy oracle
@pytest.mark.parametrize("case", CASES, ids=tc.case_id)
def test_reference_op_matches_oracle(case):
    rows, base = tc.make_case(*case)
    k = case[4]
    tc.check(R.trimmed_delta_sum(rows, base, k), rows, base, k)
    tc.check(ops.trimmed_delta_sum(rows, base, k), rows, base, k)      # (the registered op, CPU dispatch)


def test_reference_op_row_idx():
    rows, base = tc.make_case(*tc.NINE_ROWS)
    idx = [7, 2, 5, 2, 8, 0]
    out = R.trimmed_delta_sum(rows, base, 2, idx)
    tc.check(out, rows[idx], base, 2)
    again = R.trimmed_delta_sum(rows, base, 2, torch.tensor(idx))
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_reference_op_degenerate_shapes():
    total, kept, high = R.trimmed_delta_sum(torch.randn(0, 7), torch.randn(7), 0)
    assert total.dtype == torch.float64 and tuple(total.shape) == (7,) and not total.any()
    assert kept.dtype == torch.int64 and high.dtype == torch.int64 and kept.numel() == 0 and high.numel() == 0
    total, kept, high = R.trimmed_delta_sum(torch.randn(4, 0), torch.randn(0), 1)
    assert tuple(total.shape) == (0,) and kept.tolist() == [0] * 4 and high.tolist() == [0] * 4
    total, kept, high = R.trimmed_delta_sum(torch.randn(4, 7), torch.randn(7), 0, [])
    assert tuple(total.shape) == (7,) and not total.any() and kept.numel() == 0


@pytest.mark.parametrize("n,k", [(4, 2), (5, 3), (3, -1), (3, True), (3, 1.0)])
def test_reference_op_rejects_k(n, k):
    with pytest.raises(ValueError):
        R.trimmed_delta_sum(torch.randn(n, 3), torch.randn(3), k)


# --------------------------------------------------------------------------- hand case
def test_hand_case_fedavg_trimmed():
    """n = 5, k = 1, eta = 3 (so eta / (n - 2 k) = 1 exactly).  Column 0 around 0: 0 is cut low, 100
    high, 1 + 2 + 3 = 6 stay.  Column 1 around 1: -2 is cut low, 4 high, (1 - 1) + (2 - 1) + (3 - 1)
    = 3 stay."""
    finals = torch.tensor([[0.0, 4.0], [1.0, -2.0], [2.0, 1.0], [3.0, 2.0], [100.0, 3.0]])
    g = torch.tensor([0.0, 1.0])
    kept, high = agg.fedavg_trimmed(g, finals, 1, 3.0, False, 0.0, 1, 2)
    assert g.tolist() == [6.0, 4.0]
    assert kept == [0.0, 0.5, 1.0, 1.0, 0.5]
    assert high == [0.5, 0.0, 0.0, 0.0, 0.5]
    # the median of the same clients: column 0 -> 2, column 1 -> 1 + (2 - 1)
    g = torch.tensor([0.0, 1.0])
    kept, high = agg.fedavg_trimmed(g, finals, "median", 1.0, False, 0.0, 1, 2)
    assert g.tolist() == [2.0, 2.0]
    assert kept == [0.0, 0.0, 0.5, 0.5, 0.0] and high == [0.5, 0.0, 0.0, 0.5, 1.0]


# -------------------------------------------------------------------------- non-finite
def nonfinite_input():
    """Six clients, four coordinates, base 0: one NaN client at coordinate 0, two at coordinate 1,
    a +inf and a -inf client at coordinate 2, nothing special at coordinate 3."""
    x = torch.tensor([[1.0, 1.0, 1.0, 1.0],
                      [2.0, 2.0, 2.0, 2.0],
                      [float("nan"), float("nan"), float("inf"), 3.0],
                      [4.0, float("nan"), float("-inf"), 4.0],
                      [5.0, 5.0, 5.0, 5.0],
                      [6.0, 6.0, 6.0, 6.0]])
    return x, torch.zeros(4)


def check_nonfinite(total, kept, high):
    total, kept, high = total.cpu(), kept.cpu(), high.cpu()
    # coordinate 0: sorted 1 2 4 5 6 NaN, k = 1 -> 2 + 4 + 5 + 6; the NaN client counts high
    assert float(total[0]) == 17.0
    # coordinate 1: sorted 1 2 5 6 NaN NaN, k = 1 -> a NaN reaches the total
    assert bool(torch.isnan(total[1]))
    # coordinate 2: sorted -inf 1 2 5 6 inf -> both are cut
    assert float(total[2]) == 14.0
    assert float(total[3]) == 14.0
    # kept / high per client over the 4 coordinates.  Coordinate 0: lo 2, hi 6, client 0 low, the
    # NaN client 2 high.  Coordinate 1: lo 2, hi NaN, so nobody is high and client 0 is low.
    # Coordinate 2: lo 1, hi 6, client 2 (+inf) high, client 3 (-inf) low.  Coordinate 3: lo 2, hi 5,
    # client 0 low, client 5 high
    assert kept.tolist() == [1, 4, 2, 3, 4, 3]
    assert high.tolist() == [0, 0, 2, 0, 0, 1]


def test_nonfinite_values_follow_ieee():
    x, base = nonfinite_input()
    out = R.trimmed_delta_sum(x, base, 1)
    check_nonfinite(*out)
    tc.check(out, x, base, 1)


# ------------------------------------------------------------------------------ median
@pytest.mark.parametrize("n", [9, 10])
def test_median_equals_numpy_median(n):
    rows, base = tc.make_case(n, 1001, 1001, 0)
    k = agg.trim_count(n, "median")
    total, _, _ = R.trimmed_delta_sum(rows, base, k)
    deltas = rows.numpy().astype(np.float64) - base.numpy().astype(np.float64)[None]
    # n - 2 k is 1 (odd n) or 2 (even n: numpy takes the mean of the two middle deltas, and halving is exact)
    assert np.array_equal(total.numpy() / (n - 2 * k), np.median(deltas, axis=0))


@pytest.mark.parametrize("n,k", [(9, 4), (10, 4), (10, 2), (7, 0)])
def test_counts_without_ties(n, k):
    g = torch.Generator().manual_seed(n * 31 + k)
    rows = torch.randn(n, 513, generator=g)
    assert all(np.unique(col).size == n for col in rows.numpy().T)
    _, kept, high = R.trimmed_delta_sum(rows, torch.zeros(513), k)
    assert int(kept.sum()) == (n - 2 * k) * 513 and int(high.sum()) == k * 513
    assert int((513 - kept - high).sum()) == k * 513


# --------------------------------------------------------------------- through the Server
def mnist_params(tmp, **kw):
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 4000,
            "synthetic_test_size": 600, "save_dir": str(tmp), "eval_batch_size": 300}
    base.update(kw)
    return C.load_params(CFG, base)


class Recorder:
    """Wraps ``Server._aggregate`` to keep the round's client final states (the bank rows)."""

    def __init__(self, server):
        self.finals = None
        inner = server._aggregate

        def wrapped(plan, bank, local, adversarial):
            self.finals = bank[[c.final_snap for c in plan.clients]].clone()
            return inner(plan, bank, local, adversarial)
        server._aggregate = wrapped


def run_round(tmp, device=None, **kw):
    """Round 12 (attacker 41 poisons, scale 100): (before, after, finals, weight rows, n_upd, params)."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = mnist_params(tmp, **kw)
    s = Server(p, DistCtx() if device is None else DistCtx(device=device), write_outputs=False)
    rec = Recorder(s)
    before = s.global_state.clone()
    s.run_round(12)
    n_upd = s.spec.S if p["aggregate_bn_buffers"] else s.spec.P
    return before, s.global_state.clone(), rec.finals, [list(r) for r in s.csv.weight_result], n_upd, p


def check_round(result, k):
    """The attacker's kept share is the strictly smallest, the model moved, and the new global
    state is ``before`` with the oracle's total applied through ``ops.add_noise_scaled``."""
    before, after, finals, wr, n_upd, p = result
    assert len(wr) == 3
    names, kept, high = wr
    n = len(names)
    assert len(kept) == n and len(high) == n
    print(f"names {names}\nkept share {kept}\nhigh share {high}")
    i = names.index(41)
    assert all(kept[i] < v for j, v in enumerate(kept) if j != i)
    assert all(0.0 <= a <= 1.0 and 0.0 <= b <= 1.0 and a + b <= 1.0 for a, b in zip(kept, high))
    assert not torch.equal(after[:n_upd], before[:n_upd])
    assert torch.equal(after[n_upd:], before[n_upd:])
    rows = finals[:, :n_upd].cpu()
    total, want_kept, want_high = tc.oracle(rows.numpy(), before[:n_upd].cpu().numpy(), k)
    want = before.clone()
    dp_seed = (int(p["seed"]) * 7919 + 12) & 0x7FFFFFFF
    ops.add_noise_scaled(want[:n_upd], torch.from_numpy(total).to(want.device), float(p["eta"]) / (n - 2 * k),
                         float(p["sigma"]), dp_seed, bool(p["diff_privacy"]))
    assert torch.equal(after, want)
    assert kept == [float(v) / n_upd for v in want_kept.tolist()]
    assert high == [float(v) / n_upd for v in want_high.tolist()]


@pytest.fixture(scope="module")
def trim_round(tmp_path_factory):
    return run_round(tmp_path_factory.mktemp("trim"), trim_k=2)


def test_server_round_cuts_the_attacker(trim_round):
    check_round(trim_round, 2)


def test_pretrain_stays_plain_fedavg(tmp_path):
    """The benign warm start runs with trim_k cleared and puts it back."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = mnist_params(tmp_path, trim_k="median")
    s = Server(p, DistCtx(), write_outputs=False)
    seen = []
    inner = s._aggregate

    def wrapped(plan, bank, local, adversarial):
        seen.append(s.params["trim_k"])
        return inner(plan, bank, local, adversarial)
    s._aggregate = wrapped
    s.pretrain(1)
    assert seen == [None]
    assert s.params.trim_k == "median"
    assert not s.csv.weight_result                # (plain FedAvg records no weights)


def weight_rows(folder):
    with open(os.path.join(folder, "run", "weight_result.csv")) as f:
        return list(csv.reader(f))


def test_world_size_invariance(tmp_path):
    """trim_k = 2 at worlds 1, 2, 4: every rank of every world holds the same final rows after the
    gather and runs the same pass over them, so the same state bits and weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "trim_k": 2}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    i = rows1[0].index("41")
    assert all(float(rows1[1][i]) < float(v) for j, v in enumerate(rows1[1]) if j != i)
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert weight_rows(str(tmp_path / f"w{world}")) == rows1

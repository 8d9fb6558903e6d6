"""Multi-Krum (config ``krum_f`` / ``krum_m``) on CPU: the config keys, scores and selection on a
hand case, non-finite client states, the reference pairwise-distance op against a numpy fp64
oracle, a model-replacement round through ``Server`` and world-size invariance."""
import csv
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import krum_cases as kc
from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")


# ------------------------------------------------------------------------------ config
def test_krum_defaults_and_accepts():
    assert C.Params()["krum_f"] is None and C.Params().krum_f is None
    assert C.Params()["krum_m"] is None and C.Params().krum_m is None
    for f in (0, 1, 3):
        assert C.Params({"krum_f": f}).krum_f == f
    p = C.Params({"krum_f": 1, "krum_m": 1})
    assert p.krum_f == 1 and p.krum_m == 1
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")


@pytest.mark.parametrize("bad", [True, -1, 1.5, "2"])
def test_krum_rejects_values(bad):
    with pytest.raises(ValueError):
        C.Params({"krum_f": bad})
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "krum_m": bad})


def test_krum_m_zero_is_out_of_range():
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "krum_m": 0})


def test_krum_m_needs_krum_f():
    with pytest.raises(ValueError):
        C.Params({"krum_m": 2})


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_krum_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "aggregation_methods": method})
    assert C.Params({"krum_f": None, "aggregation_methods": method}).krum_f is None


def test_krum_excludes_clip_norm():
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "clip_norm": 1.0})
    with pytest.raises(ValueError):
        C.Params({"krum_f": 0, "clip_norm": "median"})


def test_krum_size_inequalities():
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "krum_f": 4})             # 10 < 2 * 4 + 3
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "krum_f": 2, "krum_m": 9})  # 9 > 10 - 2
    assert C.Params({"no_models": 10, "krum_f": 2, "krum_m": 8}).krum_m == 8
    assert C.Params({"no_models": 11, "krum_f": 4}).krum_f == 4


# --------------------------------------------------------------------------- hand case
HAND = torch.tensor([[0.0], [1.0], [2.0], [3.0], [100.0]])


def test_hand_case_scores_and_selection():
    D = ops.pairwise_sq_dists(HAND)
    scores = agg.krum_scores(D, 1)
    assert scores.dtype == torch.float64
    assert scores.tolist() == [5.0, 2.0, 2.0, 5.0, float(97 ** 2 + 98 ** 2)]
    assert agg.krum_select(scores, 1) == [1]                  # the tie goes to the lower index
    assert agg.krum_select(scores, 4) == [0, 1, 2, 3]


def test_hand_case_fedavg_krum():
    g = torch.zeros(1)
    mask, scores = agg.fedavg_krum(g, HAND, 1, None, 1.0, False, 0.0, 1, 1)
    assert mask == [1.0, 1.0, 1.0, 1.0, 0.0]                  # default m = n - f = 4
    assert scores == [5.0, 2.0, 2.0, 5.0, float(97 ** 2 + 98 ** 2)]
    assert g.tolist() == [1.5]
    g = torch.zeros(1)
    mask, _ = agg.fedavg_krum(g, HAND, 1, 1, 1.0, False, 0.0, 1, 1)
    assert mask == [0.0, 1.0, 0.0, 0.0, 0.0] and g.tolist() == [1.0]


# -------------------------------------------------------------------------- non-finite
def test_nan_client_is_never_selected():
    g = torch.Generator().manual_seed(5)
    finals = torch.randn(6, 200, generator=g)
    finals[2, 17] = float("nan")
    D = ops.pairwise_sq_dists(finals)
    off = [j for j in range(6) if j != 2]
    assert torch.isnan(D[2, off]).all() and torch.isfinite(D[off][:, off]).all()
    scores = agg.krum_scores(D, 1)
    assert scores[2] == float("inf") and torch.isfinite(scores[off]).all()
    for m in (1, 5, 6):
        sel = agg.krum_select(scores, m)
        assert 2 not in sel and len(sel) == min(m, 5)
    gl = torch.zeros(200)
    mask, _ = agg.fedavg_krum(gl, finals, 1, None, 1.0, False, 0.0, 1, 200)
    assert mask[2] == 0.0 and torch.isfinite(gl).all()


def test_all_nan_raises():
    finals = torch.full((5, 10), float("nan"))
    scores = agg.krum_scores(ops.pairwise_sq_dists(finals), 1)
    assert all(s == float("inf") for s in scores.tolist())
    with pytest.raises(RuntimeError):
        agg.krum_select(scores, 4)
    with pytest.raises(RuntimeError):
        agg.fedavg_krum(torch.zeros(10), finals, 1, None, 1.0, False, 0.0, 1, 10)


# ------------------------------------------------------- reference op vs the numpy oracle
@pytest.mark.parametrize("case", kc.CASES + [kc.FALLBACK_CASE], ids=kc.case_id)
def test_reference_op_matches_oracle(case):
    rows = kc.make_case(*case)
    D = R.pairwise_sq_dists(rows)
    kc.check(D, rows)
    assert torch.equal(D, R.pairwise_sq_dists(rows))


def test_reference_op_row_idx():
    rows = kc.make_case(9, 1001, 1001, 0)
    idx = [7, 2, 2, 5]
    D = R.pairwise_sq_dists(rows, idx)
    assert torch.equal(D, R.pairwise_sq_dists(rows[idx]))
    assert float(D[1, 2]) == 0.0
    full = kc.oracle(rows)
    np.testing.assert_allclose(D.numpy(), full[np.ix_(idx, idx)], rtol=1003 * 2.0 ** -52, atol=0)
    assert torch.equal(D, R.pairwise_sq_dists(rows, torch.tensor(idx)))


def test_reference_op_empty_and_single():
    for n in (0, 1):
        D = R.pairwise_sq_dists(torch.randn(n, 7))
        assert D.dtype == torch.float64 and tuple(D.shape) == (n, n) and not D.any()
    D = R.pairwise_sq_dists(torch.randn(4, 0))
    assert tuple(D.shape) == (4, 4) and not D.any()
    D = R.pairwise_sq_dists(torch.randn(4, 7), [])
    assert tuple(D.shape) == (0, 0)


# --------------------------------------------------------------------- through the Server
def _mnist_params(tmp, **kw):
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 4000,
            "synthetic_test_size": 600, "save_dir": str(tmp), "eval_batch_size": 300}
    base.update(kw)
    return C.load_params(CFG, base)


class _Recorder:
    """Wraps ``Server._aggregate`` to keep the round's client final states (the bank rows)."""

    def __init__(self, server):
        self.finals = None
        inner = server._aggregate

        def wrapped(plan, bank, local, adversarial):
            self.finals = bank[[c.final_snap for c in plan.clients]].clone()
            return inner(plan, bank, local, adversarial)
        server._aggregate = wrapped


def _round(tmp, **kw):
    """Round 12 (attacker 41 poisons, scale 100): (before, after, finals, weight rows, n_upd, params)."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = _mnist_params(tmp, **kw)
    s = Server(p, DistCtx(), write_outputs=False)
    rec = _Recorder(s)
    before = s.global_state.clone()
    s.run_round(12)
    n_upd = s.spec.S if p["aggregate_bn_buffers"] else s.spec.P
    return before, s.global_state.clone(), rec.finals, [list(r) for r in s.csv.weight_result], n_upd, p


@pytest.fixture(scope="module")
def krum_round(tmp_path_factory):
    return _round(tmp_path_factory.mktemp("krum"), krum_f=1)


def test_server_drops_the_attacker(krum_round):
    _, _, _, wr, _, _ = krum_round
    names, mask, scores = wr
    i = names.index(41)
    print(f"mask {mask}; scores {scores}")
    assert mask[i] == 0.0
    assert scores[i] == max(scores) and all(scores[i] > s for j, s in enumerate(scores) if j != i)
    assert sum(mask) == len(names) - 1 and set(mask) == {0.0, 1.0}       # m = n - f, f = 1


def test_server_update_is_the_selected_mean(krum_round):
    """after - before = (eta / m) * sum of the selected deltas, recomputed in fp64 from the round's
    snapshots.  The server rounds the fp64 update to fp32 once and adds it to the fp32 model:
    two fp32 roundings, each at most half an ulp of its result, so one ulp of the larger of
    |update| and |after| bounds the error."""
    before, after, finals, wr, n_upd, p = krum_round
    names, mask, _ = wr
    sel = [j for j, v in enumerate(mask) if v == 1.0]
    delta = (finals[sel].double() - before.double()[None]).sum(0)[:n_upd]
    upd = delta * (float(p["eta"]) / len(sel))
    want = before.double().clone()
    want[:n_upd] += upd
    err = (after.double() - want).abs().numpy()
    big = np.maximum(np.abs(after.numpy()), np.abs(want.numpy())).astype(np.float32)
    ulp = np.spacing(big).astype(np.float64)
    ulp[:n_upd] = np.maximum(ulp[:n_upd], np.spacing(np.abs(upd.numpy()).astype(np.float32)))
    print(f"max err / ulp {np.max(err / ulp):.3f}")
    assert np.all(err <= ulp)
    assert torch.equal(after[n_upd:], before[n_upd:])
    assert not torch.equal(after[:n_upd], before[:n_upd])


def test_server_f0_full_m_selects_everyone(tmp_path):
    p0 = _mnist_params(tmp_path / "probe")
    n = int(p0["no_models"])
    _, _, _, wr, _, _ = _round(tmp_path / "all", krum_f=0, krum_m=n)
    assert len(wr[0]) == n and wr[1] == [1.0] * n


def test_pretrain_stays_plain_fedavg(tmp_path):
    """The benign warm start runs with krum_f / krum_m cleared and puts them back."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = _mnist_params(tmp_path, krum_f=1, krum_m=2)
    s = Server(p, DistCtx(), write_outputs=False)
    seen = []
    inner = s._aggregate

    def wrapped(plan, bank, local, adversarial):
        seen.append((s.params["krum_f"], s.params["krum_m"]))
        return inner(plan, bank, local, adversarial)
    s._aggregate = wrapped
    s.pretrain(1)
    assert seen == [(None, None)]
    assert s.params.krum_f == 1 and s.params.krum_m == 2
    assert not s.csv.weight_result                # (plain FedAvg records no weights)


def _weight_rows(folder):
    with open(os.path.join(folder, "run", "weight_result.csv")) as f:
        return list(csv.reader(f))


def test_world_size_invariance(tmp_path):
    """krum_f = 1 at worlds 1, 2, 4: every rank of every world holds the same final rows after the
    gather and runs the same kernel over them, so the same state bits and weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "krum_f": 1}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = _weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    assert float(rows1[1][rows1[0].index("41")]) == 0.0
    assert sum(float(v) for v in rows1[1]) == len(rows1[0]) - 1
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert _weight_rows(str(tmp_path / f"w{world}")) == rows1

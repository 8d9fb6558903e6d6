"""Norm-clipped FedAvg (config ``clip_norm``) on CPU: the config key, the clip factors, the
reference ops against a numpy fp64 oracle, the order-free limb partials, the update-norm
invariant of a model-replacement round through ``Server``, the large-bound equivalence with plain
FedAvg, world-size invariance and the non-finite fallback."""
import csv
import math
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import clip_cases as cc
from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")


# ------------------------------------------------------------------------------ config
@pytest.mark.parametrize("bad", [0, -1, float("inf"), "mean", [1]])
def test_clip_norm_rejects(bad):
    with pytest.raises(ValueError):
        C.Params({"clip_norm": bad})


def test_clip_norm_accepts_and_defaults():
    assert C.Params()["clip_norm"] is None and C.Params().clip_norm is None
    assert C.Params({"clip_norm": 1}).clip_norm == 1.0
    assert C.Params({"clip_norm": 2.5}).clip_norm == 2.5
    assert C.Params({"clip_norm": "median"}).clip_norm == "median"
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_clip_norm_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({"clip_norm": 1.0, "aggregation_methods": method})
    assert C.Params({"clip_norm": None, "aggregation_methods": method}).clip_norm is None


# ------------------------------------------------------------------------ clip factors
def test_clip_factors_hand_cases():
    sq = torch.tensor([0.25, 4.0, 0.0, 100.0, 1.0], dtype=torch.float64)      # norms .5 2 0 10 1
    f, bound = agg.clip_factors(sq, 1.0)
    assert bound == 1.0 and f.dtype == torch.float64
    assert f.tolist() == [1.0, 0.5, 1.0, 0.1, 1.0]             # below, above, zero norm, above, at the bound
    # lower median of an even count: sorted norms [1, 2, 3, 10] -> index (4 - 1) // 2 = 1 -> 2
    f, bound = agg.clip_factors(torch.tensor([9.0, 100.0, 1.0, 4.0], dtype=torch.float64), "median")
    assert bound == 2.0 and f.tolist() == [2.0 / 3.0, 0.2, 1.0, 1.0]
    # odd count: the middle one
    f, bound = agg.clip_factors(torch.tensor([9.0, 1.0, 4.0], dtype=torch.float64), "median")
    assert bound == 2.0 and f.tolist() == [2.0 / 3.0, 1.0, 1.0]
    # a median of zero (most clients returned the global model): the others are clipped to nothing
    f, bound = agg.clip_factors(torch.tensor([0.0, 0.0, 4.0], dtype=torch.float64), "median")
    assert bound == 0.0 and f.tolist() == [1.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        agg.clip_factors(sq, "mean")


# ------------------------------------------------------- reference ops vs the numpy oracle
@pytest.mark.parametrize("case", cc.SMALL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_reference_ops_match_oracle(case):
    rows, base, scale = cc.make_case(*case)
    n = rows.shape[0]
    sq, mx = R.delta_stats(rows, base)
    cc.check_stats(sq, mx, rows, base, scale)
    sq2, _ = R.delta_stats(rows, base)
    assert torch.equal(sq, sq2)
    E = cc.exponent(mx.numpy(), n)
    limbs = R.clipped_delta_sum_fixed(rows, base, scale, E)
    assert limbs.dtype == torch.int64 and tuple(limbs.shape) == (2, base.numel())
    if base.numel() > 1:
        assert int(limbs[0].min()) < 0                        # negative deltas give negative hi limbs
    cc.check_decoded(limbs, E, rows, base, scale)
    cc.check_fp64(R.clipped_delta_sum(rows, base, scale), rows, base, scale)
    # the stats do not depend on which other rows share the call
    sq1, mx1 = R.delta_stats(rows[:1], base)
    assert torch.equal(sq1, sq[:1]) and torch.equal(mx1, mx[:1])


def test_reference_ops_empty():
    base = torch.randn(7)
    sq, mx = R.delta_stats(torch.zeros(0, 7), base)
    assert sq.shape == (0,) and mx.shape == (0,)
    assert torch.equal(R.clipped_delta_sum_fixed(torch.zeros(0, 7), base, torch.zeros(0), 3),
                       torch.zeros(2, 7, dtype=torch.int64))
    assert torch.equal(R.clipped_delta_sum(torch.zeros(0, 7), base, torch.zeros(0)),
                       torch.zeros(7, dtype=torch.float64))


def test_limb_partials_are_order_free():
    """Any split of the clients into rank partials (int64 limb sums, then added) gives the SAME
    limbs as one pass: what makes the clipped aggregate world-invariant."""
    rows, base, scale = cc.make_case(7, 1001, 1001, 0)
    _, mx = R.delta_stats(rows, base)
    E = cc.exponent(mx.numpy(), 7)
    full = R.clipped_delta_sum_fixed(rows, base, scale, E)
    for parts in ([[0, 1, 2], [3, 4, 5, 6]], [[i] for i in range(7)], [[6, 2], [0, 5], [1, 3, 4]]):
        tot = sum(R.clipped_delta_sum_fixed(rows[p], base, scale[p], E) for p in parts)
        assert torch.equal(tot, full)


# ------------------------------------------------------------- aggregation (single rank)
def test_fedavg_clipped_bounds_the_update_and_matches_fedavg_when_unclipped():
    g = torch.Generator().manual_seed(3)
    gl = torch.randn(500, generator=g)
    finals = gl[None] + torch.randn(6, 500, generator=g) * 0.01
    finals[2] = gl + (finals[2] - gl) * 100.0                # a model-replacement client
    g1 = gl.clone()
    factors, norms = agg.fedavg_clipped(g1, finals, 0.5, 1.0, 6, False, 0.0, 1, 400)
    assert torch.equal(g1[400:], gl[400:])
    assert factors[2] < 0.05 and all(f == 1.0 for i, f in enumerate(factors) if i != 2)
    assert float((g1.double() - gl.double()).norm()) <= 1.0 * (6 / 6) * 0.5 * (1 + 1e-6)
    # nothing clipped: plain FedAvg within one fp32 ulp per element
    g2, g3 = gl.clone(), gl.clone()
    agg.fedavg_clipped(g2, finals, 1e30, 0.1, 10, False, 0.0, 1, 500)
    agg.fedavg(g3, finals, 0.1, 10, False, 0.0, 1, 500)
    assert np.all(np.abs(g2.numpy() - g3.numpy()) <= np.spacing(np.maximum(np.abs(g2.numpy()), np.abs(g3.numpy()))))


def test_non_finite_update_takes_the_fp64_sum_and_reaches_the_model():
    """A NaN client update cannot be put on the fixed grid: the stats flag it (NaN squared norm,
    max |delta| = +inf), the exponent is None, and the fp64 sum carries the NaN into the global
    model (nan_check then aborts the round), as in tests/test_aggregation.py for RFA."""
    g = torch.zeros(300)
    finals = torch.randn(4, 300)
    finals[2, 7] = float("nan")
    sq, mx = R.delta_stats(finals, g)
    assert torch.isnan(sq[2]) and torch.isfinite(sq[[0, 1, 3]]).all()
    assert float(mx[2]) == float("inf") and torch.isfinite(mx[[0, 1, 3]]).all()
    assert agg.fixed_exponent(agg.max_abs(mx), 4) is None
    part = agg.clipped_part(finals, g, torch.ones(4), None)
    assert part.dtype == torch.float64 and tuple(part.shape) == (300,) and torch.isnan(part[7])
    for clip in (1.0, "median"):
        gg = g.clone()
        agg.fedavg_clipped(gg, finals, clip, 1.0, 4, False, 0.0, 1, 300)
        assert torch.isnan(gg).any()
    # an Inf delta too
    finals[2, 7] = float("inf")
    gg = g.clone()
    agg.fedavg_clipped(gg, finals, 1.0, 1.0, 4, False, 0.0, 1, 300)
    assert not torch.isfinite(gg).all()


# --------------------------------------------------------------------- through the Server
def _mnist_params(tmp, **kw):
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 4000,
            "synthetic_test_size": 600, "save_dir": str(tmp), "eval_batch_size": 300}
    base.update(kw)
    return C.load_params(CFG, base)


# The fixed bound of the invariant test.  Round 12 of this setup (attacker 41 poisons, scale 100):
# the nine benign update norms are 0.055 .. 0.148 and the attacker's 24.2 (0.242 before scaling,
# more than a tenth of the largest benign norm), so C = 0.15 clips the attacker alone and plain
# FedAvg's update (norm 0.241) is 16x the bound eta * (n / no_models) * C = 0.015.
CLIP_C = 0.15


@pytest.fixture(scope="module")
def poison_round(tmp_path_factory):
    """Round 12 of the tests/test_e2e_cpu.py MNIST setup for clip_norm None / C / 1e30:
    {clip: (global before, global after, weight_result rows, n_update, params)}."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    out = {}
    for clip in (None, CLIP_C, 1e30):
        p = _mnist_params(tmp_path_factory.mktemp("clip"), clip_norm=clip)
        s = Server(p, DistCtx(), write_outputs=False)
        before = s.global_state.clone()
        s.run_round(12)
        n_upd = s.spec.S if p["aggregate_bn_buffers"] else s.spec.P
        out[clip] = (before, s.global_state.clone(), [list(r) for r in s.csv.weight_result], n_upd, p)
    return out


def _update_norm(run):
    before, after, _, n_upd, _ = run
    return float((after.double() - before.double())[:n_upd].norm())


def test_server_update_norm_invariant(poison_round):
    _, _, wr, _, p = poison_round[CLIP_C]
    names, factors, norms = wr
    n = len(names)
    bound = float(p["eta"]) * (n / int(p["no_models"])) * CLIP_C * (1 + 1e-6)
    got = _update_norm(poison_round[CLIP_C])
    plain = _update_norm(poison_round[None])
    print(f"update norm: clipped {got:.6g}, plain FedAvg {plain:.6g}, bound {bound:.6g}; norms {norms}")
    assert got <= bound
    assert plain > bound                     # the same round without the feature violates it
    assert poison_round[None][2] == []       # and records no weights
    i = names.index(41)
    others = [f for j, f in enumerate(factors) if j != i]
    assert factors[i] < 0.1 * min(others), (factors[i], others)
    assert norms[i] * factors[i] <= CLIP_C * (1 + 1e-6)
    assert all(f == 1.0 if nr <= CLIP_C else f < 1.0 for f, nr in zip(factors, norms))


def test_server_large_bound_is_plain_fedavg(poison_round):
    _, after, wr, _, _ = poison_round[1e30]
    assert wr[1] == [1.0] * len(wr[0])       # no client clipped
    a, b = after.numpy(), poison_round[None][1].numpy()
    assert np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b))))
    assert not np.array_equal(after.numpy(), poison_round[None][0].numpy())


def _weight_rows(folder):
    with open(os.path.join(folder, "run", "weight_result.csv")) as f:
        return list(csv.reader(f))


def test_world_size_invariance(tmp_path):
    """clip_norm = median at worlds 1, 2, 4: the same bits on every rank of every world (exact
    all-reduces of the squared norms and of the int64 limbs) and the same weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "clip_norm": "median"}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = _weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    assert sum(1 for f in rows1[1] if float(f) < 1.0) >= 1
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert _weight_rows(str(tmp_path / f"w{world}")) == rows1
        S = one[0]["S"]
        ar = many[0]["comm"][0][0]
        assert ar >= 2 * S * 8 and math.isfinite(ar)       # the int64 limb all-reduce: 16 B / element

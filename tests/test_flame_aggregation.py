"""FLAME (config ``clip_norm: median`` with ``clip_flame``) on CPU: the config keys, the reference
Gram op against a numpy fp64 oracle, the admission rule on hand cases and against sklearn's HDBSCAN
with the paper's parameters, the whole rule on planted data, a model-replacement round through
``Server`` and world-size invariance."""
import math
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import flame_cases as fc
import test_aggregation_collectives as collectives
import test_trim_aggregation as trim_cpu
from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")
FLAME = {"clip_norm": "median", "clip_flame": True}


# ------------------------------------------------------------------------------ config
def test_flame_defaults_and_accepts():
    p = C.Params()
    assert p["clip_flame"] is None and p.clip_flame is None
    assert p["clip_flame_lambda"] is None and p.clip_flame_lambda is None
    p = C.Params(FLAME)
    assert p.clip_flame is True and p.clip_norm == "median" and p.clip_flame_lambda is None
    assert p.flame_lambda == 0.001 == C.FLAME_LAMBDA
    for lam in (0, 0.0, 0.01, 3):
        q = C.Params({**FLAME, "clip_flame_lambda": lam})
        assert q.clip_flame_lambda == float(lam) and q.flame_lambda == float(lam)
    assert C.Params({**FLAME, "no_models": 3}).clip_flame is True
    assert C.mean_option(C.Params(FLAME)).key == "clip_norm"
    assert "clip_flame" in C.MEAN_OPTION_KEYS and "clip_flame_lambda" in C.MEAN_OPTION_KEYS


def test_flame_off_leaves_clip_norm_alone():
    """``clip_norm: median`` without the new keys is what it was: the same option entry (it does not
    gather, it has no size rule), the same values; ``false`` reads as off, with or without clip_norm."""
    p = C.Params({"clip_norm": "median"})
    assert p.clip_norm == "median" and p.clip_flame is None and p.clip_flame_lambda is None
    opt = C.mean_option(p)
    assert opt.key == "clip_norm" and opt.gathers is False and opt.sizes is None
    assert C.MEAN_OPTIONS[0] == C.MeanOption("clip_norm", ("clip_flame", "clip_flame_lambda"), False, None)
    assert C.MEAN_OPTIONS[-1] == C.MeanOption("sparse_topk", ("sparse_clip",), False, None)
    assert len(C.MeanOption._fields) == 4
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")
    for off in (None, False):
        assert C.Params({"clip_norm": "median", "clip_flame": off}).clip_flame is None
        assert C.Params({"clip_norm": 2.5, "clip_flame": off}).clip_norm == 2.5
        assert C.Params({"clip_flame": off}).clip_flame is None
    assert C.Params({"clip_norm": "median", "diff_privacy": True}).clip_norm == "median"
    assert C.Params({"clip_norm": "median", "no_models": 2}).clip_norm == "median"


def test_flame_needs_clip_norm():
    with pytest.raises(ValueError, match=r"^clip_flame is set without clip_norm$"):
        C.Params({"clip_flame": True})
    with pytest.raises(ValueError, match="clip_flame_lambda is set without"):
        C.Params({"clip_flame_lambda": 0.01})


@pytest.mark.parametrize("clip", [1.0, 5, 0.25])
def test_flame_rejects_a_numeric_clip_norm(clip):
    with pytest.raises(ValueError, match="clip_flame needs clip_norm"):
        C.Params({"clip_norm": clip, "clip_flame": True})


@pytest.mark.parametrize("bad", [1, 0, 1.0, "true", "yes", [True], "median"])
def test_flame_rejects_values(bad):
    with pytest.raises(ValueError, match="clip_flame"):
        C.Params({"clip_norm": "median", "clip_flame": bad})


@pytest.mark.parametrize("flame", [None, False])
def test_flame_lambda_needs_flame_on(flame):
    with pytest.raises(ValueError, match="clip_flame_lambda is set without clip_flame: true"):
        C.Params({"clip_norm": "median", "clip_flame": flame, "clip_flame_lambda": 0.01})


@pytest.mark.parametrize("bad", [True, False, "0.001", [0.001], -0.001, -1, math.inf, -math.inf, math.nan])
def test_flame_lambda_rejects_values(bad):
    with pytest.raises(ValueError, match="clip_flame_lambda"):
        C.Params({**FLAME, "clip_flame_lambda": bad})


def test_flame_excludes_diff_privacy():
    with pytest.raises(ValueError, match="clip_flame cannot be combined with diff_privacy"):
        C.Params({**FLAME, "diff_privacy": True})


@pytest.mark.parametrize("n", [1, 2])
def test_flame_needs_three_clients(n):
    with pytest.raises(ValueError, match="clip_flame needs no_models >= 3"):
        C.Params({**FLAME, "no_models": n})
    with pytest.raises(ValueError, match="the round's clients >= 3"):
        agg.fedavg_flame(torch.zeros(4), torch.randn(n, 4), 0.0, 1.0, 1, 4)


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_flame_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({**FLAME, "aggregation_methods": method})


@pytest.mark.parametrize("other", [{"krum_f": 1}, {"trim_k": 1}, {"rlr_threshold": 4}, {"sparse_topk": 0.1}])
def test_flame_excludes_the_other_options(other):
    with pytest.raises(ValueError, match="cannot be combined"):
        C.Params({**FLAME, **other})


def test_shipped_recipe_loads():
    p = C.load_params(os.path.join(ROOT, "configs", "cifar_flame.yaml"))
    assert p.clip_norm == "median" and p.clip_flame is True and p["aggregation_methods"] == "mean"
    assert p.flame_lambda == 1e-5 and not p["diff_privacy"] and p.krum_f is None and p.trim_k is None
    plain = C.load_params(os.path.join(ROOT, "configs", "cifar_params.yaml"))
    keys = set(C.MEAN_OPTION_KEYS)
    assert {k: v for k, v in p.items() if k not in keys} == {k: v for k, v in plain.items() if k not in keys}


# ------------------------------------------------------- reference op vs the numpy oracle
@pytest.mark.parametrize("case", fc.SMALL_CASES + [fc.FALLBACK_CASE], ids=fc.case_id)
def test_reference_op_matches_oracle(case):
    rows, base = fc.make_case(*case)
    G = R.delta_gram(rows, base)
    fc.check(G, rows, base)
    assert torch.equal(G, R.delta_gram(rows, base))
    assert torch.equal(G, ops.delta_gram(rows, base))
    assert torch.equal(G, torch.ops.dba.delta_gram(rows, base, None))


def test_reference_op_row_idx_and_subsets():
    """Rows out of order with a repeat: the gathered call's bits, the repeated pair equal to its
    diagonal; and a subset of the rows keeps the bits it has in the full call."""
    rows, base = fc.make_case(9, 1001, 1001, 0)
    idx = [7, 2, 2, 5, 8, 0]
    G = R.delta_gram(rows, base, idx)
    assert tuple(G.shape) == (6, 6) and torch.equal(G, G.t())
    assert torch.equal(G, R.delta_gram(rows[idx], base))
    assert float(G[1, 2]) == float(G[1, 1]) == float(G[2, 2])
    assert float(G[4, 5]) == float(G[4, 4]) == float(G[5, 5])          # rows 8 and 0 are the case's twins
    assert torch.equal(G, R.delta_gram(rows, base, torch.tensor(idx)))
    full = R.delta_gram(rows, base)
    assert torch.equal(G, full[idx][:, idx])
    sub = [1, 4, 8]
    assert torch.equal(R.delta_gram(rows, base, sub), full[sub][:, sub])
    assert torch.equal(R.delta_gram(rows[sub].contiguous(), base), full[sub][:, sub])


def test_reference_op_degenerate_and_nonfinite():
    G = R.delta_gram(torch.randn(0, 7), torch.randn(7))
    assert G.dtype == torch.float64 and tuple(G.shape) == (0, 0)
    G = R.delta_gram(torch.randn(4, 0), torch.randn(0))
    assert tuple(G.shape) == (4, 4) and not G.any()
    assert tuple(R.delta_gram(torch.randn(4, 7), torch.randn(7), []).shape) == (0, 0)
    x = torch.randn(6, 300, generator=torch.Generator().manual_seed(2))
    base = torch.randn(300, generator=torch.Generator().manual_seed(3))
    off = [j for j in range(6) if j != 2]
    for bad in (float("nan"), float("inf")):
        x[2, 17] = bad
        G = R.delta_gram(x, base)
        assert not torch.isfinite(G[2]).any() and not torch.isfinite(G[:, 2]).any()
        assert torch.isfinite(G[off][:, off]).all()


# ------------------------------------------------------------------- distances, admission
def _dist(pairs, n, default=1.0):
    D = torch.full((n, n), default, dtype=torch.float64)
    D.fill_diagonal_(0.0)
    for (i, j), v in pairs.items():
        D[i, j] = D[j, i] = v
    return D


def test_distances_hand_case():
    x = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, 3.0], [0.0, 0.0], [-2.0, 0.0], [float("inf"), 1.0]])
    D = agg.flame_distances(R.delta_gram(x, torch.zeros(2)))
    assert D.dtype == torch.float64 and torch.equal(D[:5, :5], D[:5, :5].t())
    assert torch.equal(torch.diagonal(D)[:5], torch.zeros(5, dtype=torch.float64))
    assert float(D[0, 1]) == 1.0 and float(D[0, 4]) == 2.0              # orthogonal, opposite
    assert abs(float(D[0, 2]) - (1.0 - 1.0 / math.sqrt(2.0))) <= 2.0 ** -52
    assert D[3, [0, 1, 2, 4]].tolist() == [1.0] * 4                     # the zero update: distance 1
    assert torch.isnan(D[5]).all() and torch.isnan(D[:, 5]).all()       # the unusable client
    twin = agg.flame_distances(R.delta_gram(torch.tensor([[0.1, 0.7, -0.3]] * 2), torch.zeros(3)))
    assert float(twin[0, 1]) >= 0.0 and float(twin[0, 1]) <= 2.0 ** -52  # (clamped: never negative)


def test_admit_two_clusters():
    """n = 10: six tight clients and four tighter ones; only the six can hold m = 6."""
    six, four = [0, 2, 3, 5, 7, 9], [1, 4, 6, 8]
    pairs = {(a, b): 0.05 + 0.001 * (a + b) for a in six for b in six if a < b}
    pairs.update({(a, b): 0.01 + 0.0001 * (a + b) for a in four for b in four if a < b})
    assert agg.flame_admit(_dist(pairs, 10)) == six


def test_admit_chain_beats_the_tightest_pair():
    """n = 5, m = 3: the tightest pair (3, 4) stays a pair; the chain 0 - 1 - 2 is the first
    component of three, and the merge that completes it brings nobody else."""
    D = _dist({(3, 4): 0.01, (0, 1): 0.02, (1, 2): 0.03, (2, 3): 0.5}, 5)
    assert agg.flame_admit(D) == [0, 1, 2]
    # a merge of two components admits both whole: {0, 1} + {2, 3} at m = 3 of n = 5
    D = _dist({(0, 1): 0.01, (2, 3): 0.02, (1, 2): 0.03}, 5)
    assert agg.flame_admit(D) == [0, 1, 2, 3]


def test_admit_ties_go_to_the_lower_pair():
    """Every distance equal: the order is (i, j), so (0, 1), (0, 2), ... build the component."""
    assert agg.flame_admit(_dist({}, 7, default=0.3)) == [0, 1, 2, 3]
    D = _dist({(1, 2): 0.1, (3, 4): 0.1, (0, 4): 0.1}, 5)                # (0, 4) < (1, 2) < (3, 4)
    assert agg.flame_admit(D) == [0, 3, 4]


def test_admit_three_clients():
    assert agg.flame_admit(_dist({(0, 2): 0.1, (0, 1): 0.4, (1, 2): 0.6}, 3)) == [0, 2]
    assert agg.flame_admit(_dist({(1, 2): 0.0}, 3)) == [1, 2]


def test_admit_skips_an_unusable_client():
    pairs = {(a, b): 0.1 + 0.01 * (a + b) for a in range(5) for b in range(5) if a < b}
    D = _dist(pairs, 5)
    D[1, :] = math.nan
    D[:, 1] = math.nan
    assert agg.flame_admit(D) == [0, 2, 3]                               # (0, 2), then (0, 3): m = 3
    D[0, :] = math.nan
    D[:, 0] = math.nan
    assert agg.flame_admit(D) == [2, 3, 4]


def test_admit_too_few_usable_raises():
    D = _dist({}, 5, default=0.2)
    for i in (0, 1, 4):
        D[i, :] = math.nan
        D[:, i] = math.nan
    with pytest.raises(RuntimeError, match=r"^flame: "):
        agg.flame_admit(D)
    finals = torch.randn(5, 8, generator=torch.Generator().manual_seed(1))
    finals[[0, 1, 4], 3] = float("nan")
    with pytest.raises(RuntimeError, match=r"^flame: "):
        agg.fedavg_flame(torch.zeros(8), finals, 0.0, 1.0, 1, 8)


def _random_distances(rng, n, planted):
    L = 40
    x = rng.standard_normal((n, L))
    if planted:                                     # an outlier group around its own direction
        k = int(rng.integers(1, max(2, n // 2)))
        x[:k] = 3.0 * rng.standard_normal(L)[None] + 0.3 * rng.standard_normal((k, L))
        x = x[rng.permutation(n)]
    nrm = np.linalg.norm(x, axis=1)
    D = 1.0 - np.clip((x @ x.T) / nrm[:, None] / nrm[None, :], -1.0, 1.0)
    D = (D + D.T) / 2.0
    np.fill_diagonal(D, 0.0)
    return D


def test_admit_equals_hdbscan():
    """360 seeded random cosine-distance matrices without exact ties, n = 3 .. 20, with and without
    a planted outlier group: the admitted set is the one cluster sklearn's HDBSCAN labels with
    the paper's parameters."""
    try:
        from sklearn.cluster import HDBSCAN
    except ImportError:
        pytest.skip("sklearn.cluster.HDBSCAN does not import")
    rng = np.random.default_rng(20221)
    done = 0
    for n in range(3, 21):
        for rep in range(20):
            D = _random_distances(rng, n, planted=rep % 2 == 1)
            off = D[np.triu_indices(n, 1)]
            assert np.unique(off).size == off.size
            labels = HDBSCAN(min_cluster_size=n // 2 + 1, min_samples=1, allow_single_cluster=True,
                             metric="precomputed").fit(D.copy()).labels_
            assert set(labels.tolist()) <= {0, -1}
            want = [i for i in range(n) if labels[i] == 0]
            assert agg.flame_admit(torch.from_numpy(D)) == want, (n, rep, labels)
            done += 1
    assert done >= 300


# ------------------------------------------------------------------ the rule, planted data
def test_planted_margin_and_rule():
    finals, base = fc.planted()
    D = agg.flame_distances(R.delta_gram(finals, base))
    crowd = fc.PLANT_CROWD
    rest = [i for i in range(fc.PLANT_N) if i not in crowd]
    inside = max(float(D[a, b]) for a in crowd for b in crowd if a != b)
    outside = min(float(D[a, b]) for a in rest for b in range(fc.PLANT_N) if a != b)
    print(f"in-crowd distances <= {inside:.4f}, the others' >= {outside:.4f}")
    assert inside < 0.1 and outside > 0.5            # the margin no rounding can cross
    eta = 0.7
    g = base.clone()
    factors, norms, admitted = agg.fedavg_flame(g, finals, 0.0, eta, 5, fc.PLANT_L)
    adm, S = fc.check_rule(factors, norms, admitted, base, g, finals, base, eta)
    # (the first component of m clients: the crowd's m + 1 need not all be in by then)
    assert set(adm) <= set(crowd) and fc.PLANT_M <= len(adm) <= fc.PLANT_M + 1
    assert S == agg.clip_bound(norms, "median")
    assert any(0.0 < f < 1.0 for f in factors) and all(factors[i] == 0.0 for i in rest)
    # row_idx reads the same rows out of a larger bank: the same bits
    bank = torch.zeros(2 * fc.PLANT_N + 1, fc.PLANT_L + 3)
    slots = list(range(1, 2 * fc.PLANT_N + 1, 2))
    bank[slots, :fc.PLANT_L] = finals
    g2 = torch.cat([base, torch.ones(3)])
    out = agg.fedavg_flame(g2, bank, 0.0, eta, 5, fc.PLANT_L, row_idx=slots)
    assert out == (factors, norms, admitted) and torch.equal(g2[:fc.PLANT_L], g) and torch.equal(g2[fc.PLANT_L:], torch.ones(3))


def test_planted_noise_is_lambda_times_the_median_norm():
    """lambda > 0 adds exactly ``add_noise_scaled``'s N(0, (lambda S)^2) on top of the noiseless
    update (the same total, the same seed); lambda = 0 adds none."""
    finals, base = fc.planted()
    quiet, loud = base.clone(), base.clone()
    _, norms, admitted = agg.fedavg_flame(quiet, finals, 0.0, 1.0, 11, fc.PLANT_L)
    out = agg.fedavg_flame(loud, finals, 0.5, 1.0, 11, fc.PLANT_L)
    assert out[2] == admitted and out[1] == norms
    S = agg.clip_bound(norms, "median")
    zero = torch.zeros(fc.PLANT_L, dtype=torch.float64)
    noise = torch.zeros(fc.PLANT_L)
    ops.add_noise_scaled(noise, zero, 1.0, 0.5 * S, 11, True)
    assert float(noise.std()) > 0.25 * S
    got = (loud - base).double() - (quiet - base).double()
    tol = 4.0 * torch.from_numpy(np.spacing(np.maximum(loud.abs().numpy(), (loud - base).abs().numpy()))).double()
    assert torch.all((got - noise.double()).abs() <= tol)


def test_zero_norm_and_nonfinite_clients():
    """A crowd client that returned the global model is at distance 1 from everyone and is left
    out (the other m crowd clients are admitted); an outsider with an inf entry, and one with a
    NaN, are unusable: norm +inf in the record (ranking last for the median), factor 0, and the
    model stays finite."""
    finals, base = fc.planted()
    rest = [i for i in range(fc.PLANT_N) if i not in fc.PLANT_CROWD]
    finals[fc.PLANT_CROWD[2]] = base
    finals[rest[0], 100] = float("inf")
    finals[rest[1], 7] = float("nan")
    g = base.clone()
    factors, norms, admitted = agg.fedavg_flame(g, finals, 0.0, 1.0, 5, fc.PLANT_L)
    fc.check_rule(factors, norms, admitted, base, g, finals, base, 1.0)
    assert admitted == [i for i in fc.PLANT_CROWD if i != fc.PLANT_CROWD[2]] and len(admitted) == fc.PLANT_M
    assert norms[fc.PLANT_CROWD[2]] == 0.0 and factors[fc.PLANT_CROWD[2]] == 0.0
    assert norms[rest[0]] == math.inf and norms[rest[1]] == math.inf
    assert factors[rest[0]] == 0.0 and factors[rest[1]] == 0.0
    assert torch.isfinite(g).all() and not torch.equal(g, base)
    # clip_factors' zero-norm case: an admitted client that returned the global model has factor 1
    three = torch.stack([base, base, base + 1.0])
    g = base.clone()
    factors, norms, admitted = agg.fedavg_flame(g, three, 0.0, 1.0, 5, fc.PLANT_L)
    assert admitted == [0, 1] and factors == [1.0, 1.0, 0.0] and norms[:2] == [0.0, 0.0]
    assert torch.equal(g, base)


# --------------------------------------------------------------------- through the Server
def _check_round(result):
    before, after, finals, wr, n_upd, p = result
    assert len(wr) == 3
    names, factors, norms = wr
    n = len(names)
    assert len(factors) == n and len(norms) == n
    print(f"names {names}\nfactors {factors}\nnorms {norms}")
    i = names.index(41)
    assert all(norms[i] > v for j, v in enumerate(norms) if j != i)
    S = agg.clip_bound(norms, "median")
    # S / e_41 in clip_factors' arithmetic: a host float over an fp64 tensor
    clipped = float(S / torch.tensor(norms[i], dtype=torch.float64))
    assert factors[i] == 0.0 or (factors[i] == clipped and factors[i] < 1.0)
    admitted = [j for j, f in enumerate(factors) if f > 0.0]
    assert len(admitted) >= n // 2 + 1 and all(0.0 <= f <= 1.0 for f in factors)
    assert not torch.equal(after[:n_upd], before[:n_upd])
    assert torch.equal(after[n_upd:], before[n_upd:])
    # the recorded columns are the rule's on the round's snapshots
    g = before.clone()
    dp_seed = (int(p["seed"]) * 7919 + 12) & 0x7FFFFFFF
    want = agg.fedavg_flame(g, finals, p.flame_lambda, float(p["eta"]), dp_seed, n_upd)
    assert (want[0], want[1]) == (factors, norms) and torch.equal(g, after)


@pytest.fixture(scope="module")
def flame_round(tmp_path_factory):
    return trim_cpu.run_round(tmp_path_factory.mktemp("flame"), **FLAME)


def test_server_round_clips_or_drops_the_attacker(flame_round):
    _check_round(flame_round)


def test_server_round_is_bitwise_repeatable(flame_round, tmp_path):
    again = trim_cpu.run_round(tmp_path, **FLAME)
    assert torch.equal(again[1], flame_round[1]) and again[3] == flame_round[3]


def test_server_round_reduces_nothing(tmp_path):
    """Every rank holds every final row and computes the rule redundantly: no collective in
    ``_aggregate``; plain ``clip_norm: median`` keeps its three."""
    seen, s = collectives.record_round(tmp_path / "flame", **FLAME)
    assert seen == []
    assert len(s.csv.weight_result) == 3


def test_pretrain_stays_plain_fedavg(tmp_path):
    """The benign warm start runs with clip_norm / clip_flame cleared and puts them back."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = trim_cpu.mnist_params(tmp_path, **FLAME, clip_flame_lambda=0.01)
    s = Server(p, DistCtx(), write_outputs=False)
    seen = []
    inner = s._aggregate

    def wrapped(plan, bank, local, adversarial):
        seen.append((s.params["clip_norm"], s.params["clip_flame"], s.params["clip_flame_lambda"]))
        return inner(plan, bank, local, adversarial)
    s._aggregate = wrapped
    s.pretrain(1)
    assert seen == [(None, None, None)]
    assert s.params.clip_norm == "median" and s.params.clip_flame is True and s.params.clip_flame_lambda == 0.01
    assert not s.csv.weight_result                # (plain FedAvg records no weights)


def test_world_size_invariance(tmp_path):
    """FLAME at worlds 1, 2, 4 (gloo): every rank of every world holds the same final rows after the
    gather and runs the same rule over them, so the same state bits and weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, **FLAME}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = trim_cpu.weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    i = rows1[0].index("41")
    assert float(rows1[1][i]) < 1.0 and float(rows1[2][i]) == max(float(v) for v in rows1[2])
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert trim_cpu.weight_rows(str(tmp_path / f"w{world}")) == rows1

"""Robust-learning-rate FedAvg (config ``rlr_threshold``) on CPU: the config key, the three
reference ops against the numpy oracle of rlr_cases.py bit for bit, their ties to ``delta_sum`` and
``add_noise_scaled``, non-finite client values, degenerate shapes, a model-replacement round
through ``Server``, the warm start and world-size invariance."""
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import rlr_cases as rc
import test_trim_aggregation as trim_cpu
from conftest import ROOT

CFG = trim_cpu.CFG
CASES = rc.SMALL_CASES + [rc.wrap_case(rc.SWEEP)]
SEED, COEF, SIGMA = 12345, 0.1 / 3, 0.01      # (a coefficient that fp32 does not hold exactly)


# ------------------------------------------------------------------------------ config
def test_rlr_defaults_and_accepts():
    assert C.Params()["rlr_threshold"] is None and C.Params().rlr_threshold is None
    for theta in (1, 4, 10):
        assert C.Params({"no_models": 10, "rlr_threshold": theta}).rlr_threshold == theta
    assert C.Params({"rlr_threshold": 4, "diff_privacy": True}).rlr_threshold == 4
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")


@pytest.mark.parametrize("bad", [True, False, 0, -1, 1.5, 4.0, "4", "median", [4]])
def test_rlr_rejects_values(bad):
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "rlr_threshold": bad})


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_rlr_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({"rlr_threshold": 4, "aggregation_methods": method})
    assert C.Params({"rlr_threshold": None, "aggregation_methods": method}).rlr_threshold is None


def test_rlr_excludes_the_other_defences():
    for other in ({"clip_norm": 1.0}, {"clip_norm": "median"}, {"krum_f": 1}, {"trim_k": 2}, {"trim_k": "median"}):
        with pytest.raises(ValueError):
            C.Params(dict(other, rlr_threshold=4))


def test_rlr_size_inequality():
    with pytest.raises(ValueError):
        C.Params({"no_models": 10, "rlr_threshold": 11})
    assert C.Params({"no_models": 11, "rlr_threshold": 11}).rlr_threshold == 11
    # ... and again against a round's actual client count
    assert agg.rlr_theta(10, 4) == 4 and agg.rlr_theta(4, 4) == 4
    with pytest.raises(ValueError):
        agg.rlr_theta(3, 4)
    with pytest.raises(ValueError):
        agg.rlr_theta(10, None)
    with pytest.raises(ValueError):
        agg.fedavg_rlr(torch.zeros(5), torch.zeros(3, 5), 4, 0.1, 10, False, 0.0, 1, 5)


def test_shipped_recipe_loads():
    p = C.load_params(os.path.join(ROOT, "configs", "cifar_rlr.yaml"))
    assert p.rlr_threshold == 4 and p["aggregation_methods"] == "mean"
    assert p.krum_f is None and p.clip_norm is None and p.trim_k is None
    base = C.load_params(os.path.join(ROOT, "configs", "cifar_params.yaml"))
    assert {k: v for k, v in p.items() if k != "rlr_threshold"} == \
        {k: v for k, v in base.items() if k != "rlr_threshold"}


# ------------------------------------------------------------------ the oracle's own cover
def test_cases_exercise_both_sides():
    """On the oracle alone: every n = 10 case has kept and flipped coordinates at theta = 4 and a
    tied vote somewhere, so no test can pass by exercising one side only."""
    tens = [c for c in CASES if c[0] == 10]
    assert tens
    for case in tens:
        rows, base = rc.make_case(*case)
        _, votes = rc.oracle_votes(rows.numpy(), base.numpy())
        kept = np.abs(votes) >= rc.THETA
        assert kept.any() and (~kept).any() and (votes == 0).any(), case
        counts = rc.oracle_agreement(rows.numpy(), base.numpy(), votes, rc.THETA)
        assert (counts[:, 0] > 0).all() and (counts[:, 1] > 0).any()
    # a negative zero against a positive zero, and an exact-zero delta, vote 0
    assert rc.signs(np.array([[-0.0, 0.0, 1.0]], np.float32), np.array([0.0, -0.0, 1.0], np.float32)).tolist() == [[0, 0, 0]]


# ------------------------------------------------------- reference ops vs the numpy oracle
@pytest.fixture(scope="module", params=CASES, ids=rc.case_id)
def case_data(request):
    """(case, rows, base, the reference op's total, votes): computed once per case."""
    rows, base = rc.make_case(*request.param)
    total, votes = R.delta_sum_votes(rows, base)
    return request.param, rows, base, total, votes


def test_reference_votes_match_oracle(case_data):
    case, rows, base, total, votes = case_data
    rc.check_votes((total, votes), rows, base)
    got = ops.delta_sum_votes(rows, base)                                  # (the registered op, CPU dispatch)
    assert torch.equal(rc.bits(got[0]), rc.bits(total)) and torch.equal(got[1], votes)


def test_reference_total_equals_delta_sum(case_data):
    """The bits of ``delta_sum`` wherever the CPU ``delta_sum`` adds in client order: it is a
    ``torch.sum`` over the rows, which adds them one after the other up to 16 rows and in cascaded
    blocks beyond (65 rows: one last bit differs at a few coordinates).  The definition is the
    client order, which the oracle checks at every n; the HIP ``delta_sum`` kernel adds in client
    order at every n, and test_gpu_rlr.py compares with it on every case."""
    case, rows, base, total, votes = case_data
    if case[0] <= 16:
        assert torch.equal(rc.bits(total), rc.bits(ops.delta_sum(rows, base)))
    else:
        seq = torch.zeros_like(total)
        for i in range(case[0]):
            seq = seq + ops.delta_sum(rows[i:i + 1], base)
        assert torch.equal(rc.bits(total), rc.bits(seq))


def test_reference_agreement_matches_oracle(case_data):
    case, rows, base, total, votes = case_data
    for theta in rc.thetas(case[0]):
        rc.check_agreement(R.vote_agreement(rows, base, votes, theta), rows, base, votes.numpy(), theta)
    assert torch.equal(ops.vote_agreement(rows, base, votes, 1), R.vote_agreement(rows, base, votes, 1))


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
def test_reference_apply_matches_add_noise_scaled(case_data, noise):
    case, rows, base, total, votes = case_data
    n = case[0]
    for theta in rc.thetas(n):
        rc.check_apply(ops, base, total, votes, theta, COEF, SIGMA, SEED, noise)
    # all kept: add_noise_scaled itself
    got, want = base.clone(), base.clone()
    flipped = R.rlr_apply(got, total, torch.full_like(votes, n), n, COEF, SIGMA, SEED, noise)
    R.add_noise_scaled(want, total, COEF, SIGMA, SEED, noise)
    assert int(flipped) == 0 and torch.equal(rc.bits(got), rc.bits(want))


def test_theta_one_flips_exactly_the_tied_coordinates():
    rows, base = rc.make_case(*rc.TEN_ROWS)
    total, votes = R.delta_sum_votes(rows, base)
    tied = votes == 0
    assert tied.any() and not tied.all()
    got, pos, neg = base.clone(), base.clone(), base.clone()
    flipped = R.rlr_apply(got, total, votes, 1, COEF, 0.0, SEED, False)
    R.add_noise_scaled(pos, total, COEF, 0.0, SEED, False)
    R.add_noise_scaled(neg, total, -COEF, 0.0, SEED, False)
    assert int(flipped) == int(tied.sum())
    assert torch.equal(got[~tied], pos[~tied]) and torch.equal(got[tied], neg[tied])
    counts = R.vote_agreement(rows, base, votes, 1)
    s = torch.from_numpy(rc.signs(rows.numpy(), base.numpy()))
    assert int(counts.sum()) == int(((s != 0) & ~tied[None]).sum())        # every non-zero sign off a tie counts once


# --------------------------------------------------------------------------- hand case
def test_hand_case_fedavg_rlr():
    """n = 3, theta = 2, eta = 3 (so eta / no_models = 1 exactly), base 0.  Column 0: signs + + -, V
    = 1: flipped, w -= 1 + 2 - 6.  Column 1: + + +, V = 3: kept, w += 6.  Column 2: - - 0, V = -2: kept,
    w += -3.  Column 3: + - 0, V = 0: flipped, total 0."""
    finals = torch.tensor([[1.0, 1.0, -1.0, 5.0], [2.0, 2.0, -2.0, -5.0], [-6.0, 3.0, 0.0, 0.0]])
    g = torch.zeros(4)
    agree, dissent, flipped = agg.fedavg_rlr(g, finals, 2, 3.0, 3, False, 0.0, 1, 4)
    assert g.tolist() == [3.0, 6.0, -3.0, 0.0] and flipped == 2
    assert agree == [0.5, 0.5, 0.25] and dissent == [0.0, 0.0, 0.0]
    g = torch.zeros(4)
    agree, dissent, flipped = agg.fedavg_rlr(g, finals, 1, 3.0, 3, False, 0.0, 1, 4)
    assert g.tolist() == [-3.0, 6.0, -3.0, 0.0] and flipped == 1
    assert agree == [0.75, 0.75, 0.25] and dissent == [0.0, 0.0, 0.25]


# -------------------------------------------------------------------------- non-finite
def nonfinite_input():
    """Three clients, five coordinates: a NaN client, +inf and -inf clients, inf against an inf
    base, and a NaN client at a tied coordinate."""
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[nan, inf, -inf, inf, 2.0],
                      [1.0, 1.0, 1.0, 1.0, nan],
                      [2.0, -1.0, 1.0, inf, 0.0]])
    return x, torch.tensor([0.0, 0.0, 0.0, inf, 1.0])


def check_nonfinite(o, x, base):
    """``o``: the ops namespace under test; x, base on its device."""
    inf = float("inf")
    total, votes = o.delta_sum_votes(x, base)
    # signs: client 0: 0 + - 0 +, client 1: + + + - 0, client 2: + - + 0 -
    assert votes.cpu().tolist() == [2, 1, 1, -1, 0]
    t = total.cpu().tolist()
    assert np.isnan(t[0]) and t[1] == inf and t[2] == -inf and np.isnan(t[3]) and np.isnan(t[4])
    rc.check_votes((total, votes), x.cpu(), base.cpu())
    assert o.vote_agreement(x, base, votes, 1).cpu().tolist() == [[1, 1], [4, 0], [2, 1]]
    assert o.vote_agreement(x, base, votes, 2).cpu().tolist() == [[0, 0], [1, 0], [1, 0]]
    for theta in (1, 2, 3):
        rc.check_agreement(o.vote_agreement(x, base, votes, theta), x.cpu(), base.cpu(), votes.cpu().numpy(), theta)
    # a non-finite total reaches the model, with the vote's sign on an infinity
    dst = torch.zeros(5, device=x.device)
    assert int(o.rlr_apply(dst, total, votes, 2, 0.5, 0.0, 1, False)) == 4
    d = dst.cpu().tolist()
    assert np.isnan(d[0]) and d[1] == -inf and d[2] == inf and np.isnan(d[3]) and np.isnan(d[4])
    for noise in (False, True):
        rc.check_apply(o, torch.ones(5, device=x.device), total, votes, 2, COEF, SIGMA, SEED, noise)


def test_nonfinite_values_follow_ieee():
    check_nonfinite(ops, *nonfinite_input())


# -------------------------------------------------------------------- degenerate shapes
def check_degenerate(o, dev):
    total, votes = o.delta_sum_votes(torch.randn(0, 7, device=dev), torch.randn(7, device=dev))
    assert total.dtype == torch.float64 and tuple(total.shape) == (7,) and not total.any()
    assert votes.dtype == torch.int32 and tuple(votes.shape) == (7,) and not votes.any()
    assert total.device.type == dev.type and votes.device.type == dev.type
    counts = o.vote_agreement(torch.randn(0, 7, device=dev), torch.randn(7, device=dev), votes, 1)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (0, 2)
    total, votes = o.delta_sum_votes(torch.randn(4, 0, device=dev), torch.randn(0, device=dev))
    assert total.dtype == torch.float64 and votes.dtype == torch.int32 and total.numel() == 0 and votes.numel() == 0
    counts = o.vote_agreement(torch.randn(4, 0, device=dev), torch.randn(0, device=dev), votes, 2)
    assert counts.dtype == torch.int64 and counts.tolist() == [[0, 0]] * 4
    dst = torch.zeros(0, device=dev)
    assert int(o.rlr_apply(dst, total, votes, 1, 0.1, 0.0, 1, False)) == 0
    # a single row: its delta, its sign, agreeing with itself wherever it moved
    x, b = torch.randn(1, 37, device=dev), torch.randn(37, device=dev)
    x[0, 5] = b[5]
    total, votes = o.delta_sum_votes(x, b)
    assert torch.equal(total, x[0].double() - b.double())
    assert torch.equal(votes, torch.sign(x[0] - b).to(torch.int32))
    assert o.vote_agreement(x, b, votes, 1).tolist() == [[36, 0]]


def test_degenerate_shapes():
    check_degenerate(ops, torch.device("cpu"))


# --------------------------------------------------------------------- through the Server
def check_round(result, theta, strict_order=True):
    """The new global state is ``before`` with the oracle's total and votes applied through the ops
    (and equals ``add_noise_scaled`` with +coef / -coef at the kept / flipped coordinates), the
    recorded shares are the oracle's counts over ``n_upd``, nothing past ``n_upd`` moved, and the
    attacker has the strictly smallest agree share and the strictly largest dissent share."""
    before, after, finals, wr, n_upd, p = result
    assert len(wr) == 3
    names, agree, dissent = wr
    n = len(names)
    assert len(agree) == n and len(dissent) == n
    rows, base = finals[:, :n_upd].cpu(), before[:n_upd].cpu()
    total, votes = rc.oracle_votes(rows.numpy(), base.numpy())
    counts = rc.oracle_agreement(rows.numpy(), base.numpy(), votes, theta)
    flipped = rc.oracle_flipped(votes, theta)
    i = names.index(41)
    print(f"names {names}\nagree share {agree}\ndissent share {dissent}\nflipped {flipped} of {n_upd}\n"
          f"client 41: agree {agree[i]:.4f} (next lowest {min(v for j, v in enumerate(agree) if j != i):.4f}), "
          f"dissent {dissent[i]:.4f} (next highest {max(v for j, v in enumerate(dissent) if j != i):.4f})")
    assert 0 < flipped < n_upd
    dev = before.device
    dp_seed = (int(p["seed"]) * 7919 + 12) & 0x7FFFFFFF
    coef = float(p["eta"]) / int(p["no_models"])
    t_dev, v_dev = torch.from_numpy(total).to(dev), torch.from_numpy(votes).to(dev)
    want = before.clone()
    want[:n_upd] = rc.check_apply(ops, before[:n_upd].clone(), t_dev, v_dev, theta, coef, float(p["sigma"]), dp_seed,
                                  bool(p["diff_privacy"]))
    assert torch.equal(rc.bits(after), rc.bits(want))
    assert not torch.equal(after[:n_upd], before[:n_upd])
    assert torch.equal(after[n_upd:], before[n_upd:])
    assert agree == [float(v) / n_upd for v in counts[:, 0].tolist()]
    assert dissent == [float(v) / n_upd for v in counts[:, 1].tolist()]
    assert all(0.0 <= a <= 1.0 and 0.0 <= d <= 1.0 and a + d <= 1.0 for a, d in zip(agree, dissent))
    if strict_order:
        assert all(agree[i] < v for j, v in enumerate(agree) if j != i)
        assert all(dissent[i] > v for j, v in enumerate(dissent) if j != i)


@pytest.fixture(scope="module")
def rlr_round(tmp_path_factory):
    return trim_cpu.run_round(tmp_path_factory.mktemp("rlr"), rlr_threshold=rc.THETA)


def test_server_round_votes_against_the_attacker(rlr_round):
    check_round(rlr_round, rc.THETA)


def test_server_round_with_noise(tmp_path):
    """diff_privacy is allowed: the hash-RNG noise of add_noise_scaled on both sides of the vote."""
    check_round(trim_cpu.run_round(tmp_path, rlr_threshold=rc.THETA, diff_privacy=True, sigma=0.001), rc.THETA,
                strict_order=False)


def test_off_is_plain_fedavg(rlr_round, tmp_path):
    """rlr_threshold None (the default): the bits of a run that never names the key, no weight rows."""
    off = trim_cpu.run_round(tmp_path / "off", rlr_threshold=None)
    plain = trim_cpu.run_round(tmp_path / "plain")
    assert torch.equal(rc.bits(off[1]), rc.bits(plain[1])) and not off[3] and not plain[3]
    assert torch.equal(off[2], rlr_round[2])                  # (the same clients trained the same way)
    assert not torch.equal(off[1], rlr_round[1])


def test_pretrain_stays_plain_fedavg(tmp_path):
    """The benign warm start runs with rlr_threshold cleared and puts it back."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = trim_cpu.mnist_params(tmp_path, rlr_threshold=rc.THETA)
    s = Server(p, DistCtx(), write_outputs=False)
    seen = []
    inner = s._aggregate

    def wrapped(plan, bank, local, adversarial):
        seen.append(s.params["rlr_threshold"])
        return inner(plan, bank, local, adversarial)
    s._aggregate = wrapped
    s.pretrain(1)
    assert seen == [None]
    assert s.params.rlr_threshold == rc.THETA
    assert not s.csv.weight_result                # (plain FedAvg records no weights)


def test_world_size_invariance(tmp_path):
    """rlr_threshold = 4 at worlds 1, 2, 4: the clients stay on their owner ranks; the fp64 totals,
    int32 votes and int64 counts all-reduce to the same bits, so every rank of every world ends with
    the same state bits and weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "rlr_threshold": rc.THETA}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = trim_cpu.weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    assert all(0.0 < float(a) < 1.0 and 0.0 < float(d) < 1.0 for a, d in zip(rows1[1], rows1[2]))
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert trim_cpu.weight_rows(str(tmp_path / f"w{world}")) == rows1

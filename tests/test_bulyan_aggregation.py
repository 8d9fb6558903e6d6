"""Bulyan (config ``krum_f`` with ``krum_bulyan``) on CPU: the config keys, iterated Krum on hand
cases, the reference op of the median window against the numpy oracle of bulyan_cases.py bit for
bit, two identities against the trimmed sum, a model-replacement round through ``Server``, the
warm start, world-size invariance and the collectives of the aggregation."""
import logging
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import bulyan_cases as bc
import test_aggregation_collectives as collectives
import test_trim_aggregation as trim_cpu
import trim_cases as tc
from conftest import ROOT

CFG = trim_cpu.CFG
# one sweep of the launch grid of csrc/kernels/coordrank.hpp (test_gpu_bulyan.py checks it against the kernel's own)
SWEEP = 512 * bc.GRID_THREADS * bc.GRID_QUAD
CASES = bc.SMALL_CASES + [bc.wrap_case(SWEEP), bc.FALLBACK_CASE]


# ------------------------------------------------------------------------------ config
def test_bulyan_defaults_and_accepts():
    assert C.Params()["krum_bulyan"] is None and C.Params().krum_bulyan is None
    assert C.Params({"krum_f": 1, "krum_bulyan": True}).krum_bulyan is True
    for off in (None, False):
        p = C.Params({"krum_f": 1, "krum_bulyan": off})
        assert p.krum_bulyan is None and p.krum_f == 1
        assert C.Params({"krum_bulyan": off}).krum_bulyan is None          # (off needs no krum_f)
    assert C.Params({"krum_f": 0, "krum_bulyan": True, "no_models": 3}).krum_bulyan is True
    assert C.Params({"krum_f": 1, "krum_bulyan": True, "diff_privacy": True}).krum_bulyan is True
    assert "krum_bulyan" in C.MEAN_OPTION_KEYS and C.MEAN_OPTIONS[-1].key == "sparse_topk"
    assert C.mean_option(C.Params({"krum_f": 1, "krum_bulyan": True})).key == "krum_f"
    assert C.mean_option(C.Params({"krum_f": 1, "krum_bulyan": True})).gathers


@pytest.mark.parametrize("bad", [1, 0, 1.0, "true", "yes", [True]])
def test_bulyan_rejects_values(bad):
    with pytest.raises(ValueError, match="krum_bulyan"):
        C.Params({"krum_f": 1, "krum_bulyan": bad})


def test_bulyan_needs_krum_f():
    with pytest.raises(ValueError, match=r"^krum_bulyan is set without krum_f$"):
        C.Params({"krum_bulyan": True})


def test_bulyan_excludes_krum_m():
    with pytest.raises(ValueError, match="krum_bulyan cannot be combined with krum_m"):
        C.Params({"krum_f": 1, "krum_bulyan": True, "krum_m": 2})
    assert C.Params({"krum_f": 1, "krum_bulyan": False, "krum_m": 2}).krum_m == 2


def test_bulyan_size_inequality():
    with pytest.raises(ValueError, match=r"needs no_models >= 4 f \+ 3 = 11 \(got 10\)"):
        C.Params({"no_models": 10, "krum_f": 2, "krum_bulyan": True})
    assert C.Params({"no_models": 11, "krum_f": 2, "krum_bulyan": True}).krum_f == 2
    assert C.check_bulyan_sizes(10, 1) == 8 and C.check_bulyan_sizes(7, 1) == 5 and C.check_bulyan_sizes(3, 0) == 3
    with pytest.raises(ValueError, match=r"the round's clients >= 4 f \+ 3 = 7 \(got 6\)"):
        C.check_bulyan_sizes(6, 1, "the round's clients")
    with pytest.raises(ValueError):
        agg.fedavg_bulyan(torch.zeros(3), torch.zeros(6, 3), 1, 1.0, False, 0.0, 1, 3)


@pytest.mark.parametrize("other", [{"clip_norm": 1.0}, {"trim_k": 2}, {"rlr_threshold": 4}, {"sparse_topk": 0.1}])
def test_bulyan_excludes_the_other_options(other):
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "krum_bulyan": True, **other})


@pytest.mark.parametrize("method", ["geom_median", "foolsgold"])
def test_bulyan_is_an_option_of_mean_only(method):
    with pytest.raises(ValueError):
        C.Params({"krum_f": 1, "krum_bulyan": True, "aggregation_methods": method})


def test_krum_messages_unchanged():
    with pytest.raises(ValueError, match=r"^krum_f 4 needs no_models >= 2 f \+ 3 = 11 \(got 10\)$"):
        C.Params({"no_models": 10, "krum_f": 4})
    with pytest.raises(ValueError, match=r"^krum_m 9 exceeds no_models - krum_f = 8$"):
        C.Params({"no_models": 10, "krum_f": 2, "krum_m": 9})
    with pytest.raises(ValueError, match=r"^krum_m is set without krum_f$"):
        C.Params({"krum_m": 2})
    with pytest.raises(ValueError, match=r"^krum_f True: expected None or an integer >= 0$"):
        C.Params({"krum_f": True})
    assert C.check_krum_sizes(10, 2, None) == 8 and C.check_krum_sizes(10, 2, 3, "x") == 3


def test_recipe_loads():
    p = C.load_params(os.path.join(ROOT, "configs", "cifar_bulyan.yaml"))
    assert p.krum_f == 1 and p.krum_bulyan is True and p.krum_m is None and p["aggregation_methods"] == "mean"
    assert p.clip_norm is None and p.trim_k is None and p.rlr_threshold is None and p.sparse_topk is None
    n = int(p["no_models"])
    assert n == 10 and C.check_bulyan_sizes(n, p.krum_f) == 8 and 8 - 2 * p.krum_f == 6
    assert p["is_poison"] and len(p.adversary_list) == 4


# ---------------------------------------------------------------------- iterated Krum
HAND = torch.tensor([[0.0], [1.0], [2.0], [3.0], [4.0], [5.0], [100.0]])


def test_hand_case_selection():
    """Seven clients on a line at 0 1 2 3 4 5 100, f = 1, theta = 5 (squared distances).
    r = 7, k = 4: scores 30 15 10 10 15 30 and 95^2 + .. + 98^2; client 2 wins the tie with 3.
    r = 6, k = 3 over {0 1 3 4 5 100}: 26 14 9 11 21; client 3 wins with 9.
    r = 5, k = 2 over {0 1 4 5 100}: 17 10 10 17 18241; client 1 wins the tie with 4.
    r = 4, k = 1 over {0 4 5 100}: 16 1 1 9025; client 4 wins the tie with 5.
    r = 3, k = max(1, 0) = 1 over {0 5 100} (the clamp; k = 0 would score everyone 0): 25 25 9025;
    client 0 wins the tie.  Clients 5 and 100 keep their scores of that last iteration."""
    order, scores = agg.bulyan_select(ops.pairwise_sq_dists(HAND), 1)
    assert order == [2, 3, 1, 4, 0]
    assert scores == [25.0, 10.0, 10.0, 9.0, 1.0, 25.0, 9025.0]
    assert all(isinstance(s, float) for s in scores)


def test_hand_case_fedavg_bulyan():
    """The five selected values 0 1 2 3 4: beta = 3, med = 2; j = 0: 3 - 2 < 2 - 0, j = 1: 4 - 2 < 2 - 1
    is false, so a = 1 and the window is 1 2 3."""
    g = torch.zeros(1)
    share, scores, order = agg.fedavg_bulyan(g, HAND, 1, 1.0, False, 0.0, 1, 1)
    assert order == [2, 3, 1, 4, 0] and scores == [25.0, 10.0, 10.0, 9.0, 1.0, 25.0, 9025.0]
    assert share == [0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert g.tolist() == [2.0]
    # rows read in place from a larger bank, in another order
    bank = torch.cat([torch.full((2, 1), 7.0), HAND.flip(0)])
    g = torch.zeros(1)
    share, _, order = agg.fedavg_bulyan(g, bank, 1, 3.0, False, 0.0, 1, 1, row_idx=[8, 7, 6, 5, 4, 3, 2])
    assert order == [2, 3, 1, 4, 0] and share == [0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0] and g.tolist() == [6.0]


def _brute_select(D, f):
    """Iterated Krum once more, on numpy, for random matrices."""
    D = np.where(np.isfinite(D), D, np.inf)
    n = D.shape[0]
    rem, sel = list(range(n)), []
    while len(sel) < n - 2 * f:
        k = max(1, len(rem) - f - 2)
        sc = []
        for i in rem:
            s = 0.0
            for v in np.sort(np.array([D[i, j] for j in rem if j != i]))[:k]:
                s += float(v)
            sc.append(s)
        w = int(np.argmin(sc))               # (the first minimum: the lower index)
        if not np.isfinite(sc[w]):
            break
        sel.append(rem.pop(w))
    return sel


@pytest.mark.parametrize("n,f", [(3, 0), (7, 1), (10, 1), (11, 2), (15, 3), (12, 1)])
def test_clamp_iterations_and_sizes(n, f):
    """n = 4 f + 3 runs its last iteration at r = 2 f + 1 with k clamped to 1; every case selects
    theta = n - 2 f distinct clients."""
    g = torch.Generator().manual_seed(n * 10 + f)
    D = ops.pairwise_sq_dists(torch.randn(n, 50, generator=g))
    order, scores = agg.bulyan_select(D, f)
    assert len(order) == n - 2 * f and len(set(order)) == len(order) and len(scores) == n
    assert order == _brute_select(D.numpy(), f)
    assert all(np.isfinite(scores))


def test_nan_client_is_never_selected():
    g = torch.Generator().manual_seed(5)
    finals = torch.randn(8, 200, generator=g)
    finals[2, 17] = float("nan")
    order, scores = agg.bulyan_select(ops.pairwise_sq_dists(finals), 1)
    assert 2 not in order and len(order) == 6 and scores[2] == float("inf")
    gl = torch.zeros(200)
    share, _, _ = agg.fedavg_bulyan(gl, finals, 1, 1.0, False, 0.0, 1, 200)
    assert share[2] == 0.0 and torch.isfinite(gl).all()
    # two non-finite clients of eight: the six finite ones have the k = 5 finite neighbours of the first
    # iteration; the last iteration (r = 3, k = 1) is left with one finite client whose two
    # neighbours are the non-finite ones, so selection stops at t = 5 >= 2 f + 1
    finals[5, 0] = float("inf")
    order, scores = agg.bulyan_select(ops.pairwise_sq_dists(finals), 1)
    assert len(order) == 5 and not {2, 5} & set(order)
    left = [i for i in range(8) if i not in order]
    assert all(scores[i] == float("inf") for i in left)       # (the last iteration's scores)
    # a third: every first score sums five neighbours of which at most four are finite
    finals[7, 3] = float("-inf")
    with pytest.raises(RuntimeError, match="only 0 of 8"):
        agg.bulyan_select(ops.pairwise_sq_dists(finals), 1)


def test_too_few_finite_clients_raise():
    finals = torch.full((7, 10), float("nan"))
    with pytest.raises(RuntimeError, match="bulyan"):
        agg.bulyan_select(ops.pairwise_sq_dists(finals), 1)
    with pytest.raises(RuntimeError, match="bulyan"):
        agg.fedavg_bulyan(torch.zeros(10), finals, 1, 1.0, False, 0.0, 1, 10)
    # two finite clients of seven: each has one finite neighbour where k = 4 are summed
    finals[0] = 0.0
    finals[1] = 1.0
    with pytest.raises(RuntimeError, match="bulyan"):
        agg.bulyan_select(ops.pairwise_sq_dists(finals), 1)
    with pytest.raises(ValueError):
        agg.bulyan_select(torch.zeros(4, 4), 1)               # theta = 2 < 2 f + 1
    with pytest.raises(ValueError):
        agg.bulyan_select(torch.zeros(4, 4), -1)


# ------------------------------------------------------- reference op vs the numpy oracle
@pytest.mark.parametrize("case", CASES, ids=bc.case_id)
def test_reference_op_matches_oracle(case):
    rows, base = bc.make_case(*case)
    f = case[4]
    bc.check(R.bulyan_delta_sum(rows, base, f), rows, base, f)
    bc.check(ops.bulyan_delta_sum(rows, base, f), rows, base, f)       # (the registered op, CPU dispatch)


def test_window_is_not_a_symmetric_trim():
    """The recipe's shape: the window start a differs from f on a tenth of the coordinates at the
    least (from the oracle alone), so a symmetric trim cannot pass the kernel test of this case."""
    case = bc.RECIPE_CASE
    rows, base = bc.make_case(*case)
    f, L = case[4], case[1]
    a = bc.window_start(np.sort(rows.numpy(), axis=0), f)
    hist = np.bincount(a, minlength=2 * f + 1).tolist()
    total, _, _ = bc.oracle(rows.numpy(), base.numpy(), f)
    trimmed, _, _ = tc.oracle(rows.numpy(), base.numpy(), f)
    differ = int((total != trimmed).sum())
    print(f"window starts {hist}, totals that differ from the trimmed sum {differ}/{L}")
    assert hist == [63, 132, 62]
    assert (a != f).sum() >= 0.1 * L and differ >= 0.1 * L


def test_counting_rule_is_the_greedy_window():
    for case in (bc.RECIPE_CASE, (8, 257, 257, 0, 3), (7, 1029, 1031, 2, 2)):
        rows, _ = bc.make_case(*case)
        f = case[4]
        x = rows.numpy()
        s = np.sort(x, axis=0)
        a = bc.window_start(s, f)
        beta = x.shape[0] - 2 * f
        for c in range(0, x.shape[1], 3):
            assert np.array_equal(s[a[c]:a[c] + beta, c], bc.greedy_window(x[:, c], f)), (case, c)


def test_reference_op_row_idx():
    rows, base = bc.make_case(*bc.NINE_ROWS)
    idx = [7, 2, 5, 2, 8, 0, 3]
    out = R.bulyan_delta_sum(rows, base, 2, idx)
    bc.check(out, rows[idx], base, 2)
    again = R.bulyan_delta_sum(rows, base, 2, torch.tensor(idx))
    assert all(torch.equal(x, y) for x, y in zip(out, again))


def test_reference_op_degenerate_shapes():
    total, kept, high = R.bulyan_delta_sum(torch.randn(0, 7), torch.randn(7), 0)
    assert total.dtype == torch.float64 and tuple(total.shape) == (7,) and not total.any()
    assert kept.numel() == 0 and high.numel() == 0 and kept.dtype == torch.int64
    total, kept, high = R.bulyan_delta_sum(torch.randn(5, 0), torch.randn(0), 2)
    assert total.numel() == 0 and kept.tolist() == [0] * 5 and high.tolist() == [0] * 5
    total, kept, high = R.bulyan_delta_sum(torch.randn(4, 7), torch.randn(7), 0, [])
    assert tuple(total.shape) == (7,) and not total.any() and kept.numel() == 0


@pytest.mark.parametrize("t,f", [(4, 2), (3, 2), (0, 1), (5, -1), (5, 1.0), (5, True), (5, "1")])
def test_reference_op_rejects_bad_f(t, f):
    with pytest.raises(ValueError):
        R.bulyan_delta_sum(torch.randn(t, 3), torch.randn(3), f)
    with pytest.raises(ValueError):
        ops.bulyan_delta_sum(torch.randn(t, 3), torch.randn(3), f)


def _same(a, b):
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", [(8, 257, 257, 0), (9, 4099, 5000, 1), (17, 130, 131, 0)], ids=bc.case_id)
def test_f0_is_the_plain_trimmed_sum(case):
    rows, base = bc.make_case(*case)
    assert _same(ops.bulyan_delta_sum(rows, base, 0), ops.trimmed_delta_sum(rows, base, 0))


@pytest.mark.parametrize("case", [(3, 5, 5, 0), (9, 4099, 5000, 1), (17, 130, 131, 0)], ids=bc.case_id)
def test_odd_t_full_f_is_the_median(case):
    """Odd t with 2 f = t - 1: beta = 1 and the window is one value.  s_{j+1} - med < med - s_j is false
    from j = m on (the left side is >= 0, the right <= 0) and true below m unless s_j already
    equals the median, so s_a has the median's value: the coordinate-wise median of the trimmed
    sum, the same thresholds and the same counts.  Where several values tie with the median, a may
    be a lower rank than m; among tied zeros that rank may hold the other zero, so the totals are
    compared as values (``==`` ignores the sign of a zero, which the rule leaves open) and every
    non-zero total bit for bit."""
    rows, base = bc.make_case(*case)
    t = case[0]
    got = ops.bulyan_delta_sum(rows, base, (t - 1) // 2)
    want = ops.trimmed_delta_sum(rows, base, (t - 1) // 2)
    assert torch.equal(got[0], want[0]) and not torch.isnan(want[0]).any()
    nz = want[0] != 0
    assert torch.equal(got[0][nz].view(torch.int64), want[0][nz].view(torch.int64))
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_nonfinite_values_follow_the_rule():
    x, base = trim_cpu.nonfinite_input()
    for f in (0, 1, 2):
        bc.check(R.bulyan_delta_sum(x, base, f), x, base, f, tag=f"f={f} ")
    # f = 1, coordinate 0: sorted 1 2 4 5 6 NaN, med = 4, beta = 4; j = 0: 6 - 4 < 4 - 1, j = 1: NaN - 4 < 4 - 2
    # is false: a = 1, the window 2 4 5 6.  Coordinate 1: sorted 1 2 5 6 NaN NaN, med = 5; j = 0: NaN, j = 1: NaN:
    # a = 0, the window 1 2 5 6.  Coordinate 2: -inf 1 2 5 6 inf, med = 2; j = 0: 6 - 2 < 2 + inf, j = 1: inf < 1
    # is false: a = 1, the window 1 2 5 6.  Coordinate 3: 1 2 3 4 5 6, med = 3; j = 0: 5 - 3 < 3 - 1 is false (a tie
    # goes to the lower value): a = 0, the window 1 2 3 4
    total, kept, high = R.bulyan_delta_sum(x, base, 1)
    assert total.tolist() == [17.0, 14.0, 14.0, 10.0]


# --------------------------------------------------------------------- through the Server
def check_round(result, f):
    """The attacker is not selected, the model moved, the new global state is ``before`` with the
    oracle's total over the selected rows applied through ``ops.add_noise_scaled``, and
    weight_result holds (names, kept share, score)."""
    before, after, finals, wr, n_upd, p = result
    assert len(wr) == 3
    names, share, scores = wr
    n = len(names)
    assert len(share) == n and len(scores) == n
    print(f"names {names}\nkept share {share}\nscores {scores}")
    i = names.index(41)
    rows = finals[:, :n_upd].cpu()
    # (the distances on the rows' own device: the server's bits)
    order, want_scores = agg.bulyan_select(ops.pairwise_sq_dists(finals[:, :n_upd]), f)
    sel = sorted(order)
    assert len(sel) == n - 2 * f and i not in sel
    assert share[i] == 0.0 and scores[i] == max(scores)
    assert scores == want_scores
    assert [j for j, v in enumerate(share) if v > 0.0] == sel
    total, want_kept, _ = bc.oracle(rows[sel].numpy(), before[:n_upd].cpu().numpy(), f)
    want = before.clone()
    dp_seed = (int(p["seed"]) * 7919 + 12) & 0x7FFFFFFF
    ops.add_noise_scaled(want[:n_upd], torch.from_numpy(total).to(want.device), float(p["eta"]) / (n - 4 * f),
                         float(p["sigma"]), dp_seed, bool(p["diff_privacy"]))
    assert torch.equal(after, want)
    assert not torch.equal(after[:n_upd], before[:n_upd])
    assert torch.equal(after[n_upd:], before[n_upd:])
    assert [share[j] for j in sel] == [float(v) / n_upd for v in want_kept.tolist()]
    return [names[j] for j in order]


def test_server_round_drops_the_attacker(tmp_path, monkeypatch):
    said = []
    log = logging.getLogger("logger")            # (the server sets it up without propagation: wrap its info)
    inner = log.info
    monkeypatch.setattr(log, "info", lambda msg, *a, **kw: (said.append(str(msg)), inner(msg, *a, **kw))[1])
    result = trim_cpu.run_round(tmp_path, krum_f=1, krum_bulyan=True)
    chosen = check_round(result, 1)
    lines = [m for m in said if m.startswith("[bulyan agg]")]
    assert len(lines) == 1
    n = len(result[3][0])
    assert f"f: 1  theta: {n - 2}  beta: {n - 4}  selected (in order): {chosen}  adversaries selected: 0/{n - 2}" \
        in lines[0]
    assert "kept share (* adversary): " in lines[0] and "41*: 0.0000" in lines[0]
    assert not any(m.startswith("[krum agg]") for m in said)


def test_server_round_with_diff_privacy(tmp_path):
    check_round(trim_cpu.run_round(tmp_path, krum_f=1, krum_bulyan=True, diff_privacy=True, sigma=0.001), 1)


def test_krum_bulyan_false_is_multi_krum(tmp_path):
    off = trim_cpu.run_round(tmp_path / "off", krum_f=1, krum_bulyan=False)
    plain = trim_cpu.run_round(tmp_path / "plain", krum_f=1)
    assert torch.equal(off[1], plain[1]) and off[3] == plain[3]
    assert set(off[3][1]) == {0.0, 1.0}                       # (Multi-Krum's selection mask)


def test_round_checks_the_client_count(tmp_path):
    """n >= 4 f + 3 against the round's own client count: no_models passes the config, the round
    has fewer clients."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    s = Server(trim_cpu.mnist_params(tmp_path, krum_f=1, krum_bulyan=True), DistCtx(), write_outputs=False)
    s.params["krum_f"] = 2                                    # 10 clients < 4 * 2 + 3
    with pytest.raises(ValueError, match=r"needs the round's clients >= 4 f \+ 3 = 11 \(got 10\)"):
        s.run_round(12)


def test_pretrain_stays_plain_fedavg(tmp_path):
    """The benign warm start runs with krum_f / krum_bulyan cleared and puts them back."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = trim_cpu.mnist_params(tmp_path, krum_f=1, krum_bulyan=True)
    s = Server(p, DistCtx(), write_outputs=False)
    seen = []
    inner = s._aggregate

    def wrapped(plan, bank, local, adversarial):
        seen.append((s.params["krum_f"], s.params["krum_bulyan"]))
        return inner(plan, bank, local, adversarial)
    s._aggregate = wrapped
    s.pretrain(1)
    assert seen == [(None, None)]
    assert s.params.krum_f == 1 and s.params.krum_bulyan is True
    assert not s.csv.weight_result                # (plain FedAvg records no weights)


def test_world_size_invariance(tmp_path):
    """Bulyan at worlds 1, 2, 4: every rank of every world holds the same final rows after the
    gather and does the same arithmetic on them, so the same state bits and weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "krum_f": 1,
            "krum_bulyan": True}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1 = trim_cpu.weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 3 and "41" in rows1[0]
    assert float(rows1[1][rows1[0].index("41")]) == 0.0
    assert sum(1 for v in rows1[1] if float(v) > 0.0) == len(rows1[0]) - 2
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, [12])
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert trim_cpu.weight_rows(str(tmp_path / f"w{world}")) == rows1


def test_no_collective_beyond_multi_krum(tmp_path):
    krum, _ = collectives.record_round(tmp_path / "krum", krum_f=1)
    bulyan, s = collectives.record_round(tmp_path / "bulyan", krum_f=1, krum_bulyan=True)
    assert bulyan == krum == []
    assert len(s.csv.weight_result) == 3

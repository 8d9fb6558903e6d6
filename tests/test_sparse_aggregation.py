"""SparseFed (config ``sparse_topk`` / ``sparse_clip``) on CPU: the config keys, the reference ops
against the numpy oracle of topk_cases.py bit for bit, a two-round hand case, the equivalences with
plain and norm-clipped FedAvg at full support, two rounds through ``Server`` replayed by the oracle,
the warm start, checkpoint / resume and world-size invariance."""
import csv
import os

import numpy as np
import pytest
import torch

from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.fl import aggregate as agg
from dba_mod_amd.ops import reference as R

import rlr_cases as rc
import topk_cases as tk
import test_trim_aggregation as trim_cpu
from conftest import ROOT

CFG = trim_cpu.CFG
CPU = torch.device("cpu")
FRAC = 0.05
ROUNDS = [12, 13]


# ------------------------------------------------------------------------------ config
def test_sparse_defaults_and_accepts():
    p = C.Params()
    assert p["sparse_topk"] is None and p.sparse_topk is None and p["sparse_clip"] is None and p.sparse_clip is None
    for f in (0.05, 1e-9, 0.5, 1.0):
        assert C.Params({"sparse_topk": f}).sparse_topk == f
    assert C.Params({"sparse_topk": 0.1, "sparse_clip": "median"}).sparse_clip == "median"
    assert C.Params({"sparse_topk": 0.1, "sparse_clip": 2}).sparse_clip == 2.0
    assert C.MEAN_OPTIONS[-1] == C.MeanOption("sparse_topk", ("sparse_clip",), False, None)
    assert C.mean_option(C.Params({"sparse_topk": 0.1})).key == "sparse_topk"
    assert C.AGGREGATIONS == ("mean", "geom_median", "foolsgold")


@pytest.mark.parametrize("bad", [True, False, 0, 1, 2, -0.5, 0.0, 1.5, float("nan"), float("inf"), "0.05", "all", [0.05]])
def test_sparse_topk_rejects_values(bad):
    with pytest.raises(ValueError, match="sparse_topk"):
        C.Params({"sparse_topk": bad})


@pytest.mark.parametrize("bad", [True, 0, -1.0, float("inf"), float("nan"), "mean", [1.0]])
def test_sparse_clip_rejects_values(bad):
    with pytest.raises(ValueError, match="sparse_clip"):
        C.Params({"sparse_topk": 0.05, "sparse_clip": bad})


def test_sparse_clip_needs_sparse_topk():
    with pytest.raises(ValueError, match="sparse_clip is set without sparse_topk"):
        C.Params({"sparse_clip": 1.0})
    with pytest.raises(ValueError, match="sparse_clip is set without sparse_topk"):
        C.Params({"sparse_clip": "median", "clip_norm": 1.0})


@pytest.mark.parametrize("other", [{"clip_norm": 1.0}, {"krum_f": 1}, {"trim_k": 2}, {"rlr_threshold": 4}])
def test_sparse_excludes_the_other_defences(other):
    with pytest.raises(ValueError, match="sparse_topk cannot be combined with clip_norm, krum_f, trim_k or rlr_threshold"):
        C.Params({"sparse_topk": 0.05, **other})


def test_sparse_excludes_diff_privacy_and_other_aggregations():
    with pytest.raises(ValueError, match="sparse_topk cannot be combined with diff_privacy"):
        C.Params({"sparse_topk": 0.05, "diff_privacy": True})
    for method in ("geom_median", "foolsgold"):
        with pytest.raises(ValueError, match="sparse_topk is an option of aggregation 'mean'"):
            C.Params({"sparse_topk": 0.05, "aggregation_methods": method})
        assert C.Params({"sparse_topk": None, "aggregation_methods": method}).sparse_topk is None


def test_existing_messages_are_unchanged():
    with pytest.raises(ValueError, match=r"^clip_norm 0: expected None, a finite number > 0 or 'median'$"):
        C.Params({"clip_norm": 0})
    with pytest.raises(ValueError, match=r"^rlr_threshold cannot be combined with clip_norm, krum_f or trim_k$"):
        C.Params({"rlr_threshold": 4, "trim_k": 1})
    with pytest.raises(ValueError, match=r"^krum_f and clip_norm cannot be combined$"):
        C.Params({"krum_f": 1, "clip_norm": 1.0})


def test_sparse_count():
    assert agg.sparse_count(2_802_430, 0.05) == 140_121
    assert [agg.sparse_count(L, 0.05) for L in (1, 19, 20, 39, 40)] == [1, 1, 1, 1, 2]
    assert agg.sparse_count(7, 1.0) == 7 and agg.sparse_count(7, 1e-9) == 1
    with pytest.raises(ValueError):
        agg.sparse_count(10, None)
    with pytest.raises(ValueError):
        agg.sparse_count(10, 1)


def test_shipped_recipe_loads():
    p = C.load_params(os.path.join(ROOT, "configs", "cifar_sparse.yaml"))
    assert p.sparse_topk == 0.05 and p.sparse_clip == "median" and p["aggregation_methods"] == "mean"
    assert p.clip_norm is None and p.krum_f is None and p.trim_k is None and p.rlr_threshold is None
    assert not p["diff_privacy"]


# -------------------------------------------------------- reference ops vs the numpy oracle
@pytest.mark.parametrize("name", tk.SMALL_CASES + [tk.WRAP_CASE])
def test_reference_ops_match_oracle(name):
    tk.check_case(ops, CPU, name)                  # (the registered ops, CPU dispatch)


def test_reference_module_is_what_the_ops_dispatch():
    resid0, total, dst0, ks = tk.case("ties")
    for k in ks[:3]:
        a, b = tk.run(ops, CPU, resid0, total, dst0, k), tk.run(R, CPU, resid0, total, dst0, k)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_keys_order_magnitudes():
    v = torch.tensor([0.0, -0.0, 5e-324, -1e-310, 1.0, -1.0, 1e308, float("inf"), float("-inf"), float("nan")],
                     dtype=torch.float64)
    keys = R.topk_keys(v).tolist()
    assert keys[0] == keys[1] == 0 and keys[4] == keys[5] and keys[7] == keys[8] == 0x7FF0000000000000
    assert keys[1] < keys[2] < keys[3] < keys[4] < keys[6] < keys[7] < keys[9]


def test_alignment_does_not_change_the_bits():
    tk.check_offsets(ops, CPU)


def test_degenerate_inputs():
    tk.check_degenerate(ops, CPU)


def test_full_support_is_add_noise_scaled():
    """(The reference ``add_noise_scaled`` multiplies by the Python coefficient, the HIP one and both
    ``topk_apply`` by its fp32 rounding: on CPU the equivalence is stated at a coefficient fp32 holds.)"""
    tk.check_full_support_is_fedavg(ops, CPU, 0.125)


# --------------------------------------------------------------------------- hand case
def test_hand_case_two_rounds():
    tk.check_hand_case(CPU)


# ------------------------------------------------------------------------ equivalences
def _clients(n=10, S=1203, seed=3):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(S, generator=g)
    finals = base[None] + 0.1 * torch.randn(n, S, generator=g)
    finals[3] = base + 30.0 * torch.randn(S, generator=g)          # one client far out: clipping bites
    return base, finals


def check_equivalences(dev, eta):
    """A ``sparse_topk: 1.0`` round from a zero residual has the bits of plain FedAvg, with
    ``sparse_clip`` those of ``clip_norm`` (and the same factors and norms), and the residual
    stays all zeros: twice in a row."""
    base, finals = (t.to(dev) for t in _clients())
    n, S = finals.shape
    n_upd = S - 3
    for clip in (None, "median", 2.5):
        w, v = base.clone(), base.clone()
        resid = torch.zeros(n_upd, dtype=torch.float64, device=dev)
        for _ in range(2):
            factors, norms, m, thr = agg.fedavg_sparse(w, finals, n_upd, clip, resid, eta, n, n_upd)
            if clip is None:
                agg.fedavg(v, finals, eta, n, False, 0.0, 1, n_upd)
                assert factors == [1.0] * n
            else:
                want = agg.fedavg_clipped(v, finals, clip, eta, n, False, 0.0, 1, n_upd)
                assert (factors, norms) == want and min(factors) < 1.0
            assert torch.equal(tk.bits(w), tk.bits(v)) and not torch.equal(w, base)
            assert m == n_upd and not tk.bits(resid).any()
            assert torch.equal(w[n_upd:], base[n_upd:])


def test_full_support_round_is_fedavg_and_clip_norm():
    check_equivalences(CPU, 1.25)                  # eta / n = 0.125: see test_full_support_is_add_noise_scaled


# --------------------------------------------------------------------- through the Server
class Recorder:
    """Wraps ``Server._aggregate`` to keep every round's global state before it and client final states."""

    def __init__(self, server):
        self.rounds, self.options = [], []
        inner = server._aggregate

        def wrapped(plan, bank, local, adversarial):
            self.options.append(server.params["sparse_topk"])
            self.rounds.append((server.global_state.clone(), bank[[c.final_snap for c in plan.clients]].clone()))
            return inner(plan, bank, local, adversarial)
        server._aggregate = wrapped


def make_server(tmp, device=None, write=False, **kw):
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    p = trim_cpu.mnist_params(tmp, **kw)
    return Server(p, DistCtx() if device is None else DistCtx(device=device), write_outputs=write)


def run_rounds(tmp, device=None, rounds=ROUNDS, **kw):
    """Rounds 12 (attacker 41 poisons, scale 100) and 13 of the MNIST synthetic run: (server, recorder)."""
    s = make_server(tmp, device, **kw)
    rec = Recorder(s)
    for e in rounds:
        s.run_round(e)
    return s, rec


def check_rounds(s, rec, frac=FRAC):
    """The final state and residual are the oracle's, replayed from the recorded final states: per
    round the fp64 delta sum in client order, added into the residual, the k largest applied."""
    p = s.params
    n_upd = s.spec.S if p["aggregate_bn_buffers"] else s.spec.P
    k = agg.sparse_count(n_upd, frac)
    coef = float(p["eta"]) / int(p["no_models"])
    resid = np.zeros(n_upd)
    kept_sets = []
    assert len(rec.rounds) == len(ROUNDS)
    for i, (before, finals) in enumerate(rec.rounds):
        b = before.cpu().numpy()
        total, _ = rc.oracle_votes(finals[:, :n_upd].cpu().numpy(), b[:n_upd])
        kept_sets.append(tk.keys_of(resid + total) >= tk.oracle(resid, total, b[:n_upd], k, coef)[2])
        resid, w, T, m = tk.oracle(resid, total, b[:n_upd], k, coef)
        after = rec.rounds[i + 1][0] if i + 1 < len(rec.rounds) else s.global_state
        tk.same_bits(after[:n_upd], w, ("state", i))
        assert torch.equal(after[n_upd:].cpu(), before[n_upd:].cpu())
        assert k <= m < n_upd
    tk.same_bits(s.sparse_residual, resid, "residual")
    assert resid.any() and not np.array_equal(kept_sets[0], kept_sets[1])
    wr = s.csv.weight_result
    assert len(wr) == 3 * len(ROUNDS)
    for i, (before, finals) in enumerate(rec.rounds):
        names, factors, norms = wr[3 * i:3 * i + 3]
        assert len(names) == finals.shape[0] and list(factors) == [1.0] * len(names)
        d = finals[:, :n_upd].double().cpu() - before[:n_upd].double().cpu()[None]
        np.testing.assert_allclose(norms, d.norm(dim=1).tolist(), rtol=1e-12)
    assert 41 in list(wr[0])


@pytest.fixture(scope="module")
def sparse_rounds(tmp_path_factory):
    return run_rounds(tmp_path_factory.mktemp("sparse"), sparse_topk=FRAC)


def test_server_rounds_equal_the_oracle(sparse_rounds):
    check_rounds(*sparse_rounds)


def test_off_is_plain_fedavg(tmp_path):
    """``sparse_topk: null`` takes plain FedAvg's path: the state after round 12 is ``before`` with the
    oracle's delta sum applied through ``ops.add_noise_scaled``; no residual, no weight rows."""
    s, rec = run_rounds(tmp_path, rounds=[12], sparse_topk=None, sparse_clip=None)
    before, finals = rec.rounds[0]
    n_upd = s.spec.S
    total, _ = rc.oracle_votes(finals[:, :n_upd].numpy(), before[:n_upd].numpy())
    want = before.clone()
    ops.add_noise_scaled(want[:n_upd], torch.from_numpy(total), float(s.params["eta"]) / 10, 0.0, 1, False)
    assert torch.equal(tk.bits(s.global_state), tk.bits(want))
    assert s.sparse_residual is None and not s.csv.weight_result


def test_pretrain_stays_plain_and_leaves_the_residual(tmp_path):
    s = make_server(tmp_path, sparse_topk=FRAC, sparse_clip="median")
    rec = Recorder(s)
    s.pretrain(1)
    assert rec.options == [None]
    assert s.params.sparse_topk == FRAC and s.params.sparse_clip == "median"
    assert s.sparse_residual is None and not s.csv.weight_result


def test_no_collective_beyond_the_borrowed_rule(tmp_path):
    """The [n] norms, then plain FedAvg's reduction or clip_norm's: select and apply add none."""
    import test_aggregation_collectives as coll
    seen, s = coll.record_round(tmp_path / "plain", sparse_topk=FRAC)
    n, n_upd = coll.sizes(s)
    assert seen == [("sum", coll.F64, (n,)), ("sum", coll.F64, (n_upd,))]
    seen, s = coll.record_round(tmp_path / "clip", sparse_topk=FRAC, sparse_clip="median")
    assert seen == [("sum", coll.F64, (n,)), coll.MAX, ("sum", coll.I64, (2, n_upd))]


# ------------------------------------------------------------------------------ resume
def test_resume_continues_with_the_same_bits(tmp_path, sparse_rounds):
    """Rounds 12 and 13 in one run against round 12, a checkpoint, and round 13 in a resumed run."""
    whole = sparse_rounds[0]
    first = make_server(tmp_path, write=True, save_model=True, sparse_topk=FRAC)
    first.run_round(12)
    name = os.path.join(first.folder, "model_last.pt.tar")
    aux = torch.load(name + ".aux", weights_only=True)
    assert aux["sparse_residual"].dtype == torch.float64 and aux["sparse_residual"].device.type == "cpu"
    assert torch.equal(tk.bits(aux["sparse_residual"]), tk.bits(first.sparse_residual)) and aux["sparse_residual"].any()
    rel = os.path.relpath(name, str(tmp_path))
    second = make_server(tmp_path, resumed_model=True, resumed_model_name=rel, sparse_topk=FRAC)
    assert second.start_epoch == 13
    assert torch.equal(tk.bits(second.sparse_residual), tk.bits(first.sparse_residual))
    second.run_round(13)
    assert torch.equal(tk.bits(second.global_state), tk.bits(whole.global_state))
    assert torch.equal(tk.bits(second.sparse_residual), tk.bits(whole.sparse_residual))


def test_aux_without_sparse_topk_has_no_residual(tmp_path):
    s = make_server(tmp_path, write=True, save_model=True, is_poison=False)
    s.run_round(12)
    name = os.path.join(s.folder, "model_last.pt.tar")
    assert "sparse_residual" not in torch.load(name + ".aux", weights_only=True)
    # ... and such an .aux resumes a sparse_topk run from a zero residual
    again = make_server(tmp_path, resumed_model=True, resumed_model_name=os.path.relpath(name, str(tmp_path)),
                        sparse_topk=FRAC)
    assert again.sparse_residual is None


# -------------------------------------------------------------------------- world size
def weight_rows(folder):
    with open(os.path.join(folder, "run", "weight_result.csv")) as f:
        return list(csv.reader(f))


def test_world_size_invariance(tmp_path):
    """sparse_topk with sparse_clip = median over rounds 12 and 13 at worlds 1, 2, 4: the total is
    the exact fixed-point clipped sum and every rank selects and applies on it redundantly, so the
    same state bits on every rank and the same weight_result rows."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "sparse_topk": FRAC,
            "sparse_clip": "median"}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, ROUNDS)
    rows1 = weight_rows(str(tmp_path / "w1"))
    assert len(rows1) == 6 and "41" in rows1[0]
    assert min(float(v) for v in rows1[1]) < 1.0                # (the attacker's update was clipped)
    for world in (2, 4):
        many = run_world(world, str(tmp_path / f"w{world}"), CFG, over, ROUNDS)
        for r in range(world):
            assert torch.equal(many[r]["state"], one[0]["state"]), (world, r)
        assert weight_rows(str(tmp_path / f"w{world}")) == rows1

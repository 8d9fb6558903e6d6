"""The norm-bounded (PGD) attacker through the trainer and the server on the CPU: round 12 of the
synthetic MNIST setup of test_clip_aggregation.py (attacker 41 poisons for 10 epochs at scale 100;
its free update has norm 24.2, the nine benign ones 0.055 .. 0.148).

DELTA = 0.15 is that file's CLIP_C: above every benign norm, 160x below the free attacker's, so the
attacker projects (radius 0.0015 before scaling, 0.15 under ``baseline``) and nobody else is clipped.
"""
import csv
import json
import os
import types

import pytest
import torch

from dba_mod_amd import config as C

from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")
DELTA = 0.15
ATTACKER = 41


def _params(tmp, **kw):
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 4000,
            "synthetic_test_size": 600, "save_dir": str(tmp), "eval_batch_size": 300}
    base.update(kw)
    return C.load_params(CFG, base)


def _round(tmp, aggregate=False, **kw):
    """Train round 12 (and aggregate it): {"global", "n_upd", "res": name -> ClientResult, "final":
    name -> final state, "weights": weight_result rows}."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    s = Server(_params(tmp, **kw), DistCtx(), write_outputs=False)
    before = s.global_state.clone()
    st = s._train_begin(12, evaluate=False)
    results = st["handle"].collect()
    res = {r.name: r for r in results}
    final = {c.name: res[c.name].snapshots[c.final_snap].clone() for c in st["plan"].clients}
    out = {"global": before, "n_upd": s.spec.S if s.params["aggregate_bn_buffers"] else s.spec.P, "res": res,
           "final": final, "radius": s.trainer.pgd_radius}
    if aggregate:
        st["handle"] = types.SimpleNamespace(collect=lambda: results)
        s._train_end(st)
        out["weights"] = [list(r) for r in s.csv.weight_result]
    return out


def _update_norm(run, name):
    n = run["n_upd"]
    return float((run["final"][name].double() - run["global"].double())[:n].norm())


@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    mk = tmp_path_factory.mktemp
    return {
        "free": _round(mk("free"), aggregate=True, clip_norm=DELTA),
        "pgd": _round(mk("pgd"), aggregate=True, clip_norm=DELTA, poison_pgd_norm=DELTA),
        "baseline": _round(mk("base"), poison_pgd_norm=DELTA, baseline=True),
        "huge": _round(mk("huge"), poison_pgd_norm=1e30),
    }


def test_scaled_update_stays_within_delta(rounds):
    run = rounds["pgd"]
    assert run["radius"] == DELTA / 100.0
    r = run["res"][ATTACKER]
    got, free = _update_norm(run, ATTACKER), _update_norm(rounds["free"], ATTACKER)
    print(f"attacker update norm: {got!r} with poison_pgd_norm {DELTA}, {free!r} without; projected "
          f"{r.pgd_steps}/{r.steps} steps, last norm before projection {r.pgd_last_norm!r}")
    assert got <= DELTA * (1 + 1e-5)        # (scaling by gamma: one more fp32 rounding per entry)
    assert free > 10 * DELTA                # the same round without the key violates it
    assert 0 < r.pgd_steps <= r.steps
    assert r.pgd_last_norm > run["radius"]
    # the trainer's "distance before scaling" is within the radius by construction
    assert r.scale_norms[12][2] <= run["radius"] * (1 + 1e-5)


def test_baseline_update_stays_within_delta(rounds):
    run = rounds["baseline"]
    assert run["radius"] == DELTA
    r = run["res"][ATTACKER]
    got = _update_norm(run, ATTACKER)
    print(f"attacker update norm under baseline: {got!r}; projected {r.pgd_steps}/{r.steps} steps")
    assert got <= DELTA * (1 + 1e-5)
    assert r.pgd_steps > 0


def test_benign_clients_keep_their_bits(rounds):
    a, b = rounds["pgd"], rounds["free"]
    assert a["final"].keys() == b["final"].keys() and len(a["final"]) == 10
    for name in a["final"]:
        if name != ATTACKER:
            assert torch.equal(a["final"][name], b["final"][name]), name
            assert a["res"][name].pgd_steps == 0 and a["res"][name].pgd_last_norm == 0.0
    assert not torch.equal(a["final"][ATTACKER], b["final"][ATTACKER])


def test_huge_delta_changes_nothing(rounds):
    a, b = rounds["huge"], rounds["free"]
    for name in a["final"]:
        assert torch.equal(a["final"][name], b["final"][name]), name
    r = a["res"][ATTACKER]
    assert r.pgd_steps == 0 and 0.0 < r.pgd_last_norm < 1.0     # (the norm is still published)
    assert b["res"][ATTACKER].pgd_steps == 0 and b["res"][ATTACKER].pgd_last_norm == 0.0


def test_server_no_longer_clips_the_attacker(rounds):
    names, factors, norms = rounds["pgd"]["weights"]
    i = names.index(ATTACKER)
    print(f"clip factor of the attacker: {factors[i]!r} (norm {norms[i]!r}) with poison_pgd_norm, "
          f"{rounds['free']['weights'][1][i]!r} without")
    assert abs(factors[i] - 1.0) <= 1e-5
    assert norms[i] <= DELTA * (1 + 1e-5)
    names0, factors0, _ = rounds["free"]["weights"]
    assert names0 == names and factors0[i] < 0.1


def _rank0_files(folder):
    with open(os.path.join(folder, "run", "weight_result.csv")) as f:
        rows = list(csv.reader(f))
    with open(os.path.join(folder, "run", "metrics.jsonl")) as f:
        pgd = [json.loads(line)["pgd"] for line in f if line.strip()]
    return rows, pgd


def test_world_size_invariance(tmp_path):
    """Worlds 1 and 2 under gloo: the same global model bits on every rank, the same clip factors and
    the same projected-step count in rank 0's metrics.jsonl (the attacker trains on one rank; its
    two numbers travel in the per-client scalar all-reduce)."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 12, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200, "clip_norm": DELTA,
            "poison_pgd_norm": DELTA}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [12])
    rows1, pgd1 = _rank0_files(str(tmp_path / "w1"))
    assert list(pgd1[0]) == [str(ATTACKER)] and pgd1[0][str(ATTACKER)]["pgd_steps"] > 0
    two = run_world(2, str(tmp_path / "w2"), CFG, over, [12])
    for r in range(2):
        assert torch.equal(two[r]["state"], one[0]["state"]), r
    assert _rank0_files(str(tmp_path / "w2")) == (rows1, pgd1)

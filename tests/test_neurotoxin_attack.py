"""The Neurotoxin attacker through the trainer and the server on the CPU: rounds 11 (benign: it only
builds the mask) and 12 (attacker 41 poisons for 10 epochs at scale 100, under round 11's mask) of the
synthetic MNIST setup of test_pgd_attack.py; rounds 13 / 14 (attacker 73) for the resume.

Everything is exact: outside the mask the attacker's submitted update is 0 bit for bit, the mask is
the numpy oracle's (neurotoxin_cases.py) for the previous round's two global models, and a resumed
run, a two-rank run and a ``rho = 1.0`` run reproduce the bits they must.
"""
import json
import logging
import math
import os
import types

import pytest
import torch

import neurotoxin_cases as K
from dba_mod_amd import config as C

from conftest import ROOT

CFG = os.path.join(ROOT, "configs", "mnist_params.yaml")
RHO = 0.9
ATTACKER = 41
DELTA = 0.15        # test_pgd_attack.py's bound


def _params(tmp, **kw):
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 4000,
            "synthetic_test_size": 600, "save_dir": str(tmp), "eval_batch_size": 300}
    base.update(kw)
    return C.load_params(CFG, base)


def _server(tmp, write=False, **kw):
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    return Server(_params(tmp, **kw), DistCtx(), write_outputs=write)


def _keep(mask, P):
    return K.unpack(mask.cpu(), P)


def _two_rounds(tmp, **kw):
    """Round 11 through the server, then round 12 trained (and aggregated): the global models, round
    11's mask, every client's final state and result, and round 12's record."""
    s = _server(tmp, **kw)
    g10 = s.global_state.clone()
    s.run_round(11)
    rec11 = dict(s.last_round)
    g11 = s.global_state.clone()
    mask = s.trainer.ntx_mask.clone() if s.trainer.ntx_mask is not None else None
    st = s._train_begin(12, evaluate=False)
    results = st["handle"].collect()
    res = {r.name: r for r in results}
    final = {c.name: res[c.name].snapshots[c.final_snap].clone() for c in st["plan"].clients}
    st["handle"] = types.SimpleNamespace(collect=lambda: results)
    pend = s._train_end(st)
    return {"s": s, "g10": g10, "g11": g11, "g12": s.global_state.clone(), "mask": mask, "res": res, "final": final,
            "rec11": rec11, "pend": pend, "P": s.spec.P}


@pytest.fixture(scope="module")
def rounds(tmp_path_factory):
    mk = tmp_path_factory.mktemp
    return {
        "free": _two_rounds(mk("free")),
        "ntx": _two_rounds(mk("ntx"), poison_neurotoxin_ratio=RHO),
        "one": _two_rounds(mk("one"), poison_neurotoxin_ratio=1.0),
        "both": _two_rounds(mk("both"), poison_neurotoxin_ratio=RHO, poison_pgd_norm=DELTA),
    }


def test_yaml_int_is_not_a_ratio(tmp_path):
    with pytest.raises(ValueError, match="poison_neurotoxin_ratio"):
        _params(tmp_path, poison_neurotoxin_ratio=1)
    for other in ({"aggregation_methods": "foolsgold"}, {"aggr_epoch_interval": 2}, {"is_poison": False}):
        with pytest.raises(ValueError, match="poison_neurotoxin_ratio"):
            _params(tmp_path, poison_neurotoxin_ratio=RHO, **other)


def test_mask_is_the_oracles_for_the_previous_round(rounds):
    run = rounds["ntx"]
    P = run["P"]
    k = max(1, math.floor(RHO * P))
    want, T, m = K.mask_oracle(run["g11"].cpu(), run["g10"].cpu(), P, k)
    assert torch.equal(run["mask"].cpu(), want)
    rec = run["rec11"]["neurotoxin"]
    thr = float(torch.tensor([T], dtype=torch.int32).view(torch.float32)[0])
    assert (rec["rho"], rec["k"], rec["kept"], rec["threshold"]) == (RHO, k, m, thr) and k <= m < P
    assert "clients" not in rec                     # (a benign round: nobody trained with a trigger)
    # the round after: from g12 and g11, and nothing past P (the BN-free MNIST net has S == P; tail bits 0)
    want12, _, _ = K.mask_oracle(run["g12"].cpu(), run["g11"].cpu(), P, k)
    assert torch.equal(run["s"].trainer.ntx_mask.cpu(), want12) and not torch.equal(want12, want)


def test_attackers_update_is_zero_outside_the_mask(rounds):
    run = rounds["ntx"]
    P = run["P"]
    keep = _keep(run["mask"], P)
    upd = (run["final"][ATTACKER] - run["g11"])[:P]
    outside = int((~keep).sum())
    print(f"attacker update: {int((upd != 0).sum())} of {P} entries non-zero, {outside} entries outside the mask")
    assert outside > 0 and bool((upd[~keep] == 0).all())
    assert torch.equal(run["final"][ATTACKER][:P][~keep], run["g11"][:P][~keep])      # (bit for bit: a copy)
    assert bool((upd[keep] != 0).any())
    r = run["res"][ATTACKER]
    assert r.ntx_steps == r.steps > 0
    # the same round's free attacker moves entries outside that mask
    free = (rounds["free"]["final"][ATTACKER] - rounds["free"]["g11"])[:P]
    assert bool((free[~keep] != 0).any())


def test_benign_clients_keep_their_bits(rounds):
    a, b = rounds["ntx"], rounds["free"]
    assert torch.equal(a["g11"], b["g11"])
    assert a["final"].keys() == b["final"].keys() and len(a["final"]) == 10
    for name in a["final"]:
        if name != ATTACKER:
            assert torch.equal(a["final"][name], b["final"][name]), name
            assert a["res"][name].ntx_steps == 0
    assert not torch.equal(a["final"][ATTACKER], b["final"][ATTACKER])
    assert b["res"][ATTACKER].ntx_steps == 0 and b["mask"] is None and "neurotoxin" not in b["rec11"]


def test_ratio_one_gives_the_bits_of_the_key_off(rounds):
    a, b = rounds["one"], rounds["free"]
    assert torch.equal(a["mask"].cpu(), K.pack(torch.ones(a["P"], dtype=torch.bool)))
    for name in a["final"]:
        assert torch.equal(a["final"][name], b["final"][name]), name
    assert torch.equal(a["g12"], b["g12"])
    assert a["res"][ATTACKER].ntx_steps == a["res"][ATTACKER].steps


def test_with_pgd_the_update_is_inside_the_mask_and_the_bound(rounds):
    run = rounds["both"]
    P = run["P"]
    keep = _keep(run["mask"], P)
    assert torch.equal(run["mask"], rounds["ntx"]["mask"])
    upd = (run["final"][ATTACKER].double() - run["g11"].double())[:P]
    got = float(upd.norm())
    r = run["res"][ATTACKER]
    print(f"attacker update norm {got!r} (bound {DELTA}); projected {r.pgd_steps}/{r.steps} steps, restored after "
          f"{r.ntx_steps}")
    assert bool((upd[~keep] == 0).all()) and bool((upd[keep] != 0).any())
    assert got <= DELTA * (1 + 1e-5)            # test_pgd_attack.py's bound
    assert r.pgd_steps > 0 and r.ntx_steps == r.steps


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_first_round_is_unconstrained_and_says_so(tmp_path):
    h = _Lines()
    lg = logging.getLogger("logger")
    s = _server(tmp_path, start_epoch=12, poison_neurotoxin_ratio=RHO)
    lg.addHandler(h)
    try:
        assert not s.ntx_have_mask
        assert torch.equal(s.trainer.ntx_mask.cpu(), K.pack(torch.ones(s.spec.P, dtype=torch.bool)))
        s.run_round(12)
    finally:
        lg.removeHandler(h)
    rec = s.last_round["neurotoxin"]
    assert rec["masked"] is False and s.ntx_have_mask
    assert rec["clients"] == {str(ATTACKER): {"ntx_steps": rec["clients"][str(ATTACKER)]["steps"],
                                              "steps": rec["clients"][str(ATTACKER)]["steps"]}}
    ours = [ln for ln in h.lines if ln.startswith("[neurotoxin]")]
    assert len(ours) == 3, ours
    assert any("unconstrained" in ln for ln in ours) and any(f"local model {ATTACKER}" in ln for ln in ours)
    assert any(f"k: {rec['k']}" in ln and f"kept: {rec['kept']}/" in ln for ln in ours)
    # the same round with the key off: the same global model (an all-kept mask restores nothing)
    s0 = _server(tmp_path / "off", start_epoch=12)
    s0.run_round(12)
    assert torch.equal(s.global_state, s0.global_state)


def test_warm_start_builds_no_mask(tmp_path):
    s = _server(tmp_path, start_epoch=12, pretrain_rounds=1, poison_neurotoxin_ratio=RHO)
    assert not s.ntx_have_mask
    assert torch.equal(s.trainer.ntx_mask.cpu(), K.pack(torch.ones(s.spec.P, dtype=torch.bool)))


# ------------------------------------------------------------------------------ resume
def test_resume_continues_with_the_same_bits(tmp_path):
    """Rounds 13 and 14 (attacker 73 poisons under round 13's mask) in one run against round 13, a
    checkpoint, and round 14 in a resumed run."""
    whole = _server(tmp_path / "whole", start_epoch=13, poison_neurotoxin_ratio=RHO)
    whole.run_round(13)
    whole.run_round(14)
    assert whole.last_round["neurotoxin"]["masked"] is True and list(whole.last_round["neurotoxin"]["clients"]) == ["73"]
    first = _server(tmp_path, write=True, save_model=True, start_epoch=13, poison_neurotoxin_ratio=RHO)
    first.run_round(13)
    name = os.path.join(first.folder, "model_last.pt.tar")
    aux = torch.load(name + ".aux", weights_only=True)
    nw = K.n_words(first.spec.P)
    assert aux["neurotoxin_mask"].dtype == torch.int64 and aux["neurotoxin_mask"].shape == (nw,)
    assert torch.equal(aux["neurotoxin_mask"], first.trainer.ntx_mask.cpu())
    rel = os.path.relpath(name, str(tmp_path))
    second = _server(tmp_path, resumed_model=True, resumed_model_name=rel, poison_neurotoxin_ratio=RHO)
    assert second.start_epoch == 14 and second.ntx_have_mask
    assert torch.equal(second.trainer.ntx_mask, first.trainer.ntx_mask)
    second.run_round(14)
    assert second.last_round["neurotoxin"] == whole.last_round["neurotoxin"]
    assert torch.equal(second.global_state, whole.global_state)
    assert torch.equal(second.trainer.ntx_mask, whole.trainer.ntx_mask)
    # the attacker of round 14 did use that mask: the free run differs
    off = _server(tmp_path / "off", start_epoch=13)
    off.run_round(13)
    off.run_round(14)
    assert not torch.equal(off.global_state, whole.global_state)


def test_aux_without_the_key_resumes_all_kept(tmp_path):
    s = _server(tmp_path, write=True, save_model=True, start_epoch=13)
    s.run_round(13)
    name = os.path.join(s.folder, "model_last.pt.tar")
    assert "neurotoxin_mask" not in torch.load(name + ".aux", weights_only=True)
    again = _server(tmp_path, resumed_model=True, resumed_model_name=os.path.relpath(name, str(tmp_path)),
                    poison_neurotoxin_ratio=RHO)
    assert not again.ntx_have_mask
    assert torch.equal(again.trainer.ntx_mask.cpu(), K.pack(torch.ones(again.spec.P, dtype=torch.bool)))


# -------------------------------------------------------------------------- world size
def _rank0_records(folder):
    with open(os.path.join(folder, "run", "metrics.jsonl")) as f:
        return [json.loads(line)["neurotoxin"] for line in f if line.strip()]


def test_world_size_invariance(tmp_path):
    """Worlds 1 and 2 under gloo over rounds 11 and 12: every rank builds the same mask (integer keys
    and counts), so the same global model bits on every rank and the same k, m, threshold and
    per-client step counts in rank 0's metrics.jsonl."""
    from dba_mod_amd.tools.dist_check import run_world
    over = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 3000,
            "synthetic_test_size": 400, "save_dir": str(tmp_path), "eval_batch_size": 200,
            "poison_neurotoxin_ratio": RHO}
    one = run_world(1, str(tmp_path / "w1"), CFG, over, [11, 12])
    rec1 = _rank0_records(str(tmp_path / "w1"))
    assert len(rec1) == 2 and rec1[1]["masked"] is True and list(rec1[1]["clients"]) == [str(ATTACKER)]
    assert rec1[1]["clients"][str(ATTACKER)]["ntx_steps"] > 0
    two = run_world(2, str(tmp_path / "w2"), CFG, over, [11, 12])
    for r in range(2):
        assert torch.equal(two[r]["state"], one[0]["state"]), r
    assert _rank0_records(str(tmp_path / "w2")) == rec1

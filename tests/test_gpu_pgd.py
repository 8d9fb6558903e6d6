"""The norm-bounded (PGD) attacker on the GPU: ``project_to_ball`` (flat.hip ballnorm_kernel /
ballproj_kernel) on the cases of pgd_cases.py against the fp64 oracle, bit for bit run to run and
one replica alone against inside the group; the projection inside the captured training step
(graph replay vs eager, the solo tail) and on LOAN's per-step path."""
import os

import numpy as np
import pytest
import torch

import pgd_cases as K

pytestmark = pytest.mark.gpu
WHO = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip  # noqa: F401  (must load: no silent fallback)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def H(dev):
    from dba_mod_amd.ops import hip
    return hip


@pytest.mark.parametrize("case", K.PGD_CASES, ids=K.pgd_id)
def test_project_to_ball(H, dev, case):
    a = K.run_pgd(H, case, dev, WHO)
    K.same_bits(a, K.run_pgd(H, case, dev, WHO), "run to run")
    for g in range(K.G):      # a replica's result does not depend on its neighbours
        K.same_bits(K.pick(a, g), K.pick(K.run_pgd(H, case, dev, WHO, sel=g), g), "G = 1 vs G = 6")


@pytest.mark.parametrize("case", K.EXACT_CASES, ids=K.pgd_id)
def test_project_to_ball_exact_boundary(H, dev, case):
    a = K.run_exact(H, case, dev, WHO)
    K.same_bits(a, K.run_exact(H, case, dev, WHO), "run to run")


def test_project_to_ball_is_graph_capturable(H, dev):
    """No host read, no atomics: the two launches replay from a captured graph with the eager bits."""
    n, lay = 2049, "packed"
    i = K.pgd_inputs(n, lay)
    outs = []
    for capture in (False, True):
        _, w = K.place(i["w"], 0, n + K.PAD, dev)
        _, base = K.place(i["base"], 0, n + K.PAD, dev)
        trig, active = i["trig"].to(dev), i["active"].to(dev)
        norm = torch.zeros(K.G, dtype=torch.float64, device=dev)
        count = torch.zeros(K.G, dtype=torch.int32, device=dev)
        if capture:
            keep = w.clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                H.project_to_ball(w, base, n, trig, active, i["r"], norm, count)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                H.project_to_ball(w, base, n, trig, active, i["r"], norm, count)
            w.copy_(keep)
            norm.zero_()
            count.zero_()
            g.replay()
        else:
            H.project_to_ball(w, base, n, trig, active, i["r"], norm, count)
        torch.cuda.synchronize()
        outs.append({"w": w.cpu(), "norm": norm.cpu(), "count": count.cpu()})
    assert outs[0]["count"].tolist() == [1, 0, 0, 0, 0, 0]
    K.same_bits(outs[0], outs[1], "graph replay vs eager")


# ------------------------------------------------------------------ inside the training step
DELTA = 0.15         # tests/test_pgd_attack.py: above every benign MNIST update norm, 160x below the attacker's


def _small_params(**kw):
    from dba_mod_amd import config as C
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 6000,
            "synthetic_test_size": 1000, "save_model": False, "eval_batch_size": 256, "poison_pgd_norm": DELTA}
    base.update(kw)
    return C.load_params(os.path.join(ROOT, "configs", "mnist_params.yaml"), base)


def test_graph_replay_matches_eager(dev, tmp_path):
    """The projection's two launches and its counter live in the captured step: the same global
    model bits and the same projected-step count as the eager step."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    outs = []
    for cap in (False, True):
        s = Server(_small_params(graph_capture=cap, save_dir=str(tmp_path)), DistCtx(device=dev), write_outputs=False)
        assert s.trainer.use_graph == cap and s.trainer.pgd_radius == DELTA / 100.0
        s.run_round(11)
        assert "pgd" not in s.last_round              # a benign round
        s.run_round(12)                               # attacker 41 poisons
        outs.append((s.global_state.clone(), s.last_round["pgd"]))
    assert list(outs[0][1]) == ["41"] and outs[0][1]["41"]["pgd_steps"] > 0
    assert outs[1][1] == outs[0][1]
    assert torch.equal(outs[1][0], outs[0][0])


def test_solo_tail_bitwise(dev, tmp_path):
    """The attacker's tail in the G = 1 graph (its projection counter and last norm carried across
    the hand-off) against a run that keeps it in the group graph: the same bits, the same counts."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    got = []
    for solo in (0, 4):
        s = Server(_small_params(save_dir=str(tmp_path / f"s{solo}")), DistCtx(device=dev), write_outputs=False)
        s.trainer.SOLO_MIN_STEPS = solo
        st = s._train_begin(12)
        if solo:
            assert s.trainer._solo_tail(st["plan"].clients, max(len(c.steps) for c in st["plan"].clients))
        got.append({r.name: r for r in st["handle"].collect()})
    a, b = got
    assert a.keys() == b.keys() and a[41].pgd_steps > 0
    for name in a:
        ra, rb = a[name], b[name]
        assert ra.snapshots.keys() == rb.snapshots.keys()
        for k in ra.snapshots:
            assert torch.equal(ra.snapshots[k], rb.snapshots[k]), (name, k)
        assert np.array_equal(ra.stats, rb.stats), name
        assert (ra.pgd_steps, ra.pgd_last_norm) == (rb.pgd_steps, rb.pgd_last_norm), name


def _loan_round(dev, tmp, **kw):
    from dba_mod_amd import config as C
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    base = {"resumed_model": False, "pretrain_rounds": 0, "synthetic_data": True, "synthetic_train_size": 60000,
            "synthetic_test_size": 4000, "save_model": False, "save_dir": str(tmp)}
    base.update(kw)
    s = Server(C.load_params(os.path.join(ROOT, "configs", "loan_params.yaml"), base), DistCtx(device=dev),
               write_outputs=False)
    before = s.global_state.clone()
    st = s._train_begin(13)                   # attacker MO poisons: 10 epochs, then scaling by 30
    res = {r.name: r for r in st["handle"].collect()}
    adv = [c for c in st["plan"].clients if any(ph.poison for ph in c.phases)]
    assert len(adv) == 1
    n_upd = s.spec.S if s.params["aggregate_bn_buffers"] else s.spec.P
    upd = (res[adv[0].name].snapshots[adv[0].final_snap].double() - before.double())[:n_upd]
    return s, res[adv[0].name], float(upd.norm())


def test_loan_round_takes_the_per_step_path(dev, tmp_path):
    """LOAN with the key on: the persistent launch (no per-step hook) is off, the round trains on the
    per-step path, and the attacker's scaled update stays within delta.  delta is a quarter of the
    update norm the same round's free attacker submits (measured here, with the key off)."""
    s0, _, free = _loan_round(dev, tmp_path / "free")
    assert s0.trainer.persistent and s0.trainer.pgd_radius is None
    delta = free / 4
    s, r, got = _loan_round(dev, tmp_path / "pgd", poison_pgd_norm=delta)
    assert not s.trainer.persistent and s.trainer.use_graph
    assert s.trainer.pgd_radius == delta / float(s.params["scale_weights_poison"])
    print(f"LOAN attacker update norm: {got!r} with poison_pgd_norm {delta!r}, {free!r} without; projected "
          f"{r.pgd_steps}/{r.steps} steps")
    assert got <= delta * (1 + 1e-5)
    assert 0 < r.pgd_steps <= r.steps

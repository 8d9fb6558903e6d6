"""The Neurotoxin attacker on the GPU: ``neurotoxin_mask`` (nmask.hip) and ``mask_restore`` (flat.hip
maskrestore_kernel) on the cases of neurotoxin_cases.py against the numpy oracle, bit for bit, run
to run and one replica alone against inside the group; the restore inside the captured training
step (graph replay vs eager, the mask rewritten in place between replays, the solo tail) and on
LOAN's per-step path."""
import os

import numpy as np
import pytest
import torch

import neurotoxin_cases as K

pytestmark = pytest.mark.gpu
WHO = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 0.9


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


def test_cases_sit_on_the_kernels_grid_rule(H):
    assert H.nmask_geometry() == (K.NMASK_SWEEP, K.NMASK_BLOCKS_MAX)
    sweep, blocks = H.nmask_geometry()
    for P, want in ((1, 1), (sweep, 1), (sweep + 1, 2), (sweep * blocks, blocks), (sweep * blocks + 1029, blocks)):
        assert int(H._L.dba_nmask_blocks(P)) == want, P


@pytest.mark.parametrize("case", K.MASK_CASES, ids=K.mask_id)
def test_neurotoxin_mask(H, dev, case):
    a = K.run_mask(H, case, dev, WHO, make_ws=H.neurotoxin_workspace)
    K.same_bits(a, K.run_mask(H, case, dev, WHO, make_ws=H.neurotoxin_workspace), "run to run")
    K.same_bits(a, K.run_mask(H, case, dev, WHO), "a fresh workspace per call")


@pytest.mark.parametrize("k", [0, -1, 11])
def test_neurotoxin_mask_rejects_k(H, dev, k):
    w = torch.arange(10, dtype=torch.float32, device=dev)
    words = torch.full((1,), K.CANARY, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="neurotoxin_mask"):
        H.neurotoxin_mask(w, torch.zeros_like(w), 10, k, words)
    # the entry point itself: hipErrorInvalidValue (1), nothing launched
    sel, ws = torch.zeros(2, dtype=torch.int64, device=dev), H.neurotoxin_workspace(dev)
    rc = H._L.dba_neurotoxin_mask(w.data_ptr(), w.data_ptr(), 10, k, words.data_ptr(), sel.data_ptr(), ws.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 1 and words.tolist() == [K.CANARY] and sel.tolist() == [0, 0]


@pytest.mark.parametrize("case", K.RESTORE_CASES, ids=K.restore_id)
def test_mask_restore(H, dev, case):
    a = K.run_restore(H, case, dev, WHO)
    K.same_bits(a, K.run_restore(H, case, dev, WHO), "run to run")
    for g in range(K.G):      # a replica's result does not depend on its neighbours
        K.same_bits(K.pick(a, g), K.pick(K.run_restore(H, case, dev, WHO, sel=g), g), "G = 1 vs G = 6")


def test_mask_restore_replays_under_a_mask_rewritten_in_place(H, dev):
    """No host read: the launch replays from a captured graph with the eager bits, and a replay after
    the mask buffer was rewritten in place obeys the new mask (nothing is re-captured)."""
    n, lay = 2049, "packed"
    i = K.restore_inputs(n, lay, 0.5)
    _, w = K.place(i["w"], 0, n + K.PAD, dev)
    _, base = K.place(i["base"], 0, n + K.PAD, dev)
    trig, active = i["trig"].to(dev), i["active"].to(dev)
    count = torch.zeros(K.G, dtype=torch.int32, device=dev)
    mask = K.pack(i["keep"]).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        H.mask_restore(w, base, n, trig, active, mask, count)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        H.mask_restore(w, base, n, trig, active, mask, count)
    other = ~i["keep"]
    for keep in (i["keep"], other):
        w.copy_(i["w"].to(dev))
        count.zero_()
        mask.copy_(K.pack(keep).to(dev))            # in place: the graph holds this pointer
        g.replay()
        torch.cuda.synchronize()
        K.check_exact(w, K.restore_oracle(i["w"], i["base"], n, keep, K.GATED), K.OP_RESTORE, "w, graph replay", WHO)
        assert count.tolist() == [int(q) for q in K.GATED]


# ------------------------------------------------------------------ inside the training step
def _small_params(**kw):
    from dba_mod_amd import config as C
    base = {"resumed_model": False, "start_epoch": 11, "synthetic_data": True, "synthetic_train_size": 6000,
            "synthetic_test_size": 1000, "save_model": False, "eval_batch_size": 256, "poison_neurotoxin_ratio": RHO}
    base.update(kw)
    return C.load_params(os.path.join(ROOT, "configs", "mnist_params.yaml"), base)


def _attacker_update(s, epoch, name):
    """Train round ``epoch`` (not aggregated): (update of client ``name`` over the parameters, its result)."""
    before = s.global_state.clone()
    st = s._train_begin(epoch, evaluate=False)
    res = {r.name: r for r in st["handle"].collect()}
    c = next(c for c in st["plan"].clients if c.name == name)
    return (res[name].snapshots[c.final_snap] - before)[:s.spec.P].cpu(), res[name]


def test_graph_replay_matches_eager_and_obeys_each_rounds_mask(dev, tmp_path):
    """The restore and its counter live in the captured step: the same global model bits and the same
    record as the eager step.  The graphs captured in round 11 replay in rounds 12 and 14 under the
    masks of rounds 11 and 13, written in place into the one buffer they point at."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    outs = []
    for cap in (False, True):
        s = Server(_small_params(graph_capture=cap, save_dir=str(tmp_path)), DistCtx(device=dev), write_outputs=False)
        assert s.trainer.use_graph == cap and s.trainer.ntx_mask is not None
        ptr = s.trainer.ntx_mask.data_ptr()
        g10 = s.global_state.clone()
        s.run_round(11)
        assert s.last_round["neurotoxin"]["masked"] is False and "clients" not in s.last_round["neurotoxin"]
        P = s.spec.P
        want, T, m = K.mask_oracle(s.global_state.cpu(), g10.cpu(), P, s.last_round["neurotoxin"]["k"])
        assert torch.equal(s.trainer.ntx_mask.cpu(), want) and s.last_round["neurotoxin"]["kept"] == m
        graphs = {key: b.graph for key, b in s.trainer._bufs.items()}
        s.run_round(12)                               # attacker 41 poisons under round 11's mask
        outs.append((s.global_state.clone(), s.last_round["neurotoxin"]))
        if cap:
            s.run_round(13)
            mask13 = s.trainer.ntx_mask.clone()
            assert not torch.equal(mask13.cpu(), want)
            upd, r = _attacker_update(s, 14, 73)      # attacker 73 poisons under round 13's mask
            keep = K.unpack(mask13.cpu(), P)
            assert bool((upd[~keep] == 0).all()) and bool((upd[keep] != 0).any()) and r.ntx_steps == r.steps > 0
            assert s.trainer.ntx_mask.data_ptr() == ptr
            for key, gr in graphs.items():            # nothing was re-captured
                assert gr is not None and s.trainer._bufs[key].graph is gr, key
    rec = outs[0][1]
    assert rec["masked"] is True and list(rec["clients"]) == ["41"] and rec["clients"]["41"]["ntx_steps"] > 0
    assert outs[1][1] == rec
    assert torch.equal(outs[1][0], outs[0][0])


def test_solo_tail_bitwise(dev, tmp_path):
    """The attacker's tail in the G = 1 graph (the same mask buffer, its step counter carried across
    the hand-off) against a run that keeps it in the group graph: the same bits, the same counts; and
    the update it submits is 0 outside the mask."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    got = []
    for solo in (0, 4):
        s = Server(_small_params(save_dir=str(tmp_path / f"s{solo}")), DistCtx(device=dev), write_outputs=False)
        s.trainer.SOLO_MIN_STEPS = solo
        s.run_round(11)
        before, keep = s.global_state.clone(), K.unpack(s.trainer.ntx_mask.cpu(), s.spec.P)
        st = s._train_begin(12)
        if solo:
            assert s.trainer._solo_tail(st["plan"].clients, max(len(c.steps) for c in st["plan"].clients))
        res = {r.name: r for r in st["handle"].collect()}
        c = next(c for c in st["plan"].clients if c.name == 41)
        upd = (res[41].snapshots[c.final_snap] - before)[:s.spec.P].cpu()
        assert bool((upd[~keep] == 0).all()) and bool((upd[keep] != 0).any())
        got.append(res)
    a, b = got
    assert a.keys() == b.keys() and a[41].ntx_steps == a[41].steps > 0
    for name in a:
        ra, rb = a[name], b[name]
        assert ra.snapshots.keys() == rb.snapshots.keys()
        for k in ra.snapshots:
            assert torch.equal(ra.snapshots[k], rb.snapshots[k]), (name, k)
        assert np.array_equal(ra.stats, rb.stats), name
        assert ra.ntx_steps == rb.ntx_steps, name


def test_loan_round_takes_the_per_step_path(dev, tmp_path):
    """LOAN with the key on: the persistent launch (no per-step hook) is off, the rounds train on the
    per-step graph, and the attacker's update is 0 outside the mask the round before left."""
    from dba_mod_amd import config as C
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    over = {"resumed_model": False, "pretrain_rounds": 0, "synthetic_data": True, "synthetic_train_size": 60000,
            "synthetic_test_size": 4000, "save_model": False, "save_dir": str(tmp_path)}
    cfg = os.path.join(ROOT, "configs", "loan_params.yaml")
    s0 = Server(C.load_params(cfg, dict(over)), DistCtx(device=dev), write_outputs=False)
    assert s0.trainer.persistent and s0.trainer.ntx_mask is None
    s = Server(C.load_params(cfg, dict(over, poison_neurotoxin_ratio=RHO)), DistCtx(device=dev), write_outputs=False)
    assert not s.trainer.persistent and s.trainer.use_graph
    g0 = s.global_state.clone()
    s._train_half(12, evaluate=False)
    P = s.spec.P
    k = max(1, int(RHO * P))
    want, T, m = K.mask_oracle(s.global_state.cpu(), g0.cpu(), P, k)
    assert torch.equal(s.trainer.ntx_mask.cpu(), want) and s.ntx_have_mask
    before = s.global_state.clone()
    st = s._train_begin(13)                   # attacker MO poisons: 10 epochs, then scaling by 30
    res = {r.name: r for r in st["handle"].collect()}
    adv = [c for c in st["plan"].clients if any(ph.poison for ph in c.phases)]
    assert len(adv) == 1
    r = res[adv[0].name]
    upd = (r.snapshots[adv[0].final_snap] - before)[:P].cpu()
    keep = K.unpack(want, P)
    print(f"LOAN: P {P}, k {k}, kept {m}; attacker update non-zero at {int((upd != 0).sum())} entries; restored "
          f"after {r.ntx_steps}/{r.steps} steps")
    assert int((~keep).sum()) > 0 and bool((upd[~keep] == 0).all()) and bool((upd[keep] != 0).any())
    assert r.ntx_steps == sum(1 for q in adv[0].steps if q.trig >= 0) > 0

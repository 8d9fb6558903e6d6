"""``neurotoxin_mask`` and ``mask_restore`` (the Neurotoxin attacker's two ops): the cases of
neurotoxin_cases.py through the CPU reference ops against the numpy oracle, bit for bit, as the GPU
test runs them (test_gpu_neurotoxin.py), and the grammar of the config key
``poison_neurotoxin_ratio``."""
import pytest
import torch

import neurotoxin_cases as K
from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.ops import reference as R

CPU = torch.device("cpu")
WHO = "ref"
ON = {"is_poison": True}


def test_cases_cover_the_grid_rule_the_tail_and_the_alignments():
    sweep, blocks = K.NMASK_SWEEP, K.NMASK_BLOCKS_MAX
    assert set(K.MASK_P) == {1, 63, 64, 65, sweep - 1, sweep, sweep + 1, sweep * blocks + 1029}
    assert {c[1] for c in K.MASK_CASES} == set(K.KEY_SETS)
    assert K.ks_of(1, "normal") == [1] and K.ks_of(65, "normal") == [1, 32, 64, 65]
    assert {c[0] for c in K.RESTORE_CASES} == {1, 2047, 2048, 2049, 256 * 2048 + 1029}
    assert {c[1] for c in K.RESTORE_CASES} == {"aligned", "shifted", "packed", "mixed"}
    assert {c[2] for c in K.RESTORE_CASES} == {0.95, 0.5}
    assert K.GATED == [True, True, False, False, True, True]


@pytest.mark.parametrize("case", K.MASK_CASES, ids=K.mask_id)
def test_reference_mask_matches_oracle(case):
    K.run_mask(R, case, CPU, WHO)


@pytest.mark.parametrize("case", K.RESTORE_CASES, ids=K.restore_id)
def test_reference_restore_matches_oracle(case):
    a = K.run_restore(R, case, CPU, WHO)
    if case[0] <= 2049:     # each replica alone: the same bits as inside the group
        for g in range(K.G):
            K.same_bits(K.pick(a, g), K.pick(K.run_restore(R, case, CPU, WHO, sel=g), g), "G = 1 vs G = 6")


def test_all_kept_mask_has_zero_tail_bits():
    for P in (1, 63, 64, 65, 128, 1000):
        m = R.neurotoxin_all_kept(P)
        assert m.dtype == torch.int64 and m.numel() == K.n_words(P)
        assert torch.equal(m, K.pack(torch.ones(P, dtype=torch.bool))), P


@pytest.mark.parametrize("k", [0, -1, 11, True, 2.0, None])
def test_mask_rejects_k(k):
    w = torch.arange(10, dtype=torch.float32)
    with pytest.raises(ValueError, match="neurotoxin_mask"):
        R.neurotoxin_mask(w, torch.zeros(10), 10, k, torch.zeros(1, dtype=torch.int64))


def test_ops_are_dispatched():
    assert "neurotoxin_mask" in ops._OPS and "mask_restore" in ops._OPS
    w_new, w_old = torch.tensor([5.0, 1.0, -3.0, 2.0, 9.0]), torch.tensor([4.0, 1.0, 0.0, 0.0, 0.0])
    words = torch.full((1,), -1, dtype=torch.int64)
    sel = ops.neurotoxin_mask(w_new, w_old, 4, 2, words)        # |u| = 1, 0, 3, 2 (the fifth is not ranked)
    assert sel.tolist() == [torch.tensor(1.0).view(torch.int32).item(), 2] and words.tolist() == [0b0011]
    w, base = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0]]), torch.zeros(1, 5)
    count, one = torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int32)
    ops.mask_restore(w, base, 4, one, one, words, count)
    assert torch.equal(w, torch.tensor([[1.0, 2.0, 0.0, 0.0, 5.0]])) and count.tolist() == [1]


# ------------------------------------------------------------------------------ config grammar
def test_default_is_off():
    assert C.Params().poison_neurotoxin_ratio is None and C.Params()["poison_neurotoxin_ratio"] is None
    assert C.Params(ON).poison_neurotoxin_ratio is None


def test_accepts_fractions():
    for v in (0.95, 1.0, 1e-9):
        p = C.Params({"poison_neurotoxin_ratio": v, **ON})
        assert p.poison_neurotoxin_ratio == v and isinstance(p.poison_neurotoxin_ratio, float)


@pytest.mark.parametrize("bad", [True, False, 1, 0, "0.95", "all", [0.5], 0.0, -0.5, 1.0000001, 2.0, float("inf"),
                                 float("-inf"), float("nan")])
def test_rejects_values(bad):
    with pytest.raises(ValueError, match="poison_neurotoxin_ratio"):
        C.Params({"poison_neurotoxin_ratio": bad, **ON})


@pytest.mark.parametrize("other", [{"aggregation_methods": "foolsgold"}, {"aggr_epoch_interval": 2},
                                   {"is_poison": False}])
def test_rejects_combinations(other):
    with pytest.raises(ValueError, match="poison_neurotoxin_ratio"):
        C.Params({"poison_neurotoxin_ratio": 0.9, **ON, **other})
    C.Params({**ON, **other})        # (the other key alone is fine)


@pytest.mark.parametrize("other", [{"clip_norm": 2.0}, {"clip_norm": "median", "clip_flame": True}, {"krum_f": 1},
                                   {"trim_k": 1}, {"rlr_threshold": 2}, {"sparse_topk": 0.5},
                                   {"aggregation_methods": "geom_median"}, {"alpha_loss": 0.5},
                                   {"diff_privacy": True}, {"baseline": True}, {"poison_pgd_norm": 1.0}])
def test_combines_with(other):
    assert C.Params({"poison_neurotoxin_ratio": 0.9, **ON, **other}).poison_neurotoxin_ratio == 0.9

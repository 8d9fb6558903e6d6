"""``project_to_ball`` (the norm-bounded attacker's per-step projection): the cases of pgd_cases.py
through the CPU reference op against the fp64 oracle, with the bounds the GPU test uses
(test_gpu_pgd.py), and the grammar of the config key ``poison_pgd_norm``."""
import pytest
import torch

import pgd_cases as K
from dba_mod_amd import config as C
from dba_mod_amd import ops
from dba_mod_amd.ops import reference as R

CPU = torch.device("cpu")
WHO = "ref"
ON = {"is_poison": True}


def test_cases_cover_the_grid_rule_and_the_alignments():
    assert {c[0] for c in K.PGD_CASES} == {1, 2047, 2048, 2049, 256 * 2048 + 1029}
    assert {c[1] for c in K.PGD_CASES} == {"aligned", "shifted", "packed", "mixed"}
    assert all(n >= 16 for n, _ in K.EXACT_CASES) and len(K.EXACT_CASES) == 16


@pytest.mark.parametrize("case", K.PGD_CASES, ids=K.pgd_id)
def test_reference_matches_oracle(case):
    a = K.run_pgd(R, case, CPU, WHO)
    if case[0] <= 2049:     # each replica alone: the same bits as inside the group
        for g in range(K.G):
            K.same_bits(K.pick(a, g), K.pick(K.run_pgd(R, case, CPU, WHO, sel=g), g), "G = 1 vs G = 6")


@pytest.mark.parametrize("case", K.EXACT_CASES, ids=K.pgd_id)
def test_reference_exact_boundary(case):
    K.run_exact(R, case, CPU, WHO)


def test_op_is_dispatched():
    assert "project_to_ball" in ops._OPS
    w, base = torch.tensor([[3.0, 4.0, 9.0]]), torch.zeros(1, 3)
    norm, count = torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    one = torch.ones(1, dtype=torch.int32)
    ops.project_to_ball(w, base, 2, one, one, 2.5, norm, count)
    assert norm.tolist() == [5.0] and count.tolist() == [1]
    assert torch.equal(w, torch.tensor([[1.5, 2.0, 9.0]]))


# ------------------------------------------------------------------------------ config grammar
def test_default_is_off():
    assert C.Params().poison_pgd_norm is None and C.Params()["poison_pgd_norm"] is None
    assert C.Params(ON).poison_pgd_norm is None


def test_accepts_numbers():
    p = C.Params({"poison_pgd_norm": 3, **ON})
    assert p.poison_pgd_norm == 3.0 and isinstance(p.poison_pgd_norm, float)
    assert C.Params({"poison_pgd_norm": 0.25, **ON}).poison_pgd_norm == 0.25


@pytest.mark.parametrize("bad", [True, False, "10", "median", [1], 0, 0.0, -1, -0.5, float("inf"), float("-inf"),
                                 float("nan")])
def test_rejects_values(bad):
    with pytest.raises(ValueError, match="poison_pgd_norm"):
        C.Params({"poison_pgd_norm": bad, **ON})


@pytest.mark.parametrize("other", [{"aggregation_methods": "foolsgold"}, {"aggr_epoch_interval": 2},
                                   {"is_poison": False}])
def test_rejects_combinations(other):
    with pytest.raises(ValueError, match="poison_pgd_norm"):
        C.Params({"poison_pgd_norm": 1.0, **ON, **other})
    C.Params({**ON, **other})        # (the other key alone is fine)


@pytest.mark.parametrize("other", [{"clip_norm": 2.0}, {"clip_norm": "median", "clip_flame": True}, {"krum_f": 1},
                                   {"trim_k": 1}, {"rlr_threshold": 2}, {"sparse_topk": 0.5},
                                   {"aggregation_methods": "geom_median"}, {"alpha_loss": 0.5},
                                   {"diff_privacy": True}, {"baseline": True}])
def test_combines_with(other):
    assert C.Params({"poison_pgd_norm": 1.0, **ON, **other}).poison_pgd_norm == 1.0

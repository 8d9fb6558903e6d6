"""The per-step kernel cases (step_kernel_cases.py) through the CPU reference ops, in fp32 and
with ``COMPUTE_DTYPE`` fp64, against the fp64 oracles with the bounds the GPU tests use
(test_gpu_step_kernels.py).  This validates oracles, generators and bounds without a GPU, pins
the CPU fallback path at the same edge shapes, and asserts the property the head cases are
generated for: every valid row's top-2 logit gap is at least 100 x the bound of its logits."""
import pytest
import torch

import step_kernel_cases as K
from dba_mod_amd.ops import reference as R

CPU = torch.device("cpu")


@pytest.fixture(params=["ref fp32", "ref fp64"])
def who(request):
    old = R.COMPUTE_DTYPE
    R.COMPUTE_DTYPE = torch.float32 if request.param == "ref fp32" else torch.float64
    yield request.param
    R.COMPUTE_DTYPE = old


def ref_head_train(x, w, b, labels, nvalid, dw, db, stats=None, slot=None, mean=True):
    """ops.hip.head_train's signature composed of reference ops: avgpool, the linear layer,
    softmax_xent and the linear layer's backward in the compute dtype; ``dw`` / ``db`` overwritten
    for the active replicas only."""
    G, N, H, W, C = x.shape
    cdt = R._cdt()
    pooled = R.avgpool_global(x.to(cdt)).reshape(G, N, C)
    logits = torch.einsum("gnc,gkc->gnk", pooled, w.to(cdt)) + b.to(cdt)[:, None, :]
    loss, correct, dl = R.softmax_xent(logits, labels, mean, True, stats, slot, nvalid)
    for g in range(G):
        if int(nvalid[g]) > 0:
            dw[g] = torch.einsum("nk,nc->kc", dl[g], pooled[g]).to(dw.dtype)
            db[g] = dl[g].sum(0).to(db.dtype)
    dpool = torch.einsum("gnk,gkc->gnc", dl, w.to(cdt)).to(x.dtype)
    return loss.float(), correct.float(), dpool.reshape(G, N, 1, 1, C)


def test_tables_name_every_boundary():
    """The case ids hold every shape the kernels' dispatch turns on."""
    xc, xb = {c[0] for c in K.XENT_CASES}, {c[1] for c in K.XENT_CASES}
    assert xc == {1, 2, 16, 17, 31, 200, 512, 513, 577} and xb == {1, 15, 16, 17, 255, 256, 257, 288, 289}
    for sliced in (False, True):
        some = [c for c in K.XENT_CASES if (c[1] > K.XENT_ONE_LAUNCH) == sliced]
        assert {(c[2], c[3]) for c in some} == {(m, g) for m in (False, True) for g in (False, True)}
        assert {c[4] for c in some} == set(K.XENT_ROWS) and {c[5] for c in some} == {"none", "last"}
        for lanes in (lambda C: C <= 16, lambda C: 16 < C <= 512, lambda C: C > 512):
            assert any(lanes(c[0]) for c in some)
    assert any(c[1] % K.XENT_SLICE == 1 and c[1] > K.XENT_ONE_LAUNCH and c[5] == "last" for c in K.XENT_CASES)
    assert len({K.xent_id(c) for c in K.XENT_CASES}) == len(K.XENT_CASES)
    hc = K.HEAD_CASES
    assert {c[0] for c in hc} == {1, 2, 10, 16} and {c[1] for c in hc} == {4, 60, 64, 68, 512}
    assert {c[2] for c in hc} == {1, 3, 4, 5, 17, 64, 256} and {c[3][0] * c[3][1] for c in hc} == {1, 15, 16, 17, 64}
    assert {c[5] for c in hc} == {True, False} and any(c[4] % 4 in (2, 3) for c in hc)
    assert all(0 < c[4] <= c[2] for c in hc)
    assert {c[0] for c in K.SGD_CASES} == {4, 1020, 1024, 1028, 4 * (1024 * 256 + 5)}
    assert set(K.DIST_CASES) == {1, 2047, 2048, 2049, 256 * 2048 + 1029}
    assert {c[1] for c in K.GRAM_CASES} == {1, 3, 4, 5, 1023, 1024, 1025, 5000}
    assert {c[0] for c in K.GRAM_CASES} == {1, 15, 16, 17, 37}


@pytest.mark.parametrize("case", K.XENT_CASES, ids=K.xent_id)
def test_softmax_xent(case, who):
    K.run_xent(R, case, CPU, who)


@pytest.mark.parametrize("case", K.HEAD_CASES, ids=K.head_id)
def test_head_inputs_keep_the_logit_gap(case):
    """No valid row's argmax can turn on an fp32-level error of its logits; labels at and beyond
    nvalid are -1."""
    i = K.head_inputs(case)
    o = K.head_oracle(i["x"], i["W"], i["b"], i["labels"], i["nvalid"], case[5])
    assert K.head_gap(o, i["labels"]) >= 100.0
    assert bool((i["labels"][~o["rows"]] == -1).all())
    assert i["x"].stride(0) > i["x"][0].numel() and i["x"].data_ptr() % 16 == 0 and not i["W"].is_contiguous()


@pytest.mark.parametrize("case", K.HEAD_CASES, ids=K.head_id)
def test_head(case, who):
    K.run_head(ref_head_train, case, CPU, who)


@pytest.mark.parametrize("case", K.SGD_CASES, ids=K.sgd_id)
def test_sgd_step(case, who):
    K.run_sgd(R, case, CPU, who)


@pytest.mark.parametrize("P", K.DIST_CASES, ids=lambda P: f"P{P}")
def test_dist_loss_grad(P, who):
    K.run_dist(R, P, CPU, who)


@pytest.mark.parametrize("case", K.POOL_CASES, ids=K.pool_id)
def test_maxpool(case, who):
    K.run_maxpool(R, case, CPU, who)


@pytest.mark.parametrize("case", K.AVG_CASES, ids=lambda c: f"HW{c[0][0] * c[0][1]}-C{c[1]}")
def test_avgpool(case, who):
    K.run_avgpool(R, case, CPU, who)


@pytest.mark.parametrize("n", K.RELU_CASES, ids=lambda n: f"n{n}")
def test_relu_mask_bwd(n, who):
    K.run_relu(R, n, CPU, who, bitwise=False)


@pytest.mark.parametrize("case", K.DROPOUT_CASES, ids=lambda c: f"per{c[0]}-G{c[1]}-p{c[2]}")
def test_dropout(case, who):
    K.run_dropout(R, case, CPU, who)


@pytest.mark.parametrize("L", K.FLAT_L, ids=lambda L: f"L{L}")
def test_scale_from_base(L, who):
    K.run_scale(R, L, CPU, who)


@pytest.mark.parametrize("case", K.NOISE_CASES, ids=lambda c: f"L{c[0]}-{c[1]}")
def test_add_noise_scaled(case, who):
    K.run_noise_add(R, case, CPU, who)


@pytest.mark.parametrize("case", K.DELTA_CASES, ids=lambda c: f"rows{c[0]}-L{c[1]}")
def test_delta_sum(case, who):
    K.run_delta_sum(R, case, CPU, who)


@pytest.mark.parametrize("L", K.SQDIST_L, ids=lambda L: f"L{L}")
def test_sq_dists(L, who):
    K.run_sq_dists(R, L, CPU, who)


@pytest.mark.parametrize("case", K.WSUM_CASES, ids=lambda c: f"n{c[0]}-L{c[1]}")
def test_weighted_sum(case, who):
    K.run_weighted_sum(R, case, CPU, who)


@pytest.mark.parametrize("case", K.WSUM_CASES, ids=lambda c: f"n{c[0]}-L{c[1]}")
def test_weighted_sum_fixed(case, who):
    K.run_weighted_sum_fixed(R, case, CPU, who)


@pytest.mark.parametrize("case", K.GRAM_CASES, ids=K.gram_id)
def test_gram(case, who):
    K.run_gram(R, case, CPU, who)


def test_zz_report_measured_errors(capsys):
    """Prints the largest error of the reference ops against the oracles (shown with ``-s``)."""
    with capsys.disabled():
        print("\n" + K.report())

"""The per-step HIP kernels (loss.hip, optim.hip, elementwise.hip, flat.hip) at their dispatch
boundaries against the fp64 oracles of step_kernel_cases.py (GPU only): the same cases, oracles
and bounds as the CPU reference run in test_step_kernel_cases.py.  Every comparison is
element-wise and in fp64; exact outputs are compared bit for bit; each op's bits are also checked
run to run and, for the grouped ops, against a launch holding one replica alone."""
import pytest
import torch

import step_kernel_cases as K

pytestmark = pytest.mark.gpu
WHO = "hip"


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    return hip


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _twice(run):
    """The run's outputs, after checking that a second run gives the same bits."""
    a = run()
    K.same_bits(a, run(), "run to run")
    return a


@pytest.mark.parametrize("case", K.XENT_CASES, ids=K.xent_id)
def test_softmax_xent(H, dev, case):
    a = _twice(lambda: K.run_xent(H, case, dev, WHO))
    if a["dl"] is not None:       # the fp64-loss launch writes the same dlogits
        K.check_exact(a["dl2"], a["dl"], "softmax_xent", "dlogits of the fp64-loss launch", WHO)
    # group 1 (scattered -1 labels, valid rows ending mid-slice) alone in a launch: the same bits
    K.same_bits(K.pick(a, 1), K.run_xent(H, case, dev, WHO, sel=1), "G = 1 vs G = 3")


@pytest.mark.parametrize("case", K.HEAD_CASES, ids=K.head_id)
def test_head(H, dev, case, monkeypatch):
    monkeypatch.setattr(H, "_FUSED_HEAD", True)
    a = _twice(lambda: K.run_head(H.head_train, case, dev, WHO))
    K.same_bits(K.pick(a, 1), K.run_head(H.head_train, case, dev, WHO, sel=1), "G = 1 vs G = 3")


def test_head_rejects_shapes_outside_its_contract(H, dev, monkeypatch):
    """C not a multiple of 4, more than 16 classes, more than 256 rows or 64 pixels: head_ok is
    False and head_train refuses (no launch)."""
    monkeypatch.setattr(H, "_FUSED_HEAD", True)
    for (K_, C, N, HW) in ((10, 62, 4, 4), (17, 64, 4, 4), (10, 64, 257, 4), (10, 64, 4, 65), (10, 516, 4, 4)):
        x = torch.zeros(1, N, 1, HW, C, device=dev)
        w = torch.zeros(1, K_, C, device=dev)
        assert not H.head_ok(x, w)
        with pytest.raises(AssertionError):
            H.head_train(x, w, torch.zeros(1, K_, device=dev), torch.zeros(1, N, dtype=torch.int32, device=dev),
                         torch.ones(1, dtype=torch.int32, device=dev), torch.zeros_like(w),
                         torch.zeros(1, K_, device=dev))


@pytest.mark.parametrize("case", K.SGD_CASES, ids=K.sgd_id)
def test_sgd_step(H, dev, case):
    a = _twice(lambda: K.run_sgd(H, case, dev, WHO))
    K.same_bits(K.pick(a, 1), K.run_sgd(H, case, dev, WHO, sel=1), "G = 1 vs G = 3")


@pytest.mark.parametrize("P", K.DIST_CASES, ids=lambda P: f"P{P}")
def test_dist_loss_grad(H, dev, P):
    _twice(lambda: K.run_dist(H, P, dev, WHO))


@pytest.mark.parametrize("case", K.POOL_CASES, ids=K.pool_id)
def test_maxpool(H, dev, case):
    _twice(lambda: K.run_maxpool(H, case, dev, WHO))


@pytest.mark.parametrize("case", K.AVG_CASES, ids=lambda c: f"HW{c[0][0] * c[0][1]}-C{c[1]}")
def test_avgpool(H, dev, case):
    _twice(lambda: K.run_avgpool(H, case, dev, WHO))


@pytest.mark.parametrize("n", K.RELU_CASES, ids=lambda n: f"n{n}")
def test_relu_mask_bwd(H, dev, n):
    _twice(lambda: K.run_relu(H, n, dev, WHO))


@pytest.mark.parametrize("case", K.DROPOUT_CASES, ids=lambda c: f"per{c[0]}-G{c[1]}-p{c[2]}")
def test_dropout(H, dev, case):
    _twice(lambda: K.run_dropout(H, case, dev, WHO))


@pytest.mark.parametrize("L", K.FLAT_L, ids=lambda L: f"L{L}")
def test_scale_from_base(H, dev, L):
    _twice(lambda: K.run_scale(H, L, dev, WHO))


@pytest.mark.parametrize("case", K.NOISE_CASES, ids=lambda c: f"L{c[0]}-{c[1]}")
def test_add_noise_scaled(H, dev, case):
    _twice(lambda: K.run_noise_add(H, case, dev, WHO))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_add_noise_scaled_element_independent_of_length(H, dev, dt):
    """Element i's update and noise do not depend on the buffer length: a short buffer's result
    is the prefix of the result of the case that wraps the launch grid (same inputs there)."""
    short = K.run_noise_add(H, (257, dt), dev, WHO)
    wrap = K.run_noise_add(H, (K.FLAT_WRAP, dt), dev, WHO)
    K.same_bits(short, {k: v[:257] for k, v in wrap.items()}, "prefix of the wrap case")


@pytest.mark.parametrize("case", K.DELTA_CASES, ids=lambda c: f"rows{c[0]}-L{c[1]}")
def test_delta_sum(H, dev, case):
    _twice(lambda: K.run_delta_sum(H, case, dev, WHO))


@pytest.mark.parametrize("L", K.SQDIST_L, ids=lambda L: f"L{L}")
def test_sq_dists(H, dev, L):
    _twice(lambda: K.run_sq_dists(H, L, dev, WHO))


@pytest.mark.parametrize("case", K.WSUM_CASES, ids=lambda c: f"n{c[0]}-L{c[1]}")
def test_weighted_sum(H, dev, case):
    _twice(lambda: K.run_weighted_sum(H, case, dev, WHO))


@pytest.mark.parametrize("case", K.WSUM_CASES, ids=lambda c: f"n{c[0]}-L{c[1]}")
def test_weighted_sum_fixed(H, dev, case):
    _twice(lambda: K.run_weighted_sum_fixed(H, case, dev, WHO))


@pytest.mark.parametrize("case", K.GRAM_CASES, ids=K.gram_id)
def test_gram(H, dev, case):
    _twice(lambda: K.run_gram(H, case, dev, WHO))


def test_zz_report_measured_errors(H, capsys):
    """Prints the kernels' largest error against the oracles (shown with ``-s``)."""
    with capsys.disabled():
        print("\n" + K.report())

"""The batch-ingest kernels (csrc/kernels/data.hip) and the evaluation BN fold
(csrc/kernels/bn.hip) against the oracles of ingest_cases.py (GPU only): gathers bit for bit,
also past one sweep of the capped launch grid; the fold element-wise in fp64 within the a-priori
fp32 bounds, with and without a conv bias, past one sweep of its grid; the batched fold bit for
bit against one fold per conv."""
import pytest
import torch

import ingest_cases as I
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


@pytest.mark.parametrize("name", [c.name for c in I.ROWS_CASES])
def test_gather_rows(H, dev, name):
    a = I.run_rows(H.gather_rows, name, dev, WHO)
    K.same_bits(a, I.run_rows(H.gather_rows, name, dev, WHO), "run to run")


def test_gather_rows_group_alone(H, dev):
    for g in (0, 5):
        I.run_rows(H.gather_rows, "edges", dev, WHO, sel=g)


@pytest.mark.parametrize("name", [c.name for c in I.IMG_CASES])
def test_gather_images(H, dev, name):
    a = I.run_images(H.gather_images, name, dev, WHO)
    K.same_bits(a, I.run_images(H.gather_images, name, dev, WHO), "run to run")


@pytest.mark.parametrize("name", ["6x7x3-flip", "32x32x3-flip"])
def test_gather_images_group_alone(H, dev, name):
    """A seed's flip pattern (and everything else of the group) is the same at G = 1."""
    for g in (0, 5):
        I.run_images(H.gather_images, name, dev, WHO, sel=g)


@pytest.mark.parametrize("name", [c.name for c in I.FOLD_CASES])
def test_bn_fold(H, dev, name):
    wf, bf = I.run_fold(H.bn_fold, name, dev, WHO)
    wf2, bf2 = I.run_fold(H.bn_fold, name, dev, WHO)
    K.check_exact(wf2, wf, "bn_fold", "wf run to run", "invariant")
    K.check_exact(bf2, bf, "bn_fold", "bf run to run", "invariant")
    for s in range(wf.shape[0]):     # max |wf| per slot: exact against the kernel's own wf
        assert I.amax_value(wf._dba_amax, s) == wf[s].abs().max().item(), (name, s)


@pytest.mark.parametrize("n", I.BATCH_N)
def test_bn_fold_batch(H, dev, n):
    """n folds in one launch per 24 == one bn_fold per conv, bit for bit (wf, bf, max |wf|), and
    within the oracle's bounds."""
    slots, convs = 3, I.batch_convs(n)
    ps = I.fold_state(slots, convs, n, dev)
    buf = H.amax_slots(n, slots, dev)
    got = H.bn_fold_batch([(p["w"].view(slots, co, 1, 1, k), p["gamma"], p["beta"], p["rm"], p["rv"], buf[i])
                           for i, (p, (co, k)) in enumerate(zip(ps, convs))], I.EPS)
    assert len(got) == n
    for i, (p, (wf, bf)) in enumerate(zip(ps, got)):
        wr, br = H.bn_fold(p["w"], None, p["gamma"], p["beta"], p["rm"], p["rv"], I.EPS, torch.float32, split=False)
        K.check_exact(wf, wr, "bn_fold_batch", f"wf of conv {i} / {n}", "invariant")
        K.check_exact(bf, br, "bn_fold_batch", f"bf of conv {i} / {n}", "invariant")
        assert torch.equal(wf._dba_amax.max(0).values, wr._dba_amax.max(0).values), i
        wwf, wbf, bw, bb = I.fold_oracle(p, False)
        K.check_bound(wf, wwf, bw, "bn_fold_batch", "wf", WHO)
        K.check_bound(bf, wbf, bb, "bn_fold_batch", "bf", WHO)


def test_zz_report_measured_errors(H, capsys):
    with capsys.disabled():
        print("\n" + K.report())

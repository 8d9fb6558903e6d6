"""The ingest and BN-fold cases (ingest_cases.py) through ``ops/reference.py`` on the CPU: the
case tables hold every edge (launch-grid caps with a remainder, -1 rows, poison counts, trigger
content, flips), the numpy oracles agree bit for bit with the reference gathers and with
mlp_cases' gather, and the reference fold in fp32 and fp64 stays within the a-priori bounds the
GPU tests use (test_gpu_ingest.py)."""
import numpy as np
import pytest
import torch

import ingest_cases as I
import mlp_cases as M
from dba_mod_amd.ops import reference as R

CPU = torch.device("cpu")


@pytest.fixture(params=["ref fp32", "ref fp64"])
def who(request):
    old = R.COMPUTE_DTYPE
    R.COMPUTE_DTYPE = torch.float32 if request.param == "ref fp32" else torch.float64
    yield request.param
    R.COMPUTE_DTYPE = old


def test_tables_name_every_edge():
    items = {c.name: c.G * c.B * c.F for c in I.ROWS_CASES}
    assert 0 < items["over-cap"] - I.GATHER_CAP < 256 * 8 and (items["over-cap"] - I.GATHER_CAP) % 256
    assert 0 < I.GATHER_CAP - items["under-cap"] < 256
    items = {c.name: c.G * c.B * c.H * c.W for c in I.IMG_CASES}
    assert 0 < items["over-cap"] - I.GATHER_CAP < 256 * 8 and (items["over-cap"] - I.GATHER_CAP) % 256
    assert 0 < I.GATHER_CAP - items["under-cap"] < 256 * 4
    assert {(c.H, c.W, c.C) for c in I.IMG_CASES} >= {(28, 28, 1), (32, 32, 3), (6, 7, 3), (32, 31, 3)}
    assert {c.flip for c in I.IMG_CASES if c.G == I.SMALL_G} == {True, False}
    per = {c.name: c.Cout * c.K for c in I.FOLD_CASES}
    assert 0 < per["over-cap-bias"] - I.FOLD_CAP < I.FOLD_CAP and (per["over-cap-bias"] - I.FOLD_CAP) % 256
    assert {c.bias for c in I.FOLD_CASES} == {True, False}
    assert any(c.K == 1 for c in I.FOLD_CASES) and any(c.Cout == 1 for c in I.FOLD_CASES)
    assert I.BATCH_N == [1, I.FOLD_BATCH, I.FOLD_BATCH + 1]
    assert {a * b for a, b in I.batch_convs(25)} >= {I.FOLD_CHUNK - 1, I.FOLD_CHUNK, I.FOLD_CHUNK + 1}
    assert np.float32(1) / np.float32(255) == I.INV255          # the kernel's 1.0f / 255.0f


def test_small_groups_hold_the_edges():
    for inp in (I.rows_inputs("edges"), I.img_inputs("32x32x3-flip")):
        idx, trig, pn = inp["idx"], inp["trig"], inp["pn"]
        valid = (idx >= 0).sum(1)
        assert idx[0, 0] == idx[0, 3] == idx[0, 7] == -1 and valid[0] == 5 and valid[1] == 0
        assert {0, 1, I.SMALL_B} <= set(pn.tolist()) and pn[5] == valid[5] + 1 and trig[5] >= 0
        assert trig[2] == -1 and pn[2] > 0 and trig[1] >= 0 and pn[1] > 0
    m = I.img_inputs("6x7x3-flip")["masks"]
    assert m[0, 0].any() and m[0, -1].any() and m[0, :, 0].any() and m[0, :, -1].any() and not m[2].any()
    assert not np.array_equal(m[0], m[0][:, ::-1])


@pytest.mark.parametrize("name", [c.name for c in I.IMG_CASES if c.flip])
def test_flips(name):
    """Some stamped row is flipped and some is not; rows flip both ways; a seed's pattern is the
    same alone as in the group."""
    i = I.img_inputs(name)
    bits = I.flip_bits(i["seeds"], i["idx"].shape[1])
    st = [(g, b) for g in range(len(i["trig"])) for b in range(min(int(i["pn"][g]), bits.shape[1]))
          if i["trig"][g] >= 0 and i["idx"][g, b] >= 0 and i["masks"][i["trig"][g]].any()]
    assert {bool(bits[g, b]) for g, b in st} == {True, False}
    for g in range(len(i["seeds"])):
        assert np.array_equal(I.flip_bits(i["seeds"][g:g + 1], bits.shape[1])[0], bits[g])


@pytest.mark.parametrize("name", [c.name for c in I.ROWS_CASES])
def test_gather_rows(name):
    I.run_rows(R.gather_rows, name, CPU, "ref")


def test_rows_oracle_is_the_mlp_oracles_gather():
    i = I.rows_inputs("edges")
    wx, wy = I.rows_expected("edges")
    for g in range(I.SMALL_G):
        x, y = M.gather(i["src"], i["labels"], i["idx"][g], int(i["pn"][g]), int(i["trig"][g]), target=I.TARGET)
        assert np.array_equal(x.view(np.int32), wx[g].view(np.int32)) and np.array_equal(y, wy[g])
    assert (wx[0, 1, [0, 90]] == [10.0, 80.0]).all() and (wx[3, 0, [7, 45]] == [80.0, 5.5]).all()   # last duplicate wins
    assert (wx[0, 0] == 0).all() and wy[0, 0] == -1 and (wy[2] != -1).all() and wy[5, 4] == I.TARGET


@pytest.mark.parametrize("name", [c.name for c in I.IMG_CASES])
def test_gather_images(name):
    I.run_images(R.gather_images, name, CPU, "ref")


def test_images_oracle_values():
    i = I.img_inputs("6x7x3-noflip")
    wx, wy = I.img_expected("6x7x3-noflip")
    assert wx.max() == 1.0 and wx.min() == 0.0 and (wx[1] == 0).all() and (wy[1] == -1).all()
    assert (wx[0, 1][i["masks"][0] != 0] == 1.0).all() and wy[0, 1] == I.TARGET
    s = i["idx"][3, 0]
    assert np.array_equal(wx[3, 0], i["src"][s].astype(np.float32) * I.INV255) and wy[3, 0] == I.TARGET   # zero mask
    assert wy[2, 0] == i["labels"][i["idx"][2, 0]] and wy[5, 5] == -1


@pytest.mark.parametrize("name", [c.name for c in I.FOLD_CASES])
def test_bn_fold(name, who):
    I.run_fold(R.bn_fold, name, CPU, who)


def test_fold_inputs_and_oracle():
    p = I.fold_state(3, [(64, 288)], 0)[0]
    assert (p["rv"][:, :3] == torch.tensor(I.RV_EDGES, dtype=torch.float32)).all() and (p["rv"][:, 3:] >= 0.5).all()
    assert (p["gamma"][:, 3] == 0).all() and bool((p["gamma"] < 0).any())
    q = I.fold_state(3, [(1, 50)], 0)[0]
    assert q["rv"][:, 0].tolist() == [float(np.float32(e)) for e in I.RV_EDGES]
    with_b, without = I.fold_oracle(p, True), I.fold_oracle(p, False)
    live = p["gamma"].double().abs() > 0.1
    assert bool(((with_b[1] - without[1]).abs()[live] > 1e3 * with_b[3][live]).float().mean() > 0.9)
    assert bool((with_b[0][:, 3] == 0).all()) and torch.equal(with_b[1][:, 3], p["beta"][:, 3].double())

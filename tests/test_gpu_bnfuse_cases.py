"""The fused training BatchNorm (bnfuse.hpp, xbn.hip, the record code of the conv epilogues and
stem.hip) at its own boundaries against the fp64 oracles of bn_cases.py (GPU only): the same cases,
oracles and bounds as the CPU emulation in test_bn_cases.py.  Every comparison is element-wise and
in fp64 against an a-priori bound, or bit for bit: YMAX / YMIN, the forward bound slot against the
stored output's max, d, the same statistics from every producer of the records, run to run and
alone against in a group, the empty replica's rows, the sentinels around every strided view."""
import math

import pytest
import torch

import bn_cases as B
import conv_cases as CC
from dba_mod_amd.ops import bnstate as bs

pytestmark = pytest.mark.gpu
WHO = B.HIP


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    return hip


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _name(c):
    return c.name


def _pick(bits, g):
    return {k: (None if v is None else v[g:g + 1]) for k, v in bits.items()}


FWD_ROWS = (bs.MEAN, bs.INV, bs.SCALE, bs.SHIFT)


# ================================================================= table 0: the standalone mode-1 pass
@pytest.mark.parametrize("c", B.ROWS_CASES, ids=_name)
def test_rows_statistics(H, dev, c):
    i = B.rows_inputs(c)
    rows = [n * c.H * c.W for n in i["nvalid"]]
    y, nvalid = i["y"].to(dev), torch.tensor(i["nvalid"], dtype=B.I32, device=dev)
    op = "bnx_rows mode 1"

    def run(sel=None):
        prm = B.Prm(3, c.C, (0, len(c.name)), dev, sel=sel)
        s = slice(None) if sel is None else slice(sel, sel + 1)
        st = B.hip_rows_stats(H, y[s].contiguous(), nvalid[s].contiguous(), prm, c.relu)
        return st, prm

    st, prm = run()
    B.check_stats(y, rows, st.coef, prm, op, WHO)
    B.check_fwd_bound_slot(H, y, st, c.relu, nvalid, rows, op)
    a = B.fwd_bits(st, prm, rows)
    st2, prm2 = run()
    B.same_bits(a, B.fwd_bits(st2, prm2, rows), "run to run")
    st1, prm1 = run(1)
    B.same_bits(_pick(a, 1), B.fwd_bits(st1, prm1, rows[1:2]), "replica 1 alone vs in its group")


# ======================================================= table 1: the standalone pass and finalize
@pytest.mark.parametrize("c", B.FIN_CASES, ids=_name)
def test_bn_finish(H, dev, c):
    out = B.run_finish(H, c, dev, WHO)
    B.check_finish_d(c, out, WHO)
    B.check_finish(B.fin_inputs(c), out, c.two, "bn_finish", WHO)
    a = B.finish_bits(out)
    B.same_bits(a, B.finish_bits(B.run_finish(H, c, dev, WHO)), "run to run")
    if not c.full:
        B.same_bits(_pick(a, 1), B.finish_bits(B.run_finish(H, c, dev, WHO, sel=1)), "replica 1 alone vs in its group")


def test_dy_bound_met_with_equality(H, dev):
    """AL_CASES: each replica's largest |dy| is the whole of |A| dmax + max |B y + K|, so the bound
    slot has only its (1 + 2^-10) above it: the inequality at its tightest, and the slot against its
    formula on 24 more replicas."""
    for c in B.AL_CASES:
        out = B.run_finish(H, c, dev, WHO)
        B.check_finish_d(c, out, WHO)
        B.check_finish(B.fin_inputs(c), out, c.two, "bn_finish", WHO)


# ================================================== table 2: statistics from every record producer
def _stats_bits(r):
    b = B.fwd_bits(r["st"], r["prm"], r["rows"])
    b["y"] = CC._mask(r["y"], [n // max(1, r["y"].shape[2] * r["y"].shape[3]) for n in r["rows"]]).cpu()
    return b


@pytest.mark.parametrize("c", B.STATS_CASES, ids=CC.case_id)
def test_conv_bn_stats(H, dev, c):
    op = f"conv_bn_stats [{c.path}]"
    r = B.run_conv_stats(H, c, dev, WHO)
    assert r["path"] == c.path                         # the row ran on the producer it names
    y, st, prm, rows, nvalid, relu = r["y"], r["st"], r["prm"], r["rows"], r["nvalid"], r["relu"]
    # y: channel 0 (zero weights) exactly zero, the rest against the conv oracle's two bounds
    inp, o = CC.inputs(c), CC.oracle("fwd", c, "")
    yo = y.cpu().clone()
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv:
            assert bool((yo[g, :nv, ..., 0] == 0).all()), f"{c.name}: the zero-weight channel is not 0"
            yo[g, :nv, ..., 0] = o[g].want[..., 0].float()
    B.check_act_out("fwd", c, yo, "", WHO, c.path)
    # the statistics of the kernel's own y, the constant channel exactly
    B.check_stats(y, rows, st.coef, prm, op, WHO)
    inv0 = torch.tensor([1.0 / math.sqrt(B.f32(B.EPS))]).float()
    for g, n in enumerate(rows):
        if n:
            B.check_exact(st.coef[g, bs.INV, :1], inv0, op, "inv of the constant channel", WHO)
    B.check_fwd_bound_slot(H, y, st, relu, nvalid, rows, op)
    # the same bits whichever producer: the standalone pass over the stored y
    a = _stats_bits(r)
    prm2 = B.stats_prm(c, dev)
    st2 = B.hip_rows_stats(H, y, nvalid, prm2, relu)
    clean = B.fwd_bits(st2, prm2, rows)
    B.same_bits({k: v for k, v in a.items() if k != "y"}, clean, f"{c.path} vs the standalone pass")
    B.same_bits(a, _stats_bits(B.run_conv_stats(H, c, dev, WHO)), "run to run")
    if c.G > 1:
        g = CC.solo_replica(c)
        B.same_bits(_pick(a, g), _stats_bits(B.run_conv_stats(H, c, dev, WHO, sel=g)), f"replica {g} alone vs in its group")
    # a NaN in one channel of one valid pixel: that channel's rows are NaN, nothing else moves
    ch = c.Cout - 1
    yn = y.clone()
    yn[0, 0, 0, 0, ch] = B.NAN
    prm3 = B.stats_prm(c, dev)
    got = B.fwd_bits(B.hip_rows_stats(H, yn, nvalid, prm3, relu), prm3, rows)["rows"]
    assert bool(torch.isnan(got[0, FWD_ROWS, ch]).all()), f"{c.name}: NaN y, rows {got[0, :4, ch].tolist()}"
    keep = torch.ones(c.Cout, dtype=torch.bool)
    keep[ch] = False
    B.check_exact(got[0][:, keep], clean["rows"][0][:, keep], op, "other channels beside a NaN", WHO)
    B.check_exact(got[1:], clean["rows"][1:], op, "other replicas beside a NaN", WHO)


@pytest.mark.parametrize("name", ["stem-3x3", "stem-7x7"])
def test_stem_records_stop_at_the_valid_rows(H, dev, name):
    """stem.hip's own record loop with a row count off 32, on what the stem really reads: images in
    [0, 1].  Two output channels have weights of one sign, so every valid y there is > 0 (< 0): a
    record that took in the zero-filled tile rows beyond the valid ones would move YMIN (YMAX) to 0."""
    c = next(x for x in B.STATS_CASES if x.name == name)
    op = "conv_bn_stats [stem, images]"
    inp = CC.inputs(c)
    g = B.gen(26, len(name))
    x = B.garbage(torch.rand(c.G, c.N, c.H, c.W, c.Cin, generator=g), inp["nvalid"], g)
    w = inp["w"].clone()
    w[:, 4], w[:, 5] = w[:, 4].abs() + 0.01, -w[:, 5].abs() - 0.01
    wsel, nvalid, _ = CC._maps_dev(inp, dev, None)
    prm, rows = B.stats_prm(c, dev), B.stats_rows(c)
    assert all(n % 32 for n in rows if n)
    y, st = H.conv_bn_stats(x.to(dev), w.to(dev), wsel, c.s, c.p, nvalid, prm.bn(), True)
    assert CC.launched_path(H) == "stem"
    for r in range(c.G):
        nv = inp["nvalid"][r]
        if nv == 0:
            continue
        xs, ws = x[r, :nv].double(), w[CC.slot(inp, r)].double()
        got = y[r, :nv].cpu()
        B.check_bound(got, CC.lin_fwd(xs, ws, c), B.bound32(c.K + 2, CC.lin_fwd(xs.abs(), ws.abs(), c)), op, "y", WHO)
        assert bool((got[..., 4] > 0).all()) and bool((got[..., 5] < 0).all())
    B.check_stats(y, rows, st.coef, prm, op, WHO)
    B.check_fwd_bound_slot(H, y, st, True, nvalid, rows, op)
    prm2 = B.stats_prm(c, dev)
    st2 = B.hip_rows_stats(H, y, nvalid, prm2, True)
    B.same_bits(B.fwd_bits(st, prm, rows), B.fwd_bits(st2, prm2, rows), "stem vs the standalone pass")


def test_conv_bn_stats_refuses_cout_off_4(H, dev):
    c = B.STATS_DECLINE
    inp = CC.inputs(c)
    x, = CC._dev(inp, dev, None, "x")
    wsel, nvalid, _ = CC._maps_dev(inp, dev, None)
    prm = B.Prm(c.G, c.Cout, (3, 0), dev)
    with CC.settings(H, c, dev), pytest.raises(RuntimeError):
        H.conv_bn_stats(x, inp["w"].to(dev), wsel, c.s, c.p, nvalid, prm.bn(), True)
    torch.cuda.synchronize()
    B.check_exact(prm.flat, prm.flat0, "conv_bn_stats", "parameter rows after a refused launch", WHO)


# ============================================ table 3: mask + reduce in the data-gradient epilogue
@pytest.mark.parametrize("p", B.DFIN_CASES, ids=B.dfin_id)
def test_dgrad_finish(H, dev, p):
    c, mask, two, accum = p
    out = B.run_dgrad_finish(H, p, dev, WHO)
    assert out["path"] == c.path
    B.check_dgrad_d(p, out, WHO)
    B.check_finish(B.dfin_inputs(c, mask), out, two, f"conv2d_dgrad finish [{c.path}]", WHO)
    a = B.finish_bits(out)
    B.same_bits(a, B.finish_bits(B.run_dgrad_finish(H, p, dev, WHO)), "run to run")
    if c.G > 1:
        g = CC.solo_replica(c)
        B.same_bits(_pick(a, g), B.finish_bits(B.run_dgrad_finish(H, p, dev, WHO, sel=g)), f"replica {g} alone vs in its group")


def test_dgrad_finish_refuses_cin_off_4(H, dev):
    c = B.DFIN_DECLINE
    with pytest.raises(RuntimeError):
        B.run_dgrad_finish(H, (c, "out", False, False), dev, WHO)
    torch.cuda.synchronize()


# ================================================================ table 4: stored elementwise passes
@pytest.mark.parametrize("c", B.APPLY_CASES, ids=_name)
def test_bn_apply(H, dev, c):
    B.check_apply(c, B.run_apply(H, c, dev, WHO), WHO)


@pytest.mark.parametrize("c", B.DY_CASES, ids=_name)
def test_bnx_dy(H, dev, c):
    B.check_dy(c, B.run_dy(H, c, dev, WHO), WHO)


def test_elementwise_passes_refuse_c_off_4(H, dev):
    for table, run in ((B.APPLY_CASES, B.run_apply), (B.DY_CASES, B.run_dy)):
        c = table[1]._replace(C=6)
        with pytest.raises(RuntimeError):
            run(H, c, dev, WHO)
    torch.cuda.synchronize()


def test_report():
    """(Not a check: prints the err / bound table of ARCHITECTURE 6.2 with ``pytest -s``.)"""
    print("\n" + B.report())

"""CPU half of the fused training-BN edge-shape tests (bn_cases.py): the fp64 oracles against
independent formulations (``math.fsum``; ``torch.nn.functional.batch_norm`` + autograd), the CPU
emulation of the header's arithmetic held to the bounds on every table row (so every row is known
to be passable before a GPU sees it), ``ops/reference.py`` in fp64 through the same cases at
``bound64``, and every row shown to reach the path it names from the re-derived dispatch."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_cases as B
import conv_cases as CC
from dba_mod_amd.ops import bnstate as bs

EMU = "emulation"
REF = "reference fp64"


def _name(c):
    return c.name


# ================================================================================== the tables
def test_tables_are_well_formed():
    for table in (B.ROWS_CASES, B.FIN_CASES, B.APPLY_CASES, B.DY_CASES, B.STATS_CASES):
        names = [c.name for c in table]
        assert len(names) == len(set(names))
        assert all(c.why for c in table)
    rows = {n * c.H * c.W for c in B.FIN_CASES if not c.pool for n in B.fin_nvalid(c)}
    assert {1, 31, 32, 33, 127, 128, 129, 8160, 8192, 8193} <= rows             # the issue's row counts
    assert {(c.C, c.N) for c in B.FIN_CASES if c.H * c.W == 1} >= {(C, n) for C in (4, 60, 64, 68) for n in (33, 129)}
    assert {c.mask for c in B.FIN_CASES} == {"out", "lazy", "none"} and {c.two for c in B.FIN_CASES} == {True, False}
    assert {c.H * c.W for c in B.FIN_CASES if c.pool} == {1, 4, 16}
    for c in B.FIN_CASES:
        if c.pool:
            assert 0 < c.nv1 < c.N                                                   # nvalid inside the batch
    # nvalid cutting inside a 32-row group at HW 4 and 9
    assert any(c.H * c.W == 4 and (c.nv1 * 4) % 32 for c in B.FIN_CASES) and any(
        c.H * c.W == 9 and (c.nv1 * 9) % 32 for c in B.FIN_CASES)
    assert sum(c.full for c in B.FIN_CASES) == 1
    assert {c.kind for c in B.ROWS_CASES} == set(B.FWD_KINDS)
    assert {n * c.H * c.W for c in B.ROWS_CASES for n in B.rows_nvalid(c)} >= {0, 1, 2, 31, 33, 129, 8193}
    for c in B.APPLY_CASES + B.DY_CASES:
        if c.full:     # every thread of the capped grid takes a second trip
            assert c.N * c.H * c.W * (c.C // 4) > (8192 // 3) * 256
    assert {(c.res, c.relu_b) for c in B.APPLY_CASES} == {("t", False), ("bn", False), ("bn", True), ("", False)}
    assert {c.relu for c in B.APPLY_CASES} == {True, False}
    for c in B.STATS_CASES:
        assert c.Cout % 4 == 0 and c.path and c.why
    assert B.STATS_DECLINE.Cout % 4 and B.DFIN_DECLINE.Cin % 4
    for c, mask, two, accum in B.DFIN_CASES:
        assert c.Cin % 4 == 0


def test_mask_specials_sit_in_valid_rows():
    """+0, -0, a positive denormal, a NaN and a negative denormal of the stored mask give +0, +0, g,
    +0, +0."""
    c = next(x for x in B.FIN_CASES if x.name == "f-n33-c68")
    i = B.fin_inputs(c)
    m = i["mask_out"][0].view(-1)[:5]
    assert m[0] == 0 and m[1] == 0 and math.copysign(1, float(m[1])) < 0 and 0 < float(m[2]) < 1.2e-38 and bool(
        torch.isnan(m[3])) and float(m[4]) < 0
    d, g = i["want_d"][0].view(-1)[:5], i["g"][0].view(-1)[:5]
    B.check_exact(d, torch.tensor([0.0, 0.0, float(g[2]), 0.0, 0.0]), "bn_finish", "d at the mask specials", "oracle")


# ==================================================================== the oracles' witnesses
@pytest.mark.parametrize("c", [c for c in B.ROWS_CASES if c.N <= 129 or c.kind == "m1e3"], ids=_name)
def test_stats_oracle_against_fsum(c):
    """Mean and biased variance of the first and last channel by exactly rounded sums."""
    i = B.rows_inputs(c)
    for g, n in enumerate(n_ * c.H * c.W for n_ in i["nvalid"]):
        if n == 0:
            continue
        yv = B.valid_rows(i["y"][g], n)
        z = torch.zeros(c.C)
        o = B.stats_oracle(yv, z + 1, z, z, z + 1)
        for ch in (0, c.C - 1):
            col = [float(v) for v in yv[:, ch]]
            m = math.fsum(col) / n
            var = math.fsum((v - m) ** 2 for v in col) / n
            assert abs(float(o["mean"][ch]) - m) <= 4 * B.U64 * (abs(m) + 1e-300) * max(1, math.log2(n + 1))
            assert abs(float(o["var"][ch]) - var) <= 1e-13 * var + 4 * n * B.U64 * abs(m) * math.sqrt(var + 1e-300) + 1e-300
            assert float(o["ymax"][ch]) == max(col) and float(o["ymin"][ch]) == min(col)


@pytest.mark.parametrize("c", [c for c in B.FIN_CASES if 1 < c.N <= 129 and not c.pool and c.mask != "lazy"][:8], ids=_name)
def test_oracles_against_batch_norm_autograd(c):
    """stats_oracle's scale / shift, finish_oracle's dgamma / dbeta / A / B / K and dy_oracle against
    F.batch_norm(training=True) + autograd in fp64."""
    i = B.fin_inputs(c)
    g, n = 0, i["rows"][0]
    y = B.valid_rows(i["ya"][g], n).double()
    d = B.valid_rows(i["want_d"][g], n).double()
    p = B.Prm(3, c.C, (9, 9), "cpu", special=False)
    gamma, beta = p.v0["gamma"][g].double().requires_grad_(), p.v0["beta"][g].double().requires_grad_()
    yy = y.clone().requires_grad_()
    rm, rv = p.v0["rmean"][g].double().clone(), p.v0["rvar"][g].double().clone()
    z = F.batch_norm(yy.t()[None], rm, rv, gamma, beta, training=True, momentum=B.f32(B.MOMENTUM), eps=B.f32(B.EPS))[0].t()
    (z * d).sum().backward()
    o = B.stats_oracle(y, gamma.detach(), beta.detach(), p.v0["rmean"][g], p.v0["rvar"][g])
    tol = lambda t: 1e-10 * (t.abs().max() + 1e-30)   # noqa: E731
    zo = y * o["scale"] + o["shift"]
    assert bool(((zo - z.detach()).abs() <= tol(z.detach())).all())
    assert bool(((o["rmean"] - rm).abs() <= tol(rm)).all()) and bool(((o["rvar"] - rv).abs() <= tol(rv)).all())
    cf = torch.zeros(bs.ROWS, c.C, dtype=torch.float64)
    cf[bs.MEAN], cf[bs.INV], cf[bs.YMAX], cf[bs.YMIN] = o["mean"], o["inv"], o["ymax"].double(), o["ymin"].double()
    zero = torch.zeros(c.C)
    fo = B.finish_oracle(d, y, cf, gamma.detach(), zero, zero)
    assert bool(((fo["dgamma"] - gamma.grad).abs() <= tol(gamma.grad)).all())
    assert bool(((fo["dbeta"] - beta.grad).abs() <= tol(beta.grad)).all())
    cf[bs.A], cf[bs.B], cf[bs.K] = fo["A"], fo["B"], fo["K"]
    dy, _ = B.dy_oracle(d, y, cf)
    assert bool(((dy - yy.grad).abs() <= tol(yy.grad)).all())


# ============================================================== the emulation within the bounds
def _emu_fwd(yv, prm, g, relu, op, sharp=None):
    v = prm.v0
    o = B.stats_oracle(yv, v["gamma"][g], v["beta"][g], v["rmean"][g], v["rvar"][g])
    e = B.emulate_stats(yv, v["gamma"][g], v["beta"][g], v["rmean"][g], v["rvar"][g], relu)
    for name in ("mean", "inv", "scale", "shift", "rmean", "rvar"):
        B.check_bound(e[name], o[name], o["b_" + name], op, name, EMU)
    B.check_exact(e["ymax"], o["ymax"], op, "ymax", EMU)
    B.check_exact(e["ymin"], o["ymin"], op, "ymin", EMU)
    if sharp:
        assert float((o["b_inv"] / o["inv"]).max()) < 1e-6, (op, sharp)
    return o, e


@pytest.mark.parametrize("c", B.ROWS_CASES, ids=_name)
def test_emulated_statistics_within_bounds(c):
    i = B.rows_inputs(c)
    prm = B.Prm(3, c.C, (0, len(c.name)), "cpu")
    for g, n in enumerate(n_ * c.H * c.W for n_ in i["nvalid"]):
        if n:
            _emu_fwd(B.valid_rows(i["y"][g], n), prm, g, c.relu, "bnx_rows mode 1", c.kind in B.SHARP_KINDS and c.kind)


def test_constant_rows_reach_the_clamp():
    """S2 / n - m^2 of a constant 1e6 channel is below -eps for some channel: without the clamp inv
    is NaN there (the rows have teeth)."""
    hit = 0
    for c in B.ROWS_CASES:
        if c.kind != "const":
            continue
        i = B.rows_inputs(c)
        prm = B.Prm(3, c.C, (0, len(c.name)), "cpu")
        for g, n in enumerate(n_ * c.H * c.W for n_ in i["nvalid"]):
            if n > 1:
                v = prm.v0
                e = B.emulate_stats(B.valid_rows(i["y"][g], n), v["gamma"][g], v["beta"][g], v["rmean"][g], v["rvar"][g],
                                    c.relu, clamp=False)
                hit += int(torch.isnan(e["inv"]).sum())
    assert hit > 0


@pytest.mark.parametrize("c", B.STATS_CASES, ids=CC.case_id)
def test_emulated_conv_statistics_within_bounds(c):
    """The statistics of each conv row's output (the fp64 conv oracle, rounded to fp32)."""
    inp = CC.inputs(c)
    prm = B.Prm(c.G, c.Cout, (3, len(c.name)), "cpu")
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv == 0:
            continue
        w = inp["w"][CC.slot(inp, g)].double().clone()
        w[0] = 0
        y = CC.lin_fwd(inp["x"][g, :nv].double(), w, c).float()
        o, _ = _emu_fwd(B.valid_rows(y, nv * c.Ho * c.Wo), prm, g, B.stats_relu(c), "conv_bn_stats", "conv")
        assert float(o["var"][0]) == 0.0 and float(o["inv"][0]) == 1.0 / math.sqrt(B.f32(B.EPS))     # the constant channel


def _emu_bwd(d, y, cf, prm, g, op):
    v = prm.v0
    o = B.finish_oracle(d, y, cf, v["gamma"][g], v["dgamma"][g], v["dbeta"][g])
    e = B.emulate_finish(d, y, cf, v["gamma"][g], v["dgamma"][g], v["dbeta"][g])
    for name in ("dgamma", "dbeta", "A", "B", "K"):
        B.check_bound(e[name], o[name], o["b_" + name], op, name, EMU)
    top = float(e["dy"].abs().max())
    assert top <= e["dbound"] <= o["dbound_max"], (op, top, e["dbound"], o["dbound_max"])
    cf_e = cf.clone()
    cf_e[bs.A], cf_e[bs.B], cf_e[bs.K] = e["A"], e["B"], e["K"]
    want = B.dbound_formula(cf_e, d)
    B.check_bound(torch.tensor([e["dbound"]]), torch.tensor([want], dtype=torch.float64), B.bound32(3, want), op,
                  "dy bound slot vs its formula", EMU)


@pytest.mark.parametrize("c", B.FIN_CASES, ids=_name)
def test_emulated_finish_within_bounds(c):
    i = B.fin_inputs(c)
    pa, pb = B.Prm(3, c.C, (1, len(c.name)), "cpu"), B.Prm(3, c.C, (2, len(c.name)), "cpu")
    for g, n in enumerate(i["rows"]):
        if n == 0:
            continue
        d = B.valid_rows(i["want_d"][g], n)
        _emu_bwd(d, B.valid_rows(i["ya"][g], n), i["cfa"][g], pa, g, "bn_finish")
        if c.two:
            _emu_bwd(d, B.valid_rows(i["yb"][g], n), i["cfb"][g], pb, g, "bn_finish")


def test_dy_bound_factor_has_teeth():
    """AL_CASES: the emulated bound holds on every replica, and without its (1 + 2^-10) it falls below
    the emulated max |dy| on some of them."""
    below = 0
    for c in B.AL_CASES:
        i = B.fin_inputs(c)
        pa = B.Prm(3, c.C, (1, len(c.name)), "cpu")
        for g, n in enumerate(i["rows"]):
            if n == 0:
                continue
            d, y, v = B.valid_rows(i["want_d"][g], n), B.valid_rows(i["ya"][g], n), pa.v0
            _emu_bwd(d, y, i["cfa"][g], pa, g, "bn_finish")
            e = B.emulate_finish(d, y, i["cfa"][g], v["gamma"][g], v["dgamma"][g], v["dbeta"][g], factor=False)
            below += e["dbound"] < float(e["dy"].abs().max())
    assert below >= 3, below


def test_aligned_kind_meets_the_bound_terms():
    """kind "al": the element carrying max |d| also carries the extreme y with |A d| and |B y + K|
    adding, so |dy| there is the whole of |A| dmax + max|B y + K| (up to roundings)."""
    c = next(x for x in B.FIN_CASES if x.name == "f-n129-c60")
    i = B.fin_inputs(c)
    pa = B.Prm(3, c.C, (1, len(c.name)), "cpu")
    n = i["rows"][0]
    d, y = B.valid_rows(i["want_d"][0], n), B.valid_rows(i["ya"][0], n)
    o = B.finish_oracle(d, y, i["cfa"][0], pa.v0["gamma"][0], pa.v0["dgamma"][0], pa.v0["dbeta"][0])
    cf = i["cfa"][0].double().clone()
    cf[bs.A], cf[bs.B], cf[bs.K] = o["A"], o["B"], o["K"]
    dy, _ = B.dy_oracle(d, y, cf)
    top = float(dy.abs().max())
    assert top >= (1 - 1e-6) * o["dbound_max"] / (1 + 2.0 ** -9), (top, o["dbound_max"])


@pytest.mark.parametrize("p", B.DFIN_CASES, ids=B.dfin_id)
def test_emulated_dgrad_finish_within_bounds(p):
    c, mask, two, accum = p
    inp, i = CC.inputs(c), B.dfin_inputs(c, mask)
    pa, pb = B.Prm(c.G, c.Cin, (4, len(c.name)), "cpu"), B.Prm(c.G, c.Cin, (5, len(c.name)), "cpu")
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv == 0:
            continue
        dx = CC.lin_dgrad(inp["dy"][g, :nv].double(), inp["w"][CC.slot(inp, g)].double(), c)
        if accum:
            dx = dx + inp["acc"][g, :nv].double()
        d = torch.where(i["mask"][g, :nv], dx.float(), torch.zeros(()))
        n = i["rows"][g]
        _emu_bwd(B.valid_rows(d, n), B.valid_rows(i["ya"][g], n), i["cfa"][g], pa, g, "conv2d_dgrad finish")
        if two:
            _emu_bwd(B.valid_rows(d, n), B.valid_rows(i["yb"][g], n), i["cfb"][g], pb, g, "conv2d_dgrad finish")


# ============================================================ ops/reference.py in fp64 at bound64
@pytest.mark.parametrize("c", B.FIN_CASES, ids=_name)
def test_reference_bn_finish(c):
    with B.reference64() as R:
        out = B.run_finish(R, c, "cpu", REF, dt=torch.float64)
    B.check_finish_d(c, out, REF)
    B.check_finish(B.fin_inputs(c), out, c.two, "bn_finish", REF, ref64=True)


@pytest.mark.parametrize("c", B.STATS_CASES, ids=CC.case_id)
def test_reference_conv_bn_stats(c):
    with B.reference64() as R:
        r = B.run_conv_stats(R, c, "cpu", REF, dt=torch.float64)
    B.check_stats(r["y"], r["rows"], r["st"].coef, r["prm"], "conv_bn_stats", REF, ref64=True)


@pytest.mark.parametrize("p", B.DFIN_CASES, ids=B.dfin_id)
def test_reference_dgrad_finish(p):
    c, mask, two, accum = p
    with B.reference64() as R:
        out = B.run_dgrad_finish(R, p, "cpu", REF, dt=torch.float64)
    i = B.dfin_inputs(c, mask)
    for g, n in enumerate(out["rows"]):       # (the conv itself is test_conv_cases.py's)
        if n:
            off = B.valid_rows(out["d"][g], n)[~B.valid_rows(i["mask"][g], n)]
            assert bool((off == 0).all())
    B.check_finish(i, out, two, "conv2d_dgrad finish", REF, ref64=True)


@pytest.mark.parametrize("c", B.APPLY_CASES, ids=_name)
def test_reference_bn_apply(c):
    with B.reference64() as R:
        B.check_apply(c, B.run_apply(R, c, "cpu", REF, dt=torch.float64), REF, ref64=True)


@pytest.mark.parametrize("c", B.DY_CASES, ids=_name)
def test_reference_lazy_grad_value(c):
    with B.reference64() as R:
        B.check_dy(c, B.run_dy(R, c, "cpu", REF, dt=torch.float64), REF, ref64=True)


# ==================================================================== the dispatch, re-derived
@pytest.mark.parametrize("c", B.STATS_CASES, ids=CC.case_id)
def test_stats_rows_reach_the_producer_they_name(c):
    assert B.stats_path(c) == c.path
    if c.path == "stem":       # PIX = 256 / (Cout / 8) is a multiple of the 32-row group, M is not
        assert (256 // (c.Cout // 8)) % 32 == 0 and (c.N * c.Ho * c.Wo) % 32 != 0
    if c.path.endswith("reduce"):
        assert c.G > 1 and not CC.opt(c, "arena")          # slabs + bnx_tile_kernel mode 1


def test_statistics_change_the_dispatch():
    """The whole-image and staged kernels decline statistics: their rows land on xhalo / the GEMM."""
    by = {c.name: c for c in CC.FWD_CASES}
    plain = lambda c: c._replace(opt=tuple(kv for kv in c.opt if kv[0] != "pre"))   # noqa: E731
    assert CC.fwd_path(by["s16-frag"]) == "xstage16" and B.stats_path(plain(by["s16-frag"])) == "xhalo w16"
    assert CC.fwd_path(by["i8-cs32-n32-nopre"]) == "ximg" and B.stats_path(by["i8-cs32-n32-nopre"]).startswith(("gemm", "splitk"))
    with pytest.raises(AssertionError):
        B.stats_path(by["stem-5x5"])


@pytest.mark.parametrize("p", B.DFIN_CASES, ids=B.dfin_id)
def test_dgrad_finish_rows_reach_the_path_they_name(p):
    c = p[0]
    assert CC.dgrad_path(c) == c.path
    assert (c.s == 1) == (not c.path.startswith("classes"))      # stride 2: bn_finish after the class launch

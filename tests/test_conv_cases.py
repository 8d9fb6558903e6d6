"""CPU half of the conv-family edge-shape tests (conv_cases.py): the fp64 oracles against a direct
numpy im2col, the emulated fp16-pair arithmetic held to both bounds on every case (so the bounds
are not vacuous), ``ops/reference.py`` through every case in fp32 and fp64, and every row shown to
reach the kernel it names (from the library's exported decisions where there are any, from the
re-derived dispatch conditions otherwise)."""
import ctypes

import pytest
import torch

import conv_cases as C
from dba_mod_amd.ops import reference as R

OPS = (("fwd", C.FWD_CASES), ("dgrad", C.DGRAD_CASES), ("wgrad", C.WGRAD_CASES))
ALL = [(op, c) for op, cases in OPS for c in cases]
KINDS = {"fwd": lambda c: C.fwd_kind(c), "dgrad": lambda c: "a", "wgrad": lambda c: ""}


def _id(p):
    return f"{p[0]}-{p[1].name}"


@pytest.fixture(scope="module")
def lib():
    from dba_mod_amd.ops import hip     # host-side entry points only: no GPU is touched
    return hip._L


def test_tables_are_well_formed():
    names = [c.name for _, c in ALL]
    assert len(names) == len(set(names))
    for op, c in ALL:
        assert c.why and c.path, c
        inp = C.inputs(c)
        assert max(t.numel() for t in inp.values() if torch.is_tensor(t)) <= 1_100_000, c
        if c.G >= 3 and not C.opt(c, "scale"):
            nv = inp["nvalid"]
            assert nv[0] == c.N and nv[2] == 0 and 0 < nv[1] <= c.N, c
        if inp["wsel"] is not None and c.G >= 3:
            assert len(set(inp["wsel"])) < c.G and len(set(inp["wsel"])) < inp["slots"], c   # repeated and skipped


# the 14 smallest cases of EACH op (by multiply-adds), so every oracle meets its numpy witness
SMALL = [(op, c) for op, cases in OPS
         for c in sorted(cases, key=lambda c: c.N * c.Ho * c.Wo * c.K * c.Cout)[:14]]


def test_every_oracle_has_a_numpy_witness():
    for op, _ in OPS:
        assert sum(1 for o, _ in SMALL if o == op) >= 10, op


@pytest.mark.parametrize("p", SMALL, ids=_id)
def test_oracle_against_numpy_im2col(p):
    """torch is not its own witness: the three fp64 oracles (value and magnitude) against numpy."""
    op, c = p
    inp = C.inputs(c)
    for g in range(c.G):
        if inp["nvalid"][g] == 0:
            continue
        a, b = C.operands(op, c, inp, g)
        want, A = C.np_lin(op, a, b, c), C.np_lin(op, a.abs(), b.abs(), c)
        got = C.LIN[op](a.double(), b.double(), c)
        assert bool(((got - want).abs() <= 1e-12 * A).all()), (op, c, g)
        gotA = C.LIN[op](a.double().abs(), b.double().abs(), c)
        assert bool(((gotA - A).abs() <= 1e-12 * A).all()), (op, c, g)


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_emulation_within_both_bounds(p):
    """The emulated arithmetic, in each of its summation orders, stays inside the a-priori bound
    (and, by construction, E_pair): the reference alone satisfies what the kernels are held to."""
    op, c = p
    kind = KINDS[op](c)
    inp = C.inputs(c)
    o = C.oracle(op, c, kind)
    for g in range(c.G):
        if o[g] is None:
            continue
        a, b = C.operands(op, c, inp, g)
        for order in range(3):
            e = C.epilogue32(op, c, inp, g, C.emulate(op, c, a, b, order), kind)
            C.check_bound(e, o[g].want, o[g].apriori, f"{op} emulation", "a-priori", f"order {order}")
            C.check_bound(e, o[g].want, C.sharp(o[g]), f"{op} emulation", "4 E_pair", f"order {order}")
        assert o[g].E <= float(o[g].apriori.max()), (c, g)


@pytest.fixture()
def compute_dtype():
    old = R.COMPUTE_DTYPE
    yield
    R.COMPUTE_DTYPE = old


def _reference(op, c, dt):
    """ops/reference.py on the valid images of every replica (its ops take whole replicas)."""
    inp = C.inputs(c)
    R.COMPUTE_DTYPE = dt
    outs = []
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv == 0:
            outs.append(None)
            continue
        sl = C.slot(inp, g)
        wsel = torch.tensor([sl], dtype=torch.int32)
        kind = KINDS[op](c)
        if op == "fwd":
            y = R.conv2d(inp["x"][g:g + 1, :nv].to(dt), inp["w"].to(dt), wsel, c.s, c.p,
                         bias=inp["bias"].to(dt) if "b" in kind else None,
                         residual=inp["res"][g:g + 1, :nv].to(dt) if "r" in kind else None, relu="R" in kind)[0]
        elif op == "dgrad":
            y = R.conv2d_dgrad(inp["dy"][g:g + 1, :nv].to(dt), inp["w"].to(dt), wsel, c.s, c.p, (c.H, c.W),
                               accum=inp["acc"][g:g + 1, :nv].to(dt))[0]
        else:
            dw = inp["dw_old"][g:g + 1].to(dt).clone()
            R.conv2d_wgrad(inp["dy"][g:g + 1, :nv].to(dt), inp["x"][g:g + 1, :nv].to(dt), c.s, c.p, c.KH, c.KW, dw)
            y = dw[0]
        outs.append(y)
    return outs


@pytest.mark.parametrize("p", ALL, ids=_id)
def test_reference_ops_fp64_and_fp32(p, compute_dtype):
    op, c = p
    o = C.oracle(op, c, KINDS[op](c))
    for dt in (torch.float64, torch.float32):
        for g, y in enumerate(_reference(op, c, dt)):
            if y is None:
                continue
            bound = C.bound64(o[g].A) if dt == torch.float64 else C.bound32(C.red_len(op, c) + 2, o[g].A)
            C.check_bound(y, o[g].want, bound, f"{op} reference", "value", str(dt))


@pytest.mark.parametrize("c", C.FWD_CASES, ids=C.case_id)
def test_forward_rows_reach_their_kernel(c, lib):
    assert C.fwd_path(c) == c.path
    if c.path != "stem" and not C.opt(c, "policy") and c.name != "stem-eval-mfma":
        n = int(lib.dba_xconv_ws_floats(c.G, c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW))
        k = int(lib.dba_xconv_sk_ints(c.G, c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW))
        if c.path.startswith("splitk"):
            s = int(c.path.split()[0][len("splitk"):])
            assert n == s * c.G * c.N * c.Ho * c.Wo * c.Cout, (c, n)
            # counters are offered (an arena) only in the rows that say so: in-launch needs both
            assert (k > 0 and bool(C.opt(c, "arena"))) == c.path.endswith("inlaunch"), (c, k)
        elif c.path.startswith("gemm"):
            assert n == 0, (c, n)


@pytest.mark.parametrize("c", C.DGRAD_CASES, ids=C.case_id)
def test_dgrad_rows_reach_their_kernel(c, lib):
    assert C.dgrad_path(c) == c.path
    if c.s == 1:
        n = int(lib.dba_xconv_ws_floats(c.G, c.N, c.H, c.W, c.Cout, c.Cin, c.KH, c.KW))
        k = int(lib.dba_xconv_sk_ints(c.G, c.N, c.H, c.W, c.Cout, c.Cin, c.KH, c.KW))
        if c.path.startswith("splitk"):
            s = int(c.path.split()[0][len("splitk"):])
            assert n == s * c.G * c.N * c.H * c.W * c.Cin, (c, n)
            assert (k > 0 and bool(C.opt(c, "arena"))) == c.path.endswith("inlaunch"), (c, k)
        elif c.path.startswith("gemm"):
            assert n == 0, (c, n)


@pytest.mark.parametrize("c", C.WGRAD_CASES, ids=C.case_id)
def test_wgrad_rows_reach_their_kernel(c, lib):
    path, Z, mchunk = C.wgrad_path(c)
    assert path == c.path, (c, path, Z, mchunk)
    if path == "stem":
        assert int(lib.dba_xwgrad_stem_ws_floats(c.G, c.N, c.H, c.W, c.Cin, c.Cout)) == Z * c.G * c.Cout * c.K
    else:
        assert C.wgrad_path(c, lib) == (path, Z, mchunk)
        mc = ctypes.c_int(0)
        n = int(lib.dba_xwgrad_ws_floats(c.G, c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW, ctypes.byref(mc)))
        assert n == (Z * c.G * c.Cout * c.K if Z > 1 else 0)


def test_dgrad_entry_points_refuse_stride_above_two(lib):
    """The parity-class tables hold s * s <= 4 entries: dba_xconv_dgrad / dba_xtranspose return
    their error code for stride 3 before anything is built or launched (null pointers suffice)."""
    rc = lib.dba_xconv_dgrad(None, 0, None, 0, None, None, None, 0, None, 1, 1, 8, 8, 4, 3, 3, 4, 3, 3, 3, 1, None, 0, None,
                             0, None, 0, None, 0, None, 0, None, None)
    assert rc == -110
    desc = torch.tensor([[0, 0, 0, 4, 3, 3, 4, 3, 1, 0]], dtype=torch.int64)
    assert lib.dba_xtranspose(desc.data_ptr(), 1, 1, 144, None, None) == -110
    from dba_mod_amd.ops import hip
    dy, w = torch.zeros(1, 1, 3, 3, 4), torch.zeros(1, 4, 3, 3, 4)
    with pytest.raises(ValueError, match="stride 3"):
        hip.conv2d_dgrad(dy, w, None, 3, 1, (8, 8))
    with pytest.raises(ValueError, match="stride 3"):
        hip.prepare_dgrad_weights(w, [(w, None, 3, 1, (8, 8), None, 1)])
    with pytest.raises(ValueError, match="stride 0"):
        hip.conv2d_dgrad(dy, w, None, 0, 1, (8, 8))

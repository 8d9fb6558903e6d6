"""CPU half of the evaluation-path tests (eval_cases.py): the emulated arithmetic of the fused blocks
held to the a-priori bound on every row (so that bound is not vacuous; E_pair is the emulation's own
error), a coarser mid scale shown to miss the sharp bound, ``ops/reference.py`` in fp32 and fp64
through every row, the bit-exact expectations (probes, dead mid activations, all-zero
replicas) shown on the emulation, the shortcut rescale's overflow under the rule it replaced, and
the numpy oracles of the operand helpers against their definitions."""
import numpy as np
import pytest
import torch

import conv_cases as C
import eval_cases as E


def test_table_is_well_formed():
    ids = [repr(r) for r in E.ROWS]
    assert len(ids) == len(set(ids))
    for r in E.ROWS:
        assert r.why and r.G <= 3 and r.N <= 6, r
        assert r.wsel is not None or r.G == r.slots, r
        d = E.inputs(r)
        assert all(bool(torch.isfinite(t).all()) for t in d.values()), r
    for name, ops_ in (("one", "BSD"), ("groups", "BSD"), ("bands", "BS"), ("deadmid", "BS"), ("black", "S"), ("oddpix", "D")):
        assert {r.op for r in E.ROWS if r.name == name} == set(ops_), name
    groups = next(r for r in E.ROWS if r.name == "groups")
    assert groups.nvalid == (5, 2, 0) and groups.wsel == (1, 0, 1) and groups.N * 4 - 1 == 19
    assert tuple(p for r in E.ROWS if r.name.startswith("apart") for p in E.ropt(r, "pairs")) == E.APART
    # every weight operand of every op is scaled by a scale-w row and probed by a probe row
    for op, ws in E.WEIGHTS.items():
        for kind in ("scale", "probe"):
            assert {r.name.split("-")[1] for r in E.ROWS if r.op == op and r.name.startswith(kind + "-w")} == set(ws), (op, kind)


def test_garbage_does_not_reach_the_oracle():
    """The two garbage fillings of ``groups`` differ only past nvalid."""
    for r in (r for r in E.ROWS if E.ropt(r, "garbage2")):
        a, b = E.inputs(r), E.inputs(r, 1e30)
        for k in a:
            for g in range(r.G):
                nv = E.nvalid_of(r, g)
                if k in ("x", "x2"):
                    assert torch.equal(a[k][g, :nv], b[k][g, :nv])
                    assert nv == r.N or not torch.equal(a[k][g, nv:], b[k][g, nv:])


@pytest.mark.parametrize("r", E.ROWS, ids=E.row_id)
def test_emulation_and_reference_hold_the_bounds(r):
    """Every summation order of the emulation and ``ops/reference.py`` in fp32 stay inside the a-priori
    bound on every element (E_pair is the largest of the emulation's errors by construction); the fp64
    reference is the oracle and agrees with a direct conv chain."""
    d, o = E.inputs(r), E.oracle(r)
    for g in range(r.G):
        if o[g] is None:
            assert E.nvalid_of(r, g) == 0
            continue
        assert bool(torch.isfinite(o[g].want).all()) and bool((o[g].apriori > 0).all())
        assert bool((o[g].A >= o[g].want.abs() * (1 - 1e-12)).all())
        for order in range(3):
            em = E.emulate(r, d, g, order)
            E.check_bound(em, o[g].want, o[g].apriori, E.OPNAME[r.op], "y: a-priori", f"emulation order {order}")
        E.check_bound(E.reference(r, g, torch.float32), o[g].want, o[g].apriori, E.OPNAME[r.op], "y: a-priori", "reference fp32")
        E.check_bound(_direct64(r, d, g), o[g].want, 1e-12 * o[g].A, E.OPNAME[r.op], "y: fp64", "direct chain")


def _direct64(r, d, g):
    """The op written out conv by conv in fp64 (the oracle's witness)."""
    nv, s = E.nvalid_of(r, g), E.slot_of(r, g)
    x = d["x"][g, :nv].double()
    p = lambda k: d[k][s].double()     # noqa: E731
    if r.op == "D":
        return torch.relu(E.cv(x, p("w2")) + p("b2") + E.cv(d["x2"][g, :nv].double(), p("wsc"), 2, 0) + p("bsc"))
    if r.op == "S":
        x = torch.relu(E.cv(x, p("w0")) + p("b0"))
    h = torch.relu(E.cv(x, p("w1")) + p("b1"))
    return torch.relu(E.cv(h, p("w2")) + p("b2") + x)


EXACT_ROWS = [r for r in E.ROWS if E.ropt(r, "exact") or E.ropt(r, "dead") or E.ropt(r, "zero") is not None]


@pytest.mark.parametrize("r", EXACT_ROWS, ids=E.row_id)
def test_exact_expectations_hold_on_the_emulation(r):
    """Probes: the fp64 oracle is fp32-representable and every order of the emulation returns it bit
    for bit.  Dead mid activations and all-zero replicas: the documented epilogue alone."""
    d, o, seen = E.inputs(r), E.oracle(r), 0
    for g in range(r.G):
        m, want = E.exact_expect(r, g)
        if want is None:
            continue
        seen += 1
        if E.ropt(r, "exact"):
            assert bool((want.double() == o[g].want).all()), "the probe's oracle is not exact in fp32"
            assert bool((o[g].E == 0).all() if torch.is_tensor(o[g].E) else o[g].E == 0)
            assert float(want.max()) > 0 and len(torch.unique(want)) >= 9
        for order in range(3):
            em = E.emulate(r, d, g, order)
            mm = torch.ones_like(em, dtype=torch.bool) if m is None else m.expand_as(em)
            E.check_exact(em[mm] + 0.0, want[mm], E.OPNAME[r.op], f"exact [{r.name}] replica {g}", f"emulation order {order}")
    assert seen


def test_deadmid_rows_have_a_dead_band():
    for r in (r for r in E.ROWS if E.ropt(r, "dead")):
        d = E.inputs(r)
        for g in range(r.G):
            s = E.slot_of(r, g)
            x = d["x"][g, :1].double()
            if r.op == "S":
                x = torch.relu(E.cv(x, d["w0"][s].double()) + d["b0"][s].double())
            h = torch.relu(E.cv(x, d["w1"][s].double()) + d["b1"][s].double())
            if g == 0:
                assert float(h[:, 7:17].max()) == 0 and float(h[:, :6].max()) > 0 and float(h[:, 18:].max()) > 0
            else:
                assert float(h.max()) == 0


@pytest.mark.parametrize("op", ["B", "S"])
def test_bands_row_excludes_a_coarser_mid_scale(op):
    """Replica 2 of ``bands`` (a mid contrast of 2^24): the mid activation split with the image's
    maximum instead of the band's misses 4 E_pair in the quiet bands 16 .. 23 and 24 .. 31, by far; the
    documented rule holds it there with the relative accuracy of the loud band."""
    r = next(r for r in E.ROWS if r.name == "bands" and r.op == op)
    d, o = E.inputs(r), E.oracle(r)[2]
    assert float(o.want[:, :5].max()) > 2.0 ** 20 * float(o.want[:, 16:].max()) > 0
    bad = (E.emulate(r, d, 2, 2, mid="image").double() - o.want).abs() / E.sharp(o)
    good = (E.emulate(r, d, 2, 2).double() - o.want).abs() / E.sharp(o)
    assert float(good.max()) <= 0.25 + 1e-9
    assert float(bad[:, 16:24].max()) > 8 and float(bad[:, 24:].max()) > 8, (float(bad[:, 16:24].max()), float(bad[:, 24:].max()))
    rel = float(((E.emulate(r, d, 2, 2).double() - o.want).abs()[:, 24:] / o.want[:, 24:].abs().max()).max())
    assert rel < 2.0 ** -20, rel


def test_probe_taps_are_distinct_and_decode():
    """A flipped or shifted tap changes the expected pattern: the nine taps differ pairwise, also in
    magnitude, and the two slots order them differently."""
    for s in range(2):
        t = E._taps(s).view(-1)
        assert len(set(t.abs().tolist())) == 9 and (t < 0).sum() == 2
    assert not torch.equal(E._taps(0), E._taps(1)) and not torch.equal(E._taps(0), E._taps(0).flip(0, 1))
    for name in ("probe-w1", "probe-w2"):      # every one-hot of S's conv probes lies in the channel the taps read
        r = next(r for r in E.ROWS if r.op == "S" and r.name == name)
        x = E.inputs(r)["x"]
        assert int((x[..., 1] != 0).sum()) == r.G * r.N and not bool(x[..., 0].any()) and not bool(x[..., 2].any())
    r = next(r for r in E.ROWS if repr(r) == "S-probe-w0")
    w0 = E.inputs(r)["w0"]
    for s in range(2):
        for ch in range(3):
            assert len(set(w0[s, E.PAIR[s][0], :, :, ch].abs().view(-1).tolist())) == 9


def test_unbounded_shortcut_shift_overflows():
    """The defect the ``apart`` rows found: under the rule before the shift bound the emulated rescale
    pushes finite accumulators to inf where max |a| >= 1e6 meets a vanishing x2; the bounded rule is
    finite and moves no bit where the old shift was at most 80."""
    bad = []
    for r in (r for r in E.ROWS if r.name.startswith("apart")):
        d = E.inputs(r)
        for g, pair in enumerate(E.ropt(r, "pairs")):
            nv, s = E.nvalid_of(r, g), E.slot_of(r, g)
            sa, sw2, sx, swsc = E.sc_scales(d["x"][g, :nv], d["w2"][s], d["x2"][g, :nv], d["wsc"][s], bounded=False)
            old, new = E.emulate(r, d, g, 2, bounded=False), E.emulate(r, d, g, 2)
            assert bool(torch.isfinite(new).all()), pair
            if sx + swsc - sa - sw2 <= E.SC_SHIFT_MAX:
                assert torch.equal(old, new), pair
            if not bool(torch.isfinite(old).all()):
                bad.append(pair)
    assert bad == [(1e6, 0.0), (1e30, 0.0), (1e30, 1e-30)]


# ================================================================================ operand helpers
def test_np_split_matches_its_definition():
    """``np_split`` against conv_cases.split (torch) and against the definition written out in fp64."""
    g = E.gen(5)
    w = E.split_values(5, 1025, g)
    got = E.np_split(w.numpy())
    for s in range(5):
        sc = C.hexp(C.amax(w[s]))
        h, l = C.split(w[s], sc)
        assert np.array_equal(got[s, 0], h.half().numpy().view(np.uint16)), s
        # (-0.0 - -0.0 = +0.0 in both, so the low planes agree in their zero signs too)
        assert np.array_equal(got[s, 1], l.half().numpy().view(np.uint16)), s
        ws = w[s].double().numpy() * 2.0 ** sc
        h64 = ws.astype(np.float16)
        assert np.array_equal(got[s, 0], h64.view(np.uint16))
        assert np.array_equal(got[s, 1], (ws - h64.astype(np.float64)).astype(np.float16).view(np.uint16))
    assert not got[2].any() or set(np.unique(got[2])) <= {0, 0x8000}          # the all-zero slot
    assert E.np_hexp(E.np_amax_bits(w[3].numpy())) == 100                       # 1e-30: the cap
    assert E.np_hexp(E.np_amax_bits(w[4].numpy())) < -80                        # 1e30
    low = got[0, 1, 2].view(np.float16)
    assert low != 0 and abs(float(low)) < 2.0 ** -14                            # an fp16 subnormal low plane
    assert got[0, 0, 1] == 0x8000 and got[0, 1, 1] == 0                         # -0.0 -> (-0.0, +0.0)


def test_np_frag_is_the_documented_permutation():
    rng = np.random.default_rng(3)
    for ncol, cs in E.FRAG_SHAPES:
        per = ncol * 9 * cs
        planes = rng.integers(0, 65536, (2, 2, per), dtype=np.uint16)
        planes[:, 0] = np.arange(per, dtype=np.uint32).astype(np.uint16)     # plane 0 carries (index mod 2^16)
        f = E.np_frag(planes, ncol, cs)
        assert f.shape == (2, 2 * per)
        for s in range(2):
            assert np.array_equal(np.sort(f[s]), np.sort(planes[s].reshape(-1)))
    # by hand (test_gpu_ximg2.py's example): Cout = Cin = 64, column 37, tap 4, channel 45, low plane
    per = 64 * 9 * 64
    planes = rng.integers(0, 65536, (1, 2, per), dtype=np.uint16)
    assert E.np_frag(planes, 64, 64)[0, 64301] == planes[0, 1, 21613]


def test_np_amax_bits():
    f = lambda v: int(np.float32(v).view(np.int32))     # noqa: E731
    assert E.np_amax_bits([1.0, -3.0, 2.0]) == f(3.0)
    assert E.np_amax_bits([1.0, -3.0, 2.0], 1) == f(1.0)
    assert E.np_amax_bits([1.0, -3.0], 0) == 0
    assert E.np_amax_bits([-0.0]) == 0
    assert E.np_amax_bits([1e-40, -2e-40]) == f(2e-40)
    assert E.np_amax_bits([1.0, float("nan"), 0.5]) == f(1.0)       # fmaxf drops the NaN
    assert E.np_amax_bits([float("nan")]) == 0
    assert E.np_amax_bits([1.0, -float("inf")]) == f(float("inf"))

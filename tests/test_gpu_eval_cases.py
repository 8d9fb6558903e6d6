"""The evaluation path on the HIP kernels against eval_cases.py (GPU only): the fused blocks
(xblock.hip, xhalo.hpp's fused shortcut) on every row, element-wise and in fp64, against the a-priori
bound and 4 E_pair, with the kernel form each row reached, run-to-run / alone-vs-grouped /
weight-form bit equality, the folded output maximum and the rows' bit-exact expectations; and the
operand helpers (xaux.hip) against bit-exact numpy oracles."""
import ctypes

import numpy as np
import pytest
import torch

import eval_cases as E

pytestmark = pytest.mark.gpu
WHO = "hip"
SENT = 3e38           # between weight slots / behind segments: a maximum that must never be read
SENT16 = 0x5A5A       # behind plane buffers


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    return hip


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _same(a, b, what):
    for k in a:
        E.check_exact(a[k], b[k], what, k, "invariant")


# ================================================================================== fused blocks
@pytest.mark.parametrize("r", E.ROWS, ids=E.row_id)
def test_block(H, dev, r):
    """Both bounds on every valid element of every replica, the form the row names, the exact
    expectations, the folded maximum; bits run to run and of a replica alone against in its group."""
    form = E.FORM_DEFAULT[r.op]
    a, path = E.run(H, r, dev)
    assert path == form
    b, _ = E.run(H, r, dev)
    _same(a, b, f"{r!r}: run to run")
    E.check_out(r, a, form, WHO)
    for g in range(r.G if r.G > 1 else 0):
        s, path = E.run(H, r, dev, sel=g)
        assert path == form
        E.check_exact(a["y"][g:g + 1], s["y"], repr(r), f"y: replica {g} alone vs in its group", WHO)
        E.check_exact(a["amax"][g:g + 1], s["amax"], repr(r), f"folded max: replica {g} alone vs in its group", WHO)


@pytest.mark.parametrize("r", [r for r in E.ROWS if E.ropt(r, "garbage2")], ids=E.row_id)
def test_block_ignores_what_lies_past_nvalid(H, dev, r):
    """Garbage of scale 777 against 1e30 behind nvalid (and in the empty replica): the valid outputs
    and the folded maxima are the same bits."""
    a, _ = E.run(H, r, dev)
    b, path = E.run(H, r, dev, garbage=1e30)
    assert path == E.FORM_DEFAULT[r.op]
    _same(a, b, f"{r!r}: garbage 777 vs 1e30")
    E.check_out(r, b, path, WHO, garbage=1e30)
    assert int(a["amax"][2]) == 0          # the empty replica folds nothing


@pytest.mark.parametrize("r", E.XSTAGE_ROWS, ids=E.row_id)
def test_block_weight_forms_give_the_same_bits(H, dev, r):
    """set_xstage(1) / (2) / (3): each reaches the form it selects (the launch record), all three the
    same bits, each inside the bounds."""
    outs = {}
    for mode in (1, 2, 3):
        outs[mode], path = E.run(H, r, dev, xstage=mode)
        assert path == E.form_under(r.op, mode), (mode, path)
        E.check_out(r, outs[mode], path, WHO)
    _same(outs[1], outs[2], f"{r!r}: set_xstage(1) vs (2)")
    _same(outs[3], outs[2], f"{r!r}: set_xstage(3) vs (2)")


def test_launch_record_of_the_plain_halo_conv_has_no_shortcut(H, dev):
    """``form`` stays 0 for the halo conv without the fused shortcut (kind 2)."""
    x = torch.randn(1, 1, 16, 16, 64, device=dev)
    w = torch.randn(1, 32, 3, 3, 64, device=dev) * 0.05
    H.conv2d(x, w, None, 1, 1)
    l = H.last_conv_launch()
    assert (l["kind"], l["kernel"], l["tile"], l["form"]) == (2, "xhalo", 16, 0)


# ================================================================================== split planes
def _bits16(t):
    return t.cpu().numpy().view(np.uint16)


def _split_direct(H, dev, w_cpu, sstride):
    """dba_xsplit_w on rows ``sstride`` apart with sentinels between the slots and behind the planes."""
    slots, per = w_cpu.shape
    buf = torch.full((slots, sstride), SENT, device=dev)
    buf[:, :per] = w_cpu.to(dev)
    am = H._amax(buf, sstride, per)
    pad = 64
    planes = torch.full((slots * 2 * per + pad,), SENT16, dtype=torch.int16, device=dev)
    H._call("dba_xsplit_w", buf.data_ptr(), sstride, per, slots, am.data_ptr(), am.shape[1], planes.data_ptr(), H._stream())
    torch.cuda.synchronize()
    assert bool((planes[slots * 2 * per:] == SENT16).all()), "wrote past the planes"
    assert bool((buf[:, per:] == SENT).all())
    return _bits16(planes[:slots * 2 * per]).reshape(slots, 2, per), am


@pytest.mark.parametrize("per", E.SPLIT_PERS + (E.SPLIT_SWEEP,))
def test_split_weights_against_numpy(H, dev, per):
    slots = 5 if per < E.SPLIT_SWEEP else 2
    w = E.split_values(slots, per, E.gen(41, per))
    want = E.np_split(w.numpy())
    for sstride in (per, per + 3):
        got, am = _split_direct(H, dev, w, sstride)
        bits = am.max(0).values[:slots].cpu().numpy()
        assert [int(b) for b in bits] == [E.np_amax_bits(w[s].numpy()) for s in range(slots)]
        assert np.array_equal(got, want), (per, sstride, int((got != want).sum()))


def _mixed_weights(n, dev, g):
    """n weights of mixed sizes (3x3 shapes that get fragment planes, and plain ones), 3 slots."""
    ws = []
    for i in range(n):
        if i % 3 == 0:
            co, ci = E.FRAG_SHAPES[(i // 3) % 4]
            shape = (3, co, 3, 3, ci)
        else:
            shape = (3, E.SPLIT_PERS[i % len(E.SPLIT_PERS)])
        per = int(np.prod(shape[1:]))
        ws.append(E.split_values(3, per, g).view(shape).to(dev))
    return ws


@pytest.mark.parametrize("n", [1, 24, 25])
def test_split_and_fragment_batches_against_numpy_and_single_calls(H, dev, n):
    """split_weights_batch / frag_weights_batch over n descriptors (one launch per 24) against the
    numpy oracles and against one call per weight."""
    ws = _mixed_weights(n, dev, E.gen(43, n))
    items = [(w, w[0].numel(), w[0].numel(), H._amax(w, w[0].numel(), w[0].numel())) for w in ws]
    H.split_weights_batch(items)
    torch.cuda.synchronize()
    nfrag = 0
    for w, _, per, am in items:
        want = E.np_split(w.cpu().view(3, per).numpy())
        assert np.array_equal(_bits16(w._dba_planes), want), tuple(w.shape)
        single = w.clone()
        H.split_weights(single, per, per, am)
        assert torch.equal(single._dba_planes, w._dba_planes)
        if w.dim() == 5:
            nfrag += 1
            wf = E.np_frag(want, w.shape[1], w.shape[4])
            assert np.array_equal(_bits16(w._dba_fplanes), wf), tuple(w.shape)
            assert torch.equal(single._dba_fplanes, w._dba_fplanes)
        else:
            assert not hasattr(w, "_dba_fplanes")
    assert nfrag == (n + 2) // 3


@pytest.mark.parametrize("n", [24, 25])
def test_fragment_batches_of_24_and_25(H, dev, n):
    g = E.gen(47, n)
    ws = []
    for i in range(n):
        co, ci = E.FRAG_SHAPES[i % 4]
        w = E.split_values(2, co * 9 * ci, g).view(2, co, 3, 3, ci).to(dev)
        w._dba_planes = torch.from_numpy(E.np_split(w.cpu().view(2, -1).numpy()).view(np.int16)).to(dev)
        ws.append(w)
    H.frag_weights_batch(ws)
    torch.cuda.synchronize()
    for w in ws:
        want = E.np_frag(_bits16(w._dba_planes), w.shape[1], w.shape[4])
        assert np.array_equal(_bits16(w._dba_fplanes), want), tuple(w.shape)


def test_fragment_launcher_refuses_and_writes_nothing(H, dev):
    per = 32 * 9 * 32
    planes = torch.zeros(2 * per + 8, dtype=torch.int16, device=dev)
    out = torch.full((2 * per + 8,), SENT16, dtype=torch.int16, device=dev)
    for p, o, ncol, cs in ((planes, out, 48, 32), (planes, out, 32, 48), (planes[1:], out, 32, 32), (planes, out[4:], 32, 32)):
        d = torch.tensor([[p.data_ptr(), o.data_ptr(), ncol, cs, 0]], dtype=torch.int64)
        assert H._L.dba_xfrag_w_batch(ctypes.c_void_p(d.data_ptr()), 1, 1, H._stream()) == -105
    torch.cuda.synchronize()
    assert bool((out == SENT16).all())
    # a bad 25th descriptor, behind a full first batch of 24 good ones: refused before the first launch
    outs = torch.full((25, 2 * per), SENT16, dtype=torch.int16, device=dev)
    d = torch.tensor([[planes.data_ptr(), outs[i].data_ptr(), 32, 48 if i == 24 else 32, 0] for i in range(25)], dtype=torch.int64)
    assert H._L.dba_xfrag_w_batch(ctypes.c_void_p(d.data_ptr()), 25, 1, H._stream()) == -105
    torch.cuda.synchronize()
    assert bool((outs == SENT16).all())


# ================================================================================== operand maxima
def _amax_bits(H, t, gstride, n_per_g, nvalid=None, per_item=0):
    a = H._amax(t, gstride, n_per_g, nvalid, per_item)
    torch.cuda.synchronize()
    return a.cpu()


def _flat_view(dev, rows_cpu, gstride, lead):
    """The rows at ``gstride`` floats apart, ``lead`` floats into a 16-B aligned buffer; sentinels elsewhere."""
    G, n = rows_cpu.shape
    buf = torch.full((lead + G * gstride + 8,), SENT, device=dev)
    v = buf[lead:lead + G * gstride].view(G, gstride)
    v[:, :n] = rows_cpu.to(dev)
    return v


AMAX_N = (1, 2, 3, 4, 5, 6, 7, 1023, 4096, 4097, 4098, 4099)


@pytest.mark.parametrize("n", AMAX_N + (E.AMAX_SWEEP,))
def test_amax_against_numpy(H, dev, n):
    """n % 4 of 0 .. 3, the maximum (negative) in the last element: the vector path's scalar tail; a
    misaligned base and a ``gstride % 4 != 0`` (the scalar path) give the aligned copy's bits."""
    G = 2
    x = torch.randn(G, n, generator=E.gen(51, n))
    x[:, -1] = torch.tensor([-7.5, 9.25])
    want = [E.np_amax_bits(x[g].numpy()) for g in range(G)]
    stride4 = (n + 3) // 4 * 4
    for gstride, lead in ((stride4, 0), (stride4, 1), (stride4 + 1, 0), (stride4 + 4, 4)):
        v = _flat_view(dev, x, gstride, lead)
        got = _amax_bits(H, v, gstride, n)
        assert [int(b) for b in got.max(0).values[:G]] == want, (n, gstride, lead)


def test_amax_valid_prefix_only(H, dev):
    """nvalid 0, a middle value and N, with garbage behind it."""
    G, N, per_item = 3, 4, 37
    x = torch.randn(G, N, per_item, generator=E.gen(53))
    nv = [0, 2, 4]
    for g in range(G):
        x[g, nv[g]:] = 1e30
        if nv[g]:
            x[g, nv[g] - 1, -1] = -50.0 - g
    t = x.to(dev)
    got = _amax_bits(H, t, N * per_item, N * per_item, torch.tensor(nv, dtype=torch.int32, device=dev), per_item)
    assert [int(b) for b in got.max(0).values[:G]] == [E.np_amax_bits(x[g].numpy(), nv[g] * per_item) for g in range(G)]
    assert int(got[:, 0].max()) == 0


def test_amax_special_values(H, dev):
    f = lambda v: int(np.float32(v).view(np.int32))     # noqa: E731
    rows = torch.tensor([[-3.0, -1.0, -2.0, -0.5, -0.25], [-0.0, -0.0, 0.0, -0.0, 0.0], [1e-40, -3e-40, 0.0, 2e-40, -0.0],
                         [1.0, float("-inf"), 2.0, 3.0, 4.0]])
    got = _amax_bits(H, rows.to(dev), 5, 5)
    assert [int(b) for b in got.max(0).values[:4]] == [f(3.0), 0, f(3e-40), f(float("inf"))]
    assert [int(b) for b in got.max(0).values[:4]] == [E.np_amax_bits(rows[g].numpy()) for g in range(4)]


@pytest.mark.parametrize("c", range(16))
def test_amax_sub_slots(H, dev, c):
    """16 blocks of one sweep: the maximum in block c's 1024 elements lands in sub-slot c, and the
    16-way maximum is numpy's."""
    n = 16 * 4096
    x = torch.randn(1, n, generator=E.gen(55)) * 0.1
    x[0, c * 1024 + 3] = -11.0 - c
    got = _amax_bits(H, x.to(dev), n, n)
    assert int(got[:, 0].max()) == E.np_amax_bits(x.numpy())
    assert int(got[:, 0].argmax()) == c


def test_amax_drops_a_nan_and_the_conv_still_propagates_it(H, dev):
    """amax_kernel folds with fmaxf, which returns the other operand for a NaN: the slot holds the
    maximum of the remaining elements (``if (b > 0.f)`` stores nothing for an all-NaN block).  The
    consuming conv multiplies the NaN element by that finite scale, splits NaN planes and the MFMAs
    carry it: exactly the outputs that read the element are NaN, and - the scale being that of the
    clean input - every other output keeps its bits."""
    x = torch.randn(1, 1, 8, 8, 4, generator=E.gen(57))
    x[0, 0, 0, 0, 0] = 5.0                     # the maximum, away from the NaN's outputs
    xn = x.clone()
    xn[0, 0, 5, 4, 2] = float("nan")
    want = E.np_amax_bits(x.numpy())
    for t in (x, xn):
        got = _amax_bits(H, t.to(dev), t.numel(), t.numel())
        assert int(got[:, 0].max()) == want
    got = _amax_bits(H, torch.full((1, 8), float("nan"), device=dev), 8, 8)
    assert int(got[:, 0].max()) == 0
    w = (torch.randn(1, 8, 3, 3, 4, generator=E.gen(59)) * 0.2).to(dev)
    y, yn = H.conv2d(x.to(dev), w, None, 1, 1).cpu(), H.conv2d(xn.to(dev), w, None, 1, 1).cpu()
    hit = torch.zeros(8, 8, dtype=torch.bool)
    hit[4:7, 3:6] = True
    assert bool(torch.isnan(yn[0, 0][hit]).all()) and torch.equal(yn[0, 0][~hit], y[0, 0][~hit])


def _segments(lengths, flat, offs4):
    """Segments of the given lengths laid along ``flat`` [G, S] with gaps, the i-th at an offset with
    ``off % 4 == offs4[i % 4]``; the element before and after each holds SENT, its last element the
    segment's maximum."""
    segs, pos = [], 2
    for i, n in enumerate(lengths):
        while pos % 4 != offs4[i % len(offs4)]:
            pos += 1
        flat[:, pos - 1] = SENT
        flat[:, pos + n] = SENT
        if n:
            flat[:, pos + n - 1] = -(20.0 + i)
        segs.append((pos, n))
        pos += n + 2
    return segs


@pytest.mark.parametrize("nseg", [1, 64])
def test_weight_amax_against_numpy(H, dev, nseg):
    """amax_segments_kernel loads 16 bytes at a time only where ``(off | gstride) % 4 == 0`` on a
    16-B aligned base, and then only the float4s with ``e + 3 < n``; everything else is scalar.  So with
    the row stride S a multiple of 4 the segments at ``off % 4 == 0`` take the vector path - lengths
    4095 and 4097 with a scalar tail of 3 and 1, 4096 with none, the maximum in the last element, a
    larger value just before and after - and those at ``off % 4`` of 1 .. 3 the scalar path; with S
    odd (``gstride % 4 != 0``) every segment of the launch is scalar."""
    lengths = [(0, 1, 4095, 4096, 4097, 5, 33)[i % 7] for i in range(nseg)] if nseg > 1 else [4097]
    G, S4 = 2, (sum(lengths) + 8 * nseg + 16 + 3) // 4 * 4
    for S in (S4, S4 + 1):
        for offs4 in ((0, 1, 2, 3), (1,), (0,)):
            flat = torch.randn(G, S, generator=E.gen(61, nseg)) * 0.1
            segs = _segments(lengths, flat, offs4)
            assert all(off % 4 == offs4[i % len(offs4)] for i, (off, _) in enumerate(segs))
            dflat = flat.to(dev)
            assert dflat.data_ptr() % 16 == 0 and dflat.stride(0) == S
            slots = H.weight_amax(dflat, segs)
            torch.cuda.synchronize()
            assert len(slots) == nseg
            for (off, n), a in zip(segs, slots):
                got = [int(b) for b in a.max(0).values[:G].cpu()]
                assert got == [E.np_amax_bits(flat[g, off:off + n].numpy()) for g in range(G)], (S, off, n)


def test_weight_amax_refuses_65_segments(H, dev):
    flat = torch.zeros(1, 1024, device=dev)
    with pytest.raises(RuntimeError):
        H.weight_amax(flat, [(4 * i, 4) for i in range(65)])


def test_report():
    """(Not a check: prints the err / bound table of ARCHITECTURE 6.2 with ``pytest -s``.)"""
    print("\n" + E.report())

"""The fp16-pair conv family (xconv*.hip/hpp, xhalo.hpp, xwgrad*.hip, xblock.hip, stem.hip) at its
dispatch boundaries against the fp64 oracles of conv_cases.py (GPU only): the same cases, oracles
and bounds as the CPU emulation in test_conv_cases.py.  Every comparison is element-wise and in
fp64, against the a-priori bound and against 4 E_pair; each op's bits are also checked run to run
and against a launch holding one replica alone; exact properties (zero operands, empty replicas,
sentinels) bit for bit.  The last section pins the non-finite contract of ARCHITECTURE 6.1: a NaN
operand reaches every output that reads it through every fused ReLU, and nothing else moves."""
import pytest
import torch

import conv_cases as C
from dba_mod_amd.ops import bnstate as bs

pytestmark = pytest.mark.gpu
WHO = "hip"
NAN = float("nan")


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
    a = run()
    C.same_bits(a, run(), "run to run")
    return a


def _solo(c, a, run, keys):
    g = C.solo_replica(c)
    if c.G == 1:
        return
    b = run(g)
    for k in keys:
        C.check_exact(a[k][g:g + 1], b[k], c.name, f"{k}: replica {g} alone vs in its group", WHO)


def _exact_zeros(op, c, got, kind):
    """Outputs no product reaches (and no epilogue term) are exactly 0: uncovered rows / columns,
    empty parity classes, an all-zero operand."""
    inp = C.inputs(c)
    for g, o in enumerate(C.oracle(op, c, kind)):
        if o is None:
            continue
        nv = inp["nvalid"][g]
        z = (o.A == 0)
        if bool(z.any()):
            v = got[g, :nv].cpu()[z]
            assert bool((v == 0).all()), f"{c.name}: replica {g}: {int((v != 0).sum())} outputs of no product are not 0"


# ============================================================================== forward
@pytest.mark.parametrize("c", C.FWD_CASES, ids=C.case_id)
def test_conv2d(H, dev, c):
    kind = C.fwd_kind(c)
    a = _twice(lambda: C.run_fwd(H, c, dev))
    assert C.launched_path(H) == c.path       # the row ran on the kernel it names
    C.check_act_out("fwd", c, a["y"], kind, WHO, c.path)
    _exact_zeros("fwd", c, a["y"], kind)
    _solo(c, a, lambda g: C.run_fwd(H, c, dev, sel=g), ["y"])


EPI_CASES = [c for c in C.FWD_CASES if c.name in ("h32-n28", "h16-n36", "h32-n28-pre", "t-co33-ci20-m25", "t-co132-ci36-m25",
                                                  "i8-cs96-n96", "k-inlaunch-800", "k-kslab-512", "stem-3x3")]


@pytest.mark.parametrize("kind", ["", "b", "r", "bR"])
@pytest.mark.parametrize("c", EPI_CASES, ids=C.case_id)
def test_conv2d_epilogues(H, dev, c, kind):
    """With and without bias / residual / ReLU (the table's rows run all three)."""
    a = C.run_fwd(H, c, dev, kind=kind)
    C.check_act_out("fwd", c, a["y"], kind, WHO, c.path)


def test_conv2d_presplit_planes_give_the_same_bits(H, dev):
    """Planes split once (evaluation) against the split while staging, at the halo edge shapes."""
    for name in ("h32-n28-pre", "h16-n36-pre"):
        c = next(x for x in C.FWD_CASES if x.name == name)
        plain = c._replace(opt=tuple(kv for kv in c.opt if kv[0] != "pre"))
        C.same_bits(C.run_fwd(H, c, dev), C.run_fwd(H, plain, dev, inp=C.inputs(c)), name)


# ============================================================================== data gradient
@pytest.mark.parametrize("prepared", [False, True], ids=["own-transpose", "prepared"])
@pytest.mark.parametrize("accum", [False, True], ids=["plain", "accum"])
@pytest.mark.parametrize("c", C.DGRAD_CASES, ids=C.case_id)
def test_conv2d_dgrad(H, dev, c, accum, prepared):
    kind = "a" if accum else ""
    a = _twice(lambda: C.run_dgrad(H, c, dev, accum=accum, prepared=prepared))
    assert C.launched_path(H) == c.path
    C.check_act_out("dgrad", c, a["dx"], kind, WHO, c.path)
    _exact_zeros("dgrad", c, a["dx"], kind)
    if not prepared:
        _solo(c, a, lambda g: C.run_dgrad(H, c, dev, sel=g, accum=accum), ["dx"])
    else:
        C.same_bits(a, C.run_dgrad(H, c, dev, accum=accum, prepared=False), "prepared vs own transpose")


# ============================================================================== weight gradient
@pytest.mark.parametrize("c", C.WGRAD_CASES, ids=C.case_id)
def test_conv2d_wgrad(H, dev, c):
    keys = ["dw", "db"]
    a = _twice(lambda: C.run_wgrad(H, c, dev))
    assert C.launched_path(H) == c.path
    assert bool(H.last_conv_launch()["lazy"]) == bool(C.opt(c, "lzx") or C.opt(c, "lzg"))
    C.check_wgrad_out(c, a, WHO, c.path)
    b = _twice(lambda: C.run_wgrad(H, c, dev, defer=True))
    C.check_wgrad_out(c, b, WHO, c.path + " flush")
    if C.wgrad_path(c)[1] <= 4:     # the batched reduce's z-groups are the serial z order up to 4 slabs
        for k in keys:
            C.check_exact(b[k], a[k], c.name, f"{k}: defer + wgrad_flush vs immediate", WHO)
    g = C.solo_replica(c)
    s = C.run_wgrad(H, c, dev, sel=g)
    for k in keys:
        C.check_exact(a[k][g:g + 1], s[k], c.name, f"{k}: replica {g} alone vs in its group", WHO)
    C.check_wgrad_out(c, s, WHO, c.path, sel=g)


def test_wgrad_flush_mixed_batches(H, dev):
    """One flush over 28 queued reductions: more than one descriptor batch (24), 4- and 16-z-group
    entries, a ``per % 4 != 0`` entry (its batch takes the scalar form, the next the vector form):
    every entry gets the bits of a flush of its own."""
    by = {c.name: c for c in C.WGRAD_CASES}
    order = [by["w-z2"], by["w-z32"], by["w-per-odd"], by["w-zpart"]] + [by["w-z2"], by["w-per-odd"]] * 10 \
        + [by["w-z32"], by["w-z2"], by["w-zpart"], by["w-halo16"]]
    assert len(order) == 28
    want = {c.name: C.run_wgrad(H, c, dev, defer=True) for c in set(order)}      # a flush of its own
    queue, outs = [], []
    for c in order:
        outs.append((c, C.run_wgrad(H, c, dev, queue=queue)))
    assert len(queue) == 28
    H.wgrad_flush(queue)
    for c, o in outs:
        for k in ("dw", "db"):
            C.check_exact(o[k], want[c.name][k], c.name, f"{k}: one of 28 in a flush vs a flush of its own", WHO)
        C.check_wgrad_out(c, o, WHO, c.path + " flush")


def test_dgrad_refuses_stride_above_two(H, dev):
    dy, w = torch.zeros(1, 1, 3, 3, 4, device=dev), torch.zeros(1, 4, 3, 3, 4, device=dev)
    with pytest.raises(ValueError, match="stride 3"):
        H.conv2d_dgrad(dy, w, None, 3, 1, (8, 8))
    with pytest.raises(ValueError, match="stride 4"):
        H.prepare_dgrad_weights(w, [(w, None, 4, 1, (12, 12), None, 1)])


# ============================================================================== non-finite operands
def _nan_inputs(c):
    """The case's inputs with one NaN in a corner pixel and one in an interior pixel of replica 0's
    first image, and one NaN weight in replica 1's slot (replica 0 reads another slot).  Returns
    (inputs, per-replica masks of the outputs that must be NaN, masks excluded from the bounds)."""
    inp = dict(C.inputs(c))
    x, w = inp["x"].clone(), inp["w"].clone()
    x[0, 0, 0, 0, 0] = NAN
    x[0, 0, c.H // 2, c.W // 2, c.Cin - 1] = NAN
    kh, kw = c.KH // 2, c.KW // 2
    s1 = -1
    if c.G > 1:                     # (a lone replica: the pixels only)
        s1 = C.slot(inp, 1)
        assert s1 != C.slot(inp, 0)
        w[s1, c.Cout - 1, kh, kw, 0] = NAN
    inp["x"], inp["w"] = x, w
    must, skip = [], []
    for g in range(c.G):
        nv = inp["nvalid"][g]
        m = torch.zeros(nv, c.Ho, c.Wo, c.Cout, dtype=torch.bool)
        e = m.clone()
        if g == 0:
            ind = torch.isnan(x[0, :nv]).double()
            hit = C.lin_fwd(ind, torch.ones(1, c.KH, c.KW, c.Cin, dtype=C.F64), c) > 0
            m |= hit
            e |= hit
        if C.slot(inp, g) == s1 and nv:
            wi = torch.zeros(1, c.KH, c.KW, c.Cin, dtype=C.F64)
            wi[0, kh, kw, 0] = 1
            hit = C.lin_fwd(torch.ones(nv, c.H, c.W, c.Cin, dtype=C.F64), wi, c)[..., 0] > 0   # the tap lands in the image
            m[..., c.Cout - 1] |= hit
            e[..., c.Cout - 1] = True          # (the tap over the zero padding: 0 x NaN, either way)
        must.append(m)
        skip.append(e)
    return inp, must, skip


NAN_CASES = [c for c in C.FWD_CASES if c.name in (
    "t-co33-ci20-m25", "t-co50-ci36-m127", "t-co160-ci96-m25", "g-7x5-s2", "h32-n28", "h16-n36-pre", "i8-cs96-n96",
    "i4-cs32-n96-ring", "s16-frag", "k-inlaunch-800", "k-reduce-800", "k-kslab-512", "stem-3x3", "stem-7x7",
    "stem-eval-mfma")]


@pytest.mark.parametrize("c", NAN_CASES, ids=C.case_id)
def test_conv2d_relu_passes_nan(H, dev, c):
    """bias + residual + ReLU epilogue: a NaN pixel / weight makes every output that reads it NaN
    (fmaxf(NaN, 0) = 0 laundered it), and every other valid output keeps both bounds: the operand
    maxima ignore NaN, so no scale moves."""
    kind = "brR"
    inp, must, skip = _nan_inputs(c)
    y = C.run_fwd(H, c, dev, kind=kind, inp=inp)["y"].cpu()
    assert C.launched_path(H) == c.path
    o = C.oracle("fwd", c, kind)
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv == 0:
            continue
        got = y[g, :nv]
        lost = must[g] & ~torch.isnan(got)
        assert not bool(lost.any()), f"{c.name}: replica {g}: {int(lost.sum())} of {int(must[g].sum())} outputs lost the NaN"
        clean = torch.where(skip[g], o[g].want.float(), got)
        if c.path == "stem":
            C.check_bound(clean, o[g].want, C.bound32(c.K + 2, o[g].A), "conv2d [stem]", "y beside a NaN", WHO)
        else:
            C.check_pair(clean, o[g], "conv2d", c.path, "y beside a NaN", WHO)


def _split(H, w):
    per = w[0].numel()
    H.split_weights(w, per, per, H._amax_w(w, per, per))
    return w


def _block_nan_check(run, x, img_shape, reach, ref, what, pixels=None):
    """``run(x)`` with a NaN corner / interior pixel in image 0 of replica 0: NaN everywhere within
    ``reach`` pixels, the other images bit-equal to the clean run, the rest of the image at the
    existing tests' fp32 level against the fp64 reference ``ref`` (the clean result)."""
    clean = run(x)
    for (h, w) in pixels or ((0, 0), (img_shape[0] // 2, img_shape[1] // 2 + 1)):
        xn = x.clone()
        xn[0, 0, h, w, 1] = NAN
        y = run(xn)
        Ho, Wo = y.shape[2:4]
        sh, sw = img_shape[0] // Ho, img_shape[1] // Wo
        hh, ww = torch.arange(Ho).view(-1, 1) * sh, torch.arange(Wo).view(1, -1) * sw
        near = ((hh - h).abs() <= reach) & ((ww - w).abs() <= reach) if sh == 1 else \
            ((hh == h - h % 2) & (ww == w - w % 2) & (h % 2 == 0) & (w % 2 == 0))
        got = y[0, 0].cpu()
        assert bool(torch.isnan(got[near]).all()), f"{what}: the NaN at {(h, w)} was laundered"
        rest = ~torch.isnan(got)
        assert bool(rest[~near].all()), f"{what}: NaN outside the receptive field of {(h, w)}"
        r = ref[0, 0].cpu()
        e = ((got.double() - r)[rest].norm() / r[rest].norm()).item()
        assert e < 2e-6, (what, e)
        assert torch.equal(y[0, 1:], clean[0, 1:]) and torch.equal(y[1:], clean[1:]), f"{what}: other images moved"


def test_block_evals_pass_nan(H, dev):
    """basic_block_eval, stem_block_eval, down_block_eval: both fused ReLUs of each."""
    from dba_mod_amd.ops import reference as R
    old, R.COMPUTE_DTYPE = R.COMPUTE_DTYPE, torch.float64
    try:
        g = C.gen(31)
        G, N, slots = 2, 2, 2
        wsel = torch.tensor([1, 0], dtype=C.I32, device=dev)
        nvalid = torch.tensor([2, 2], dtype=C.I32, device=dev)
        c64 = lambda t: t.double().cpu()   # noqa: E731
        x = torch.randn(G, N, 32, 32, 32, generator=g).to(dev)
        w1 = _split(H, (torch.randn(slots, 32, 3, 3, 32, generator=g) / 17).to(dev))
        w2 = _split(H, (torch.randn(slots, 32, 3, 3, 32, generator=g) / 17).to(dev))
        b1, b2 = torch.randn(slots, 32, generator=g).to(dev) * 0.1, torch.randn(slots, 32, generator=g).to(dev) * 0.1
        assert H.basic_block_ok(x, w1, w2)
        ref = R.basic_block_eval(c64(x), c64(w1), c64(b1), c64(w2), c64(b2), wsel.cpu())
        _block_nan_check(lambda t: H.basic_block_eval(t, w1, b1, w2, b2, wsel, nvalid), x, (32, 32), 2, ref, "basic_block_eval")
        w1n = w1.clone()
        w1n[1, 5, 1, 1, 0] = NAN          # replica 0 reads slot 1: its mid channel 5, so all of its output
        w1n = _split(H, w1n)
        yw, yc = H.basic_block_eval(x, w1n, b1, w2, b2, wsel, nvalid), H.basic_block_eval(x, w1, b1, w2, b2, wsel, nvalid)
        assert bool(torch.isnan(yw[0]).all()) and torch.equal(yw[1], yc[1]), "basic_block_eval: a NaN conv1 weight"
        img = torch.rand(G, N, 32, 32, 3, generator=g).to(dev)
        w0 = _split(H, (torch.randn(slots, 32, 3, 3, 3, generator=g) / 5).to(dev))
        b0 = torch.randn(slots, 32, generator=g).to(dev) * 0.1
        assert H.stem_block_ok(img, w0, w1, w2)
        ref = R.stem_block_eval(c64(img), c64(w0), c64(b0), c64(w1), c64(b1), c64(w2), c64(b2), wsel.cpu())
        _block_nan_check(lambda t: H.stem_block_eval(t, w0, b0, w1, b1, w2, b2, wsel, nvalid), img, (32, 32), 3, ref,
                         "stem_block_eval")
        w0n = w0.clone()
        w0n[1, 5, 1, 1, 0] = NAN
        w0n = _split(H, w0n)
        yw = H.stem_block_eval(img, w0n, b0, w1, b1, w2, b2, wsel, nvalid)
        yc = H.stem_block_eval(img, w0, b0, w1, b1, w2, b2, wsel, nvalid)
        assert bool(torch.isnan(yw[0]).all()) and torch.equal(yw[1], yc[1]), "stem_block_eval: a NaN stem weight"
        a = torch.randn(G, N, 16, 16, 64, generator=g).to(dev)
        x2 = torch.randn(G, N, 32, 32, 32, generator=g).to(dev)
        wd = _split(H, (torch.randn(slots, 64, 3, 3, 64, generator=g) / 24).to(dev))
        wsc = _split(H, (torch.randn(slots, 64, 1, 1, 32, generator=g) / 6).to(dev))
        bd, bsc = torch.randn(slots, 64, generator=g).to(dev) * 0.1, torch.randn(slots, 64, generator=g).to(dev) * 0.1
        assert H.down_block_ok(a, wd, x2, wsc)
        ref = R.down_block_eval(c64(a), c64(wd), c64(bd), c64(x2), c64(wsc), c64(bsc), wsel.cpu())
        _block_nan_check(lambda t: H.down_block_eval(t, wd, bd, x2, wsc, bsc, wsel, nvalid), a, (16, 16), 1, ref,
                         "down_block_eval (conv input)")
        _block_nan_check(lambda t: H.down_block_eval(a, wd, bd, t, wsc, bsc, wsel, nvalid), x2, (32, 32), 0, ref,
                         "down_block_eval (shortcut input)", pixels=((0, 0), (16, 18), (16, 17)))
        yc = H.down_block_eval(a, wd, bd, x2, wsc, bsc, wsel, nvalid)
        for which in ("conv2", "shortcut"):      # a NaN weight of either operand pair: its output channel 5
            wdn, wscn = wd.clone(), wsc.clone()
            if which == "conv2":
                wdn[1, 5, 1, 1, 0] = NAN
            else:
                wscn[1, 5, 0, 0, 0] = NAN
            yw = H.down_block_eval(a, _split(H, wdn), bd, x2, _split(H, wscn), bsc, wsel, nvalid)
            assert bool(torch.isnan(yw[0, ..., 5]).all()), f"down_block_eval: a NaN {which} weight"
            oth = torch.ones(64, dtype=torch.bool)
            oth[5] = False
            got, r = yw[0][..., oth].double().cpu(), ref[0][..., oth]
            assert bool(torch.isfinite(got).all()) and ((got - r).norm() / r.norm()).item() < 2e-6, which
            assert torch.equal(yw[1], yc[1]), which
    finally:
        R.COMPUTE_DTYPE = old


def _lazy(H, x, dev, seed):
    """``x`` as the never-stored relu(BN(x)) of a previous BN with fixed coefficients."""
    G, N, Hh, Ww, Cc = x.shape
    z = torch.zeros(G, Cc, device=dev)
    p0 = bs.BnParams(z + 1, z.clone(), z.clone(), z + 1, z.clone(), z.clone(), 0.1, 1e-5)
    st0 = H._bnf_fwd(p0, True, G, N * Hh * Ww, Cc, dev)[1]
    g = C.gen(seed)
    coef = torch.zeros(G, bs.ROWS, Cc)
    coef[:, bs.SCALE] = torch.rand(G, Cc, generator=g) + 0.5
    coef[:, bs.SHIFT] = torch.randn(G, Cc, generator=g) * 0.3
    st0.coef.copy_(coef.to(dev))
    xr = torch.nan_to_num(x) * coef[:, bs.SCALE].to(dev).view(G, 1, 1, 1, Cc) + coef[:, bs.SHIFT].to(dev).view(G, 1, 1, 1, Cc)
    st0.bound[0, :G] = xr.relu().abs().amax(dim=(1, 2, 3, 4)).float().view(torch.int32)
    return bs.LazyBN(x, st0, True)


@pytest.mark.parametrize("shape", [(32, 32, 32), (16, 64, 64), (8, 32, 48)], ids=["halo32", "halo16", "gemm"])
def test_lazy_bn_relu_operand_passes_nan(H, dev, shape):
    """A conv and a weight gradient staging relu(BN(y)) from y (xconv.hpp / xhalo.hpp LZ,
    xwgrad.hip / xwgrad_halo.hip XLZ), and the stored bn_apply output (xbn.hip)."""
    W, Cin, Cout = shape
    G, N = 2, 3
    g = C.gen(41, W, Cin)
    x = torch.randn(G, N, W, W, Cin, generator=g).to(dev)
    w = (torch.randn(G, Cout, 3, 3, Cin, generator=g) / (3 * Cin ** 0.5)).to(dev)
    dy = torch.randn(G, N, W, W, Cout, generator=g).to(dev)
    nvalid = torch.tensor([N, N], dtype=C.I32, device=dev)
    h0, w0, ci = W // 2, 3, 5
    xn = x.clone()
    xn[0, 1, h0, w0, ci] = NAN       # an interior pixel of image 1
    xn[0, 2, 0, 0, 1] = NAN          # the corner pixel of image 2

    def prm():
        z = torch.zeros(G, Cout, device=dev)
        return bs.BnParams(z + 1, z.clone(), z.clone(), z + 1, z.clone(), z.clone(), 0.1, 1e-5)
    y, st = H.conv_bn_stats(_lazy(H, xn, dev, 5), w, None, 1, 1, nvalid, prm(), True)
    yc, _ = H.conv_bn_stats(_lazy(H, x, dev, 5), w, None, 1, 1, nvalid, prm(), True)
    near = torch.zeros(W, W, dtype=torch.bool)
    near[h0 - 1:h0 + 2, w0 - 1:w0 + 2] = True
    got = y[0, 1].cpu()
    assert bool(torch.isnan(got[near]).all()), "lazy BN+ReLU conv operand laundered the NaN"
    assert torch.equal(got[~near], yc[0, 1].cpu()[~near]) and torch.equal(y[1], yc[1]) and torch.equal(y[0, 0], yc[0, 0])
    corner = torch.zeros(W, W, dtype=torch.bool)
    corner[:2, :2] = True
    got = y[0, 2].cpu()
    assert bool(torch.isnan(got[corner]).all()), "lazy BN+ReLU conv operand laundered the corner NaN"
    assert torch.equal(got[~corner], yc[0, 2].cpu()[~corner])
    # one NaN weight: its output channel everywhere (the centre tap is always inside the image)
    wn = w.clone()
    wn[0, 3, 1, 1, 2] = NAN
    yw, _ = H.conv_bn_stats(_lazy(H, x, dev, 5), wn, None, 1, 1, nvalid, prm(), True)
    assert bool(torch.isnan(yw[0, ..., 3]).all()), "a NaN weight did not reach its output channel"
    others = torch.ones(Cout, dtype=torch.bool)
    others[3] = False
    assert torch.equal(yw[0][..., others], yc[0][..., others]) and torch.equal(yw[1], yc[1])
    # weight gradient reading the lazy operand: the NaN pixel's channel, every tap
    dw, dwc = torch.zeros(G, Cout, 3, 3, Cin, device=dev), torch.zeros(G, Cout, 3, 3, Cin, device=dev)
    H.conv2d_wgrad(dy, _lazy(H, xn, dev, 5), 1, 1, 3, 3, dw, None, nvalid=nvalid)
    H.conv2d_wgrad(dy, _lazy(H, x, dev, 5), 1, 1, 3, 3, dwc, None, nvalid=nvalid)
    assert bool(torch.isnan(dw[0, :, :, :, ci]).all()), "lazy BN+ReLU weight-gradient operand laundered the NaN"
    assert bool(torch.isnan(dw[0, :, :2, :2, 1]).all()), "... the corner NaN (the taps whose dy lies in the image)"
    assert torch.equal(dw[0, :, 2, :, 1], dwc[0, :, 2, :, 1]) and torch.equal(dw[0, :, :, 2, 1], dwc[0, :, :, 2, 1])
    keep = torch.ones(Cin, dtype=torch.bool)
    keep[ci] = keep[1] = False
    assert torch.equal(dw[0][..., keep], dwc[0][..., keep]) and torch.equal(dw[1], dwc[1])
    # the stored output relu(BN(y) + residual), both residual forms
    yn = yc.clone()
    yn[0, 1, h0, w0, 2] = NAN
    stc = H.conv_bn_stats(x, w, None, 1, 1, nvalid, prm(), True)[1]
    res = torch.randn_like(yc)
    for r_n, r_c in ((res, res), (bs.LazyBN(yn, stc, True), bs.LazyBN(yc, stc, True))):
        out = H.bn_apply(bs.LazyBN(yn, stc, False), r_n, True, nvalid)
        outc = H.bn_apply(bs.LazyBN(yc, stc, False), r_c, True, nvalid)
        hit = torch.zeros_like(out, dtype=torch.bool)
        hit[0, 1, h0, w0, 2] = True
        assert bool(torch.isnan(out[hit]).all()), "bn_apply + ReLU laundered the NaN"
        assert torch.equal(out[~hit], outc[~hit])


def test_training_step_nan_pixel_reaches_the_loss(H, dev):
    """A 3-replica, 4-image ResNet-18 CIFAR training step with one NaN pixel in replica 1: its loss
    and gradient are NaN (fl/trainer.py sets nan_flag from isnan(loss)); replicas 0 and 2 are finite
    and bit-equal to the clean step."""
    from dba_mod_amd import ops
    from dba_mod_amd.models import program as prog
    from dba_mod_amd.models.spec import get_spec
    spec = get_spec("resnet18_cifar")
    G, N = 3, 4
    g = C.gen(51)
    state = spec.init_flat(0).to(dev)[None].repeat(G, 1).contiguous()
    x0 = torch.rand(G, N, 32, 32, 3, generator=g).to(dev)
    labels = torch.randint(0, 10, (G, N), generator=g, dtype=torch.int32).to(dev)
    nvalid = torch.full((G,), N, dtype=C.I32, device=dev)

    def step(x):
        grads = torch.zeros(G, spec.P, device=dev)
        st = state.clone()
        ctx = prog.Ctx(spec, st, st, None, train=True, grads=grads, nvalid=nvalid, act_dtype=torch.float32)
        logits = prog.forward(ctx, x)
        loss, _, dl = ops.softmax_xent(logits, labels, True, True, grad_dtype=torch.float32)
        ctx.tape.backward(logits, dl)
        torch.cuda.synchronize()
        return loss.clone(), grads

    loss_c, grads_c = step(x0)
    xn = x0.clone()
    xn[1, 2, 7, 9, 1] = NAN
    loss, grads = step(xn)
    assert bool(torch.isfinite(loss_c).all()) and bool(torch.isfinite(grads_c).all())
    assert bool(torch.isnan(loss[1])), f"the NaN pixel never reached the loss: {loss.tolist()}"
    assert bool(torch.isnan(grads[1]).any()), "the NaN pixel never reached the gradient"
    for r in (0, 2):
        assert torch.equal(loss[r], loss_c[r]) and torch.equal(grads[r], grads_c[r]), f"replica {r} moved"


def test_report():
    """(Not a check: prints the err / bound table of ARCHITECTURE 6.2 with ``pytest -s``.)"""
    print("\n" + C.report())

"""The LDS-DMA weight stages of the evaluation convs (``set_xstage``: ``xblock.hip`` with ``GL``,
``xconv_fwd.hip xstage16_kernel``) against the LDS weight ring they replace (``set_xstage(2)``)
(GPU only).

Both forms run the same MFMA sequence per output element (the same k order, half-steps, plane
products and operand scales), so their outputs and folded output maxima are equal bit for bit;
the fp64-oracle comparisons of tests/test_gpu_xblock.py and tests/test_gpu_f32.py then cover the
new forms through the default.  Selector 1 takes the staged form in the kernels whose default is
on, 3 in every kernel that has one: both are compared with 2.  Weights without whole
fragment-ordered planes, and shapes the staged kernels do not take, must still run (through
today's kernels).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    prev = hip.set_xstage(-1)
    yield hip
    hip.set_xstage(prev)


def _weights(H, slots, dev, g, cout, cin):
    w = (torch.randn(slots, cout, 3, 3, cin, generator=g) / (3 * cin ** 0.5)).to(dev)
    per = w[0].numel()
    H.split_weights(w, per, per, H._amax_w(w, per, per))
    return w


def _ab(H, G, dev, run, mode, forms=None):
    """run() under selector ``mode`` and 2 -> [(y, folded max |y|)] of both.  ``forms``: the launch
    record (kind, form) each of the two runs must leave (ops.hip.last_conv_launch)."""
    outs = []
    prev = H.set_xstage(-1)
    try:
        for m in (mode, 2):
            H.set_xstage(m)
            assert H.set_xstage(-1) == m
            with H.amax_arena(G, dev):
                y = run()
                if forms is not None:
                    l = H.last_conv_launch()
                    assert (l["kind"], l["form"]) == forms[len(outs)], (m, l)
                outs.append((y, y._dba_amax.clone()))
    finally:
        H.set_xstage(prev)
    torch.cuda.synchronize()
    return outs


def _assert_equal(outs, G, N, nv):
    (y1, a1), (y2, a2) = outs
    for i in range(G):
        n = N if nv is None else nv[i]
        assert torch.equal(y1[i, :n], y2[i, :n]), f"replica {i}"
        if n:
            assert y1[i, :n].abs().max().item() > 0
    assert torch.equal(a1, a2)


def _wsel(G, dev):
    return torch.tensor([1, 0, 1][:G] if G == 3 else [1] * G, dtype=torch.int32, device=dev)   # a slot reused


# one image (all four row tiles of it: blocks whose top / bottom halo rows lie outside the image);
# a partly valid and an empty replica with a slot map that reuses a slot (blocks of both
# ownership groups of conv1's third row tile: blockIdx.x up to 19); a wide dynamic range
_BLOCK_CASES = [(1, 1, (1,), 1.0), (3, 5, (5, 2, 0), 1.0), (2, 4, None, 1e-3)]


def _block_inputs(G, N, nv, scale, stem, dev, H):
    g = torch.Generator().manual_seed(G * 100 + N * 10 + int(stem))
    slots = 2
    if stem:
        x = (torch.randn(G, N, 32, 32, 3, generator=g) * scale).to(dev)
        w0 = (torch.randn(slots, 32, 3, 3, 3, generator=g) * 0.3).to(dev)
        H.split_weights(w0, 32 * 27, 32 * 27, H._amax_w(w0, 32 * 27, 32 * 27))
    else:
        x = torch.relu(torch.randn(G, N, 32, 32, 32, generator=g) * scale).to(dev)
        w0 = None
    w1, w2 = _weights(H, slots, dev, g, 32, 32), _weights(H, slots, dev, g, 32, 32)
    b0, b1, b2 = [(torch.randn(slots, 32, generator=g) * 0.1 * scale).to(dev) for _ in range(3)]
    nvalid = None if nv is None else torch.tensor(nv, dtype=torch.int32, device=dev)
    return x, w0, b0, w1, b1, w2, b2, _wsel(G, dev), nvalid


def _block_run(H, stem, x, w0, b0, w1, b1, w2, b2, wsel, nvalid):
    if stem:
        assert H.stem_block_ok(x, w0, w1, w2)
        return lambda: H.stem_block_eval(x, w0, b0, w1, b1, w2, b2, wsel, nvalid)
    assert H.basic_block_ok(x, w1, w2)
    return lambda: H.basic_block_eval(x, w1, b1, w2, b2, wsel, nvalid)


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("stem", [False, True])
@pytest.mark.parametrize("G,N,nv,scale", _BLOCK_CASES)
def test_block_stages_bits_equal_ring(H, G, N, nv, scale, stem, mode):
    dev = torch.device("cuda")
    args = _block_inputs(G, N, nv, scale, stem, dev, H)
    assert args[3]._dba_fplanes.shape == (2, 2 * 32 * 288) and args[5]._dba_fplanes.shape == (2, 2 * 32 * 288)
    # the selector reached the weight form it names: staged (form 1) under 3, and under 1 where the
    # kernel's default is on (the plain block; the stem variant's is off); the ring (form 0) under 2
    kind = 11 if stem else 10
    staged = 1 if (mode == 3 or not stem) else 0
    _assert_equal(_ab(H, G, dev, _block_run(H, stem, *args), mode, ((kind, staged), (kind, 0))), G, N, nv)


@pytest.mark.parametrize("stem", [False, True])
def test_block_without_fragment_planes_runs_the_ring(H, stem):
    """One conv's fragment planes removed: the call succeeds under selector 3 and equals the
    ring form."""
    dev = torch.device("cuda")
    G, N, nv = 2, 3, (3, 1)
    args = _block_inputs(G, N, nv, 1.0, stem, dev, H)
    del args[5]._dba_fplanes
    kind = 11 if stem else 10
    _assert_equal(_ab(H, G, dev, _block_run(H, stem, *args), 3, ((kind, 0), (kind, 0))), G, N, nv)


# the 16-wide conv (W 16, 64 -> 64): with residual and ReLU, a partly valid replica; one image
# (both 8-row tiles of it) without residual
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("G,N,nv,res", [(2, 3, (3, 1), True), (1, 1, (1,), False)])
def test_conv16_stages_bits_equal_ring(H, G, N, nv, res, mode):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(G * 1000 + N * 10 + 16)
    slots = 2
    x = torch.relu(torch.randn(G, N, 16, 16, 64, generator=g)).to(dev)
    w = _weights(H, slots, dev, g, 64, 64)
    assert w._dba_fplanes.shape == (slots, 2 * 64 * 576)
    b = (torch.randn(slots, 64, generator=g) * 0.1).to(dev)
    r = torch.randn(G, N, 16, 16, 64, generator=g).to(dev) if res else None
    wsel = _wsel(G, dev)
    nvalid = torch.tensor(nv, dtype=torch.int32, device=dev)
    run = lambda: H.conv2d(x, w, wsel, 1, 1, bias=b, residual=r, relu=res, nvalid=nvalid)
    _assert_equal(_ab(H, G, dev, run, mode), G, N, nv)


@pytest.mark.parametrize("cout,planes", [(32, True), (64, False)])
def test_conv16_fallback_runs_todays_kernel(H, cout, planes):
    """A 64 -> 32 weight (not the staged kernel's tile), and a 64 -> 64 weight whose fragment
    planes have been removed: the call succeeds under selector 3 and equals selector 2."""
    dev = torch.device("cuda")
    G, N, nv = 2, 2, (2, 1)
    g = torch.Generator().manual_seed(cout)
    x = torch.relu(torch.randn(G, N, 16, 16, 64, generator=g)).to(dev)
    w = _weights(H, 2, dev, g, cout, 64)
    if not planes:
        del w._dba_fplanes
    b = (torch.randn(2, cout, generator=g) * 0.1).to(dev)
    wsel = _wsel(G, dev)
    nvalid = torch.tensor(nv, dtype=torch.int32, device=dev)
    run = lambda: H.conv2d(x, w, wsel, 1, 1, bias=b, relu=True, nvalid=nvalid)
    _assert_equal(_ab(H, G, dev, run, 3), G, N, nv)


def test_selector_round_trip(H):
    prev = H.set_xstage(-1)
    assert prev in (1, 2, 3)
    assert H.set_xstage(2) == prev and H.set_xstage(-1) == 2
    assert H.set_xstage(3) == 2 and H.set_xstage(-1) == 3
    assert H.set_xstage(prev) == 3 and H.set_xstage(-1) == prev

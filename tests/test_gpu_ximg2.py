"""The fragment-ordered-weight form of the whole-image halo conv (``xconv_fwd.hip ximg2_kernel``,
``set_ximg(1)``) against the LDS-weight-ring form it replaces (``ximg_kernel``, ``set_ximg(2)``),
and the weight layout it reads (``xaux.hip xfrag_w_kernel``) (GPU only).

Both forms run the same MFMA sequence per output element (chunk-major k order, taps 0..8, the
same plane products), so their outputs and folded output maxima are equal bit for bit; the
oracle comparisons of tests/test_gpu_ximg.py then cover the new form through the default.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    yield hip
    hip.set_ximg(1)


# a partial 8-image tile and two column tiles; the BN-64 path; an empty replica and a single
# chunk pair; one chunk (the refill path never runs)
@pytest.mark.parametrize("G,N,nv,W,Cin,Cout,res", [
    (3, 5, (5, 2, 4), 8, 128, 128, True), (2, 9, (9, 6), 4, 256, 256, True),
    (1, 11, (11,), 4, 128, 64, False), (2, 3, (3, 0), 8, 64, 64, False),
    (1, 1, (1,), 8, 32, 32, False)])
def test_ximg2_bits_equal_ximg(H, G, N, nv, W, Cin, Cout, res):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(G * 1000 + N * 10 + W)
    slots = 2
    x = torch.relu(torch.randn(G, N, W, W, Cin, generator=g)).to(dev)
    w = (torch.randn(slots, Cout, 3, 3, Cin, generator=g) / (3 * Cin ** 0.5)).to(dev)
    per = Cout * 9 * Cin
    H.split_weights(w, per, per, H._amax_w(w, per, per))
    assert w._dba_fplanes.shape == (slots, 2 * per)
    b = (torch.randn(slots, Cout, generator=g) * 0.1).to(dev)
    r = torch.randn(G, N, W, W, Cout, generator=g).to(dev) if res else None
    wsel = torch.tensor([1, 0, 1][:G] if G == 3 else [1] * G, dtype=torch.int32, device=dev)   # a slot reused
    nvalid = torch.tensor(nv, dtype=torch.int32, device=dev)
    outs = {}
    for mode in (1, 2):
        H.set_ximg(mode)
        with H.amax_arena(G, dev):
            y = H.conv2d(x, w, wsel, 1, 1, bias=b, residual=r, relu=True, nvalid=nvalid)
            outs[mode] = (y, y._dba_amax.clone())
    H.set_ximg(1)
    torch.cuda.synchronize()
    (y1, a1), (y2, a2) = outs[1], outs[2]
    for i in range(G):
        n = nv[i]
        assert torch.equal(y1[i, :n], y2[i, :n]), f"replica {i}"
        if n:
            assert y1[i, :n].abs().max().item() > 0
    assert torch.equal(a1, a2)


def test_fragment_ordered_planes_are_a_permutation(H):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    slots, Cout, Cin = 2, 64, 64
    w = (torch.randn(slots, Cout, 3, 3, Cin, generator=g) * 0.05).to(dev)
    per = Cout * 9 * Cin
    H.split_weights(w, per, per, H._amax_w(w, per, per))
    planes, frag = w._dba_planes.cpu(), w._dba_fplanes.cpu()
    assert frag.dtype == torch.int16 and frag.shape == (slots, 2 * per)
    for s in range(slots):
        assert torch.equal(planes[s].flatten().sort().values, frag[s].sort().values)
    # by hand: the low plane of column 37 (tile 1, row 5), tap 4, input channel 45 (chunk 1, element
    # 13: 16-B unit 1 = half-step 0, upper half-wave -> lane 32 + 5, element 5 of the unit).
    # K = 576, 18 k-steps per tile, k-step 1 * 9 + 4 = 13; 16-B unit index
    # ((1 * 18 + 13) * 4 + 0 * 2 + 1) * 64 + 37 = 8037 -> fp16 index 8037 * 8 + 5
    assert 8037 * 8 + 5 == 64301 and 37 * 576 + 4 * 64 + 45 == 21613
    assert torch.equal(frag[:, 64301], planes[:, 1, 21613])
    # the whole layout from its definition
    K, NK = 9 * Cin, 9 * Cin // 32
    idx = torch.arange(per // 4)
    lane, f, tt = idx & 63, (idx >> 6) & 3, idx >> 8
    t, nt = tt % NK, tt // NK
    e = (nt * 32 + (lane & 31)) * K + (t % 9) * Cin + (t // 9) * 32 + ((f >> 1) * 2 + (lane >> 5)) * 8
    src = ((f & 1) * per + e)[:, None] + torch.arange(8)[None, :]
    for s in range(slots):
        assert torch.equal(frag[s].view(-1, 8), planes[s].flatten()[src])


def test_only_whole_image_conv_shapes_get_fragment_planes(H):
    dev = torch.device("cuda")
    for shape, want in (((1, 64, 3, 3, 32), True), ((1, 64, 1, 1, 32), False), ((1, 32, 3, 3, 3), False),
                        ((1, 48, 3, 3, 32), False)):
        w = torch.randn(*shape, device=dev) * 0.05
        per = w[0].numel()
        H.split_weights(w, per, per, H._amax_w(w, per, per))
        assert hasattr(w, "_dba_fplanes") == want, shape

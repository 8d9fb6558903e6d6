"""Case tables, seeded generators, fp64 oracles, the CPU emulation and the bounds of the evaluation
path's tests: the fused blocks (csrc/kernels/xblock.hip ``basic_block_eval`` / ``stem_block_eval``,
xhalo.hpp ``xhalo_kernel<SC>`` behind ``down_block_eval``) and the operand helpers that feed them
(xaux.hip: weight planes, fragment order, operand maxima).  test_eval_cases.py (CPU) and
test_gpu_eval_cases.py (HIP) run the same rows against the same oracles with the same bounds.  The
split, ``hexp``, ``gemm3``, ``im2col`` and the bookkeeping are conv_cases.py's / step_kernel_cases.py's.

Ops (``op`` of a row): ``B`` y = relu(conv2(h) + b2 + x), h = relu(conv1(x) + b1) on [.., 32, 32, 32];
``S`` the same with x = s = relu(stem(img) + b0) computed in the launch from [.., 32, 32, 3] images;
``D`` y = relu(conv3x3(a, w2) + conv1x1_s2(x2, wsc) + (b2 + bsc)) on [.., 16, 16, 64] / [.., 32, 32, 32].

Oracle
------
``ops/reference.py``'s ``basic_block_eval`` / ``stem_block_eval`` / ``down_block_eval`` under
``COMPUTE_DTYPE = float64``, per replica through ``wsel``, on the valid images only (the rest of an
activation holds finite garbage).  The magnitude ``A`` is the same chain over absolute values with the
biases and the residual included.

The documented arithmetic (what ``emulate`` implements and these tests pin)
---------------------------------------------------------------------------
Every operand is split as in conv_cases.py (``x 2^s = h + l + e``, ``s = hexp(max)``), every product
is ``hh' + hl' + lh'`` accumulated in fp32 and the scale is removed at the end.  Which maximum:

* weights: the slot's max |w| (planes split once, xaux.hip).
* B conv1: the replica's max |x| over its valid images.  h = relu(. + b1) in fp32.  A workgroup owns
  the 8 output rows h0 .. h0+7 (h0 = 0, 8, 16, 24) of one image; its mid rows h0-1 .. h0+8 are zero
  outside the image and are split with hexp(max h over those 10 rows), the band's own scale, so rows
  h0-1 and h0+8 are split twice, by two workgroups, with two scales.  conv2 runs at that scale; then
  (acc + b2) + x with the fp32 x, then ReLU.
* S: per band the image rows h0-3 .. h0+10 clipped to the image are split with hexp(max |img| over
  them); the stem (K = 27 in one 32-deep k-step) runs on planes against the slot's pre-split w0;
  s = relu(. + b0) on patch rows h0-2 .. h0+9, exactly 0 (not relu(b0)) on rows outside the image; s is
  re-split with the band's max s, conv1 / the mid / conv2 as in B, the residual is the fp32 s.
* D: the 3x3 at the replica / slot scales sa, sw2 of a and w2 (s3 = sa + sw2); the shortcut's single
  k-step at swsc = hexp(max |wsc|) and
      sx = max(-126, min(hexp(max |x2| over the whole valid tensor, odd pixels included), s3 + 80 - swsc)),
  the accumulators rescaled by the power of two 2^(sx + swsc - s3) <= 2^80 before it (xhalo.hpp; without
  the bound a vanishing x2 shifted finite accumulators past fp32's range).  b2 + bsc are summed
  first, then added, then ReLU.

The a-priori bound (nothing in it is measured)
----------------------------------------------
One conv stage with operand magnitudes |a| (kernel-side: |oracle a| + the previous stage's bound) and
|w| has, exactly as in conv_cases.py,

    repr  <= 3 2^-22 (1 + 2^-10) A0 + (1 + 2^-9) (q_a Sw + q_w Sa) + 5 q_a q_w Kc
    stage <= conv(|w|, e_prev) + repr + (n + 2) 2^-24 A + 2^-149

with A0 = conv(|a|, |w|), Sa = conv(|a|, 1), Sw = conv(1, |w|), Kc = conv(1, 1), A = A0 + |bias| (+ the
residual's magnitude), n = 3 pad32(R) + the epilogue adds (1 bias, +1 residual: the exact-fp32
residual costs that one rounding), and 2^-149 for a result the scale removal rounds into the
subnormals.  ReLU is 1-Lipschitz, so a stage's element bound ``e_prev`` enters the next stage through
``conv(|w|, e_prev)`` and, for S's residual, directly.  R is 27 (the stem, padded to 32: it runs on
MFMA planes here and takes this bound, not ``bound32``), 288 (B / S) or 576 + 32 (D, one stage with two
products, n = 3 x 608 + 3: the bias sum, the bias add, and one for the rescaled accumulator).
The floor ``q = 2^-25 2^-s`` uses the scale the kernel documents for the operand.  Maxima of given
inputs (x, img, a, x2, the weights) are exact in the kernel, so s is the oracle's.  A band maximum of
a computed operand (s, h) differs from the oracle's M by at most the largest bound E of the stage over
the band's rows, and may fall on the other side of a power of two: s = hexp(M + E) - 1, one binade
coarser than the largest maximum the kernel can see.  D's x2 uses the bounded sx above, and adds
2^-149 2^-(sx + swsc) for accumulators a negative shift rounds into the subnormals.
For B / S the chain is evaluated once per band with that band's scales and the band's 8 output rows
are taken from it.

The sharp bound
---------------
``SHARP_FACTOR E_pair + 2^-23 |oracle|`` with ``E_pair`` the largest element error of ``emulate`` (the
rules above, fp32, over ``gemm3``'s three summation orders) against the oracle.  For D it is taken per
replica, as in conv_cases.py; for B / S per replica, image and band, the stricter reading: the bands
carry their own scales, and a replica-wide maximum would let a loud band hide an error in a quiet one.

Operand helpers
---------------
Bit-exact numpy oracles: ``np_split`` (h = f16(w 2^s), l = f16(w 2^s - h), round to nearest even,
s = min(100, 141 - (bits(max |w[slot]|) >> 23))), ``np_frag`` (the fragment order from its definition),
``np_amax_bits`` (max |x| over the valid prefix as float bits; fmaxf semantics: a NaN is dropped).
"""
import contextlib
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as C
from conv_cases import GARBAGE, SCALE_PEAKS, SHARP_FACTOR, amax, gemm3, hexp, im2col, nchw, nhwc, split, wk  # noqa: F401
from dba_mod_amd.ops import reference as R
from step_kernel_cases import F64, I32, U32, check_bound, check_exact, gen, report  # noqa: F401

F32 = torch.float32
BANDS = (0, 8, 16, 24)
SC_SHIFT_MAX = 80          # xhalo.hpp kScShiftMax
TINY = 2.0 ** -149

# expected launch records (ops.hip.last_conv_launch): the kernel and weight form a row must reach
FORM_DEFAULT = {"B": "xblock staged", "S": "xblock_stem ring", "D": "xhalo w16 pre sc"}


def launched(ops):
    l = ops.last_conv_launch()
    if l["kind"] in (10, 11):
        return f"{l['kernel']} " + ("staged" if l["form"] else "ring")
    if l["kind"] == 2:
        return f"xhalo w{l['tile']}" + (" pre" if l["pre"] else "") + (" sc" if l["form"] else "")
    return f"kind {l['kind']}"


def form_under(op, xstage):
    """The form ``set_xstage(xstage)`` selects: 1 the kernel's default, 2 the ring, 3 staged."""
    if op == "D":
        return FORM_DEFAULT[op]
    if xstage in (None, 1):
        return FORM_DEFAULT[op]
    return FORM_DEFAULT[op].split()[0] + (" ring" if xstage == 2 else " staged")


# ====================================================================================== rows
class Row(namedtuple("Row", "name op G N nvalid wsel slots why make opt")):
    __slots__ = ()

    def __repr__(self):
        return f"{self.op}-{self.name}"

    def __hash__(self):
        return hash((self.name, self.op))

    def __eq__(self, o):
        return (self.name, self.op) == (o.name, o.op)


def row_id(r):
    return repr(r)


def ropt(r, key, default=None):
    return dict(r.opt).get(key, default)


def shapes(op):
    """(activation [H, W, C], second activation or None, output [H, W, C])."""
    if op == "B":
        return (32, 32, 32), None, (32, 32, 32)
    if op == "S":
        return (32, 32, 3), None, (32, 32, 32)
    return (16, 16, 64), (32, 32, 32), (16, 16, 64)


WEIGHTS = {"B": ("w1", "w2"), "S": ("w0", "w1", "w2"), "D": ("w2", "wsc")}
BIASES = {"B": ("b1", "b2"), "S": ("b0", "b1", "b2"), "D": ("b2", "bsc")}
WSHAPE = {"B": {"w1": (32, 3, 3, 32), "w2": (32, 3, 3, 32)},
          "S": {"w0": (32, 3, 3, 3), "w1": (32, 3, 3, 32), "w2": (32, 3, 3, 32)},
          "D": {"w2": (64, 3, 3, 64), "wsc": (64, 1, 1, 32)}}


def ordinary(r, g, scale=1.0):
    """The existing tests' normalisation (test_gpu_xblock.py / test_gpu_xdown.py)."""
    G, N, S = r.G, r.N, r.slots
    sh, sh2, _ = shapes(r.op)
    d = {}
    if r.op == "S":
        d["x"] = torch.randn(G, N, *sh, generator=g) * scale
    else:
        d["x"] = torch.relu(torch.randn(G, N, *sh, generator=g) * scale)
    if sh2:
        d["x2"] = torch.relu(torch.randn(G, N, *sh2, generator=g) * scale)
    for k in WEIGHTS[r.op]:
        ws = WSHAPE[r.op][k]
        norm = 0.3 if k == "w0" else 1.0 / math.sqrt(ws[3]) if k == "wsc" else 1.0 / (3 * math.sqrt(ws[3]))
        d[k] = torch.randn(S, *ws, generator=g) * norm
    for k in BIASES[r.op]:
        d[k] = torch.randn(S, shapes(r.op)[2][2], generator=g) * (0.1 * scale)
    return d


def _acts(r):
    return ("x", "x2") if r.op == "D" else ("x",)


@functools.lru_cache(maxsize=None)
def inputs(r, garbage=GARBAGE):
    """Every operand of the row, fp32 on the CPU (never modified by a test); images at and past
    ``nvalid`` hold finite garbage of scale ``garbage``."""
    g = gen(11, r.G, r.N, len(r.name), ord(r.op), sum(map(ord, r.name)))
    d = r.make(r, g)
    gg = gen(13, int(math.log10(garbage)), len(r.name))
    if r.nvalid is not None:
        for k in _acts(r):
            for i, nv in enumerate(r.nvalid):
                if nv < r.N:
                    d[k][i, nv:] = garbage * torch.randn(d[k][i, nv:].shape, generator=gg)
    return d


def nvalid_of(r, g):
    return r.N if r.nvalid is None else r.nvalid[g]


def slot_of(r, g):
    return g if r.wsel is None else r.wsel[g]


# ------------------------------------------------------------------------------- generators
def _mk_ordinary(r, g):
    return ordinary(r, g)


def _mk_scale_act(r, g):
    """Replica i's activations at SCALE_PEAKS[i] with its own slot's biases at that scale; the zero
    replica's slot has non-positive b0 / b1, so its output follows from b2 (+ bsc) alone."""
    d = ordinary(r, g)
    for i, m in enumerate(SCALE_PEAKS):
        for k in _acts(r):
            d[k][i] = d[k][i].clamp(-4, 4) * (0.1 * m)
            if m:
                d[k][i, nvalid_of(r, i) - 1].view(-1)[-1] = m
        for k in BIASES[r.op]:
            d[k][i] = d[k][i] * (m if m else 1.0)
            if not m and k in ("b0", "b1"):
                d[k][i] = -d[k][i].abs()
    return d


def _mk_scale_w(r, g):
    d = ordinary(r, g)
    k = ropt(r, "w")
    for i, m in enumerate(SCALE_PEAKS):
        d[k][i] = d[k][i].clamp(-1, 1) * (0.5 * m)
        if m:
            d[k][i].view(-1)[-1] = -m
    return d


def _mk_denorm(r, g):
    d = ordinary(r, g)
    for k in _acts(r):
        v = d[k].view(-1)
        v[torch.randperm(v.numel(), generator=g)[:40]] = 1e-40
        v[7] = -1e-40
    return d


def _mk_bands(r, g):
    """Replica 0: rows 8 .. 15 of the input 2^12 larger than the rest.  Replica 1 (its own slot): a
    mild (x 3) input contrast that a negative per-channel b1 turns into a large one in the mid
    activation only (the quiet bands pass the threshold rarely and barely)."""
    d = ordinary(r, g)
    d["x"][0, :, 8:16] *= 4096.0
    d["x"][1, :, 16:24] *= 3.0
    sigma = 0.58 if r.op == "B" else 0.5          # conv1's output spread in the quiet rows
    d["b1"][1] = -(2.2 + 0.6 * torch.rand(32, generator=g)) * sigma
    # Replica 2 (slot 2, all biases 0): the first rows ordinary, the rest 2^-24 of them, so the mid
    # activation of bands 16 .. 23 and 24 .. 31 lies 2^24 below that of band 0 .. 7 and the output
    # there is conv2 of it alone.  B: the quiet x are integers k 2^-32, k < 64, exact in the high
    # plane (as fp16 subnormals) at the replica's scale, so conv1 carries no floor from the loud rows; S splits the
    # image per band.  A mid operand split with an image-wide (or the neighbouring band's) scale
    # pushes the quiet bands' planes into the fp16 subnormals: 2^-13 relative, against 2^-22.
    if r.op == "B":
        d["x"][2, :, 6:] = torch.randint(0, 64, d["x"][2, :, 6:].shape, generator=g).float() * 2.0 ** -32
    else:
        d["x"][2, :, 5:] *= 2.0 ** -24
    for k in BIASES[r.op]:
        d[k][2] = 0.0
    return d


def _grid(shape, g, lo, hi):
    """Signed powers of two 2^lo .. 2^hi: sums of a few of them are exact in fp32."""
    e = torch.randint(lo, hi + 1, shape, generator=g).double()
    sgn = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return (sgn * 2.0 ** e).float()


def _mk_deadmid(r, g):
    """Replica 0: rows 6 .. 17 of the block's input are 2^-8 of the rest and b1 sits between the two, so
    h == 0 on the ten mid rows of band 8 .. 15 only.  Replica 1: b1 = -1e3, h == 0 everywhere.  For S
    the image and the stem are on a grid of powers of two, so the fp32 s (the residual) is known
    exactly."""
    d = ordinary(r, g)
    if r.op == "S":
        d["x"] = _grid(d["x"].shape, g, -2, 1)
        d["w0"] = _grid(d["w0"].shape, g, -4, -2)
        d["b0"] = -torch.randint(0, 5, d["b0"].shape, generator=g).float() / 16
    lo, hi = (5, 19) if r.op == "S" else (6, 18)     # S: s rows 6 .. 17 read image rows 5 .. 18
    d["x"][0, :, lo:hi] *= 2.0 ** -8
    d["b1"][0] = -0.05 - 0.01 * torch.rand(32, generator=g)
    d["b1"][1] = -1e3
    return d


POS32 = ((0, 0), (0, 31), (31, 0), (31, 31), (7, 5), (8, 5), (15, 16), (16, 15), (23, 31), (24, 0))
TAP_SIGN = (1, 1, -1, 1, 1, 1, -1, 1, 1)


def _taps(s):
    """Nine distinct powers of two, tap k -> +-2^-k (slot 1: the exponents reversed)."""
    e = [k if s == 0 else 8 - k for k in range(9)]
    return torch.tensor([TAP_SIGN[k] * 2.0 ** -e[k] for k in range(9)]).view(3, 3)


PAIR = ((9, 5), (30, 17))       # the (cout, cin) pair of slot 0 / 1


def _identity(w):
    for o in range(min(w.shape[1], w.shape[4])):
        w[:, o, w.shape[2] // 2, w.shape[3] // 2, o] = 1.0
    return w


def _mk_probe(r, g):
    """One-hot inputs and power-of-two weights: every split and product is exact (``which`` names the
    probed conv; the other convs are centre-tap identities)."""
    which = ropt(r, "probe")
    G, N, S = r.G, r.N, r.slots
    sh, sh2, so = shapes(r.op)
    d = {"x": torch.zeros(G, N, *sh)}
    for k in WEIGHTS[r.op]:
        d[k] = torch.zeros(S, *WSHAPE[r.op][k])
    for k in BIASES[r.op]:
        d[k] = torch.zeros(S, so[2])
    pos = [(p if r.op != "D" else (p[0] // 2, p[1] // 2)) for p in POS32]
    for i in range(G):
        s = slot_of(r, i)
        co, ci = PAIR[s]
        for n in range(N):
            (pr, pc), v = pos[(i * N + n) % len(pos)], 2.0 ** (n % 3 - 1)
            if r.op == "B":
                d["x"][i, n, pr, pc, ci] = v
            elif r.op == "S":      # w0 probed: every image channel in turn; w1 / w2: the channel the taps read
                d["x"][i, n, pr, pc, n % 3 if which == "w0" else 1] = v
            elif which == "w2":
                d["x"][i, n, :, :, ci] = 0.125
                d["x"][i, n, pr, pc, ci] += v
    for s in range(S):
        co, ci = PAIR[s]
        if r.op in "BS":
            for k in ("w1", "w2"):
                if k == which:
                    d[k][s, co, :, :, 1 if r.op == "S" else ci] = _taps(s)
                else:
                    _identity(d[k][s:s + 1])
            d["b1"][s], d["b2"][s] = 2.0 ** -3, -2.0 ** -5
            if which == "w1":
                d["b1"][s], d["b2"][s] = 2.0 ** -4, 0.0
        if r.op == "S":
            if which == "w0":       # the stem's 27 (tap, channel) entries: +-2^-((4 tap + 3 ch) % 11)
                for t in range(9):
                    for ch in range(3):
                        d["w0"][s, co, t // 3, t % 3, ch] = TAP_SIGN[(t + ch) % 9] * 2.0 ** -((4 * t + 3 * ch + s) % 11)
            else:                   # the stem copies the image into channels 0 .. 2, over a b0 background
                _identity(d["w0"][s:s + 1])
                d["b0"][s] = 2.0 ** -3
        if r.op == "D":
            d["b2"][s], d["bsc"][s] = 2.0 ** -4, 2.0 ** -5
            if which == "w2":       # the 3x3 probed; the shortcut adds a constant 2^-2
                d["w2"][s, co, :, :, ci] = _taps(s)
                d["wsc"][s, :, 0, 0, 3] = 1.0
            else:                   # the 1x1 probed with a one-hot x2 over loud odd pixels
                _identity(d["w2"][s:s + 1])
                for o in range(64):
                    d["wsc"][s, o, 0, 0, ci] = TAP_SIGN[o % 9] * 2.0 ** -((o + s) % 10)
    if r.op == "D":
        d["x2"] = torch.zeros(G, N, *sh2)
        if which == "w2":
            d["x2"][..., 3] = 0.25
        else:
            d["x"][:] = 0.125
            for i in range(G):
                ci = PAIR[slot_of(r, i)][1]
                d["x2"][i, :, 1::2, :, ci] = 8.0
                d["x2"][i, :, :, 1::2, ci] = 8.0
                for n in range(N):
                    pr, pc = pos[(i * N + n) % len(pos)]
                    d["x2"][i, n, 2 * pr, 2 * pc, ci] = 1.0
    return d


def _mk_black(r, g):
    d = ordinary(r, g)
    d["x"][0, 0] = 0.0                                   # every band's maximum is 0
    d["x"][0, 1, 5:19] = 0.0                             # rows 5 .. 18: exactly band 8 .. 15 sees only zeros
    d["x"][1] = torch.rand(d["x"][1].shape, generator=g)  # the workload's range
    return d                                             # replica 2: signed images


APART = ((1.0, 1.0), (1e-4, 1.0), (30.0, 1e-3), (1e3, 0.0), (1e6, 0.0), (1e30, 0.0), (1e30, 1e-30), (0.0, 1e30), (1e-30, 1e30))


def _mk_apart(r, g):
    d = ordinary(r, g)
    for i, (sa, sx) in enumerate(ropt(r, "pairs")):
        d["x"][i] *= sa
        d["x2"][i] *= sx
        d["b2"][i] *= sa if sa else 1.0
        d["bsc"][i] *= sx if sx else 1.0
    return d


def _mk_oddpix(r, g):
    d = ordinary(r, g)
    d["x2"][:, :, 1::2] *= 64.0
    d["x2"][:, :, 0::2, 1::2] *= 64.0
    return d


def _rows():
    rows = []

    def add(name, ops_, G, N, nvalid, wsel, why, make, slots=2, **o):
        for op in ops_:
            rows.append(Row(name, op, G, N, nvalid, wsel, slots, why, make, tuple(sorted(o.items()))))

    add("one", "BSD", 1, 1, (1,), (1,), "every row tile of one image (4 bands / 2 tiles), halo rows outside the image on both",
        _mk_ordinary)
    add("groups", "BSD", 3, 5, (5, 2, 0), (1, 0, 1),
        "a reused slot, a partly valid and an empty replica, blockIdx.x up to 19: both ownership groups of conv1's third row tile",
        _mk_ordinary, xstage=1, garbage2=1)
    add("nvalid-none", "BSD", 2, 2, None, (1, 0), "no nvalid: every image is valid", _mk_ordinary)
    add("wsel-none", "BSD", 2, 2, (2, 1), None, "no wsel: G == slots, replica g takes slot g", _mk_ordinary)
    add("scale-act", "BSD", 3, 2, (2, 1, 2), None, "activation maximum 1e-30 (the scale cap), 1e30, exactly 0 per replica",
        _mk_scale_act, slots=3, xstage=1, zero=2)
    for k, ops_ in (("w0", "S"), ("w1", "BS"), ("w2", "BSD"), ("wsc", "D")):
        add(f"scale-{k}", ops_, 3, 2, (2, 1, 2), None, f"{k}'s slots at 1e-30 / 1e30 / 0", _mk_scale_w, slots=3, w=k, xstage=1)
    add("denorm", "BSD", 1, 2, (2,), (0,), "a few 1e-40 denormals in an ordinary input", _mk_denorm)
    add("bands", "BS", 3, 1, (1, 1, 1), (0, 1, 2),
        "one band 2^12 louder in the input; a contrast in the mid activation only (b1); a mid contrast of 2^24 over quiet bands",
        _mk_bands, slots=3, xstage=1)
    add("deadmid", "BS", 2, 1, (1, 1), (0, 1), "h == 0 in one band (its maximum is 0: hexp at the cap), then everywhere",
        _mk_deadmid, dead=1)
    for which, ops_ in (("w0", "S"), ("w1", "BS"), ("w2", "BSD"), ("wsc", "D")):
        add(f"probe-{which}", ops_, 2, 5, (5, 5), (0, 1), f"exact: one-hot input, {which}'s entries distinct powers of two",
            _mk_probe, probe=which, exact=1)
    add("black", "S", 3, 2, (2, 2, 2), (0, 1, 1), "an all-zero image, one with rows 5 .. 18 zero, images in [0, 1], signed images",
        _mk_black)
    for i in range(3):
        pairs = APART[3 * i:3 * i + 3]
        add(f"apart-{i}", "D", 3, 2, (2, 2, 1), None, "a and x2 far apart: " + ", ".join(f"({a:g}, {b:g})" for a, b in pairs),
            _mk_apart, slots=3, pairs=pairs, finite=1)
    add("oddpix", "D", 1, 2, (2,), (1,), "odd rows / columns of x2 64 x louder: the shortcut reads (2h, 2w) only", _mk_oddpix)
    return rows


ROWS = _rows()
XSTAGE_ROWS = [r for r in ROWS if ropt(r, "xstage") and r.op != "D"]


# ====================================================================================== oracle
@contextlib.contextmanager
def ref_dtype(dt):
    old = R.COMPUTE_DTYPE
    R.COMPUTE_DTYPE = dt
    try:
        yield
    finally:
        R.COMPUTE_DTYPE = old


def _rep_args(r, d, g, dt):
    nv, s = nvalid_of(r, g), slot_of(r, g)
    a = lambda k: d[k][g:g + 1, :nv].to(dt)      # noqa: E731
    w = lambda k: d[k][s:s + 1].to(dt)           # noqa: E731
    if r.op == "B":
        return a("x"), w("w1"), w("b1"), w("w2"), w("b2")
    if r.op == "S":
        return a("x"), w("w0"), w("b0"), w("w1"), w("b1"), w("w2"), w("b2")
    return a("x"), w("w2"), w("b2"), a("x2"), w("wsc"), w("bsc")


REF = {"B": R.basic_block_eval, "S": R.stem_block_eval, "D": R.down_block_eval}


def reference(r, g, dt, d=None):
    """ops/reference.py on replica g's valid images in ``dt``."""
    d = d or inputs(r)
    with ref_dtype(dt):
        return REF[r.op](*_rep_args(r, d, g, dt), torch.zeros(1, dtype=torch.int64))[0]


def cv(x, w, stride=1, pad=1):
    return nhwc(F.conv2d(nchw(x), wk(w), None, stride=stride, padding=pad))


def _band_rows(t, h0, lo, hi):
    """Rows h0+lo .. h0+hi clipped to the image of [n, H, W, C]."""
    return t[:, max(h0 + lo, 0):min(h0 + hi + 1, t.shape[1])]


def _bmax(t, h0, lo, hi):
    """Per image max over the band's rows: [n, 1, 1, 1]."""
    return _band_rows(t, h0, lo, hi).reshape(t.shape[0], -1).max(1).values.view(-1, 1, 1, 1)


def _q(m, coarser=0):
    """2^-25 2^-s per image from maxima [n, 1, 1, 1] (fp64)."""
    return torch.tensor([2.0 ** (-25 - (hexp(float(v)) - coarser)) for v in m.view(-1)], dtype=F64).view(-1, 1, 1, 1)


def _stage(aabs, e_prev, w, qa, qw, n, extra, stride=1, pad=1):
    """(element bound, magnitude) of one conv stage; see the module docstring."""
    wa, ow, oa = w.abs(), torch.ones_like(w), torch.ones_like(aabs)
    A0, Sa = cv(aabs, wa, stride, pad), cv(aabs, ow, stride, pad)
    Sw, Kc = cv(oa, wa, stride, pad), cv(oa, ow, stride, pad)
    rep = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) * A0 + (1 + 2.0 ** -9) * (qa * Sw + qw * Sa) + 5 * qa * qw * Kc
    A = A0 + extra
    return cv(e_prev, wa, stride, pad) + rep + (n + 2) * U32 * A + TINY, A


def _qw(w):
    return 2.0 ** (-25 - hexp(amax(w)))


Oracle = namedtuple("Oracle", "want A apriori E")


def sc_scales(a, w2, x2, wsc, bounded=True):
    """(sa, sw2, sx, swsc) of the down block; ``bounded=False``: the rule before the shift bound."""
    sa, sw2, swsc = hexp(amax(a)), hexp(amax(w2)), hexp(amax(wsc))
    sx = hexp(amax(x2))
    if bounded:
        sx = max(-126, min(sx, sa + sw2 + SC_SHIFT_MAX - swsc))
    return sa, sw2, sx, swsc


def _apriori(r, d, g):
    """(A, a-priori bound) of replica g, fp64 [nv, H, W, C]."""
    nv, s = nvalid_of(r, g), slot_of(r, g)
    x = d["x"][g, :nv].double()
    if r.op == "D":
        w2, wsc, x2 = d["w2"][s].double(), d["wsc"][s].double(), d["x2"][g, :nv].double()
        sa, sw2, sx, swsc = sc_scales(d["x"][g, :nv], d["w2"][s], d["x2"][g, :nv], d["wsc"][s])
        bias = d["b2"][s].double().abs() + d["bsc"][s].double().abs()
        z = torch.zeros_like(x)
        e3, A3 = _stage(x.abs(), z, w2, 2.0 ** (-25 - sa), 2.0 ** (-25 - sw2), 0, 0.0)
        esc, Asc = _stage(x2.abs(), torch.zeros_like(x2), wsc, 2.0 ** (-25 - sx), 2.0 ** (-25 - swsc), 0, 0.0, 2, 0)
        A = A3 + Asc + bias
        n = 3 * 608 + 3
        return A, e3 + esc + (n + 2) * U32 * A + TINY * (1 + 2.0 ** -(sx + swsc))
    w1, w2 = d["w1"][s].double(), d["w2"][s].double()
    b1, b2 = d["b1"][s].double(), d["b2"][s].double()
    n1 = 3 * 288 + 1
    if r.op == "B":
        qx = 2.0 ** (-25 - hexp(amax(d["x"][g, :nv])))
        e1, A1 = _stage(x.abs(), torch.zeros_like(x), w1, qx, _qw(d["w1"][s]), n1, b1.abs())
        h = torch.relu(cv(x, w1) + b1)
        Apure = cv(cv(x.abs(), w1.abs()) + b1.abs(), w2.abs()) + b2.abs() + x.abs()
    else:
        w0, b0 = d["w0"][s].double(), d["b0"][s].double()
        sv = torch.relu(cv(x, w0) + b0)
        h = torch.relu(cv(sv, w1) + b1)
        As = cv(x.abs(), w0.abs()) + b0.abs()
        Apure = cv(cv(As, w1.abs()) + b1.abs(), w2.abs()) + b2.abs() + As
    out = torch.zeros(nv, 32, 32, 32, dtype=F64)
    for h0 in BANDS:
        if r.op == "S":
            qi = _q(_bmax(x.abs(), h0, -3, 10))                                   # a given input: exact
            e0, A0 = _stage(x.abs(), torch.zeros_like(x), w0, qi, _qw(d["w0"][s]), 3 * 32 + 1, b0.abs())
            qs = _q(_bmax(sv, h0, -2, 9) + _bmax(e0, h0, -2, 9), 1)
            sk = sv + e0                                                          # |s| as the kernel may hold it
            e1, A1 = _stage(sk, e0, w1, qs, _qw(d["w1"][s]), n1, b1.abs())
            resid, eres = sk, e0
        else:
            resid, eres = x.abs(), 0.0
        qh = _q(_bmax(h, h0, -1, 8) + _bmax(e1, h0, -1, 8), 1)
        e2, _ = _stage(h + e1, e1, w2, qh, _qw(d["w2"][s]), 3 * 288 + 2, b2.abs() + resid)
        out[:, h0:h0 + 8] = (e2 + eres)[:, h0:h0 + 8]
    return Apure, out


# ====================================================================================== emulation
@functools.lru_cache(maxsize=None)
def _geo(R_, W, Cin, Cout, k=3, s=1, p=1):
    return C._case("geo", 1, 1, (R_, W), Cin, Cout, k, s, p, "", "")


def _planes(w):
    """(h, l, s) of one slot's weights at the slot's scale, as xsplit_w_kernel stores them."""
    s = hexp(amax(w))
    h, l = split(w, s)
    return h, l, s


def _conv_em(a, sa, W, order, k=3, stride=1, pad=1):
    """One emulated conv of the zero-padded rows ``a`` [n, R, W, Ci] at operand scale sa against the
    planes W: fp32 accumulation of the scaled planes, the scale removed at the end."""
    wh, wl, sw = W
    c = _geo(a.shape[1], a.shape[2], a.shape[3], wh.shape[0], k, stride, pad)
    ah, al = split(a, sa)
    o = gemm3(im2col(ah, c), im2col(al, c), wh.reshape(wh.shape[0], -1).t(), wl.reshape(wh.shape[0], -1).t(), order)
    return o.view(a.shape[0], c.Ho, c.Wo, -1), sa + sw


def _unscale(acc, s):
    return (acc.double() * 2.0 ** -s).float()        # ldexpf(acc, -s): one rounding at most


def _take(t, r0, n):
    """Rows r0 .. r0+n-1 of the image t [H, W, C] as [1, n, W, C], zeros outside the image."""
    out = torch.zeros(1, n, t.shape[1], t.shape[2], dtype=t.dtype)
    lo, hi = max(r0, 0), min(r0 + n, t.shape[0])
    out[0, lo - r0:hi - r0] = t[lo:hi]
    return out


def _inside(r0, n, H=32):
    return torch.tensor([1.0 if 0 <= r0 + i < H else 0.0 for i in range(n)]).view(1, n, 1, 1)


def emulate(r, d, g, order, bounded=True, mid="band"):
    """Replica g's valid images through the documented arithmetic, fp32.  ``mid="image"``: the mid
    activation split with the image's maximum instead of the band's (what the ``bands`` rows exclude)."""
    nv, s = nvalid_of(r, g), slot_of(r, g)
    x = d["x"][g, :nv]
    if r.op == "D":
        x2 = d["x2"][g, :nv]
        sa, sw2, sx, swsc = sc_scales(x, d["w2"][s], x2, d["wsc"][s], bounded)
        acc, s3 = _conv_em(x, sa, _planes(d["w2"][s]), order)
        acc = (acc.double() * 2.0 ** (sx + swsc - s3)).float()          # the exact rescale (or its overflow)
        sc, ssc = _conv_em(x2[:, ::2, ::2].contiguous(), sx, _planes(d["wsc"][s]), order, 1, 1, 0)
        v = _unscale(acc + sc, ssc)
        return torch.relu(v + (d["b2"][s] + d["bsc"][s]))
    W1, W2 = _planes(d["w1"][s]), _planes(d["w2"][s])
    b1, b2 = d["b1"][s], d["b2"][s]
    sx = hexp(amax(x)) if r.op == "B" else None
    out = torch.zeros(nv, 32, 32, 32)
    for i in range(nv):
        coarse = 0.0
        for h0 in BANDS * (2 if mid == "image" else 1):      # (first pass: the image's largest mid value)
            if r.op == "S":
                img = _take(x[i], h0 - 3, 14)
                acc, s0 = _conv_em(img, hexp(amax(img)), _planes(d["w0"][s]), order)
                x12 = torch.relu(_unscale(acc[:, 1:13], s0) + d["b0"][s]) * _inside(h0 - 2, 12)
                sx12 = hexp(amax(x12))
            else:
                x12, sx12 = _take(x[i], h0 - 2, 12), sx
            acc, s1 = _conv_em(x12, sx12, W1, order)
            hm = torch.relu(_unscale(acc[:, 1:11], s1) + b1) * _inside(h0 - 1, 10)
            coarse = max(coarse, amax(hm))
            acc, s2 = _conv_em(hm, hexp(coarse if mid == "image" else amax(hm)), W2, order)
            out[i, h0:h0 + 8] = torch.relu((_unscale(acc[0, 1:9], s2) + b2) + x12[0, 2:10])
    return out


@functools.lru_cache(maxsize=None)
def oracle(r, garbage=GARBAGE):
    """Per replica (None for an empty one): fp64 result, magnitude, a-priori bound, E_pair (D: a
    number per replica; B / S: per image and band, broadcast over [nv, 32, 1, 1])."""
    d, out = inputs(r, garbage), []
    for g in range(r.G):
        nv = nvalid_of(r, g)
        if nv == 0:
            out.append(None)
            continue
        want = reference(r, g, F64, d)
        A, ap = _apriori(r, d, g)
        err = torch.zeros_like(want)
        for order in range(3):
            err = torch.maximum(err, (emulate(r, d, g, order).double() - want).abs())
        if r.op == "D":
            E = float(err.max())
        else:
            E = err.view(nv, 4, -1).max(2).values.repeat_interleave(8, 1).view(nv, 32, 1, 1)
        out.append(Oracle(want, A, ap, E))
    return out


def sharp(o):
    return SHARP_FACTOR * o.E + 2.0 ** -23 * o.want.abs()


OPNAME = {"B": "basic_block_eval", "S": "stem_block_eval", "D": "down_block_eval"}


def check_rep(got, o, r, form, who):
    """One replica's valid output against both bounds, every element."""
    check_bound(got, o.want, o.apriori, f"{OPNAME[r.op]} [{form}]", "y: a-priori", who)
    check_bound(got, o.want, sharp(o), f"{OPNAME[r.op]} [{form}]", "y: 4 E_pair", who)


def exact_expect(r, g, d=None):
    """(mask [nv, H, 1, 1] or None, expected fp32) of what the row pins bit for bit in replica g.  The
    kernels' ReLU is maximum(v, +0): every zero it returns is +0, so the expectation's are (+ 0.0)."""
    d = d or inputs(r)
    nv, s = nvalid_of(r, g), slot_of(r, g)
    if ropt(r, "exact"):
        return None, reference(r, g, F64, d).float() + 0.0
    if ropt(r, "zero") == g:
        b = d["b2"][s] + d["bsc"][s] if r.op == "D" else d["b2"][s]
        return None, (torch.relu(b) + 0.0).expand(nv, *shapes(r.op)[2]).contiguous()
    if ropt(r, "dead"):
        x = d["x"][g, :nv]
        if r.op == "S":      # the grid makes the fp32 s exact
            x = torch.relu(cv(x.double(), d["w0"][s].double()) + d["b0"][s].double()).float()
        y = torch.relu(d["b2"][s] + x) + 0.0
        if g == 0:
            m = torch.zeros(nv, 32, 1, 1, dtype=torch.bool)
            m[:, 8:16] = True
            return m, y
        return None, y
    return None, None


# ====================================================================================== HIP runner
def _mask(y, nvs):
    y = y.clone()
    for i, n in enumerate(nvs):
        y[i, n:] = 0
    return y


def run(ops, r, dev, sel=None, garbage=GARBAGE, xstage=None):
    """The row on the HIP kernels -> ({"y": masked output (CPU), "amax": folded max bits [G]}, path)."""
    d = inputs(r, garbage)
    sl = slice(None) if sel is None else slice(sel, sel + 1)
    G = r.G if sel is None else 1
    nvs = [nvalid_of(r, g) for g in range(r.G)][sl]
    acts = {k: d[k][sl].to(dev) for k in _acts(r)}
    wsl = sl if r.wsel is None else slice(None)
    par = {}
    for k in WEIGHTS[r.op]:
        w = d[k][wsl].to(dev).clone()
        per = w[0].numel()
        ops.split_weights(w, per, per, ops._amax_w(w, per, per))
        par[k] = w
    for k in BIASES[r.op]:
        par[k] = d[k][wsl].to(dev).contiguous()
    wsel = None if r.wsel is None else torch.tensor(list(r.wsel)[sl], dtype=I32, device=dev)
    nvalid = None if r.nvalid is None else torch.tensor(nvs, dtype=I32, device=dev)
    prev = ops.set_xstage(-1) if xstage is None else ops.set_xstage(xstage)
    try:
        with ops.amax_arena(G, dev):
            if r.op == "B":
                assert ops.basic_block_ok(acts["x"], par["w1"], par["w2"])
                y = ops.basic_block_eval(acts["x"], par["w1"], par["b1"], par["w2"], par["b2"], wsel, nvalid)
            elif r.op == "S":
                assert ops.stem_block_ok(acts["x"], par["w0"], par["w1"], par["w2"])
                y = ops.stem_block_eval(acts["x"], par["w0"], par["b0"], par["w1"], par["b1"], par["w2"], par["b2"], wsel, nvalid)
            else:
                assert ops.down_block_ok(acts["x"], par["w2"], acts["x2"], par["wsc"])
                y = ops.down_block_eval(acts["x"], par["w2"], par["b2"], acts["x2"], par["wsc"], par["bsc"], wsel, nvalid)
            path = launched(ops)
            am = y._dba_amax.clone()
    finally:
        ops.set_xstage(prev)
    return {"y": _mask(y.cpu(), nvs), "amax": am.max(0).values[:G].cpu()}, path


def check_out(r, out, form, who, sel=None, garbage=GARBAGE):
    """Both bounds on every valid element, the row's bit-exact expectations, and the folded output
    maximum against the kernel's own y."""
    o = oracle(r, garbage)
    reps = range(r.G) if sel is None else [sel]
    for i, g in enumerate(reps):
        nv = nvalid_of(r, g)
        y = out["y"][i, :nv]
        want_max = y.abs().max().view(1) if nv else torch.zeros(1)
        check_exact(out["amax"][i:i + 1].view(torch.float32), want_max, OPNAME[r.op], f"folded max |y| [{r.name}]", who)
        if nv == 0:
            continue
        check_rep(y, o[g], r, form, who)
        m, want = exact_expect(r, g, inputs(r, garbage))
        if want is not None:
            if m is None:
                check_exact(y, want, OPNAME[r.op], f"exact [{r.name}] replica {g}", who)
            else:
                mm = m.expand_as(y)
                check_exact(y[mm], want[mm], OPNAME[r.op], f"exact rows [{r.name}] replica {g}", who)


# ====================================================================================== operand helpers
def np_hexp(maxbits):
    return min(100, 141 - (int(maxbits) >> 23))


def np_amax_bits(x, n=None):
    """max |x[:n]| as int32 float bits; fmaxf semantics (a NaN operand is dropped), 0 for n = 0."""
    v = np.abs(np.asarray(x, dtype=np.float32).reshape(-1)[:n])
    m = np.float32(np.fmax.reduce(v, initial=np.float32(0))) if v.size else np.float32(0)
    if np.isnan(m):
        m = np.float32(0)
    return int(np.float32(m).view(np.int32))


def np_split(w):
    """[slots, per] fp32 -> [slots, 2, per] uint16: the fp16 pair of every slot at the slot's scale."""
    w = np.asarray(w, dtype=np.float32)
    out = np.zeros((w.shape[0], 2, w.shape[1]), dtype=np.uint16)
    for s in range(w.shape[0]):
        sc = np_hexp(np_amax_bits(w[s]))
        with np.errstate(over="ignore", invalid="ignore"):
            ws = w[s] * np.float32(2.0 ** sc)
            h = ws.astype(np.float16)
            l = (ws - h.astype(np.float32)).astype(np.float16)
        out[s, 0], out[s, 1] = h.view(np.uint16), l.view(np.uint16)
    return out


def np_frag(planes, ncol, cs):
    """[slots, 2, per] -> [slots, 2 per]: xfrag_w_kernel's order from its definition (16-B unit idx:
    lane = idx & 63, plane = (idx >> 6) & 1, half-step kk = (idx >> 7) & 1, k-step t = (idx >> 8) % NK
    (chunk t / 9, tap t % 9), column tile nt = (idx >> 8) / NK)."""
    planes = np.asarray(planes)
    K, NK = 9 * cs, 9 * cs // 32
    per = ncol * K
    idx = np.arange(per // 4)
    lane, f, tt = idx & 63, (idx >> 6) & 3, idx >> 8
    t, nt = tt % NK, tt // NK
    e = (nt * 32 + (lane & 31)) * K + (t % 9) * cs + (t // 9) * 32 + ((f >> 1) * 2 + (lane >> 5)) * 8
    src = ((f & 1) * per + e)[:, None] + np.arange(8)[None, :]
    return planes.reshape(planes.shape[0], -1)[:, src.reshape(-1)]


SPLIT_PERS = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097)
SPLIT_SWEEP = 1024 * 1024 + 3         # one sweep of the single kernel's capped grid, plus 3
FRAG_SHAPES = ((32, 32), (64, 64), (128, 64), (32, 128))
AMAX_SWEEP = 256 * 4096 + 5           # one element past one sweep of amax_kernel's 256-block grid


def split_values(slots, per, g):
    """Weights with the edges a split meets: fp16-subnormal low planes, -0.0, a slot of zeros (>= 3
    slots), a slot at 1e-30 (the scale cap) and one at 1e30 (>= 5 slots)."""
    w = torch.randn(slots, per, generator=g) * 0.05
    if per >= 4:
        w[:, 1] = -0.0
        w[:, 2] = w[:, 0] * 2.0 ** -13          # its low plane is an fp16 subnormal
        w[:, 3] = w[:, 0] * 2.0 ** -26          # below the low plane's quantum
    w[:, -1] = -w.abs().max(1).values * 1.5     # the maximum in the last element, negative
    if slots >= 3:
        w[2] = 0.0
    if slots >= 5:
        w[3] *= 1e-30 / 0.075
        w[4] *= 1e30 / 0.075
    return w

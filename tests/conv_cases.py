"""Shared case tables, seeded generators, fp64 oracles, the CPU emulation of the fp16-pair split and
the bounds of the conv-family tests (csrc/kernels/xconv*.hip/hpp, xhalo.hpp, xwgrad*.hip, stem.hip):
test_conv_cases.py (CPU) and test_gpu_conv_cases.py (HIP) run the same cases against the same
oracles with the same bounds.  Bookkeeping (``check_bound``, ``ERRORS``, ``report``) is
step_kernel_cases.py's.

Oracles
-------
Plain torch fp64 on the CPU, per replica through the ``wsel`` map: ``F.conv2d``,
``torch.nn.grad.conv2d_input`` / ``conv2d_weight``; bias, residual, ReLU, ``accum``, ``dw_old`` and
``db_old`` applied in fp64.  Each oracle returns its magnitude ``A`` (the same op over absolute
values; forward: ``|bias| + |res| + conv(|x|, |w|)``) and the sums the floor term below needs.
Only the images below ``nvalid`` exist for an oracle: the rest of an activation is undefined by
contract and is filled with large finite garbage in every input, so a kernel that read it (or
folded it into an operand maximum) would be caught.

The fp16-pair split and its a-priori bound (from the xmfma.hpp header)
----------------------------------------------------------------------
An operand with per-replica / per-slot maximum ``M`` is scaled by ``2^s``,
``s = min(100, 141 - (bits(M) >> 23))`` so that ``M 2^s`` lies in ``[2^14, 2^15)`` (below the cap),
and split as ``a 2^s = h + l + e``, ``h = f16(a 2^s)``, ``l = f16(a 2^s - h)``.  Both roundings are to
11 significant bits while the value is a normal fp16 number (``>= 2^-14`` scaled) and to the
subnormal quantum ``2^-24`` below, so with ``q = 2^-25 2^-s`` (half that quantum, unscaled; at most
``2^-39 M`` when the cap is not reached - the header's "under max 2^-40" holds for the upper half of
the binade only, so the derived constant is used here)

    |e| <= 2^-22 |a| + q,        |l| <= 2^-11 (1 + 2^-11) |a| + 2 q.

A product is evaluated as ``hh' + hl' + lh'`` (fp16 x fp16 is exact in fp32), so
``ab - (hh' + hl' + lh') = ll' + e b + e' (a - e)`` and, summed over an output's products with
``A0 = sum |a||b|``, ``Sa = sum |a|``, ``Sb = sum |b|`` and ``Kc`` the number of products,

    repr <= 3 2^-22 (1 + 2^-10) A0 + (1 + 2^-9) (q_a Sb + q_b Sa) + 5 q_a q_b Kc.

The first term is the issue's "3 x 2^-22 |xy|" (two operand representations and the dropped
``l l'``), the second its floor for elements below ``M 2^-17``.  The three plane products of every
reduction element are accumulated in fp32 (the scaling by powers of two is exact), the slabs of a
split reduction are summed in fp32 and the epilogue adds bias / residual / accum / the old gradient:
``(n + 2) 2^-24 A`` with ``n = 3 pad32(R) + slabs + epilogue adds`` (``R`` the reduction length; every
tile's reduction is padded to 32-deep k-steps).  ``apriori = repr + (n + 2) 2^-24 A``: no evaluation
order of the documented arithmetic can exceed it, and no constant in it was measured.

The sharp bound
---------------
``E_pair`` is the largest element error, per replica, of the CPU emulation of exactly that
arithmetic (``emulate_*``: the split above, ``hh' + hl' + lh'`` in fp32, ``2^-(sa+sb)`` removed at the
end) against the oracle, over three summation orders: torch's own, the reduction reversed, and
32-deep k-steps summed one after the other.  A kernel must stay within
``SHARP_FACTOR E_pair + 2^-23 |oracle|``: the 4 is the factor the project already grants over a
same-precision evaluation (test_gpu_f32.py's "4 x torch-fp32").  It was fixed before the first GPU
run.  ``E_pair`` is taken per replica (not over the whole tensor) because the operand-scale cases
put replicas 60 orders of magnitude apart; that is the stricter reading.

Exact-fp32 kernels take ``bound32(n, A)``: the stem.hip forward with ``n`` the FMA chain ``K`` plus
the two epilogue adds; xwgrad_stem.hip with ``n = M + 1`` (the ``M`` row products of an element are
summed within 256-row slabs, the ``Z`` slab sums onto each other and onto the old ``dw``: ``M`` adds
in all however they are grouped, so the slab sums are inside the ``M``).  The bias gradient (fp64
sums, ``db += (float)t``) takes ``bound64(A) + 2 x 2^-24 (|db_old| + |t|)``.

Lazily formed operands (``lzx``: x = relu(fma(y, scale, shift)) of a LazyBN; ``lzg``: dy =
fma(A, d, fma(B, y, K)) of a LazyGrad) are never stored: the oracle's operand is the fp32-rounded
value and ``2 x 2^-24`` of the magnitude behind that rounding, carried through the op, is added to
every bound (``wgrad_slack``).
"""
import contextlib
import functools
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from step_kernel_cases import (F64, I32, U32, bound32, bound64, check_bound, check_exact, gen,  # noqa: F401
                               report, same_bits)

F32 = torch.float32
SHARP_FACTOR = 4.0
GARBAGE = 777.0            # scale of the undefined rows beyond nvalid
SENTINEL = 777.25          # behind every strided dw / db view
SPLIT_DEFAULT = dict(target=128, min_k=8, max_s=8, kslab_max=2, dgrad_ks=1)   # xconv.hpp SplitPolicy
MAX_SLABS = 8              # xconv.hpp kSkMax


class Case(namedtuple("Case", "name G N H W Cin Cout KH KW s p path why opt")):
    __slots__ = ()
    Ho = property(lambda c: (c.H + 2 * c.p - c.KH) // c.s + 1)
    Wo = property(lambda c: (c.W + 2 * c.p - c.KW) // c.s + 1)
    K = property(lambda c: c.KH * c.KW * c.Cin)

    def __repr__(self):
        return self.name


def _case(name, G, N, HW, Cin, Cout, k, s, p, path, why, **opt):
    H, W = HW if isinstance(HW, tuple) else (HW, HW)
    KH, KW = k if isinstance(k, tuple) else (k, k)
    return Case(name, G, N, H, W, Cin, Cout, KH, KW, s, p, path, why, tuple(sorted(opt.items())))


def opt(c, key, default=None):
    return dict(c.opt).get(key, default)


def case_id(c):
    return c.name


def maps(c):
    """(slots, wsel, nvalid): a repeated and a skipped weight slot, a full, a partly valid and
    (G >= 3) an empty replica."""
    G, N = c.G, c.N
    if opt(c, "nowsel"):
        slots, wsel = G, None
    else:
        slots = G + 1
        wsel = [slots - 1 if g % 2 == 0 else g for g in range(G)]     # G = 3: [3, 1, 3]; 0 and 2 skipped
    if opt(c, "scale"):
        nvalid = [N, (N + 1) // 2, N][:G]
    elif G >= 3:
        nvalid = [N, (N + 1) // 2, 0] + [N] * (G - 3)
    elif G == 2:
        nvalid = [N, (N + 1) // 2]
    else:
        nvalid = [max(1, N - 1)]
    return slots, wsel, nvalid


SCALE_PEAKS = (1e-30, 1e30, 0.0)    # the scale cap, a negative exponent, the all-zero operand


def _garbage(t, nvalid, g):
    for r, nv in enumerate(nvalid):
        if nv < t.shape[1]:
            t[r, nv:] = GARBAGE * torch.randn(t[r, nv:].shape, generator=g)
    return t


@functools.lru_cache(maxsize=None)
def inputs(c):
    """Every operand any of the three ops takes, fp32 on the CPU (never modified by a test)."""
    g = gen(7, c.G, c.N, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.s, c.p, len(c.name))
    slots, wsel, nvalid = maps(c)
    G, N = c.G, c.N
    x = torch.randn(G, N, c.H, c.W, c.Cin, generator=g)
    w = torch.randn(slots, c.Cout, c.KH, c.KW, c.Cin, generator=g) / math.sqrt(c.K)
    bias = torch.randn(slots, c.Cout, generator=g)
    res = torch.randn(G, N, c.Ho, c.Wo, c.Cout, generator=g)
    dy = torch.randn(G, N, c.Ho, c.Wo, c.Cout, generator=g)
    acc = torch.randn(G, N, c.H, c.W, c.Cin, generator=g)
    dw_old = torch.randn(G, c.Cout, c.KH, c.KW, c.Cin, generator=g)
    db_old = torch.randn(G, c.Cout, generator=g)
    if opt(c, "scale"):
        # per-replica operand maxima 1e-30 / 1e30 / 0; the peak element is the last element of the
        # last valid image (replica 0: the last of the tensor, in the scalar tail of the max pass)
        for r in range(G):
            m = SCALE_PEAKS[r % 3]
            for t in (x, dy):
                t[r] = t[r].clamp(-4, 4) * (0.1 * m)
                if m:
                    t[r, nvalid[r] - 1].view(-1)[-1] = m
    for t in (x, res, dy, acc):
        _garbage(t, nvalid, g)
    extra = {}
    if opt(c, "lzx"):
        # x is the never-stored relu(fma(y, scale, shift)) of a training BN (LazyBN): the oracle's
        # operand is that value rounded once to fp32, as the staging forms it; ``x_slack`` is the
        # magnitude that rounding is relative to
        sc, sh = torch.rand(G, c.Cin, generator=g) + 0.5, torch.randn(G, c.Cin, generator=g) * 0.3
        v = x.double() * sc.double().view(G, 1, 1, 1, -1) + sh.double().view(G, 1, 1, 1, -1)
        extra.update(x_raw=x, lz_scale=sc, lz_shift=sh,
                     x_slack=x.double().abs() * sc.double().view(G, 1, 1, 1, -1) + sh.double().abs().view(G, 1, 1, 1, -1))
        x = torch.relu(v).float()
    if opt(c, "lzg"):
        # dy = fma(A, d, fma(B, y, K)) of a training BN's input gradient (LazyGrad), two fp32 roundings
        A_, B_, K_ = (torch.rand(G, c.Cout, generator=g) + 0.5, torch.randn(G, c.Cout, generator=g) * 0.1,
                      torch.randn(G, c.Cout, generator=g) * 0.1)
        yb = _garbage(torch.randn(G, N, c.Ho, c.Wo, c.Cout, generator=g) * 2 + 0.5, nvalid, g)
        bc = lambda t: t.double().view(G, 1, 1, 1, -1)   # noqa: E731
        inner = (bc(B_) * yb.double() + bc(K_)).float()
        extra.update(d_raw=dy, lg_y=yb, lg_A=A_, lg_B=B_, lg_K=K_,
                     dy_slack=bc(A_) * dy.double().abs() + 2 * (bc(B_).abs() * yb.double().abs() + bc(K_).abs()))
        dy = (bc(A_) * dy.double() + inner.double()).float()
    return dict(x=x, w=w, bias=bias, res=res, dy=dy, acc=acc, dw_old=dw_old, db_old=db_old,
                wsel=wsel, nvalid=nvalid, slots=slots, **extra)


def slot(inp, g):
    return g if inp["wsel"] is None else inp["wsel"][g]


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def wk(w):
    """[Cout, KH, KW, Cin] -> torch's [Cout, Cin, KH, KW]."""
    return w.permute(0, 3, 1, 2).contiguous()


# ================================================================================ the three ops
# lin_*(a, b, c): the op on one replica's NHWC operands in their dtype (fp64: the oracle).
def lin_fwd(x, w, c):
    return nhwc(F.conv2d(nchw(x), wk(w), None, stride=c.s, padding=c.p))


def lin_dgrad(dy, w, c):
    n = dy.shape[0]
    return nhwc(torch.nn.grad.conv2d_input((n, c.Cin, c.H, c.W), wk(w), nchw(dy), stride=c.s, padding=c.p))


def lin_wgrad(dy, x, c):
    gw = torch.nn.grad.conv2d_weight(nchw(x), (c.Cout, c.Cin, c.KH, c.KW), nchw(dy), stride=c.s, padding=c.p)
    return gw.permute(0, 2, 3, 1).contiguous()


LIN = {"fwd": lin_fwd, "dgrad": lin_dgrad, "wgrad": lin_wgrad}


def operands(op, c, inp, g):
    """The two split operands (a: per-replica scale, b: per-slot / per-replica scale) of replica g,
    valid images only, fp32."""
    nv = inp["nvalid"][g]
    if op == "fwd":
        return inp["x"][g, :nv], inp["w"][slot(inp, g)]
    if op == "dgrad":
        return inp["dy"][g, :nv], inp["w"][slot(inp, g)]
    return inp["dy"][g, :nv], inp["x"][g, :nv]


def red_len(op, c):
    """Reduction length R of one output element (the kernels pad it to 32-deep k-steps)."""
    if op == "fwd":
        return c.K
    if op == "dgrad":
        return c.KH * c.KW * c.Cout
    return c.N * c.Ho * c.Wo


def chain_n(op, c):
    """fp32 operations behind one output: three plane products per padded reduction element, the
    slab sums and the epilogue adds (forward: bias, residual; dgrad: accum; wgrad: the old dw)."""
    R = red_len(op, c)
    slabs = (R // 256 + 2) if op == "wgrad" else MAX_SLABS
    return 3 * ((R + 31) // 32 * 32) + slabs + (2 if op == "fwd" else 1)


# ======================================================================= the fp16-pair emulation
def hexp(m):
    """xmfma.hpp hexp: the scale exponent from max |x| (a Python float holding an fp32 value)."""
    bits_ = int(np.float32(m).view(np.int32))
    return min(100, 141 - (bits_ >> 23))


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def split(t, s):
    """(h, l) planes of the fp32 tensor ``t`` scaled by 2^s, as fp32 tensors."""
    ts = (t.double() * 2.0 ** s).float()          # exact: a power of two, no overflow below 2^15
    h = ts.half().float()
    l = (ts - h).half().float()
    return h, l


def gemm3(Ah, Al, Bh, Bl, order):
    """hh' + hl' + lh' of A [M, R] x B [R, N] in fp32, in one of three summation orders."""
    if order == 0:      # torch's own order over the three plane products
        return torch.cat([Ah, Ah, Al], 1) @ torch.cat([Bh, Bl, Bh], 0)
    if order == 1:      # the reduction (taps, channels, rows) and the plane order reversed
        return torch.cat([Al.flip(1), Ah.flip(1), Ah.flip(1)], 1) @ torch.cat([Bh.flip(0), Bl.flip(0), Bh.flip(0)], 0)
    out = torch.zeros(Ah.shape[0], Bh.shape[1], dtype=F32)
    for r0 in range(0, Ah.shape[1], 32):     # 32-deep k-steps, one after the other
        sl = slice(r0, r0 + 32)
        out = out + Ah[:, sl] @ Bh[sl]
        out = out + Ah[:, sl] @ Bl[sl]
        out = out + Al[:, sl] @ Bh[sl]
    return out


def im2col(x, c):
    """[n, H, W, Cin] -> [n Ho Wo, KH KW Cin], tap-major as the kernels' K order."""
    n = x.shape[0]
    cols = F.unfold(nchw(x), (c.KH, c.KW), padding=c.p, stride=c.s)
    return cols.view(n, c.Cin, c.KH * c.KW, -1).permute(0, 3, 2, 1).reshape(-1, c.K)


def col2im(cols, c, n):
    t = cols.view(n, -1, c.KH * c.KW, c.Cin).permute(0, 3, 2, 1).reshape(n, c.Cin * c.KH * c.KW, -1)
    return nhwc(F.fold(t, (c.H, c.W), (c.KH, c.KW), padding=c.p, stride=c.s))


def emulate(op, c, a, b, order):
    """The op on one replica through the emulated split; fp32 result before the epilogue."""
    sa, sb = hexp(amax(a)), hexp(amax(b))
    (ah, al), (bh, bl) = split(a, sa), split(b, sb)
    n = a.shape[0]
    if op == "fwd":
        o = gemm3(im2col(ah, c), im2col(al, c), bh.reshape(c.Cout, c.K).t(), bl.reshape(c.Cout, c.K).t(), order)
        o = o.view(n, c.Ho, c.Wo, c.Cout)
    elif op == "dgrad":
        o = gemm3(ah.reshape(-1, c.Cout), al.reshape(-1, c.Cout), bh.reshape(c.Cout, c.K), bl.reshape(c.Cout, c.K), order)
        o = col2im(o, c, n)
    else:
        o = gemm3(ah.reshape(-1, c.Cout).t(), al.reshape(-1, c.Cout).t(), im2col(bh, c), im2col(bl, c), order)
        o = o.view(c.Cout, c.KH, c.KW, c.Cin)
    return (o.double() * 2.0 ** -(sa + sb)).float()      # ldexpf(acc, -s): one rounding at most


def epilogue32(op, c, inp, g, v, kind):
    """The kernels' fp32 epilogue of replica g on the emulated sum ``v``."""
    nv = inp["nvalid"][g]
    if op == "fwd":
        if "b" in kind:
            v = v + inp["bias"][slot(inp, g)]
        if "r" in kind:
            v = v + inp["res"][g, :nv]
        return torch.relu(v) if "R" in kind else v
    if op == "dgrad":
        return v + inp["acc"][g, :nv] if "a" in kind else v
    return inp["dw_old"][g] + v


Oracle = namedtuple("Oracle", "want A apriori E")


@functools.lru_cache(maxsize=None)
def oracle(op, c, kind):
    """Per replica (None for an empty one): the fp64 result, its magnitude, the a-priori bound and
    E_pair.  ``kind``: forward 'b' bias, 'r' residual, 'R' ReLU; dgrad 'a' accum."""
    inp, out = inputs(c), []
    lin = LIN[op]
    for g in range(c.G):
        nv = inp["nvalid"][g]
        if nv == 0:
            out.append(None)
            continue
        a, b = operands(op, c, inp, g)
        a64, b64 = a.double(), b.double()
        y, A0 = lin(a64, b64, c), lin(a64.abs(), b64.abs(), c)
        Sa, Sb = lin(a64.abs(), torch.ones_like(b64), c), lin(torch.ones_like(a64), b64.abs(), c)
        Kc = lin(torch.ones_like(a64), torch.ones_like(b64), c)
        A = A0.clone()
        if op == "fwd":
            if "b" in kind:
                y, A = y + inp["bias"][slot(inp, g)].double(), A + inp["bias"][slot(inp, g)].double().abs()
            if "r" in kind:
                y, A = y + inp["res"][g, :nv].double(), A + inp["res"][g, :nv].double().abs()
            if "R" in kind:
                y = torch.relu(y)
        elif op == "dgrad":
            if "a" in kind:
                y, A = y + inp["acc"][g, :nv].double(), A + inp["acc"][g, :nv].double().abs()
        else:
            y, A = inp["dw_old"][g].double() + y, A + inp["dw_old"][g].double().abs()
        qa, qb = 2.0 ** (-25 - hexp(amax(a))), 2.0 ** (-25 - hexp(amax(b)))
        rep = 3 * 2.0 ** -22 * (1 + 2.0 ** -10) * A0 + (1 + 2.0 ** -9) * (qa * Sb + qb * Sa) + 5 * qa * qb * Kc
        ap = rep + (chain_n(op, c) + 2) * U32 * A
        E = 0.0
        for order in range(3):
            e = epilogue32(op, c, inp, g, emulate(op, c, a, b, order), kind)
            E = max(E, float((e.double() - y).abs().max()))
        out.append(Oracle(y, A, ap, E))
    return out


def sharp(o):
    return SHARP_FACTOR * o.E + 2.0 ** -23 * o.want.abs()


def check_pair(got, o, op, path, what, who):
    """One replica's output against both bounds of the fp16-pair family."""
    check_bound(got, o.want, o.apriori, f"{op} [{path}]", f"{what}: a-priori", who)
    check_bound(got, o.want, sharp(o), f"{op} [{path}]", f"{what}: 4 E_pair", who)


def db_oracle(c, g):
    """(want, bound) of the bias gradient of replica g."""
    inp = inputs(c)
    nv = inp["nvalid"][g]
    d = inp["dy"][g, :nv].double().reshape(-1, c.Cout)
    t, A = d.sum(0), d.abs().sum(0)
    old = inp["db_old"][g].double()
    return old + t, bound64(A) + 2 * U32 * (old.abs() + t.abs())


# ======================================================================================= numpy
def np_im2col(x, c):
    """[n, H, W, Cin] fp64 -> [n, Ho, Wo, KH, KW, Cin], written out tap by tap."""
    n = x.shape[0]
    xp = np.zeros((n, c.H + 2 * c.p, c.W + 2 * c.p, c.Cin))
    xp[:, c.p:c.p + c.H, c.p:c.p + c.W] = x
    cols = np.zeros((n, c.Ho, c.Wo, c.KH, c.KW, c.Cin))
    for i in range(c.KH):
        for j in range(c.KW):
            cols[:, :, :, i, j] = xp[:, i:i + c.s * (c.Ho - 1) + 1:c.s, j:j + c.s * (c.Wo - 1) + 1:c.s]
    return cols


def np_lin(op, a, b, c):
    """The three ops by a direct numpy im2col + einsum in fp64 (the oracles' witness)."""
    a, b = a.double().numpy(), b.double().numpy()
    if op == "fwd":
        return torch.from_numpy(np.einsum("nhwijc,oijc->nhwo", np_im2col(a, c), b))
    if op == "wgrad":
        return torch.from_numpy(np.einsum("nhwo,nhwijc->oijc", a, np_im2col(b, c)))
    dcols = np.einsum("nhwo,oijc->nhwijc", a, b)
    n = a.shape[0]
    dxp = np.zeros((n, c.H + 2 * c.p, c.W + 2 * c.p, c.Cin))
    for i in range(c.KH):
        for j in range(c.KW):
            dxp[:, i:i + c.s * (c.Ho - 1) + 1:c.s, j:j + c.s * (c.Wo - 1) + 1:c.s] += dcols[:, :, :, i, j]
    return torch.from_numpy(dxp[:, c.p:c.p + c.H, c.p:c.p + c.W].copy())


# ================================================================================ the case tables
# Forward.  path: the kernel the row must reach (fwd_path re-derives it from the dispatch code).
#   gemm BMxBN/vecV  the implicit GEMM (xconv_kernel) tile and staging vector; BM follows the block
#                    count, so it is named by fwd_path and only BN / vec are pinned in the row
def _fwd_cases():
    c = []
    # --- tile / vector matrix: Cout on both sides of the 32 / 64 / 128 column tiles, scalar (Ncol % 4)
    # and vector epilogues; Cin for vec 1 / 4 / 32 staging and K tails; M off every row tile
    c += [
        _case("t-co1-ci1-m25", 3, 1, 5, 1, 1, 3, 1, 1, "gemm bn32 vec1", "one column, one channel, K 9, M 25"),
        _case("t-co4-ci3-m127", 3, 1, (1, 127), 3, 4, 1, 1, 0, "gemm bn32 vec1", "K 3 < one k-step, M 127, vector epilogue"),
        _case("t-co30-ci4-m129", 3, 3, (1, 45), 4, 30, (1, 3), 1, 0, "gemm bn32 vec4",
              "Ncol 30: scalar epilogue; KH != KW (1x3); M 3 x 43"),
        _case("t-co33-ci20-m25", 3, 1, 5, 20, 33, 5, 1, 2, "splitk2 reduce", "Ncol 33: one column past 32; K 500 (tail 20) splits: scalar reduce"),
        _case("t-co50-ci36-m127", 3, 1, (1, 127), 36, 50, 1, 1, 0, "gemm bn64 vec4", "K 36: a 4-deep tail k-step; Ncol 50 scalar"),
        _case("t-co65-ci96-m129", 3, 3, (1, 43), 96, 65, 1, 1, 0, "gemm bn128 vec32", "Ncol 65: one past 64; vec 32, K 96"),
        _case("t-co129-ci4-m25", 3, 1, 5, 4, 129, 3, 1, 1, "gemm bn128 vec4", "Ncol 129: one column in the second 128-tile; K 36"),
        _case("t-co132-ci36-m25", 3, 1, 5, 36, 132, 3, 1, 1, "gemm bn128 vec4", "Ncol 132: a 4-column second tile, vector epilogue; K 324"),
        _case("t-co160-ci96-m25", 3, 1, 5, 96, 160, (3, 1), 1, 1, "gemm bn128 vec32", "Ncol 160, vec 32, 3x1 taps, K 288"),
    ]
    # --- geometry
    c += [
        _case("g-7x5-s2", 3, 2, (7, 5), 4, 8, 3, 2, 1, "gemm bn32 vec4", "odd non-square input, stride 2"),
        _case("g-5x9-k5x3", 3, 2, (5, 9), 3, 6, (5, 3), 1, 1, "gemm bn32 vec1", "KH != KW (5x3), pad 1 < KH / 2, Ncol 6 scalar"),
        _case("g-1x13-k1x3", 3, 2, (1, 13), 4, 4, (1, 3), 2, 0, "gemm bn32 vec4", "one row; stride 2 with (W - k) % s == 0"),
        _case("g-8x8-p0-s2", 3, 2, 8, 4, 8, 3, 2, 0, "gemm bn32 vec4", "pad 0, (H - k) % s != 0: last row / column unread"),
        _case("g-pad2", 3, 2, 4, 4, 8, 3, 1, 2, "gemm bn32 vec4", "pad 2 for 3x3: the output is larger than the input"),
        _case("g-2x2-k3", 3, 2, 2, 4, 8, 3, 1, 1, "gemm bn32 vec4", "kernel larger than the unpadded input"),
    ]
    # --- xhalo_kernel: both shapes at the Ncol edges, plain and with pre-split planes, all
    # epilogues, N = 1 and odd N
    for ncol in (4, 28, 32):
        c.append(_case(f"h32-n{ncol}", 3, 3, 32, 32, ncol, 3, 1, 1, "xhalo w32", f"W 32 / Cs 32, Ncol {ncol}, odd N"))
    for ncol in (4, 36, 64):
        c.append(_case(f"h16-n{ncol}", 3, 3, 16, 64, ncol, 3, 1, 1, "xhalo w16", f"W 16 / Cs 64, Ncol {ncol}, odd N"))
    c += [
        _case("h32-n28-pre", 3, 1, 32, 32, 28, 3, 1, 1, "xhalo w32 pre", "pre-split planes, N = 1", pre=1),
        _case("h16-n36-pre", 3, 1, 16, 64, 36, 3, 1, 1, "xhalo w16 pre", "pre-split planes, N = 1", pre=1),
        _case("h32-n4-pre", 3, 3, 32, 32, 4, 3, 1, 1, "xhalo w32 pre", "pre-split planes, Ncol 4", pre=1),
        _case("h32-n32-pre", 3, 3, 32, 32, 32, 3, 1, 1, "xhalo w32 pre", "pre-split planes, Ncol 32", pre=1),
        _case("h16-n4-pre", 3, 3, 16, 64, 4, 3, 1, 1, "xhalo w16 pre", "pre-split planes, Ncol 4", pre=1),
        _case("h16-n64-pre", 3, 3, 16, 64, 64, 3, 1, 1, "xhalo w16 pre", "pre-split planes, Ncol 64: set_xstage(2), or the staged kernel takes it",
              pre=1, xstage=2),
        _case("h32-n32-plain", 3, 2, 32, 32, 32, 3, 1, 1, "xhalo w32", "no bias / residual / ReLU", epi=""),
        # near misses that must land on the implicit GEMM
        _case("hx-n30", 3, 1, 32, 32, 30, 3, 1, 1, "gemm bn32 vec32", "Ncol 30 (% 4 != 0) at the W-32 shape"),
        _case("hx-32x16", 3, 1, (32, 16), 64, 8, 3, 1, 1, "splitk2 reduce", "non-square 32 x 16 at Cs 64: the implicit GEMM, split in two"),
        _case("hx-h36", 3, 1, (36, 32), 32, 8, 3, 1, 1, "gemm bn32 vec32", "H 36, W 32 at Cs 32"),
    ]
    # --- whole-image kernels: W 8 / 4, Cs 32 / 96, partial second column tile in both tile widths,
    # nvalid cutting inside a block's image group
    c += [
        _case("i8-cs32-n32", 3, 3, 8, 32, 32, 3, 1, 1, "ximg2", "W 8, one 64-wide tile half used", pre=1),
        _case("i8-cs96-n96", 3, 9, 8, 96, 96, 3, 1, 1, "ximg2", "W 8, Ncol 96: partial second 64-tile, N 9 -> nvalid 5", pre=1),
        _case("i8-cs32-n160", 3, 1, 8, 32, 160, 3, 1, 1, "ximg2", "W 8, Ncol 160: partial second 128-tile, N 1", pre=1),
        _case("i4-cs96-n160", 3, 9, 4, 96, 160, 3, 1, 1, "ximg2", "W 4 (8 images per block), nvalid 5 inside the group", pre=1),
        _case("i4-cs32-n96-ring", 3, 3, 4, 32, 96, 3, 1, 1, "ximg", "set_ximg(2): the LDS weight ring form", pre=1, ximg=2),
        _case("i8-cs96-n160-ring", 3, 3, 8, 96, 160, 3, 1, 1, "ximg", "set_ximg(2), W 8", pre=1, ximg=2),
        _case("i8-cs32-n32-nopre", 3, 3, 8, 32, 32, 3, 1, 1, "ximg", "weights split while staging (no planes)"),
        _case("s16-frag", 3, 3, 16, 64, 64, 3, 1, 1, "xstage16", "16x16x64 -> 64 with fragment planes, set_xstage(3)", pre=1,
              xstage=3),
    ]
    # --- split-K: the three combine forms at uneven K slices
    c += [
        _case("k-inlaunch-800", 1, 7, 1, 800, 132, 1, 1, 0, "splitk3 inlaunch", "nkt 25 in 3 slabs (8 / 8 / 9), Ncol 132, M 6",
              arena=1),
        _case("k-inlaunch-m27", 1, 4, 3, 96, 132, 3, 1, 1, "splitk3 inlaunch", "M 27 rows (nvalid 3), nkt 27 in 3 slabs", arena=1),
        _case("k-decline-130", 1, 7, 1, 800, 130, 1, 1, 0, "splitk3 reduce", "Ncol 130: the combine declines (% 4), slabs + reduce",
              arena=1),
        _case("k-reduce-800", 3, 7, 1, 800, 132, 1, 1, 0, "splitk3 reduce", "no counters, 3 slabs > kslab_max: slabs + xsplitk_reduce"),
        _case("k-kslab-512", 3, 7, 1, 512, 132, 1, 1, 0, "splitk2 kslab", "grouped launch, 2 in-block slabs of 8 k-steps"),
        _case("k-policy-8", 3, 7, 1, 800, 132, 1, 1, 0, "splitk8 reduce", "set_split_policy(min_k=2): 8 slabs of 3 / 4 k-steps",
              policy=(("min_k", 2),)),
    ]
    # --- stem.hip (exact fp32): its three shapes, M off PIX * ITER, nvalid cutting a pixel tile
    c += [
        _case("stem-3x3", 3, 3, (5, 7), 3, 32, 3, 1, 1, "stem", "3x3 3 -> 32, M 105 / 70"),
        _case("stem-7x7", 3, 3, (9, 11), 3, 64, 7, 2, 3, "stem", "7x7 / 2 3 -> 64 on 9 x 11"),
        _case("stem-5x5", 3, 3, (7, 6), 1, 20, 5, 1, 0, "stem", "5x5 1 -> 20, pad 0"),
        _case("stem-eval-mfma", 3, 3, (9, 11), 3, 64, 7, 2, 3, "gemm bn64 vec4", "evaluation stem on the MFMAs: channels padded 3 -> 4",
              pre=1),
    ]
    # --- operand-scale edges
    c += [
        _case("scale-gemm", 3, 3, 5, 3, 6, 3, 1, 1, "gemm bn32 vec1", "max |x| 1e-30 / 1e30 / 0 per replica", scale=1, epi=""),
        _case("scale-halo", 3, 3, 16, 64, 8, 3, 1, 1, "xhalo w16", "the same through the halo kernel", scale=1, epi=""),
    ]
    return c


FWD_CASES = _fwd_cases()


def _dgrad_cases():
    c = [
        # stride 2: parity classes
        _case("d-7x5-k3", 3, 2, (7, 5), 4, 8, 3, 2, 1, "classes 4", "odd H / W: class grids 4x3, 4x2, 3x3, 3x2"),
        _case("d-k1-s2", 3, 2, 8, 8, 4, 1, 2, 0, "classes 4", "k 1: three empty classes still write accum or 0"),
        _case("d-k2-p0", 3, 2, 8, 4, 8, 2, 2, 0, "classes 4", "k 2 pad 0: one tap per class"),
        _case("d-k3-p0-h8", 3, 2, 8, 4, 8, 3, 2, 0, "classes 4", "k 3 pad 0 on H 8: the last row / column get no gradient"),
        _case("d-k5-p2", 3, 2, (7, 6), 4, 6, 5, 2, 2, "classes 4", "k 5 pad 2: classes of 9 / 6 / 6 / 4 taps; Cout 6 scalar staging"),
        _case("d-k7-p3", 3, 2, (9, 11), 3, 8, 7, 2, 3, "classes 4", "k 7 pad 3, Cin 3: scalar epilogue"),
        _case("d-k3x1-s2", 3, 2, (7, 5), 4, 8, (3, 1), 2, 0, "classes 4", "KH != KW under stride 2"),
        # stride 1: halo kernel, implicit GEMM tails, split-K forms
        _case("d-h32-ci4", 3, 3, 32, 4, 32, 3, 1, 1, "xhalo w32", "W 32: Cs = Cout 32, Ncol = Cin 4"),
        _case("d-h32-ci28", 3, 1, 32, 28, 32, 3, 1, 1, "xhalo w32", "Ncol 28, N 1"),
        _case("d-h16-ci36", 3, 3, 16, 36, 64, 3, 1, 1, "xhalo w16", "W 16: Cs 64, Ncol 36"),
        _case("d-co33-ci50", 3, 1, 5, 50, 33, 3, 1, 1, "gemm bn64 vec1", "Cs 33 scalar staging, Ncol 50 scalar epilogue"),
        _case("d-co36-ci129", 3, 1, 5, 129, 36, 3, 1, 1, "gemm bn128 vec4", "Ncol 129, K 324"),
        _case("d-inlaunch", 1, 7, 1, 132, 800, 1, 1, 0, "splitk3 inlaunch", "lone replica, counters: combined in the launch", arena=1),
        _case("d-kslab", 3, 7, 1, 132, 512, 1, 1, 0, "splitk2 kslab", "grouped: 2 in-block slabs"),
        _case("d-reduce", 3, 7, 1, 132, 800, 1, 1, 0, "splitk3 reduce", "3 slabs: workspace + xsplitk_reduce with accum"),
        _case("d-slots-g", 3, 2, 6, 8, 8, 3, 1, 1, "gemm bn32 vec4", "slots == G, no wsel: the transpose skips the empty replica's slot",
              nowsel=1),
    ]
    return c


DGRAD_CASES = _dgrad_cases()


def _wgrad_cases():
    c = [
        # tiles and staging (Z = 1: straight into dw)
        _case("w-co1-k27", 3, 2, 5, 3, 1, 3, 1, 1, "Z1", "Cout 1, K 27, scalar staging; db C 1", db=1),
        _case("w-co33-k36", 3, 2, 5, 4, 33, 3, 1, 1, "Z1", "Cout 33 (bno 64), K 36, Cout % 4 != 0: scalar staging"),
        _case("w-co50-k129", 3, 2, 5, 129, 50, 1, 1, 0, "Z1", "K 129: one column past tiles_k's 128; db C 50", db=1),
        _case("w-co65-k500", 3, 2, 5, 20, 65, 5, 1, 2, "Z1", "Cout 65 (bno 128), K 500 in 4 k-tiles"),
        _case("w-co129-k36", 3, 2, 5, 4, 129, 3, 1, 1, "Z1", "Cout 129: second 128-tile of one row"),
        _case("w-co132-k128", 3, 2, 5, 128, 132, 1, 1, 0, "Z1", "vector staging, K exactly one k-tile"),
        # geometry
        _case("w-7x5-s2", 3, 2, (7, 5), 4, 8, 3, 2, 1, "Z1", "stride 2 on odd non-square sizes"),
        _case("w-8x8-p0-s2", 3, 2, 8, 4, 8, 3, 2, 0, "Z1", "pad 0: uncovered last row / column get exactly 0"),
        _case("w-5x9-k5x3", 3, 2, (5, 9), 3, 6, (5, 3), 1, 1, "Z1", "KH != KW; db C 6", db=1),
        # slabs
        _case("w-z2", 3, 2, 16, 4, 4, 1, 1, 0, "Z2", "M 512 -> 2 slabs of 256: nvalid 1 ends on the slab edge and leaves a whole slab empty",
              db=1),
        _case("w-zpart", 3, 5, (10, 13), 4, 8, 3, 1, 1, "Zpart", "M 650: mchunk rounded to 32, partial last slab; nvalid 3 ends inside a slab"),
        _case("w-z32", 3, 8, 32, 4, 4, 1, 1, 0, "Z32", "32 slabs: the reduce's 16-z-group form; db rows 8192 / 4096", db=1),
        _case("w-per-odd", 3, 3, 16, 3, 5, 1, 1, 0, "Z3", "per 15 (% 4 != 0): the scalar reduce; db C 5, rows 768", db=1),
        # patch-reuse kernel
        _case("w-co3-db", 3, 2, 5, 4, 3, 3, 1, 1, "Z1", "db C 3 (one partial 64-column pass), rows 50 / 25", db=1),
        # lazy operands, against the oracle: x = relu(BN(y)) staged from y (XLZ), dy = A d + B y + K
        _case("w-halo32-lz", 3, 3, 32, 32, 32, 3, 1, 1, "halo", "xwgrad_halo W 32 reading a lazy BN+ReLU x", lzx=1),
        _case("w-halo16-lz", 3, 3, 16, 64, 64, 3, 1, 1, "halo", "xwgrad_halo W 16 reading a lazy BN+ReLU x", lzx=1),
        _case("w-gemm-lz", 3, 5, (10, 13), 4, 8, 3, 1, 1, "Zpart", "implicit-GEMM weight gradient reading a lazy x", lzx=1),
        _case("w-stem32-lg", 3, 3, (8, 32), 3, 32, 3, 1, 1, "stem", "xwgrad_stem W 32 forming a LazyGrad dy while staging", lzg=1),
        _case("w-stem64-lg", 3, 2, (4, 64), 3, 32, 3, 1, 1, "stem", "xwgrad_stem W 64, LazyGrad", lzg=1),
        _case("w-halo32", 3, 3, 32, 32, 32, 3, 1, 1, "halo", "W 32 / C 32, odd N, nvalid 2"),
        _case("w-halo16", 3, 3, 16, 64, 64, 3, 1, 1, "halo", "W 16 / C 64, odd N"),
        _case("w-halo16-n1", 3, 1, 16, 64, 64, 3, 1, 1, "Z1", "N = 1 at W 16: M == one slab, stays on the implicit GEMM"),
        # the stem's own kernel (exact fp32 FMAs, 256-pixel slabs through the batched reduce)
        _case("w-stem32", 3, 3, (8, 32), 3, 32, 3, 1, 1, "stem", "xwgrad_stem W 32: 3 slabs, nvalid 2 leaves one empty"),
        _case("w-stem64", 3, 2, (4, 64), 3, 32, 3, 1, 1, "stem", "xwgrad_stem W 64: one image per slab"),
    ]
    return c


WGRAD_CASES = _wgrad_cases()


# ====================================================================== dispatch, re-derived
def _ceil(a, b):
    return -(-a // b)


def xsplitk(M, Ncol, K, policy=None):
    """xconv.hpp xsplitk."""
    p = dict(SPLIT_DEFAULT, **dict(policy or ()))
    bn = 32 if Ncol <= 32 else 64 if Ncol <= 64 else 128
    tiles = _ceil(M, 64) * _ceil(Ncol, bn)
    if tiles >= p["target"]:
        return 1
    nkt = _ceil(K, 32)
    s = min(min(MAX_SLABS, p["max_s"]), _ceil(p["target"], tiles))
    while s > 1 and nkt // s < p["min_k"]:
        s -= 1
    return s


def xconv_bm(M, Ncol, G, nclass, splitk):
    bn = 32 if Ncol <= 32 else 64 if Ncol <= 64 else 128
    blocks = _ceil(M, 128) * _ceil(Ncol, bn) * G * nclass * splitk
    bm = 64 if (bn > 32 and blocks < 512) else 128
    if bn == 128 and 2 * blocks < 512:
        bm = 32
    return bm


def gemm_path(M, Ncol, Cs, G, K, c, vec_ok, stride1=True):
    """The implicit GEMM's launch form for an [M, Ncol] output reduced over K (Cs channels a tap)."""
    vec = 32 if (vec_ok and Cs % 32 == 0) else 4 if vec_ok else 1
    bn = 32 if Ncol <= 32 else 64 if Ncol <= 64 else 128
    s = xsplitk(M, Ncol, K, opt(c, "policy")) if stride1 else 1
    if s == 1:
        return f"gemm bn{bn} vec{vec}"
    p = dict(SPLIT_DEFAULT, **dict(opt(c, "policy") or ()))
    sk = (opt(c, "arena") and s <= MAX_SLABS and Ncol > 64 and xconv_bm(M, Ncol, G, 1, s) == 32 and Ncol % 4 == 0)
    if sk:
        return f"splitk{s} inlaunch"
    if s <= p["kslab_max"] and Ncol > 64 and Cs % 32 == 0 and vec >= 4:
        return f"splitk{s} kslab"
    return f"splitk{s} reduce"


def halo_path(c, Cs, Ncol, pre):
    """xhalo_try for a 3x3 stride-1 pad-1 op on a square image."""
    if (c.KH, c.KW, c.s, c.p) != (3, 3, 1, 1) or c.H != c.W or Ncol % 4:
        return None
    if c.W == 32 and Cs == 32 and Ncol <= 32 and c.H % 4 == 0:
        return "xhalo w32" + (" pre" if pre else "")
    if c.W == 16 and Cs == 64 and Ncol <= 64 and c.H % 8 == 0:
        return "xhalo w16" + (" pre" if pre else "")
    return None


def fwd_path(c):
    """ops.hip._xconv_fwd + dba_xstem_fwd + dba_xconv_fwd's dispatch, from the documented conditions."""
    pre = bool(opt(c, "pre"))
    Cin = c.Cin
    eval_mfma = pre and c.K > 64
    if Cin <= 4 and not eval_mfma and (c.KH, c.KW, Cin, c.Cout) in ((3, 3, 3, 32), (7, 7, 3, 64), (5, 5, 1, 20)):
        return "stem"
    if eval_mfma and Cin % 4:
        Cin = Cin + 4 - Cin % 4
    M, K = c.N * c.Ho * c.Wo, c.KH * c.KW * Cin
    if (c.KH, c.KW, c.s, c.p) == (3, 3, 1, 1) and c.H == c.W:
        ximg = opt(c, "ximg", 1)
        if ximg and Cin % 32 == 0 and c.Cout % 32 == 0 and c.W in (8, 4):
            return "ximg2" if (ximg == 1 and pre) else "ximg"
        # (xstage16_try: the staged form is on by default - mode 1 - and forced by 3; 2 is the ring)
        if opt(c, "xstage", 1) in (1, 3) and pre and (c.W, Cin, c.Cout) == (16, 64, 64):
            return "xstage16"
        h = halo_path(c, Cin, c.Cout, pre)
        if h:
            return h
    return gemm_path(M, c.Cout, Cin, c.G, K, c, Cin % 4 == 0, True)


def dgrad_path(c):
    if c.s > 1:
        return f"classes {c.s * c.s}"
    h = halo_path(c, c.Cout, c.Cin, False)
    if h:
        return h
    return gemm_path(c.N * c.H * c.W, c.Cin, c.Cout, c.G, c.KH * c.KW * c.Cout, c, c.Cout % 4 == 0)


def wgrad_path(c, lib=None):
    """(path, Z, mchunk): from the library's own dba_xwgrad_ws_floats where it is loaded."""
    import ctypes
    M = c.N * c.Ho * c.Wo
    if ((c.s, c.p, c.KH, c.KW, c.Cin, c.Cout) == (1, 1, 3, 3, 3, 32) and not opt(c, "db") and c.W in (32, 64)
            and c.H % (256 // c.W) == 0):      # ops.hip._stem_wgrad_ok + dba_xwgrad_stem_ws_floats
        return "stem", M // 256, 256
    if lib is not None:
        mc = ctypes.c_int(0)
        n = int(lib.dba_xwgrad_ws_floats(c.G, c.N, c.Ho, c.Wo, c.Cin, c.Cout, c.KH, c.KW, ctypes.byref(mc)))
        mchunk = mc.value
        Z = _ceil(M, mchunk) if n > 0 else 1
    else:
        hrows = 16 * c.Wo if ((c.KH, c.KW) == (3, 3) and c.Ho == c.Wo and c.Cin == c.Cout
                        and (c.Wo, c.Cin) in ((32, 32), (16, 64))) else 0
        if hrows and M > hrows:
            mchunk, Z = hrows, _ceil(M, hrows)
        else:
            bno = 32 if c.Cout <= 32 else 64 if c.Cout <= 64 else 128
            tiles = _ceil(c.Cout, bno) * _ceil(c.K, 128)
            Z = max(1, min(_ceil(256, tiles), M // 256))
            mchunk = _ceil(_ceil(M, Z), 32) * 32
            Z = _ceil(M, mchunk)
    halo = (Z > 1 and (c.s, c.p, c.KH, c.KW) == (1, 1, 3, 3) and c.Cin == c.Cout and c.H == c.W and c.H % 16 == 0
            and (c.W, c.Cin) in ((32, 32), (16, 64)) and mchunk == 16 * c.W)
    if halo:
        return "halo", Z, mchunk
    if Z == 1:
        return "Z1", Z, mchunk
    if M % mchunk:
        return "Zpart", Z, mchunk
    return f"Z{Z}", Z, mchunk


def launched_path(ops):
    """The path name of the library's last conv-family launch (ops.hip.last_conv_launch): what the
    case actually ran on, against the row's ``path``."""
    l = ops.last_conv_launch()
    k = l["kind"]
    if k == 1:
        if l["nclass"] > 1:
            return f"classes {l['nclass']}"
        if l["form"] == 0:
            return f"gemm bn{l['tile']} vec{l['vec']}"
        return f"splitk{l['slabs']} " + {1: "inlaunch", 2: "kslab", 3: "reduce"}[l["form"]]
    if k == 2:
        return f"xhalo w{l['tile']}" + (" pre" if l["pre"] else "")
    if k == 7:
        return "Z1" if l["slabs"] == 1 else "Zpart" if l["form"] else f"Z{l['slabs']}"
    return {3: "ximg", 4: "ximg2", 5: "xstage16", 6: "stem", 8: "halo", 9: "stem"}.get(k, f"kind {k}")


# ============================================================================== the HIP runners
@contextlib.contextmanager
def settings(ops, c, dev):
    """The launch settings a row asks for, restored afterwards."""
    with contextlib.ExitStack() as st:
        if opt(c, "policy"):
            ops.set_split_policy(**dict(opt(c, "policy")))
            st.callback(lambda: ops.set_split_policy(**SPLIT_DEFAULT))
        if opt(c, "ximg") is not None:
            prev = ops.set_ximg(opt(c, "ximg"))
            st.callback(lambda: ops.set_ximg(prev))
        if opt(c, "xstage") is not None:
            prev_s = ops.set_xstage(opt(c, "xstage"))
            st.callback(lambda: ops.set_xstage(prev_s))
        if opt(c, "arena"):
            st.enter_context(ops.amax_arena(1, dev, n=16, counters=4096))
        yield


def _dev(inp, dev, sel, *names):
    out = []
    for k in names:
        t = inp[k]
        out.append(None if t is None else (t if sel is None else t[sel:sel + 1]).to(dev))
    return out


def _maps_dev(inp, dev, sel):
    wsel, nv = inp["wsel"], inp["nvalid"]
    if sel is not None:
        wsel, nv = (None if wsel is None else wsel[sel:sel + 1]), nv[sel:sel + 1]
    return (None if wsel is None else torch.tensor(wsel, dtype=I32, device=dev)), torch.tensor(nv, dtype=I32, device=dev), nv


def _weights(ops, inp, dev, c, sel):
    w = inp["w"].to(dev).clone()
    if inp["wsel"] is None and sel is not None:
        w = w[sel:sel + 1].clone()
    if opt(c, "pre"):
        per = w[0].numel()
        ops.split_weights(w, per, per, ops._amax_w(w, per, per))
    return w


def _mask(t, nv):
    """The undefined images of an activation zeroed, for bitwise comparisons."""
    t = t.clone()
    for g, n in enumerate(nv):
        t[g, n:] = 0
    return t


def fwd_kind(c):
    return opt(c, "epi", "brR")


def run_fwd(ops, c, dev, sel=None, kind=None, inp=None):
    inp = inp or inputs(c)
    kind = fwd_kind(c) if kind is None else kind
    x, bias, res = _dev(inp, dev, sel, "x", "bias", "res")
    if inp["wsel"] is not None:
        bias = inp["bias"].to(dev)
    wsel, nvalid, nv = _maps_dev(inp, dev, sel)
    w = _weights(ops, inp, dev, c, sel)
    with settings(ops, c, dev):
        y = ops.conv2d(x, w, wsel, c.s, c.p, bias=bias if "b" in kind else None, residual=res if "r" in kind else None,
                       relu="R" in kind, nvalid=nvalid)
    return {"y": _mask(y, nv)}


def run_dgrad(ops, c, dev, sel=None, accum=True, prepared=False):
    inp = inputs(c)
    dy, acc = _dev(inp, dev, sel, "dy", "acc")
    wsel, nvalid, nv = _maps_dev(inp, dev, sel)
    w = _weights(ops, inp, dev, c, sel)
    with settings(ops, c, dev):
        wt = None
        if prepared:
            wt = ops.prepare_dgrad_weights(w, [(w, wsel, c.s, c.p, (c.H, c.W), nvalid, dy.shape[0])])[0]
        dx = ops.conv2d_dgrad(dy, w, wsel, c.s, c.p, (c.H, c.W), nvalid=nvalid, accum=acc if accum else None, wt=wt)
    return {"dx": _mask(dx, nv)}


def wgrad_buffers(c, inp, dev, sel=None):
    """Strided dw / db views into sentinel-filled flat rows, holding the old gradients."""
    G = c.G if sel is None else 1
    per = c.Cout * c.K
    flat = torch.full((G, per + 64), SENTINEL, device=dev)
    fb = torch.full((G, c.Cout + 8), SENTINEL, device=dev)
    dw = flat[:, :per].view(G, c.Cout, c.KH, c.KW, c.Cin)
    db = fb[:, :c.Cout]
    old_w, old_b = _dev(inp, dev, sel, "dw_old", "db_old")
    dw.copy_(old_w)
    db.copy_(old_b)
    return flat, fb, dw, db


def run_wgrad(ops, c, dev, sel=None, defer=False, queue=None):
    """``queue``: a shared defer list flushed by the caller (the outputs are then read after it)."""
    inp = inputs(c)
    dy, x = _dev(inp, dev, sel, "dy", "x")
    _, nvalid, nv = _maps_dev(inp, dev, sel)
    flat, fb, dw, db = wgrad_buffers(c, inp, dev, sel)
    if opt(c, "lzx"):
        x = _lazy_bn(ops, c, inp, dev, sel, x, nv)
    if opt(c, "lzg"):
        from dba_mod_amd.ops import bnstate as bs
        d, yb, A_, B_, K_ = _dev(inp, dev, sel, "d_raw", "lg_y", "lg_A", "lg_B", "lg_K")
        coef = torch.zeros(d.shape[0], bs.ROWS, c.Cout, device=dev)
        coef[:, bs.A], coef[:, bs.B], coef[:, bs.K] = A_, B_, K_
        dy = bs.LazyGrad(d, yb, bs.BnStat(coef, None, None))
    q = queue if queue is not None else ([] if defer else None)
    with settings(ops, c, dev):
        ops.conv2d_wgrad(dy, x, c.s, c.p, c.KH, c.KW, dw, db if opt(c, "db") else None, nvalid=nvalid, defer=q)
        if queue is None and defer:
            ops.wgrad_flush(q)
    return {"dw": dw, "db": db, "flat": flat, "fb": fb}


def _lazy_bn(ops, c, inp, dev, sel, xeff, nv):
    """The case's x as a LazyBN of its stored BN input: fixed coefficients, the bound slot holding
    max |relu(BN(y))| of the valid images."""
    from dba_mod_amd.ops import bnstate as bs
    y, sc, sh = _dev(inp, dev, sel, "x_raw", "lz_scale", "lz_shift")
    G = y.shape[0]
    z = torch.zeros(G, c.Cin, device=dev)
    p0 = bs.BnParams(z + 1, z.clone(), z.clone(), z + 1, z.clone(), z.clone(), 0.1, 1e-5)
    st = ops._bnf_fwd(p0, True, G, c.N * c.H * c.W, c.Cin, dev)[1]
    coef = torch.zeros(G, bs.ROWS, c.Cin, device=dev)
    coef[:, bs.SCALE], coef[:, bs.SHIFT] = sc, sh
    st.coef.copy_(coef)
    am = torch.stack([xeff[g, :n].abs().max() if n else xeff.new_zeros(()) for g, n in enumerate(nv)])
    st.bound[0, :G] = am.float().view(torch.int32)
    return bs.LazyBN(y, st, True)


def wgrad_slack(c, g):
    """What the fp32 rounding of a lazily formed operand may move dw by (0 for stored operands):
    one rounding of fma(y, scale, shift), two of fma(A, d, fma(B, y, K)), through the op's magnitude."""
    inp = inputs(c)
    nv = inp["nvalid"][g]
    if opt(c, "lzx"):
        return 2 * U32 * lin_wgrad(inp["dy"][g, :nv].double().abs(), inp["x_slack"][g, :nv], c)
    if opt(c, "lzg"):
        return 2 * U32 * lin_wgrad(inp["dy_slack"][g, :nv], inp["x"][g, :nv].double().abs(), c)
    return 0.0


def check_wgrad_out(c, out, who, path, sel=None):
    """dw / db of a weight-gradient run against the oracle, with the exact properties."""
    inp = inputs(c)
    per = c.Cout * c.K
    o = oracle("wgrad", c, "")
    reps = range(c.G) if sel is None else [sel]
    for i, g in enumerate(reps):
        if inp["nvalid"][g] == 0:     # an empty replica's gradients are untouched
            check_exact(out["dw"][i].cpu(), inp["dw_old"][g], "conv2d_wgrad", f"dw of the empty replica [{c.name}]", who)
            check_exact(out["db"][i].cpu(), inp["db_old"][g], "conv2d_wgrad", f"db of the empty replica [{c.name}]", who)
            continue
        slack, lz = wgrad_slack(c, g), (" lazy" if (opt(c, "lzx") or opt(c, "lzg")) else "")
        if path.startswith("stem"):
            # exact fp32: M products summed in any order - within a slab, across the Z slabs, then onto
            # the old dw - are M adds in all, however they are grouped
            check_bound(out["dw"][i], o[g].want, bound32(c.N * c.Ho * c.Wo + 1, o[g].A) + slack,
                        f"conv2d_wgrad [stem{lz}]", "dw", who)
        else:
            check_bound(out["dw"][i], o[g].want, o[g].apriori + slack, f"conv2d_wgrad [{path}{lz}]", "dw: a-priori", who)
            check_bound(out["dw"][i], o[g].want, sharp(o[g]) + slack, f"conv2d_wgrad [{path}{lz}]", "dw: 4 E_pair", who)
        if opt(c, "db"):
            want, bound = db_oracle(c, g)
            check_bound(out["db"][i], want, bound, "conv2d_wgrad [xcolsum]", "db", who)
        else:
            check_exact(out["db"][i].cpu(), inp["db_old"][g], "conv2d_wgrad", f"db not asked for [{c.name}]", who)
    assert bool((out["flat"][:, per:] == SENTINEL).all()), f"{c.name}: dw wrote past its view"
    assert bool((out["fb"][:, c.Cout:] == SENTINEL).all()), f"{c.name}: db wrote past its view"


def check_act_out(op, c, got, kind, who, path, sel=None):
    """The valid images of a forward / data-gradient output against both bounds."""
    inp = inputs(c)
    o = oracle(op, c, kind)
    reps = range(c.G) if sel is None else [sel]
    name = "conv2d" if op == "fwd" else "conv2d_dgrad"
    for i, g in enumerate(reps):
        nv = inp["nvalid"][g]
        if nv == 0:
            continue
        if path == "stem":      # exact fp32 FMAs: the chain K and the two epilogue adds
            check_bound(got[i, :nv], o[g].want, bound32(c.K + 2, o[g].A), f"{name} [stem]", "y", who)
        else:
            check_pair(got[i, :nv], o[g], name, path, "y" if op == "fwd" else "dx", who)


def solo_replica(c):
    """The replica also run alone in a launch: the partly valid one."""
    return 1 if c.G >= 2 else 0

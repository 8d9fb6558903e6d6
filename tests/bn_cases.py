"""Shared case tables, seeded generators, fp64 oracles, bounds and the CPU emulation of the fused
training BatchNorm tests (csrc/kernels/bnfuse.hpp, xbn.hip and the record code of the conv
epilogues in xconv.hpp, xhalo.hpp, stem.hip): test_bn_cases.py (CPU) and test_gpu_bnfuse_cases.py
(HIP) run the same cases against the same oracles with the same bounds.  Bookkeeping
(``check_bound``, ``check_exact``, ``same_bits``, ``ERRORS``, ``report``) is step_kernel_cases.py's;
conv inputs, ``launched_path`` and ``check_act_out`` are conv_cases.py's.

Oracles
-------
Plain torch fp64 on the CPU, per (replica, channel), over the valid rows only.

* ``stats_oracle``: two-pass mean and biased variance, ``inv = 1 / sqrt(var + fl32(eps))``, ``scale =
  gamma inv``, ``shift = beta - mean scale``, the running statistics with the unbiased variance
  (``n > 1``) and ``fl32(momentum)``, max / min of y.  It is fed the kernel's OWN y, read back: the
  conv's fp16-pair error is judged by ``conv_cases.check_act_out`` on the same run and never enters a
  statistics bound.
* ``finish_oracle``: ``sum d``, ``sum d xhat``, ``A = gamma inv``, ``B = -A inv sum(d xhat) / n``, ``K = -A
  sum(d) / n - B mean`` from the kernel's own d, read back, and the fp32 coefficient rows the test
  installed (MEAN, INV, SCALE, SHIFT, YMAX, YMIN).  ``xhat = (y - mean) inv`` is exact here; the
  kernels round it to fp32 twice (the difference, the product): ``2 x 2^-24 |d xhat|`` per term.
* ``apply_oracle`` / ``dy_oracle``: ``relu?(y sc + sh + r)`` and ``A d + B y + K`` from the fp32 rows.
* the lazy mask's sign ``fma(y, sc, sh) > 0`` is exact in fp64: ``y sc`` is exact there and a sum of two
  doubles is zero only when it is exactly zero; the generated data keeps |fma| far above the fp32
  underflow threshold, so the fp32 fma has the same sign.

Bounds (a priori, fixed before the first GPU run; u = 2^-53, n the valid rows, E2 = mean(y^2), all
from the oracle)
---------------
The records are fp64 sums of fp32 values (products of two fp32 values are exact in fp64), 32 rows
in order, then at most ``ceil(groups / 256) + 8`` further fp64 adds: fewer than n + 1 roundings each.

* mean              ``2^-24 |m| + (n + 1) u mean|y|``: the fp32 rounding of the result and the sum;
* variance          as finalised (``S2 / n - m^2`` in fp64): ``dvar = 2 (n + 4) u E2`` - both terms are
                    of size E2 and carry n + 1 and 3 roundings;
* inv               ``inv (2^-24 + dvar / (2 (var + eps)) + 8 u)``: its own rounding, the derivative of
                    ``x^-1/2`` at ``var + eps`` times dvar, the fp64 sqrt and division;
* scale             ``bound32(1, |gamma| inv) + |gamma| b_inv``: one fp32 product of the rounded inv;
* shift             ``bound32(2, |beta| + |m scale|) + |scale| b_mean + (|m| + b_mean) b_scale``;
* running mean/var  one fp32 rounding of an fp64 expression: ``bound32(1, (1 - mom) |r| + mom |s|)``
                    plus ``mom`` times the error of the statistic (``b_mean``; ``dvar n / (n - 1)``);
* sum d, sum d xhat ``b_sd = 2^-24 |sd| + (n + 1) u sum|d|``, ``b_sdx = 2^-24 |sdx| + (2 x 2^-24 (1 +
                    2^-24) + (n + 1) u) sum|d xhat|``: the fp32 rounding the finalize applies to each
                    sum, the fp64 summation, the two roundings of xhat;
* dgamma / dbeta    ``prior + fl32(sum)``: ``bound32(1, |prior| + |sum|) + b_sum``;
* A                 ``bound32(1, |A|)`` (one product of installed fp32 values);
* B                 ``-A inv sdx / n``: 4 fp32 operations, ``bound32(4, |B|) + |A inv / n| b_sdx``;
* K                 ``-A sd / n - B mean``: 6 operations behind the longer term, ``bound32(6, |A sd / n| + |B
                    mean|) + |A / n| b_sd + |mean| |A inv / n| b_sdx``;
* stored outputs    ``bn_apply``: ``bound32(3, |y sc| + |sh| + |r|)`` (the fma, the residual's fma, the
                    add); the stored dy: ``bound32(2, |A d| + |B y| + |K|)`` (two fmas).

The mean-1e3 / std-1e-2 and constant-1e6 kinds make ``dvar / var`` large on purpose: they show a
clamped, non-negative variance and a finite inv, not a sharp one.  Every other kind keeps the inv
bound under 1e-6 relative (``test_bn_cases.py`` asserts it).

Exact properties (bit for bit): YMAX / YMIN against the read-back y; the forward bound slot against
max |out| of the stored ``bn_apply`` output of the same y (fp32 fma is monotone in y, so the ends of
[ymin, ymax] carry the maximum); d = g, +0, or on the pooled path ``fl32(pool fl32(1 / HW))``; the same
statistics bits from every producer of the records, run to run, and alone or in a group; an
empty replica's rows; sentinels around every strided parameter / gradient view.  The backward bound
slot is an upper bound: ``>=`` max |dy| of the stored fp32 dy of the same d, ``<=`` the oracle's ``(|A|
dmax + max |B y + K|) (1 + 2^-9)`` (the kernel's factor is 1 + 2^-10; 2^-10 of the total covers the
fp32 roundings of A, B, K behind it for the generated kinds, as the CPU emulation shows row by row).
It is also compared with its documented formula, ``(|A| dmax + max |B y + K|) (1 + 2^-10)`` evaluated
in fp64 from the kernel's own fp32 rows, at ``bound32(3, .)`` (``dbound_formula``): with the product
and the sum fused by the compiler the bare sum already bounds the fused dy, so the inequality
cannot see the factor.
"""
import contextlib
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np
import torch

import conv_cases as CC
from conv_cases import GARBAGE, SENTINEL, check_act_out, launched_path  # noqa: F401
from step_kernel_cases import (ERRORS, F64, I32, U32, bound32, bound64, check_bound, check_exact, f32, gen,  # noqa: F401
                               report, same_bits)
from dba_mod_amd.ops import bnstate as bs

F32 = torch.float32
U64 = 2.0 ** -53
MOMENTUM, EPS = 0.1, 1e-5
NAN = float("nan")
HIP = "hip"


# ============================================================================ parameter rows
class Prm:
    """One BN layer's views into flat parameter rows [G, 4 C + 9] and gradient rows [G, 2 C + 5] as
    the trainer passes them: every element outside the six views holds SENTINEL; dgamma / dbeta hold
    non-zero prior values (the contract is ``+=``).  ``special``: channel 1 gets gamma 0, channel 2 a
    negative gamma, channel 3 beta -1e3 (an all-negative BN output) where C allows."""

    def __init__(self, G, C, key, dev, dt=F32, sel=None, special=True):
        g = gen(21, C, *key)
        flat, grads = torch.full((G, 4 * C + 9), SENTINEL, dtype=F64), torch.full((G, 2 * C + 5), SENTINEL, dtype=F64)
        v = self._views(flat, grads, C)
        v["gamma"].copy_(torch.rand(G, C, generator=g) + 0.5)
        v["beta"].copy_(torch.randn(G, C, generator=g) * 0.1)
        v["rmean"].copy_(torch.randn(G, C, generator=g) * 0.1)
        v["rvar"].copy_(torch.rand(G, C, generator=g) + 0.5)
        v["dgamma"].copy_(torch.randn(G, C, generator=g))
        v["dbeta"].copy_(torch.randn(G, C, generator=g))
        if special:
            if C > 4:
                v["gamma"][:, 1] = 0.0
                v["beta"][:, 3] = -1e3
            v["gamma"][:, 2] = -v["gamma"][:, 2]
        flat, grads = flat.float(), grads.float()          # the fp32 values both sides start from
        if sel is not None:
            flat, grads = flat[sel:sel + 1].clone(), grads[sel:sel + 1].clone()
        self.C, self.dt = C, dt
        self.flat0, self.grads0 = flat, grads
        self.flat, self.grads = flat.to(dt).to(dev), grads.to(dt).to(dev)
        self.v0 = self._views(self.flat0, self.grads0, C)
        self.v = self._views(self.flat, self.grads, C)

    @staticmethod
    def _views(flat, grads, C):
        return {"gamma": flat[:, 1:1 + C], "beta": flat[:, 1 + C:1 + 2 * C], "rmean": flat[:, 2 + 2 * C:2 + 3 * C],
                "rvar": flat[:, 2 + 3 * C:2 + 4 * C], "dgamma": grads[:, 1:1 + C], "dbeta": grads[:, 2 + C:2 + 2 * C]}

    def bn(self):
        v = self.v
        mom, eps = (MOMENTUM, EPS) if self.dt == F32 else (f32(MOMENTUM), f32(EPS))   # fp64 reference: the fp32 scalars
        return bs.BnParams(v["gamma"], v["beta"], v["rmean"], v["rvar"], v["dgamma"], v["dbeta"], mom, eps)

    def got(self):
        """The six views after a run, on the CPU."""
        return self._views(self.flat.cpu(), self.grads.cpu(), self.C)

    def check_rest(self, what, who, fwd):
        """Every element outside the views the pass may write keeps its bits (``fwd``: the running
        statistics; backward: dgamma / dbeta)."""
        C = self.C
        kf, kg = torch.ones_like(self.flat0, dtype=torch.bool), torch.ones_like(self.grads0, dtype=torch.bool)
        if fwd:
            kf[:, 2 + 2 * C:2 + 4 * C] = False
        else:
            kg[:, 1:1 + C] = False
            kg[:, 2 + C:2 + 2 * C] = False
        check_exact(self.flat.cpu().to(F32)[kf], self.flat0[kf], what, "parameter rows outside the running stats", who,
                    bitwise=self.dt == F32)
        check_exact(self.grads.cpu().to(F32)[kg], self.grads0[kg], what, "gradient rows outside dgamma / dbeta", who,
                    bitwise=self.dt == F32)


def slot_value(slot, g=None):
    """The max folded into an operand-max slot ([16, ld] int32 sub-slots of non-negative float bits)."""
    v = slot.detach().cpu().max(0).values.contiguous().view(F32)
    return v if g is None else float(v[g])


def valid_rows(t, n):
    """[n, C] valid rows of one replica's [N, H, W, C] tensor (n = images x pixels)."""
    return t.reshape(-1, t.shape[-1])[:n]


# ===================================================================== forward: oracle + bounds
def stats_oracle(y, gamma, beta, rm, rv):
    """y [n, C] (the fp32 values the statistics were taken of); fp32 parameter rows [C].  Returns the
    fp64 results and their bounds."""
    yd = y.double()
    n = yd.shape[0]
    m = yd.sum(0) / n
    var = ((yd - m) ** 2).sum(0) / n
    eps, mom = f32(EPS), f32(MOMENTUM)
    inv = 1.0 / torch.sqrt(var + eps)
    ga, be, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
    scale = ga * inv
    shift = be - m * scale
    k = n / (n - 1) if n > 1 else 1.0
    unb = var * k
    E2, A1 = (yd * yd).mean(0), yd.abs().mean(0)
    b_mean = U32 * m.abs() + (n + 1) * U64 * A1
    dvar = 2 * (n + 4) * U64 * E2
    b_inv = inv * (U32 + dvar / (2 * (var + eps)) + 8 * U64)
    b_scale = bound32(1, ga.abs() * inv) + ga.abs() * b_inv
    b_shift = bound32(2, be.abs() + m.abs() * scale.abs()) + scale.abs() * b_mean + (m.abs() + b_mean) * b_scale
    o = {"mean": m, "var": var, "inv": inv, "scale": scale, "shift": shift, "dvar": dvar,
         "rmean": (1 - mom) * rm + mom * m, "rvar": (1 - mom) * rv + mom * unb,
         "ymax": y.max(0).values, "ymin": y.min(0).values,
         "b_mean": b_mean, "b_inv": b_inv, "b_scale": b_scale, "b_shift": b_shift,
         "b_rmean": bound32(1, (1 - mom) * rm.abs() + mom * m.abs()) + mom * b_mean,
         "b_rvar": bound32(1, (1 - mom) * rv.abs() + mom * unb) + mom * dvar * k,
         "E2": E2}
    # the fp64 reference ops (bound64 of each magnitude; the variance term stays: it is the oracle's too)
    r_inv = inv * (1e-12 + dvar / (2 * (var + eps)))
    r_scale = ga.abs() * r_inv
    o.update({"r_mean": bound64(A1), "r_inv": r_inv, "r_scale": r_scale,
              "r_shift": bound64(be.abs() + m.abs() * scale.abs()) + scale.abs() * bound64(A1) + m.abs() * r_scale,
              "r_rmean": bound64((1 - mom) * rm.abs() + mom * A1),
              "r_rvar": bound64((1 - mom) * rv.abs() + mom * E2 * k) + mom * dvar * k})
    return o


STAT_ROWS = (("mean", bs.MEAN), ("inv", bs.INV), ("scale", bs.SCALE), ("shift", bs.SHIFT))


def check_stats(y, rows, coef, prm, op, who, ref64=False):
    """The forward rows of ``coef`` [G, ROWS, C] and the running statistics of ``prm`` against the
    oracle of the run's own y ([G, N, H, W, C]); ``rows[g]`` valid rows.  An empty replica's parameter
    row keeps its bits.  Returns the per-replica oracles."""
    coef, yc, got = coef.detach().cpu(), y.detach().cpu(), prm.got()
    outs = []
    for g, n in enumerate(rows):
        if n == 0:
            check_exact(prm.flat.cpu()[g].to(F32), prm.flat0[g], op, "parameter row of the empty replica", who,
                        bitwise=not ref64)
            outs.append(None)
            continue
        yv = valid_rows(yc[g], n)
        o = stats_oracle(yv, prm.v0["gamma"][g], prm.v0["beta"][g], prm.v0["rmean"][g], prm.v0["rvar"][g])
        pre = "r_" if ref64 else "b_"
        for name, row in STAT_ROWS:
            check_bound(coef[g, row], o[name], o[pre + name], op, name, who)
        for name in ("rmean", "rvar"):
            check_bound(got[name][g], o[name], o[pre + name], op, "running " + name[1:], who)
        check_exact(coef[g, bs.YMAX], o["ymax"], op, "ymax", who, bitwise=not ref64)
        check_exact(coef[g, bs.YMIN], o["ymin"], op, "ymin", who, bitwise=not ref64)
        outs.append(o)
    prm.check_rest(op, who, fwd=True)
    return outs


# ================================================================== elementwise: oracle + bounds
def _bc(row, t):
    return row.double().view(*([1] * (t.dim() - 1)), -1)


def apply_oracle(ya, ca, res, yb, cb, relu_b, relu):
    """One replica: relu?(ya sc_a + sh_a + r) from the fp32 coefficient rows; (want, magnitude)."""
    v = ya.double() * _bc(ca[bs.SCALE], ya) + _bc(ca[bs.SHIFT], ya)
    A = ya.double().abs() * _bc(ca[bs.SCALE], ya).abs() + _bc(ca[bs.SHIFT], ya).abs()
    if res is not None:
        v, A = v + res.double(), A + res.double().abs()
    elif yb is not None:
        r = yb.double() * _bc(cb[bs.SCALE], yb) + _bc(cb[bs.SHIFT], yb)
        A = A + yb.double().abs() * _bc(cb[bs.SCALE], yb).abs() + _bc(cb[bs.SHIFT], yb).abs()
        v = v + (torch.relu(r) if relu_b else r)
    return (torch.relu(v) if relu else v), A


APPLY_N = 3      # the fma, the residual's fma, the add
DY_N = 2         # two fmas


def dy_oracle(d, y, cf):
    v = _bc(cf[bs.A], d) * d.double() + _bc(cf[bs.B], d) * y.double() + _bc(cf[bs.K], d)
    A = _bc(cf[bs.A], d).abs() * d.double().abs() + _bc(cf[bs.B], d).abs() * y.double().abs() + _bc(cf[bs.K], d).abs()
    return v, A


# ==================================================================== backward: oracle + bounds
def finish_oracle(d, y, cf, gamma, dg0, db0):
    """d, y [n, C] (the kernel's own masked gradient and the BN input); ``cf`` the installed fp32
    rows [ROWS, C]; gamma and the prior gradients [C]."""
    dd, yd = d.double(), y.double()
    n = dd.shape[0]
    mean, inv, ga = cf[bs.MEAN].double(), cf[bs.INV].double(), gamma.double()
    t = dd * ((yd - mean) * inv)
    sd, S_d, sdx, S_dx = dd.sum(0), dd.abs().sum(0), t.sum(0), t.abs().sum(0)
    b_sd = U32 * sd.abs() + (n + 1) * U64 * S_d
    b_sdx = U32 * sdx.abs() + (2 * U32 * (1 + U32) + (n + 1) * U64) * S_dx
    A = ga * inv
    B = -A * inv * sdx / n
    K = -A * sd / n - B * mean
    pB = A.abs() * inv / n * b_sdx
    A_K = (A * sd / n).abs() + (B * mean).abs()
    dmax = dd.abs().max(0).values
    ymax, ymin = cf[bs.YMAX].double(), cf[bs.YMIN].double()
    up = A.abs() * dmax + torch.maximum((B * ymax + K).abs(), (B * ymin + K).abs())
    dg0, db0 = dg0.double(), db0.double()
    return {"dgamma": dg0 + sdx, "dbeta": db0 + sd, "A": A, "B": B, "K": K,
            "b_dgamma": bound32(1, dg0.abs() + sdx.abs()) + b_sdx, "b_dbeta": bound32(1, db0.abs() + sd.abs()) + b_sd,
            "b_A": bound32(1, A.abs()), "b_B": bound32(4, B.abs()) + pB,
            "b_K": bound32(6, A_K) + A.abs() / n * b_sd + mean.abs() * pB,
            "A_dgamma": dg0.abs() + S_dx, "A_dbeta": db0.abs() + S_d, "A_A": A.abs(),
            "A_B": A.abs() * inv * S_dx / n, "A_K": A.abs() * S_d / n + A.abs() * inv * S_dx / n * mean.abs(),
            "up": up, "dbound_max": float(up.max()) * (1 + 2.0 ** -9)}


def dbound_formula(cf, d):
    """The header's dy bound from the kernel's OWN fp32 rows ``cf`` [ROWS, C] and d [n, C], in fp64: max over
    the channels of ``(|A| dmax + max |B y + K|) (1 + 2^-10)``, y at both ends of [ymin, ymax].  The kernel
    forms it with at most four fp32 roundings (the product, the fma, the sum, the factor; three when the
    compiler fuses the product and the sum), none of them behind a cancellation: ``bound32(3, .)``."""
    A, B, K = cf[bs.A].double(), cf[bs.B].double(), cf[bs.K].double()
    dmax = d.double().abs().max(0).values
    F = A.abs() * dmax + torch.maximum((B * cf[bs.YMAX].double() + K).abs(), (B * cf[bs.YMIN].double() + K).abs())
    return float(F.max()) * (1 + 2.0 ** -10)


def check_finish_bn(d, y, rows, cf0, coef, prm, dbound, dy, op, who, ref64=False):
    """One BN of a finished gradient: dgamma / dbeta (accumulated onto the priors), A / B / K, and the
    dy bound slot (``dbound`` [G], ``dy`` the stored fp32 dy of the same d) against the oracle of the
    run's own d; the empty replica's gradient row keeps its bits."""
    dc, yc, coef, got = d.detach().cpu(), y.detach().cpu(), coef.detach().cpu(), prm.got()
    for g, n in enumerate(rows):
        if n == 0:
            check_exact(prm.grads.cpu()[g].to(F32), prm.grads0[g], op, "gradient row of the empty replica", who,
                        bitwise=not ref64)
            continue
        o = finish_oracle(valid_rows(dc[g], n), valid_rows(yc[g], n), cf0[g], prm.v0["gamma"][g],
                          prm.v0["dgamma"][g], prm.v0["dbeta"][g])
        for name in ("dgamma", "dbeta"):
            check_bound(got[name][g], o[name], bound64(o["A_" + name]) if ref64 else o["b_" + name], op, name, who)
        for name, row in (("A", bs.A), ("B", bs.B), ("K", bs.K)):
            check_bound(coef[g, row], o[name], bound64(o["A_" + name]) if ref64 else o["b_" + name], op, name, who)
        # the installed forward rows are read, never written
        check_exact(coef[g, :bs.A].to(F32), cf0[g, :bs.A], op, "forward rows", who, bitwise=not ref64)
        if dbound is not None:
            top = float(valid_rows(dy[g].cpu(), n).abs().max())
            assert dbound[g] >= top, f"{op} [{who}] replica {g}: dy bound {dbound[g]!r} below max |dy| {top!r}"
            assert dbound[g] <= o["dbound_max"], (f"{op} [{who}] replica {g}: dy bound {dbound[g]!r} above "
                                                  f"(|A| dmax + max|B y + K|)(1 + 2^-9) = {o['dbound_max']!r}")
            want = dbound_formula(coef[g], valid_rows(dc[g], n))      # the documented formula, from the kernel's rows
            check_bound(dbound[g:g + 1], torch.tensor([want], dtype=F64), bound32(3, want), op, "dy bound slot vs its formula", who)
    prm.check_rest(op, who, fwd=False)


# ============================================================================ the CPU emulation
# The header's arithmetic on the CPU: fp64 sums over 32-row groups in order, thread t of 256 taking
# groups t, t + 256, ... in order, the pairwise tree tid <- tid + w (w = 128 .. 1), fp32 roundings
# where bnf_finalize_channel has them.
def _groups(term, op, ident):
    n, C = term.shape
    ng = -(-n // 32)
    pad = np.full((ng * 32, C), ident)
    pad[:n] = term
    pad = pad.reshape(ng, 32, C)
    acc = np.full((ng, C), ident)
    for r in range(32):
        acc = op(acc, pad[:, r])
    return acc


def _tree(rec, op, ident):
    ng, C = rec.shape
    trips = -(-ng // 256)
    pad = np.full((trips * 256, C), ident)
    pad[:ng] = rec
    pad = pad.reshape(trips, 256, C)
    acc = pad[0].copy()
    for t in range(1, trips):
        acc = op(acc, pad[t])
    w = 128
    while w:
        acc[:w] = op(acc[:w], acc[w:2 * w])
        w //= 2
    return acc[0]


def _reduce(term, kind):
    op, ident = {"sum": (np.add, 0.0), "max": (np.maximum, -np.inf), "min": (np.minimum, np.inf)}[kind]
    return _tree(_groups(term, op, ident), op, ident)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64 (one further fp64 rounding of the sum)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_stats(y, gamma, beta, rm, rv, relu, clamp=True):
    """bnf_finalize_channel mode 1 on y [n, C] fp32: the six rows, the running statistics, the bound."""
    v = y.numpy().astype(np.float64)
    n = float(v.shape[0])
    S, S2, mx, mn = _reduce(v, "sum"), _reduce(v * v, "sum"), _reduce(v, "max"), _reduce(v, "min")
    m = S / n
    var = S2 / n - m * m
    if clamp:
        var = np.where(var < 0, 0.0, var)
    f = np.float32
    mom, eps = np.float64(f(MOMENTUM)), np.float64(f(EPS))
    with np.errstate(invalid="ignore"):
        mean, inv = m.astype(f), (1.0 / np.sqrt(var + eps)).astype(f)
    unb = var * n / (n - 1) if n > 1 else var
    ga, be = gamma.numpy().astype(f), beta.numpy().astype(f)
    sc = inv * ga
    sh = be - mean * sc
    ymax, ymin = mx.astype(f), mn.astype(f)
    hi, lo = _fma32(ymax, sc, sh), _fma32(ymin, sc, sh)
    if relu:
        hi, lo = np.maximum(hi, f(0)), np.maximum(lo, f(0))
    t = torch.from_numpy
    return {"mean": t(mean), "inv": t(inv), "scale": t(sc), "shift": t(sh), "ymax": t(ymax), "ymin": t(ymin),
            "rmean": t(((1 - mom) * rm.numpy().astype(np.float64) + mom * m).astype(f)),
            "rvar": t(((1 - mom) * rv.numpy().astype(np.float64) + mom * unb).astype(f)),
            "bound": float(np.max(np.maximum(np.abs(hi), np.abs(lo))))}


def emulate_finish(d, y, cf, gamma, dg0, db0, factor=True):
    """bnf_tile_records + bnf_finalize_channel mode 2 on d, y [n, C] fp32."""
    f = np.float32
    dv, yv = d.numpy().astype(f), y.numpy().astype(f)
    mean, inv = cf[bs.MEAN].numpy().astype(f), cf[bs.INV].numpy().astype(f)
    xh = ((yv - mean) * inv).astype(np.float64)             # two fp32 roundings
    d64 = dv.astype(np.float64)
    sd, sdx = _reduce(d64, "sum").astype(f), _reduce(d64 * xh, "sum").astype(f)
    dmax = np.maximum(_reduce(np.abs(d64), "max"), 0.0).astype(f)
    fn = f(dv.shape[0])
    ga = gamma.numpy().astype(f) * inv
    B = -ga * inv * sdx / fn
    K = -ga * sd / fn - B * mean
    hi, lo = _fma32(B, cf[bs.YMAX].numpy().astype(f), K), _fma32(B, cf[bs.YMIN].numpy().astype(f), K)
    bound = (np.abs(ga) * dmax + np.maximum(np.abs(hi), np.abs(lo))) * (f(1) + (f(2.0 ** -10) if factor else f(0)))
    dy = _fma32(np.broadcast_to(ga, dv.shape), dv, _fma32(np.broadcast_to(B, yv.shape), yv, np.broadcast_to(K, yv.shape)))
    t = torch.from_numpy
    return {"dgamma": t(dg0.numpy().astype(f) + sdx), "dbeta": t(db0.numpy().astype(f) + sd), "A": t(ga), "B": t(B),
            "K": t(K), "dbound": float(bound.max()), "dy": t(dy)}


# ================================================================================ data kinds
# Forward kinds (the issue's six): N(0.3, 1); per-channel mean +-100 / std 0.1; mean 1e3 / std 1e-2
# (cancellation in S2 / n - m^2: a clamped variance, not a sharp inv); constant channels of
# magnitude 1e6, one element an ulp off, with channel 0 exactly zero (var = 0, inv = 1 / sqrt(eps);
# S2 / n - m^2 rounds to either side of zero in the others); scales 1e-20 and 1e15.
FWD_KINDS = ("n03", "m100", "m1e3", "const", "tiny", "huge")
SHARP_KINDS = ("n03", "m100", "tiny", "huge")       # inv bound under 1e-6 relative


def fwd_values(kind, shape, g):
    C = shape[-1]
    z = torch.randn(shape, generator=g, dtype=F64)
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    if kind == "n03":
        y = 0.3 + z
    elif kind == "m100":
        y = sign * 100 + 0.1 * z
    elif kind == "m1e3":
        y = sign * 1e3 + 1e-2 * z
    elif kind == "const":
        y = (sign * 1e6 * (1 + torch.rand(C, generator=g, dtype=F64))).expand(shape).float().clone()
        # one element an ulp away: S2 / n - m^2 then carries roundings of size ulp(1e12) ~ 1e-4 >> eps
        # around a true variance of ulp(1e6)^2 / n, and comes out negative in about half the channels
        y[:, 0, 0, 0] = torch.nextafter(y[:, 0, 0, 0], torch.full_like(y[:, 0, 0, 0], math.inf))
        y[..., 0] = 0.0
    elif kind == "tiny":
        y = 1e-20 * (0.3 + z)
    else:
        y = 1e15 * (0.3 + z)
    return y.float()


def garbage(t, nvalid, g):
    """Rows beyond nvalid of every input: large finite garbage."""
    if nvalid is None:
        return t
    for r, nv in enumerate(nvalid):
        if nv < t.shape[1]:
            t[r, nv:] = GARBAGE * torch.randn(t[r, nv:].shape, generator=g)
    return t


# ============================================================ table 0: the standalone mode-1 pass
# bnx_tile_kernel mode 1 + bnx_finalize_kernel on a chosen y: the data kinds no conv can be made to
# emit, and row counts through the finalize's second trip.  (N, HW, nv1, C, kind, relu); G = 3,
# nvalid = (N, nv1, 0).  Rows per replica: 1; 2; 33 / 31; 129 / 33; 8193 / 8160 (257 / 255 groups) at
# C = 4; HW 9 with nvalid inside a group.
RowsCase = namedtuple("RowsCase", "name N H W nv1 C kind relu why")
ROWS_CASES = [
    RowsCase("r-n1-n03", 1, 1, 1, 1, 4, "n03", True, "one row: var 0, the unbiased variance not divided by n - 1"),
    RowsCase("r-n1-const", 1, 1, 1, 1, 60, "const", False, "one row of 1e6"),
    RowsCase("r-n2-m100", 2, 1, 1, 1, 64, "m100", True, "two rows / one row"),
    RowsCase("r-n33-n03", 33, 1, 1, 31, 60, "n03", True, "a second group of one row; 31 rows"),
    RowsCase("r-n33-huge", 33, 1, 1, 31, 64, "huge", False, "1e15 scale"),
    RowsCase("r-n33-const", 33, 1, 1, 32, 68, "const", True, "constant 1e6 channels: the clamp"),
    RowsCase("r-n129-m100", 129, 1, 1, 33, 68, "m100", False, "a second 128-row tile of one row; C off the 64-column tile"),
    RowsCase("r-n129-tiny", 129, 1, 1, 127, 4, "tiny", True, "1e-20 scale: var far below eps"),
    RowsCase("r-hw9-n03", 15, 3, 3, 4, 68, "n03", True, "HW 9: 135 rows, nvalid 4 cuts inside the second group"),
    RowsCase("r-n8193-n03", 8193, 1, 1, 8160, 4, "n03", True, "257 / 255 groups: the finalize's second trip"),
    RowsCase("r-n8193-m1e3", 8193, 1, 1, 8160, 4, "m1e3", False, "dvar / var 8e-3: clamped, finite"),
    RowsCase("r-n8192-const", 2048, 2, 2, 2040, 4, "const", True, "256 groups exactly, HW 4; constant channels"),
]


def rows_nvalid(c):
    return [c.N, c.nv1, 0]


@functools.lru_cache(maxsize=None)
def rows_inputs(c):
    g = gen(22, c.N, c.H * c.W, c.C, FWD_KINDS.index(c.kind))
    y = fwd_values(c.kind, (3, c.N, c.H, c.W, c.C), g)
    return {"y": garbage(y, rows_nvalid(c), g), "nvalid": rows_nvalid(c)}


def hip_rows_stats(H, y, nvalid, prm, relu):
    """dba_bnx_rows mode 1 over a stored y (the standalone producer of the level-0 records)."""
    G, N, Hh, Ww, C = y.shape
    f, st = H._bnf_fwd(prm.bn(), relu, G, N * Hh * Ww, C, y.device)
    H._call("dba_bnx_rows", ctypes.byref(f), y.data_ptr(), None, y.stride(0), H._ptr(H._i32(nvalid)), G, N, Hh * Ww,
            None, 0.0, H._stream())
    return st


def fwd_bits(st, prm, rows):
    """What the header calls the same bits whichever producer: rows MEAN .. YMIN, the running
    statistics, the bound slot (an empty replica's coefficient rows are never written: zeroed here)."""
    got = prm.got()
    cf = st.coef[:, :bs.A].cpu().clone()
    for g, n in enumerate(rows):
        if n == 0:
            cf[g] = 0
    return {"rows": cf, "rmean": got["rmean"], "rvar": got["rvar"], "bound": slot_value(st.bound)[:len(rows)]}


def check_fwd_bound_slot(H, y, st, relu, nvalid_dev, rows, op, who=HIP):
    """The bound slot equals bit for bit max |out| of the stored BN(+ReLU) output of the same y, and
    that output holds the elementwise bound against the oracle of the kernel's own rows."""
    out = H.bn_apply(bs.LazyBN(y, st, relu), None, relu, nvalid_dev)
    outc, yc, coef = out.cpu(), y.cpu(), st.coef.cpu()
    slot, aslot = slot_value(st.bound), slot_value(out._dba_amax)
    for g, n in enumerate(rows):
        if n == 0:
            continue
        o, yv = valid_rows(outc[g], n), valid_rows(yc[g], n)
        want, A = apply_oracle(yv, coef[g], None, None, None, False, relu)
        check_bound(o, want, bound32(1, A), op, "stored BN output", who)
        top = o.abs().max().reshape(1)
        check_exact(slot[g:g + 1], top, op, "forward bound slot vs max |out|", who)
        check_exact(aslot[g:g + 1], top, op, "bn_apply max slot", who)
    return out


# ===================================================== table 1: the standalone pass and finalize
# bn_finish -> bnx_tile_kernel mode 2 + bnx_finalize_kernel.  G = 3: nvalid = (N, nv1, 0), or None
# (``full``).  mask: "out" a stored output holding +0, -0, +-denormals and a NaN at the first
# elements of every replica (a NaN mask is "not > 0", a positive denormal is > 0), "lazy" the sign of
# fma(ya, scale, shift), "none".  two: a second BN (yb, sb).  kind "al": per channel, max |d| sits on
# the row of the extreme y with the sign that adds |A d| and |B y + K|, so a bound that dropped a
# term or its factor is met with equality.  pool: g is the global average pool's gradient.
FinCase = namedtuple("FinCase", "name N H W nv1 C mask two kind pool full why")


def _fin(name, N, HW, nv1, C, mask, two, why, kind="n", pool=False, full=False):
    H, W = HW
    return FinCase(name, N, H, W, nv1, C, mask, two, kind, pool, full, why)


FIN_CASES = [
    _fin("f-n1", 1, (1, 1), 1, 4, "out", False, "one row, one group, C 4"),
    _fin("f-n32-31", 32, (1, 1), 31, 60, "lazy", False, "32 rows: one full group; 31"),
    _fin("f-n33-c4", 33, (1, 1), 1, 4, "none", True, "33 rows: a group of one row; C 4", kind="al"),
    _fin("f-n33-c60", 33, (1, 1), 31, 60, "out", True, "33 rows, C 60: a partial 64-column tile", kind="al"),
    _fin("f-n33-c64", 33, (1, 1), 32, 64, "lazy", False, "33 rows, C 64: exactly one column tile"),
    _fin("f-n33-c68", 33, (1, 1), 2, 68, "out", False, "33 rows, C 68: a second column tile of 4"),
    _fin("f-n128-127", 128, (1, 1), 127, 64, "none", False, "the 128-row tile, exactly / one short", kind="al"),
    _fin("f-n129-c4", 129, (1, 1), 127, 4, "lazy", False, "129 rows: a second row tile of one row; C 4"),
    _fin("f-n129-c60", 129, (1, 1), 33, 60, "out", False, "129 rows, C 60", kind="al"),
    _fin("f-n129-c64", 129, (1, 1), 128, 64, "out", True, "129 rows, C 64, two BNs"),
    _fin("f-n129-c68", 129, (1, 1), 1, 68, "none", True, "129 rows, C 68, two BNs", kind="al"),
    _fin("f-hw4-in-group", 9, (2, 2), 5, 60, "out", True, "HW 4 (Tiny-ImageNet's last stage): 36 rows, nvalid 5 -> 20 inside a group"),
    _fin("f-hw9-in-group", 15, (3, 3), 4, 68, "lazy", False, "HW 9: 135 rows, nvalid 4 -> 36 inside the second group"),
    _fin("f-hw16", 8, (4, 4), 2, 64, "out", False, "HW 16: 128 rows / 32 rows"),
    _fin("f-full", 9, (2, 2), 9, 60, "out", True, "nvalid = None: every replica full", full=True),
    _fin("f-n8193", 8193, (1, 1), 8160, 4, "out", True, "257 / 255 groups: the finalize's second trip", kind="al"),
    _fin("f-n8192-hw4", 2048, (2, 2), 2040, 4, "lazy", False, "256 groups exactly (no second trip) / 255, HW 4"),
    _fin("f-n8193-none", 8193, (1, 1), 8192, 4, "none", False, "257 / 256 groups, unmasked"),
    _fin("f-pool-hw1", 5, (1, 1), 3, 60, "out", False, "pooled gradient at HW 1, nvalid inside the batch", pool=True),
    _fin("f-pool-hw4", 9, (2, 2), 5, 68, "out", True, "pooled gradient at HW 4: image index (m0 + row) / 4", pool=True),
    _fin("f-pool-hw16", 9, (4, 4), 5, 64, "none", False, "pooled gradient at HW 16: 144 rows, a second row tile", pool=True,
         kind="al"),
]


# The bound met with equality: small "al" problems, each replica's largest |dy| the whole of |A| dmax +
# max |B y + K| in fp32.  Evaluated unfused, fl(fl(|A| dmax) + |fma(B, y, K)|) falls an ulp below
# |fma(A, d, fma(B, y, K))| whenever the product rounds down far enough: that is what the (1 + 2^-10)
# is for (test_bn_cases.py counts such replicas on the emulation).  Where the compiler fuses the product
# and the sum the bare sum is already an upper bound, so the factor itself is pinned by the slot's
# comparison with its formula (dbound_formula), not by the inequality.
AL_CASES = [_fin(f"f-al-{k:02d}", 40 + k, (1, 1), 20 + k, 4, "none", False, "the dy bound met with equality", kind="al")
            for k in range(12)]


def fin_id(c):
    return c.name


def fin_nvalid(c):
    return [c.N] * 3 if c.full else [c.N, c.nv1, 0]


MASK_SPECIALS = (0.0, -0.0, 1e-40, NAN, -1e-40)      # -> +0, +0, g, +0, +0


def install_rows(y, rows, g, positive_scale):
    """The fp32 coefficient rows a backward test installs: MEAN / INV / YMAX / YMIN of the valid rows
    (fp64, rounded once), free SCALE / SHIFT."""
    G, C = y.shape[0], y.shape[-1]
    cf = torch.zeros(G, bs.ROWS, C)
    for r, n in enumerate(rows):
        if n == 0:
            continue
        yy = valid_rows(y[r], n).double()
        cf[r, bs.MEAN] = yy.mean(0).float()
        cf[r, bs.INV] = torch.rsqrt(yy.var(0, unbiased=False) + f32(EPS)).float()
        cf[r, bs.YMAX], cf[r, bs.YMIN] = yy.max(0).values.float(), yy.min(0).values.float()
    sc = torch.rand(G, C, generator=g) + 0.5
    cf[:, bs.SCALE] = sc if positive_scale else sc * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0)
    cf[:, bs.SHIFT] = torch.randn(G, C, generator=g) * 0.2
    return cf


def mask_of(c_mask, mask_out, ya, cfa):
    """The boolean mask of one run, exact (see the module docstring)."""
    if c_mask == "out":
        return mask_out > 0
    if c_mask == "lazy":
        G, C = ya.shape[0], ya.shape[-1]
        pre = ya.double() * cfa[:, bs.SCALE].double().view(G, 1, 1, 1, C) + cfa[:, bs.SHIFT].double().view(G, 1, 1, 1, C)
        assert float(pre.abs().min()) > 1e-30, "lazy mask: |fma| near the fp32 underflow threshold"
        return pre > 0
    return torch.ones_like(ya, dtype=torch.bool)


def align(gsrc, ya, mask, rows, cfa):
    """kind "al": per (replica, channel) the element of max y carries max |d| with the sign s for which
    A d and B y + K add there.  B y + K = -A (xhat sum(d xhat) + sum d) / n, so the other rows get the
    drift -s (xhat + 1): both sums then take the sign -s with a weight (~ n (xhat_e + 1), halved by
    the mask) that outweighs the placed element's own (amp (xhat_e^2 + 1)), and the end of max y is
    the end of the larger |B y + K|.  s alternates over the channels."""
    C = ya.shape[-1]
    cols = torch.arange(C)
    sgn = torch.where(cols % 2 == 0, 1.0, -1.0)
    for r, n in enumerate(rows):
        if n < 16:
            continue
        gv, yv, mv = valid_rows(gsrc[r], n), valid_rows(ya[r], n), valid_rows(mask[r], n)
        xh = ((yv.double() - cfa[r, bs.MEAN].double()) * cfa[r, bs.INV].double()).float()
        gv -= sgn * (xh + 1)
        top = yv.argmax(0)
        amp = 1.001 * float(gv.abs().max())       # barely the maximum
        mv[top, cols] = True
        gv[top, cols] = sgn * amp


@functools.lru_cache(maxsize=None)
def fin_inputs(c):
    """Every operand of the case, fp32 on the CPU (never modified by a test)."""
    g = gen(23, c.N, c.H * c.W, c.nv1, c.C, len(c.name))
    G, shape = 3, (3, c.N, c.H, c.W, c.C)
    nv = fin_nvalid(c)
    rows = [n * c.H * c.W for n in nv]
    ya = (0.3 + torch.randn(shape, generator=g)).float()
    yb = (-0.2 + 2 * torch.randn(shape, generator=g)).float()
    cfa, cfb = install_rows(ya, rows, g, c.mask == "lazy"), install_rows(yb, rows, g, False)
    mask_out = torch.relu(torch.randn(shape, generator=g))
    for r in range(G):
        flat = mask_out[r].view(-1)
        k = min(len(MASK_SPECIALS), flat.numel() - 1)
        flat[:k] = torch.tensor(MASK_SPECIALS[:k])
    mask = mask_of(c.mask, mask_out, ya, cfa).clone()
    pool = None
    if c.pool:
        pool = torch.randn(3, c.N, 1, 1, c.C, generator=g)
        inv_hw = (torch.tensor(1.0) / torch.tensor(float(c.H * c.W))).float()
        gsrc = (pool * inv_hw).expand(shape).contiguous()       # fl32(pool fl32(1 / HW))
    else:
        gsrc = torch.randn(shape, generator=g)
    if c.kind == "al" and not c.pool:
        align(gsrc, ya, mask, rows, cfa)
        if c.mask == "out":
            mask_out = torch.where(mask & ~(mask_out > 0), torch.ones_like(mask_out), mask_out)
    want_d = torch.where(mask, gsrc, torch.zeros_like(gsrc))
    nvl = None if c.full else nv
    for t in (ya, yb, mask_out, gsrc):
        garbage(t, nvl, g)
    if pool is not None:
        garbage(pool, nvl, g)
    return {"ya": ya, "yb": yb, "cfa": cfa, "cfb": cfb, "mask_out": mask_out, "g": gsrc, "pool": pool, "want_d": want_d,
            "nvalid": nv, "rows": rows}


def make_stat(ops, who, prm, cf, lazy, G, C, dev, dt):
    """A BnStat holding installed rows (HIP: with its slots, as the forward would have left it)."""
    if who == HIP:
        st = ops._bnf_fwd(prm.bn(), lazy, G, 1, C, dev)[1]
        st.coef.copy_(cf.to(dev))
        return st
    return bs.BnStat(cf.to(dt).to(dev), prm.bn())


def hip_dy(H, d, y, coef, nvalid_dev):
    """dba_bnx_dy (bnx_dy_kernel) with a max slot: (dy, slot)."""
    G, N, Hh, Ww, C = d.shape
    dy = torch.empty_like(d)
    slot = H.amax_slots(1, G, d.device)[0]
    H._call("dba_bnx_dy", d.data_ptr(), y.data_ptr(), coef.data_ptr(), dy.data_ptr(), d.stride(0),
            H._ptr(H._i32(nvalid_dev)), G, N, Hh * Ww, C, *H._aptr(slot), H._stream())
    return dy, slot


def _sel(t, sel):
    return None if t is None else (t if sel is None else t[sel:sel + 1])


def run_finish(ops, c, dev, who, sel=None, dt=F32):
    """bn_finish on the case; every output on the CPU."""
    i = fin_inputs(c)
    G = 3 if sel is None else 1
    T = lambda k: None if i[k] is None else _sel(i[k], sel).to(dt).to(dev).contiguous()   # noqa: E731
    nv = i["nvalid"] if sel is None else i["nvalid"][sel:sel + 1]
    rows = i["rows"] if sel is None else i["rows"][sel:sel + 1]
    nvalid = None if c.full else torch.tensor(nv, dtype=I32, device=dev)
    pa, pb = Prm(3, c.C, (1, len(c.name)), dev, dt, sel), Prm(3, c.C, (2, len(c.name)), dev, dt, sel)
    ya, yb = T("ya"), T("yb")
    sa = make_stat(ops, who, pa, _sel(i["cfa"], sel), c.mask == "lazy", G, c.C, dev, dt)
    sb = make_stat(ops, who, pb, _sel(i["cfb"], sel), False, G, c.C, dev, dt) if c.two else None
    fin = bs.Finish(ya=ya, sa=sa, mask_out=T("mask_out") if c.mask == "out" else None, lazy=c.mask == "lazy",
                    yb=yb if c.two else None, sb=sb)
    if c.pool:
        r = ops.bn_finish(None, fin, nvalid, pool=T("pool"), hw=(c.H, c.W))
    else:
        r = ops.bn_finish(T("g"), fin, nvalid)
    assert isinstance(r, bs.Fin)
    return finish_outputs(ops, who, r.d, ya, yb if c.two else None, sa, sb, pa, pb, nvalid, rows)


def finish_outputs(ops, who, d, ya, yb, sa, sb, pa, pb, nvalid, rows):
    out = {"d": d, "rows": rows, "pa": pa, "pb": pb, "coef_a": sa.coef.cpu(), "coef_b": None if sb is None else sb.coef.cpu(),
           "dbound_a": None, "dbound_b": None, "dy_a": None, "dy_b": None}
    if who == HIP:
        for tag, st, y in (("a", sa, ya), ("b", sb, yb)):
            if st is None:
                continue
            dy, slot = hip_dy(ops, d, y, st.coef, nvalid)
            out["dbound_" + tag], out["dy_" + tag], out["dyslot_" + tag] = slot_value(st.dbound), dy.cpu(), slot_value(slot)
    out["d"] = d.cpu()
    return out


def finish_bits(out):
    """The outputs compared run to run / alone vs in a group (valid rows only)."""
    d = out["d"].clone()
    for g, n in enumerate(out["rows"]):
        d[g].view(-1, d.shape[-1])[n:] = 0
    b = {"d": d, "coef_a": out["coef_a"], "coef_b": out["coef_b"], "grads_a": out["pa"].grads.cpu()}
    if out["dbound_a"] is not None:
        b["dbound_a"] = out["dbound_a"][:len(out["rows"])]
    return b


def check_finish(i, out, two, op, who, ref64=False):
    """Sums, coefficients and bound slots of a finished gradient from its own d (tables 1 and 3);
    ``i``: ya, yb, cfa, cfb on the CPU."""
    rows = out["rows"]
    check_finish_bn(out["d"], i["ya"], rows, i["cfa"], out["coef_a"], out["pa"], out["dbound_a"], out["dy_a"], op + " (BN a)",
                    who, ref64)
    if two:
        check_finish_bn(out["d"], i["yb"], rows, i["cfb"], out["coef_b"], out["pb"], out["dbound_b"], out["dy_b"],
                        op + " (BN b)", who, ref64)
    if who == HIP:     # the stored dy: elementwise, and its own max slot bit for bit
        for tag, y in (("a", i["ya"]), ("b", i["yb"])):
            if out["dy_" + tag] is None:
                continue
            for g, n in enumerate(rows):
                if n == 0:
                    continue
                dv, yv, got = valid_rows(out["d"][g], n), valid_rows(y[g], n), valid_rows(out["dy_" + tag][g], n)
                want, A = dy_oracle(dv, yv, out["coef_" + tag][g])
                check_bound(got, want, bound32(DY_N, A), "bnx_dy", "dy", who)
                check_exact(out["dyslot_" + tag][g:g + 1], got.abs().max().reshape(1), "bnx_dy", "max |dy| slot", who)


def check_finish_d(c, out, who, sel=None):
    """d bit for bit: g where the mask holds, +0 elsewhere (the reference multiplies by the mask and
    leaves -0: compared by value)."""
    i = fin_inputs(c)
    want = _sel(i["want_d"], sel)
    for g, n in enumerate(out["rows"]):
        if n:
            check_exact(valid_rows(out["d"][g], n).to(F32), valid_rows(want[g], n), "bn_finish",
                        "d" + (" (pooled)" if c.pool else ""), who, bitwise=who == HIP)


# ===================================================== table 2: statistics from every record producer
# conv_bn_stats on rows taken from, or modelled on, conv_cases.FWD_CASES (Cout % 4 == 0, no bias /
# residual / ReLU: what the launcher accepts with statistics).  ``path`` is re-derived by stats_path:
# with statistics ximg / xstage16 decline, the 5x5 stem declines, and the 3x3 / 7x7 stems keep their
# kernel (PIX = 64 / 32 are multiples of the 32-row group).  Every row: channel 0 has zero weights (a
# constant channel: var = 0, inv = 1 / sqrt(eps)); Prm's special channels give gamma 0, a negative
# gamma (the bound needs both ends of [ymin, ymax]) and an all-negative output under the ReLU.
_F = {c.name: c for c in CC.FWD_CASES}


def _model(name, G, N, HW, Cin, Cout, k, s, p, path, why, **opt):
    return CC._case(name, G, N, HW, Cin, Cout, k, s, p, path, why, **opt)


STATS_CASES = [
    # implicit-GEMM epilogue, each column-tile width, M 25 / 127 / 129 and a single partial group
    _F["t-co4-ci3-m127"], _F["g-7x5-s2"],
    _model("s-co8-ci4-m25", 3, 1, 5, 4, 8, 3, 1, 1, "gemm bn32 vec4", "bn32 at M 25"),
    _model("s-co52-ci36-m129", 3, 3, (1, 43), 36, 52, 1, 1, 0, "gemm bn64 vec4", "bn64 at M 129 / 86"),
    _model("s-co36-ci4-m25", 3, 1, 5, 4, 36, 3, 1, 1, "gemm bn64 vec4", "bn64 at M 25"),
    _F["t-co132-ci36-m25"],
    _model("s-co132-ci4-m127", 3, 1, (1, 127), 4, 132, 1, 1, 0, "gemm bn128 vec4", "bn128 at M 127"),
    _model("s-n1", 3, 1, 1, 4, 8, 1, 1, 0, "gemm bn32 vec4", "a single valid row: n = 1"),
    # xhalo_kernel
    _F["h32-n4"], _F["h32-n28"], _F["h32-n32"], _F["h16-n4"], _F["h16-n36"], _F["h16-n64"],
    # split-K: combined in the launch, in-block slabs, slabs + bnx_tile_kernel mode 1
    _F["k-inlaunch-800"], _F["k-inlaunch-m27"], _F["k-kslab-512"], _F["k-reduce-800"],
    # stem.hip's own record loop, M off 32
    _F["stem-3x3"], _F["stem-7x7"],
    # a lazy BN+ReLU input
    _model("s-h32-n28-lz", 3, 3, 32, 32, 28, 3, 1, 1, "xhalo w32", "xhalo W 32 staging a lazy BN+ReLU input", lzx=1),
    _model("s-gemm-lz", 3, 3, (1, 43), 36, 52, 1, 1, 0, "gemm bn64 vec4", "implicit GEMM staging a lazy BN+ReLU input", lzx=1),
]
STATS_DECLINE = _F["k-decline-130"]


def stats_path(c):
    """The forward dispatch with statistics, from the documented conditions: conv_cases.fwd_path with
    the whole-image and staged kernels declining (training weights are never pre-split)."""
    assert not CC.opt(c, "pre") and c.Cout % 4 == 0
    if (c.KH, c.KW, c.Cin, c.Cout) == (5, 5, 1, 20):
        raise AssertionError("the 5x5 stem declines statistics")
    keep = tuple(kv for kv in c.opt if kv[0] not in ("ximg", "xstage"))
    return CC.fwd_path(c._replace(opt=tuple(sorted(keep + (("ximg", 0), ("xstage", 0))))))


def stats_relu(c):
    return len(c.name) % 2 == 0


def stats_rows(c, sel=None):
    nv = CC.inputs(c)["nvalid"]
    rows = [n * c.Ho * c.Wo for n in nv]
    return rows if sel is None else rows[sel:sel + 1]


def stats_prm(c, dev, dt=F32, sel=None):
    return Prm(c.G, c.Cout, (3, len(c.name)), dev, dt, sel if c.G > 1 else None)


def run_conv_stats(ops, c, dev, who, sel=None, dt=F32):
    """conv_bn_stats on the case (channel 0's weights zeroed).  Returns y, the BnStat, its Prm, the
    launched path and the device nvalid."""
    inp = CC.inputs(c)
    x, = CC._dev(inp, dev, sel, "x")
    wsel, nvalid, nv = CC._maps_dev(inp, dev, sel)
    w = CC._weights(ops, inp, dev, c, sel) if who == HIP else inp["w"].clone().to(dev)
    w[:, 0] = 0
    G = x.shape[0]
    prm = stats_prm(c, dev, dt, sel)
    relu = stats_relu(c)
    if CC.opt(c, "lzx"):
        if who == HIP:
            x = CC._lazy_bn(ops, c, inp, dev, sel, x, nv)
        else:
            raw, sc, sh = CC._dev(inp, dev, sel, "x_raw", "lz_scale", "lz_shift")
            coef = torch.zeros(G, bs.ROWS, c.Cin, dtype=dt)
            coef[:, bs.SCALE], coef[:, bs.SHIFT] = sc.to(dt), sh.to(dt)
            x = bs.LazyBN(raw.to(dt), bs.BnStat(coef, None), True)
    elif dt != F32:
        x = x.to(dt)
    path = None
    if who == HIP:
        with CC.settings(ops, c, dev):
            y, st = ops.conv_bn_stats(x, w, wsel, c.s, c.p, nvalid, prm.bn(), relu)
            path = launched_path(ops)
    else:
        y, st = ops.conv_bn_stats(x, w.to(dt), wsel, c.s, c.p, nvalid, prm.bn(), relu)
    return {"y": y, "st": st, "prm": prm, "path": path, "nvalid": nvalid, "rows": stats_rows(c, sel), "relu": relu}


# ============================================== table 3: mask + reduce in the data-gradient epilogue
# conv2d_dgrad(..., finish=) on conv_cases.DGRAD_CASES rows with Cin % 4 == 0: the halo kernel, the
# implicit GEMM, the three split-K forms (``d-reduce`` sums slabs + accum in the standalone pass) and a
# stride-2 row, which goes through bn_finish.  (row, mask, two BNs, accum)
_D = {c.name: c for c in CC.DGRAD_CASES}
DFIN_CASES = [
    (_D["d-h32-ci4"], "out", True, True), (_D["d-h32-ci28"], "lazy", False, False), (_D["d-h16-ci36"], "out", False, True),
    (_D["d-slots-g"], "lazy", False, True), (_D["d-slots-g"], "out", True, False),
    (_D["d-inlaunch"], "out", True, True), (_D["d-kslab"], "lazy", False, True), (_D["d-reduce"], "out", True, True),
    (_D["d-7x5-k3"], "out", True, True), (_D["d-7x5-k3"], "lazy", False, False),
]
DFIN_DECLINE = _D["d-co33-ci50"]


def dfin_id(p):
    c, mask, two, accum = p
    return f"{c.name}-{mask}-{'two' if two else 'one'}-{'accum' if accum else 'plain'}"


@functools.lru_cache(maxsize=None)
def dfin_inputs(c, mask):
    g = gen(24, c.N, c.H, c.W, c.Cin, len(c.name), mask == "lazy")
    nv = CC.inputs(c)["nvalid"]
    shape = (c.G, c.N, c.H, c.W, c.Cin)
    rows = [n * c.H * c.W for n in nv]
    ya = (0.3 + torch.randn(shape, generator=g)).float()
    yb = (-0.2 + 2 * torch.randn(shape, generator=g)).float()
    cfa, cfb = install_rows(ya, rows, g, mask == "lazy"), install_rows(yb, rows, g, False)
    mask_out = torch.relu(torch.randn(shape, generator=g))
    for r in range(c.G):
        flat = mask_out[r].view(-1)
        flat[:len(MASK_SPECIALS)] = torch.tensor(MASK_SPECIALS)
    m = mask_of(mask, mask_out, ya, cfa).clone()
    for t in (ya, yb, mask_out):
        garbage(t, nv, g)
    return {"ya": ya, "yb": yb, "cfa": cfa, "cfb": cfb, "mask_out": mask_out, "mask": m, "nvalid": nv, "rows": rows}


def run_dgrad_finish(ops, p, dev, who, sel=None, dt=F32):
    c, mask, two, accum = p
    inp, i = CC.inputs(c), dfin_inputs(c, mask)
    dy, acc = CC._dev(inp, dev, sel, "dy", "acc")
    wsel, nvalid, nv = CC._maps_dev(inp, dev, sel)
    w = CC._weights(ops, inp, dev, c, sel) if who == HIP else inp["w"].clone()
    one = sel is not None and c.G > 1
    G = 1 if one else c.G
    T = lambda k: (i[k][sel:sel + 1] if one else i[k]).to(dt).to(dev).contiguous()   # noqa: E731
    s_ = sel if one else None
    pa, pb = Prm(c.G, c.Cin, (4, len(c.name)), dev, dt, s_), Prm(c.G, c.Cin, (5, len(c.name)), dev, dt, s_)
    ya, yb = T("ya"), T("yb")
    sa = make_stat(ops, who, pa, _sel(i["cfa"], s_), mask == "lazy", G, c.Cin, dev, dt)
    sb = make_stat(ops, who, pb, _sel(i["cfb"], s_), False, G, c.Cin, dev, dt) if two else None
    fin = bs.Finish(ya=ya, sa=sa, mask_out=T("mask_out") if mask == "out" else None, lazy=mask == "lazy",
                    yb=yb if two else None, sb=sb)
    path = None
    if who == HIP:
        with CC.settings(ops, c, dev):
            r = ops.conv2d_dgrad(dy, w, wsel, c.s, c.p, (c.H, c.W), nvalid=nvalid, accum=acc if accum else None, finish=fin)
            path = launched_path(ops)
    else:
        r = ops.conv2d_dgrad(dy.to(dt), w.to(dt), wsel, c.s, c.p, (c.H, c.W), nvalid=nvalid,
                             accum=acc.to(dt) if accum else None, finish=fin)
    assert isinstance(r, bs.Fin)
    rows = [n * c.H * c.W for n in nv]
    out = finish_outputs(ops, who, r.d, ya, yb if two else None, sa, sb, pa, pb, nvalid, rows)
    out["path"] = path
    return out


def check_dgrad_d(p, out, who, sel=None):
    """d equals the data-gradient oracle (both conv bounds) where the mask holds and is exactly +0
    where it does not."""
    c, mask, two, accum = p
    i = dfin_inputs(c, mask)
    o = CC.oracle("dgrad", c, "a" if accum else "")
    reps = range(c.G) if (sel is None or c.G == 1) else [sel]
    d = out["d"].clone()
    for k, g in enumerate(reps):
        nv = i["nvalid"][g]
        if nv == 0:
            continue
        m = i["mask"][g, :nv]
        off = d[k, :nv][~m]
        check_exact(off, torch.zeros_like(off), "conv2d_dgrad finish", "d where the mask is false", who)
        d[k, :nv] = torch.where(m, d[k, :nv], o[g].want.float())
    check_act_out("dgrad", c, d, "a" if accum else "", who, out["path"] or c.path, sel=None if c.G == 1 else sel)


# ================================================================= table 4: stored elementwise passes
# bn_apply (bnx_apply_kernel) and the stored dy (bnx_dy_kernel): 256 threads x float4, the grid capped
# at 8192 // G blocks.  (N, HW, nv1, C, residual form, relu_b, relu); residual "t" a tensor, "bn"
# another BN's value, "" none.  ``wrap``: nvalid full and rows C / 4 > (8192 // 3) 256 per replica, so
# every thread takes a second trip.
ApplyCase = namedtuple("ApplyCase", "name N H W nv1 C res relu_b relu full why")
WRAP_ROWS = ((8192 // 3) * 256) // 17 + 90       # x C / 4 = 17 quads: just past one sweep of the capped grid
APPLY_CASES = [
    ApplyCase("a-n1-c4-t", 1, 1, 1, 1, 4, "t", False, True, False, "one row, one quad"),
    ApplyCase("a-n33-c60-bn", 33, 1, 1, 31, 60, "bn", False, True, False, "a shortcut conv's BN as the residual"),
    ApplyCase("a-n33-c68-bnrelu", 33, 1, 1, 2, 68, "bn", True, False, False, "relu_b: a lazy BN+ReLU residual (the stem's), no output ReLU"),
    ApplyCase("a-n33-c60-none", 33, 1, 1, 32, 60, "", False, False, False, "no residual, no ReLU"),
    ApplyCase("a-hw4-c68-t", 9, 2, 2, 5, 68, "t", False, False, False, "nvalid mid-batch, no ReLU"),
    ApplyCase("a-hw4-c4-bnrelu", 9, 2, 2, 5, 4, "bn", True, True, False, "relu_b and ReLU"),
    ApplyCase("a-n33-c4-none-relu", 33, 1, 1, 1, 4, "", False, True, False, "the stem's BN+ReLU stored"),
    ApplyCase("a-wrap-c68-bnrelu", WRAP_ROWS // 4 + 1, 2, 2, 0, 68, "bn", True, True, True, "past the grid wrap at G = 3"),
]
DyCase = namedtuple("DyCase", "name N H W nv1 C full why")
DY_CASES = [
    DyCase("y-n1-c4", 1, 1, 1, 1, 4, False, "one row"),
    DyCase("y-n33-c60", 33, 1, 1, 31, 60, False, "33 / 31 rows"),
    DyCase("y-hw4-c68", 9, 2, 2, 5, 68, False, "nvalid mid-batch"),
    DyCase("y-wrap-c68", WRAP_ROWS // 4 + 1, 2, 2, 0, 68, True, "past the grid wrap at G = 3"),
]


def ew_nvalid(c):
    return [c.N] * 3 if c.full else [c.N, c.nv1, 0]


def _rand_rows(G, C, g):
    cf = torch.zeros(G, bs.ROWS, C)
    cf[:, bs.SCALE] = (torch.rand(G, C, generator=g) + 0.5) * torch.where(torch.arange(C) % 3 == 2, -1.0, 1.0)
    cf[:, bs.SHIFT] = torch.randn(G, C, generator=g) * 0.3
    cf[:, bs.A] = torch.rand(G, C, generator=g) + 0.5
    cf[:, bs.B], cf[:, bs.K] = torch.randn(G, C, generator=g) * 0.1, torch.randn(G, C, generator=g) * 0.1
    return cf


@functools.lru_cache(maxsize=4)
def ew_inputs(N, H, W, C, nv):
    g = gen(25, N, H * W, C, sum(nv))
    shape = (3, N, H, W, C)
    t = {k: garbage(torch.randn(shape, generator=g), list(nv), g) for k in ("ya", "yb", "res")}
    t["ca"], t["cb"] = _rand_rows(3, C, g), _rand_rows(3, C, g)
    return t


def run_apply(ops, c, dev, who, dt=F32):
    nv = ew_nvalid(c)
    i = ew_inputs(c.N, c.H, c.W, c.C, tuple(nv))
    nvalid = torch.tensor(nv, dtype=I32, device=dev)
    z = torch.zeros(3, c.C, device=dev, dtype=dt)
    p0 = bs.BnParams(z + 1, z.clone(), z.clone(), z + 1, z.clone(), z.clone(), MOMENTUM, EPS)
    sa = make_stat(ops, who, _Bare(p0), i["ca"], False, 3, c.C, dev, dt)
    ya = i["ya"].to(dt).to(dev)
    res = None
    if c.res == "t":
        res = i["res"].to(dt).to(dev)
    elif c.res == "bn":
        res = bs.LazyBN(i["yb"].to(dt).to(dev), make_stat(ops, who, _Bare(p0), i["cb"], c.relu_b, 3, c.C, dev, dt), c.relu_b)
    out = ops.bn_apply(bs.LazyBN(ya, sa, False), res, c.relu, nvalid)
    slot = slot_value(out._dba_amax) if who == HIP else None
    return {"out": out.cpu(), "slot": slot}


class _Bare:
    def __init__(self, p):
        self._p = p

    def bn(self):
        return self._p


def check_apply(c, o, who, ref64=False):
    nv = ew_nvalid(c)
    i = ew_inputs(c.N, c.H, c.W, c.C, tuple(nv))
    for g, n in enumerate(nv):
        if n == 0:
            continue
        want, A = apply_oracle(i["ya"][g, :n], i["ca"][g], i["res"][g, :n] if c.res == "t" else None,
                               i["yb"][g, :n] if c.res == "bn" else None, i["cb"][g], c.relu_b, c.relu)
        got = o["out"][g, :n]
        check_bound(got, want, bound64(A) if ref64 else bound32(APPLY_N, A), "bn_apply", "out", who)
        if o["slot"] is not None:
            check_exact(o["slot"][g:g + 1], got.abs().max().reshape(1), "bn_apply", "max |out| slot", who)
    if o["slot"] is not None and nv[2] == 0:
        assert float(o["slot"][2]) == 0.0, "bn_apply: the empty replica's slot moved"


def run_dy(ops, c, dev, who, dt=F32):
    nv = ew_nvalid(c)
    i = ew_inputs(c.N, c.H, c.W, c.C, tuple(nv))
    nvalid = torch.tensor(nv, dtype=I32, device=dev)
    d, y, coef = i["res"].to(dt).to(dev), i["ya"].to(dt).to(dev), i["ca"].to(dt).to(dev)
    if who == HIP:
        dy, slot = hip_dy(ops, d, y, coef, nvalid)
        via = ops._bnx_dy(bs.LazyGrad(d, y, bs.BnStat(coef, None)), nvalid)      # as conv2d_wgrad reaches it
        for g, n in enumerate(nv):
            check_exact(via[g, :n], dy[g, :n], "bnx_dy", "_bnx_dy vs the raw entry point", who)
        return {"dy": dy.cpu(), "slot": slot_value(slot)}
    return {"dy": ops.lazy_grad_value(bs.LazyGrad(d, y, bs.BnStat(coef, None)), nvalid).cpu(), "slot": None}


def check_dy(c, o, who, ref64=False):
    nv = ew_nvalid(c)
    i = ew_inputs(c.N, c.H, c.W, c.C, tuple(nv))
    for g, n in enumerate(nv):
        if n == 0:
            continue
        want, A = dy_oracle(i["res"][g, :n], i["ya"][g, :n], i["ca"][g])
        got = o["dy"][g, :n]
        check_bound(got, want, bound64(A) if ref64 else bound32(DY_N, A), "bnx_dy", "dy", who)
        if o["slot"] is not None:
            check_exact(o["slot"][g:g + 1], got.abs().max().reshape(1), "bnx_dy", "max |dy| slot", who)


@contextlib.contextmanager
def reference64():
    """ops/reference.py computing in fp64."""
    from dba_mod_amd.ops import reference as R
    old, R.COMPUTE_DTYPE = R.COMPUTE_DTYPE, torch.float64
    try:
        yield R
    finally:
        R.COMPUTE_DTYPE = old

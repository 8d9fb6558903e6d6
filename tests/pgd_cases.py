"""Shared cases, generators, fp64 oracle and checks of ``project_to_ball`` (flat.hip
ballnorm_kernel / ballproj_kernel, ops/reference.py): the CPU reference in test_pgd_cases.py and
the HIP kernels in test_gpu_pgd.py run the same cases against the same oracle with the same bounds
(the conventions of step_kernel_cases.py).

Lengths: ``DIST_CASES`` (the op sizes its grid as dist_loss_grad does: 2048 entries per block, at
most 256 blocks).  Rows hold ``n + PAD`` floats and sit in a flat buffer ``stride`` floats apart,
the first one ``off`` floats past a 16-byte boundary:

* ``aligned``  stride a multiple of 4, off 0 for w and base: every row is all float4;
* ``shifted``  stride a multiple of 4, off 1 for both: every row has a 3-entry head before its
               float4 body;
* ``packed``   stride n + PAD (rows back to back), off 0: the head differs from row to row;
* ``mixed``    off 1 for w and 2 for base: no common float4 alignment, every entry on its own.

Replicas (G = 6): poison at ~2 r (projected), poison at ~0.5 r, benign (trig < 0) at ~2 r, inactive at
~2 r, w == base, one NaN entry in w.  The PAD trailing entries of w differ from base's by ~100 per
entry, so a norm that read one of them would miss its bound by orders of magnitude.

Bounds: the norm accumulates in fp64 (``bound64``); a projected entry is ONE fp32 rounding of the
fp64 value base + s d, whose s differs from the oracle's by fp64 noise: ``bound32(1, |base| + s |d|)``.
"""
import math

import torch

from step_kernel_cases import (DIST_CASES, F64, I32, U32, bound32, bound64, check_bound, check_exact, gen,
                               same_bits)  # noqa: F401  (same_bits: for the tests)

OP = "project_to_ball"
PAD = 37
G = 6
LAYOUTS = ("aligned", "shifted", "packed", "mixed")
PGD_CASES = [(n, lay) for n in DIST_CASES for lay in LAYOUTS]
EXACT_CASES = [(n, lay) for n in DIST_CASES if n >= 16 for lay in LAYOUTS]
TRIG = [0, 2, -1, 1, 0, 3]
ACTIVE = [1, 1, 1, 0, 1, 1]
REL = [2.0, 0.5, 2.0, 2.0, 0.0, 2.0]     # ||w - base|| / r as generated
NAN_ROW = 5
SENTINEL = -1.0                          # norm_out before the call


def pgd_id(c):
    return f"n{c[0]}-{c[1]}"


def radius_of(n):
    """Entries of d are ~0.5 at 2 r: far above the fp32 spacing of the N(0, 1) entries of w."""
    return 0.25 * math.sqrt(n)


def _geometry(n, lay):
    width = n + PAD
    stride = width if lay == "packed" else (width + 3) // 4 * 4
    off_w, off_b = {"aligned": (0, 0), "shifted": (1, 1), "packed": (0, 0), "mixed": (1, 2)}[lay]
    return width, stride, off_w, off_b


def place(rows, off, stride, dev):
    """``rows`` [g, width] as a strided view into a fresh flat buffer on ``dev`` whose first row
    starts ``off`` floats past a 16-byte boundary (the gaps and the lead hold a canary, 7.0)."""
    g, width = rows.shape
    flat = torch.full((off + g * stride + 4,), 7.0, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + g * stride].view(g, stride)[:, :width]
    view.copy_(rows)
    assert view.data_ptr() % 16 == 4 * off and view.stride(0) == stride
    return flat, view


def pgd_inputs(n, lay):
    g = gen(41, n, LAYOUTS.index(lay))
    r = radius_of(n)
    width = n + PAD
    base = torch.randn(G, width, generator=g)
    u = torch.randn(G, width, generator=g).double()
    w = base.clone()
    for k in range(G):
        d = u[k, :n] * (REL[k] * r / float(torch.linalg.vector_norm(u[k, :n])))
        w[k, :n] = (base[k, :n].double() + d).float()
    w[:, n:] = base[:, n:] + 100.0 * torch.randn(G, PAD, generator=g)
    # the decision is far from the boundary, whatever the order of the norm's sum
    for k in range(G):
        nr = float(torch.linalg.vector_norm(w[k, :n].double() - base[k, :n].double()))
        assert nr >= 1.5 * r if REL[k] == 2.0 else nr <= 0.75 * r, (n, k, nr, r)
    assert bool((w[4, :n] == base[4, :n]).all())
    w[NAN_ROW, min(n - 1, 1234)] = float("nan")
    return {"w": w, "base": base, "r": r, "trig": torch.tensor(TRIG, dtype=I32),
            "active": torch.tensor(ACTIVE, dtype=I32)}


def pgd_oracle(w, base, n, trig, active, radius, norm0, count0):
    """(w' fp64, A, norm_out, count, projected mask): what the op is defined to do, in fp64."""
    out, A = w.double().clone(), w.double().abs()
    norm, count = norm0.clone(), count0.clone()
    proj = torch.zeros(w.shape[0], dtype=torch.bool)
    for g in range(w.shape[0]):
        if int(trig[g]) < 0 or int(active[g]) == 0:
            continue
        b = base[g, :n].double()
        d = w[g, :n].double() - b
        nr = math.sqrt(float((d * d).sum()))
        norm[g] = nr
        if math.isfinite(nr) and nr > radius:
            s = radius / nr
            out[g, :n] = b + s * d
            A[g, :n] = b.abs() + s * d.abs()
            count[g] += 1
            proj[g] = True
    return out, A, norm, count, proj


def _call(ops, w, base, n, trig, active, radius, norm, count, rows):
    if rows is None:
        ops.project_to_ball(w, base, n, trig, active, radius, norm, count)
    else:       # one replica alone in a G = 1 launch, at the address it has inside the group
        k = rows
        ops.project_to_ball(w[k:k + 1], base[k:k + 1], n, trig[k:k + 1].contiguous(), active[k:k + 1].contiguous(),
                            radius, norm[k:k + 1], count[k:k + 1])


def _check_untouched(i, fw, fb, w, base, n, lay, proj, who, what):
    """Everything but the first n entries of the projected rows keeps its bits: the other rows, the
    PAD trailing entries of every row, base, and the canaries around the rows."""
    width, stride, off_w, off_b = _geometry(n, lay)
    keep = ~proj
    check_exact(w.cpu()[keep], i["w"][keep], OP, f"w of the rows not projected ({what})", who)
    check_exact(w.cpu()[:, n:], i["w"][:, n:], OP, f"w past n ({what})", who)
    check_exact(base, i["base"], OP, f"base ({what})", who)
    for flat, off in ((fw, off_w), (fb, off_b)):
        mask = torch.ones(flat.numel(), dtype=torch.bool)
        mask[off:off + G * stride].view(G, stride)[:, :width] = False
        c = flat.cpu()[mask]
        check_exact(c, torch.full_like(c, 7.0), OP, f"the buffer around the rows ({what})", who)


def run_pgd(ops, case, dev, who, sel=None):
    """One call, checked against the oracle, then a second call on the projected state.  ``sel``: that
    replica alone in a G = 1 launch (the other replicas' rows are then untouched: checked too)."""
    n, lay = case
    width, stride, off_w, off_b = _geometry(n, lay)
    i = pgd_inputs(n, lay)
    r = i["r"]
    fw, w = place(i["w"], off_w, stride, dev)
    fb, base = place(i["base"], off_b, stride, dev)
    trig, active = i["trig"].to(dev), i["active"].to(dev)
    norm = torch.full((G,), SENTINEL, dtype=F64, device=dev)
    count = torch.zeros(G, dtype=I32, device=dev)
    want, A, norm_w, count_w, proj = pgd_oracle(i["w"], i["base"], n, i["trig"], i["active"], r,
                                                norm.cpu(), count.cpu())
    assert count_w.tolist() == [1, 0, 0, 0, 0, 0] and proj.tolist() == [True] + [False] * 5
    if sel is not None:
        only = torch.zeros(G, dtype=torch.bool)
        only[sel] = True
        proj, count_w = proj & only, torch.where(only, count_w, torch.zeros_like(count_w))
        norm_w = torch.where(only, norm_w, torch.full_like(norm_w, SENTINEL))
    _call(ops, w, base, n, trig, active, r, norm, count, sel)

    fin = torch.isfinite(norm_w)
    assert fin.tolist() == [k != NAN_ROW or (sel is not None and sel != NAN_ROW) for k in range(G)]
    check_bound(norm.cpu()[fin], norm_w[fin], bound64(norm_w[fin].abs()), OP, "norm_out", who)
    assert bool(torch.isnan(norm.cpu()[~fin]).all()), f"{OP} norm_out [{who}]: the NaN replica's norm is not NaN"
    skipped = (i["trig"] < 0) | (i["active"] == 0)
    check_exact(norm.cpu()[skipped], norm_w[skipped], OP, "norm_out of benign / inactive replicas", who)
    check_exact(count, count_w, OP, "count", who)
    if bool(proj[0]):
        check_bound(w.cpu()[0, :n], want[0, :n], bound32(1, A[0, :n]), OP, "projected w", who)
    _check_untouched(i, fw, fb, w, base, n, lay, proj, who, "first call")
    out = {"w": w.cpu().clone(), "norm": norm.cpu().clone(), "count": count.cpu().clone()}

    # a second call on the projected state: one fp32 rounding per entry moved w' by at most
    # 2^-24 |w'_k| each, so ||w' - base|| <= r + 2^-24 ||w'|| (asserted); it may project once more
    if bool(proj[0]):
        d = w.cpu()[0, :n].double() - i["base"][0, :n].double()
        wn = float(torch.linalg.vector_norm(w.cpu()[0, :n].double()))
        assert float(torch.linalg.vector_norm(d)) <= r + U32 * wn, (float(torch.linalg.vector_norm(d)), r, wn)
    _call(ops, w, base, n, trig, active, r, norm, count, sel)
    c2 = count.cpu().tolist()
    assert c2[1:] == [0] * 5 and c2[0] in ((1, 2) if bool(proj[0]) else (0,)), c2
    _check_untouched(i, fw, fb, w, base, n, lay, proj, who, "second call")
    out.update({"w2": w.cpu().clone(), "norm2": norm.cpu().clone(), "count2": count.cpu().clone()})
    return out


def pick(out, g):
    return {k: v[g:g + 1] for k, v in out.items()}


# ---- the exact boundary: base and d small integers, 16 entries of d equal to 1 and the rest 0, so
# sum d^2 = 16 exactly in any order and the norm is exactly 4.  radius = 4 does not project (the
# comparison is strict); the next double below 4 does
def exact_inputs(n, lay):
    assert n >= 16
    g = gen(43, n, LAYOUTS.index(lay))
    base = torch.randint(-3, 4, (2, n + PAD), generator=g).float()
    d = torch.zeros(2, n + PAD)
    pos = sorted({(k * (n - 1)) // 15 for k in range(16)})
    assert len(pos) == 16 and pos[0] == 0 and pos[-1] == n - 1
    d[0, pos] = 1.0
    d[1, [(p + 7) % n for p in pos]] = 1.0
    d[:, n:] = 5.0
    return {"w": base + d, "base": base}


def run_exact(ops, case, dev, who):
    n, lay = case
    width, stride, off_w, off_b = _geometry(n, lay)
    i = exact_inputs(n, lay)
    out = {}
    for tag, radius in (("eq", 4.0), ("below", math.nextafter(4.0, 0.0))):
        _, w = place(i["w"], off_w, stride, dev)
        _, base = place(i["base"], off_b, stride, dev)
        one = torch.ones(2, dtype=I32, device=dev)
        norm = torch.full((2,), SENTINEL, dtype=F64, device=dev)
        count = torch.zeros(2, dtype=I32, device=dev)
        ops.project_to_ball(w, base, n, one, one, radius, norm, count)
        check_exact(norm, torch.full((2,), 4.0, dtype=F64), OP, f"norm_out, exact case ({tag})", who)
        check_exact(base, i["base"], OP, f"base, exact case ({tag})", who)
        check_exact(w.cpu()[:, n:], i["w"][:, n:], OP, f"w past n, exact case ({tag})", who)
        if tag == "eq":
            check_exact(count, torch.zeros(2, dtype=I32), OP, "count at norm == radius", who)
            check_exact(w, i["w"], OP, "w at norm == radius", who)
        else:
            check_exact(count, torch.ones(2, dtype=I32), OP, "count just above the radius", who)
            b = i["base"][:, :n].double()
            dd = i["w"][:, :n].double() - b
            s = radius / 4.0
            check_bound(w.cpu()[:, :n], b + s * dd, bound32(1, b.abs() + s * dd.abs()), OP,
                        "projected w, exact case", who)
        out.update({f"w_{tag}": w.cpu().clone(), f"count_{tag}": count.cpu().clone()})
    return out

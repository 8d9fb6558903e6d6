"""Shared cases, generators, numpy oracle and checks of the Neurotoxin attacker's two ops,
``neurotoxin_mask`` (nmask.hip) and ``mask_restore`` (flat.hip maskrestore_kernel): the CPU
reference in test_neurotoxin_cases.py and the HIP kernels in test_gpu_neurotoxin.py run the same
cases against the same oracle.  Everything is exact: every comparison is on bits.

Mask build.  Lengths ``MASK_P``: 1, 63, 64, 65 (the last word's tail), one block's sweep - 1 / + 0 /
+ 1 and the full grid's sweep + 1029 (``NMASK_SWEEP`` coordinates per block and sweep, at most
``NMASK_BLOCKS_MAX`` blocks: nmask.hip's exported constants, which the GPU test compares with these).
For each P, k in {1, P // 2, P - 1, P}, whichever exist.  Key sets:

* ``normal``   w_old ~ N(0, 1), w_new = w_old + N(0, 0.01): u is whatever one fp32 subtraction gives;
* ``equal``    every |u| the same (signs mixed): every key ties, m = P for any k;
* ``tie``      a run of equal |u| (signs mixed) planted across rank k: m > k, exactly the tied kept;
* ``special``  +0, -0, two denormals, +inf, -inf and two quiet NaNs with different payloads among
               normal values (P >= 16).  k = 1 (T = 0, the two zeros tie), k = P - 3 (the two infs
               tie: m = P - 2) and k = P - 2 (the cut between inf and NaN).  No k inside the NaNs:
               IEEE 754 leaves the payload of an arithmetic result to the implementation, so a T
               among the NaN keys is not pinned by the op's definition;
* ``same``     w_new == w_old: every u is +0, T = 0, everything kept.

The oracle ranks with ``np.partition`` on the uint32 keys and packs the words with ``np.packbits``
(little-endian bit order).  The mask buffer holds ``ceil(P / 64)`` words of garbage and one canary
word behind them; the select workspace holds garbage before the first call and is reused, unwiped,
by the calls for the other k.

Restore.  Lengths ``DIST_CASES`` x the four row layouts of pgd_cases.py (same ``PAD``, same
canaries) x mask density 0.95 / 0.5; from 128 entries on, the mask's first 64-group is wholly kept
and its neighbour wholly dropped.  G = 6: poison, poison (a second trigger), benign, inactive, poison
with w == base, poison with one NaN at a dropped entry (restored) and one at a kept entry (stays).
The mask is one argument of the call, so "a poisoning replica under an all-kept mask" is a second
call on the same buffers with the all-kept mask: no bit of w may change, the counters go up again.
"""
import numpy as np
import torch

from pgd_cases import ACTIVE, G, LAYOUTS, PAD, TRIG, _geometry, place
from step_kernel_cases import DIST_CASES, I32, check_exact, gen, same_bits  # noqa: F401

OP_MASK, OP_RESTORE = "neurotoxin_mask", "mask_restore"
NMASK_SWEEP, NMASK_BLOCKS_MAX = 256, 1024
MASK_P = [1, 63, 64, 65, NMASK_SWEEP - 1, NMASK_SWEEP, NMASK_SWEEP + 1, NMASK_SWEEP * NMASK_BLOCKS_MAX + 1029]
KEY_SETS = ("normal", "equal", "tie", "special", "same")
MASK_CASES = [(P, ks) for P in MASK_P for ks in KEY_SETS if ks != "special" or P >= 16]
CANARY = 0x5A5A5A5A5A5A5A5A
GARBAGE = 0x3333333333333333
INF_KEY = 0x7F800000
NANS = (0x7FC00001, 0xFFC12345)
DENSITIES = (0.95, 0.5)
RESTORE_CASES = [(n, lay, d) for n in DIST_CASES for lay in LAYOUTS for d in DENSITIES]
GATED = [t >= 0 and a != 0 for t, a in zip(TRIG, ACTIVE)]
NAN_ROW = 5


def mask_id(c):
    return f"P{c[0]}-{c[1]}"


def restore_id(c):
    return f"n{c[0]}-{c[1]}-d{c[2]}"


def ks_of(P, keyset):
    if keyset == "special":
        return [1, P - 3, P - 2]
    return sorted({k for k in (1, P // 2, P - 1, P) if 1 <= k <= P})


def n_words(P):
    return (P + 63) // 64


def _f32_of_bits(b):
    return torch.from_numpy(np.array(b, dtype=np.uint32).view(np.float32).copy())


# ------------------------------------------------------------------------------ mask build
def mask_inputs(P, keyset, k):
    """(w_new, w_old) fp32 [P + 5]; the 5 entries past P hold values that would change T if ranked."""
    g = gen(51, P, KEY_SETS.index(keyset), k if keyset == "tie" else 0)
    n = P + 5
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    if keyset == "normal":
        w_old = torch.randn(n, generator=g)
        w_new = w_old + 0.01 * torch.randn(n, generator=g)
    elif keyset == "same":
        w_old = torch.randn(n, generator=g)
        w_new = w_old.clone()
    else:
        w_old = torch.zeros(n)
        u = torch.randn(n, generator=g)
        if keyset == "equal":
            u = 0.37 * sign
        elif keyset == "tie":
            order = torch.argsort(u[:P].abs())
            run = order[max(0, k - 3):min(P, k + 2)]
            u[run] = u[order[k - 1]].abs() * sign[run]
        else:
            pos = [(i * (P - 1)) // 7 for i in range(8)]
            assert len(set(pos)) == 8
            u[pos] = torch.cat([_f32_of_bits([0x00000000, 0x80000000, 0x00000001, 0x80001234, 0x7F800000,
                                              0xFF800000]), _f32_of_bits(list(NANS))])
        w_new = u
    if keyset != "same":
        w_new[P:] = 0.0          # |u| = |w_old| or 0 past P: not the ranked values
        w_old[P:] = 0.0
    return w_new.contiguous(), w_old.contiguous()


def mask_oracle(w_new, w_old, P, k):
    """(words int64 [ceil(P / 64)], T, m)."""
    u = w_new[:P].numpy() - w_old[:P].numpy()
    assert u.dtype == np.float32
    key = u.view(np.uint32) & np.uint32(0x7FFFFFFF)
    T = int(np.partition(key, k - 1)[k - 1])
    keep = key <= T
    bits = np.zeros(n_words(P) * 64, dtype=np.uint8)
    bits[:P] = keep
    words = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64).view(np.int64)
    return torch.from_numpy(words.copy()), T, int(keep.sum())


def run_mask(ops, case, dev, who, make_ws=None):
    """Every k of the case, one after the other on one mask buffer and one workspace."""
    P, keyset = case
    nw = n_words(P)
    ws = None
    if make_ws is not None:
        ws = make_ws(dev)
        ws.fill_(GARBAGE)
    out = {}
    for k in ks_of(P, keyset):
        w_new, w_old = mask_inputs(P, keyset, k)
        want, T, m = mask_oracle(w_new, w_old, P, k)
        assert m >= k
        if keyset in ("equal", "same"):
            assert m == P and (keyset == "equal" or T == 0)
        elif keyset == "tie":
            assert m == min(P, k + 2) and (m > k or k == P), (P, k, m)
        elif keyset == "special":
            assert (T, m) == {1: (0, 2), P - 3: (INF_KEY, P - 2), P - 2: (INF_KEY, P - 2)}[k], (k, T, m)
        buf = torch.full((nw + 1,), GARBAGE, dtype=torch.int64)
        buf[nw] = CANARY
        buf = buf.to(dev)
        a, b = w_new.to(dev), w_old.to(dev)
        sel = ops.neurotoxin_mask(a, b, P, k, buf[:nw], ws)
        what = f"{keyset}, P {P}, k {k}"
        assert sel.dtype == torch.int64 and sel.device.type == dev.type and sel.tolist() == [T, m], \
            f"{OP_MASK} (T, m) [{who}] ({what}): got {sel.tolist()} want {[T, m]}"
        check_exact(buf[:nw], want, OP_MASK, f"mask words ({what})", who)
        assert int(buf[nw]) == CANARY, f"{OP_MASK} [{who}] ({what}): the word behind the mask was written"
        if P % 64:
            assert (int(buf[nw - 1]) & 0xFFFFFFFFFFFFFFFF) >> (P % 64) == 0
        check_exact(a, w_new, OP_MASK, f"w_new ({what})", who)
        check_exact(b, w_old, OP_MASK, f"w_old ({what})", who)
        out[f"words{k}"], out[f"sel{k}"] = buf.cpu().clone(), sel.cpu().clone()
    return out


# -------------------------------------------------------------------------------- restore
def pack(keep):
    """bool [n] -> int64 words, little-endian bit order, tail bits 0."""
    n = keep.numel()
    bits = np.zeros(n_words(n) * 64, dtype=np.uint8)
    bits[:n] = keep.numpy()
    return torch.from_numpy(np.packbits(bits, bitorder="little").view("<u8").view(np.int64).copy())


def unpack(words, n):
    """int64 words -> bool [n]."""
    by = words.contiguous().numpy().view(np.uint8)
    return torch.from_numpy(np.unpackbits(by, bitorder="little")[:n].astype(np.bool_))


def random_keep(n, density, g):
    keep = torch.rand(n, generator=g) < density
    if n >= 128:
        keep[:64] = True
        keep[64:128] = False
    return keep


def restore_inputs(n, lay, density):
    g = gen(53, n, LAYOUTS.index(lay), int(density * 100))
    width = n + PAD
    base = torch.randn(G, width, generator=g)
    w = base + 0.1 * torch.randn(G, width, generator=g)
    w[4, :n] = base[4, :n]
    keep = random_keep(n, density, g)
    nan_at = []
    for want_kept, payload in ((False, 0x7FC00055), (True, 0xFFC000AA)):
        idx = (keep == want_kept).nonzero()
        if idx.numel():
            j = int(idx[idx.numel() // 2])
            w[NAN_ROW, j] = _f32_of_bits([payload])[0]
            nan_at.append((j, want_kept))
    return {"w": w, "base": base, "keep": keep, "nan_at": nan_at, "trig": torch.tensor(TRIG, dtype=I32),
            "active": torch.tensor(ACTIVE, dtype=I32)}


def restore_oracle(w, base, n, keep, gated):
    out = w.clone()
    for g in range(w.shape[0]):
        if gated[g]:
            out[g, :n] = torch.from_numpy(np.where(keep.numpy(), w[g, :n].numpy(), base[g, :n].numpy()))
    return out


def _check_around(fw, fb, n, lay, who, what):
    width, stride, off_w, off_b = _geometry(n, lay)
    for flat, off in ((fw, off_w), (fb, off_b)):
        mask = torch.ones(flat.numel(), dtype=torch.bool)
        mask[off:off + G * stride].view(G, stride)[:, :width] = False
        c = flat.cpu()[mask]
        check_exact(c, torch.full_like(c, 7.0), OP_RESTORE, f"the buffer around the rows ({what})", who)


def run_restore(ops, case, dev, who, sel=None):
    """One call under the case's mask, checked against the oracle, then one under the all-kept mask.
    ``sel``: that replica alone in a G = 1 launch (the other rows are then untouched: checked too)."""
    n, lay, density = case
    width, stride, off_w, off_b = _geometry(n, lay)
    i = restore_inputs(n, lay, density)
    fw, w = place(i["w"], off_w, stride, dev)
    fb, base = place(i["base"], off_b, stride, dev)
    trig, active = i["trig"].to(dev), i["active"].to(dev)
    count = torch.full((G,), 3, dtype=I32, device=dev)
    gated = [q and (sel is None or g == sel) for g, q in enumerate(GATED)]
    want = restore_oracle(i["w"], i["base"], n, i["keep"], gated)
    for j, kept in i["nan_at"]:         # the NaN at a dropped entry is gone, the one at a kept entry stays
        if gated[NAN_ROW]:
            assert bool(torch.isnan(want[NAN_ROW, j])) == kept
    out = {}
    for tag, mask in (("mask", pack(i["keep"])), ("allkept", pack(torch.ones(n, dtype=torch.bool)))):
        mask = mask.to(dev)
        keep_mask = mask.clone()
        if sel is None:
            ops.mask_restore(w, base, n, trig, active, mask, count)
        else:       # one replica alone in a G = 1 launch, at the address it has inside the group
            k = sel
            ops.mask_restore(w[k:k + 1], base[k:k + 1], n, trig[k:k + 1].contiguous(), active[k:k + 1].contiguous(),
                             mask, count[k:k + 1])
        check_exact(w, want, OP_RESTORE, f"w ({tag})", who)
        check_exact(base, i["base"], OP_RESTORE, f"base ({tag})", who)
        check_exact(mask, keep_mask, OP_RESTORE, f"the mask words ({tag})", who)
        _check_around(fw, fb, n, lay, who, tag)
        step = 1 if tag == "mask" else 2
        check_exact(count, torch.tensor([3 + step * int(q) for q in gated], dtype=I32), OP_RESTORE, f"count ({tag})",
                    who)
        out[f"w_{tag}"], out[f"count_{tag}"] = w.cpu().clone(), count.cpu().clone()
    return out


def pick(out, g):
    return {k: v[g:g + 1] for k, v in out.items()}

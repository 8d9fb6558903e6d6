"""Case tables, seeded generators, numpy oracles and bounds of the batch-ingest kernels
(csrc/kernels/data.hip: gather_rows, gather_images) and the evaluation BN fold
(csrc/kernels/bn.hip: bn_fold, bn_fold_batch).  test_ingest_cases.py runs the cases through
``ops/reference.py`` on the CPU, test_gpu_ingest.py through the HIP kernels.

Gathers are exact: a copy, or one fp32 multiply ``float32(p) * float32(1 / 255)`` (255 where the
trigger mask stamps), so ``x`` and ``y`` compare bit for bit.  The oracles are plain numpy loops
over groups; only the flip bit (``hash2(flip_seeds[g], b) & 1``) comes from ``ops/rng.py``.

The fold is compared in fp64 with a-priori bounds: ``wf = w * gamma / sqrt(rv + eps)`` is four
fp32 roundings (add, sqrt, divide, multiply); with one more ulp allowed for each of divide and
sqrt, ``|wf - oracle| <= 6 2^-24 |oracle|``.  ``bf = (b0 - rm) s + beta`` adds a subtraction and
an addition: ``(6 + 2) 2^-24 (|b0| s + |rm| s + |beta|)`` with ``s = |gamma| / sqrt(rv + eps)``.
"""
import functools
import struct
from collections import namedtuple

import numpy as np
import torch

import mlp_cases as M
import step_kernel_cases as K
from dba_mod_amd.ops import rng

GATHER_CAP = 8192 * 256          # work items of one sweep of the gather kernels' launch grid
FOLD_CAP = 4096 * 256            # elements of one sweep of bn_fold's grid (per slot)
FOLD_CHUNK, FOLD_BATCH = 2048, 24
INV255 = np.float32(1.0 / 255.0)
TARGET = 2


def _gen(*key):
    return np.random.default_rng(M._mix(*key))


# ------------------------------------------------------------------ group layouts
# Six groups of B = 8 rows hold the small cases' edges:
#   0  -1 at the head, in the middle and at the tail; trigger 0; poison_n = B
#   1  a whole group of -1 (with a trigger and poison_n > 0)
#   2  trig = -1 with poison_n > 0: nothing poisoned
#   3  the last trigger (images: the all-zero mask), poison_n = 1
#   4  trigger 1, poison_n = 0
#   5  a -1 tail of 3; poison_n = 6, one more than the valid rows
SMALL_G, SMALL_B = 6, 8
SMALL_PN = [SMALL_B, 3, 4, 1, 0, 6]


def small_idx(g, n_src):
    idx = g.integers(0, n_src, size=(SMALL_G, SMALL_B)).astype(np.int32)
    idx[0, [0, 3, 7]] = -1
    idx[1] = -1
    idx[5, 5:] = -1
    return idx


def big_idx(g, G, B, n_src):
    """Valid rows but for a few -1; poison_n inside the batch."""
    idx = g.integers(0, n_src, size=(G, B)).astype(np.int32)
    idx[0, 0] = idx[G - 1, B - 1] = idx[G // 2, B // 2] = -1
    return idx


# ------------------------------------------------------------------ gather_rows
RowsCase = namedtuple("RowsCase", "name G B F")
ROWS_CASES = [
    RowsCase("edges", SMALL_G, SMALL_B, 91),
    RowsCase("under-cap", 3, 7681, 91),       # 2 096 913 items: one sweep, the last blocks partly idle
    RowsCase("over-cap", 3, 7685, 91),        # 2 098 005 = cap + 853: a second trip for 853 items
]


@functools.lru_cache(None)
def rows_inputs(name):
    c = {x.name: x for x in ROWS_CASES}[name]
    g = _gen(1, c.G, c.B, c.F)
    n = 50
    src = g.standard_normal((n, c.F)).astype(np.float32)
    labels = g.integers(0, 9, n).astype(np.int32)
    if name == "edges":
        idx, trig, pn = small_idx(g, n), np.array([0, 1, -1, 1, 1, 0], np.int32), np.array(SMALL_PN, np.int32)
    else:
        idx, trig, pn = big_idx(g, c.G, c.B, n), np.array([0, -1, 1], np.int32), np.array([c.B, 5, c.B - 1], np.int32)
    return {"src": src, "labels": labels, "idx": idx, "cols": M.TRIG_COLS, "vals": M.TRIG_VALS, "trig": trig, "pn": pn}


def rows_oracle(src, labels, idx, cols, vals, trig, pn):
    G, B = idx.shape
    x = np.zeros((G, B, src.shape[1]), dtype=np.float32)
    y = np.full((G, B), -1, dtype=np.int32)
    for g in range(G):
        v = idx[g] >= 0
        x[g, v] = src[idx[g, v]]
        y[g, v] = labels[idx[g, v]]
        if trig[g] >= 0:
            pb = v & (np.arange(B) < pn[g])
            for c, val in zip(cols[trig[g]], vals[trig[g]]):    # table order: the last duplicate wins
                if c >= 0:
                    x[g, pb, c] = val
            y[g, pb] = TARGET
    return x, y


@functools.lru_cache(None)
def rows_expected(name):
    return rows_oracle(**rows_inputs(name))


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sel(i, sel, keys):
    return i if sel is None else {k: (v[sel:sel + 1] if k in keys and v is not None else v) for k, v in i.items()}


def run_rows(fn, name, dev, who, sel=None):
    """``fn``: ops.*.gather_rows.  ``sel``: that group alone (G = 1)."""
    i = _sel(rows_inputs(name), sel, ("idx", "trig", "pn"))
    x, y = fn(_dev(i["src"], dev), _dev(i["labels"], dev), _dev(i["idx"], dev), _dev(i["cols"], dev),
              _dev(i["vals"], dev), _dev(i["trig"], dev), _dev(i["pn"], dev), TARGET, torch.float32)
    wx, wy = rows_expected(name)
    s = slice(None) if sel is None else slice(sel, sel + 1)
    K.check_exact(x, torch.from_numpy(wx[s]), f"gather_rows[{name}]", "x", who)
    K.check_exact(y, torch.from_numpy(wy[s]), f"gather_rows[{name}]", "y", who)
    return {"x": x, "y": y}


# ------------------------------------------------------------------ gather_images
ImgCase = namedtuple("ImgCase", "name G B H W C flip")
IMG_CASES = [ImgCase(f"{n}-{'flip' if f else 'noflip'}", SMALL_G, SMALL_B, h, w, c, f)
             for (n, h, w, c) in (("28x28x1", 28, 28, 1), ("32x32x3", 32, 32, 3), ("6x7x3", 6, 7, 3)) for f in (True, False)]
IMG_CASES += [
    ImgCase("under-cap", 2, 1337, 28, 28, 1, True),     # 2 096 416 items
    ImgCase("over-cap", 3, 705, 32, 31, 3, True),       # 2 098 080 = cap + 928, odd width
]
IMG_BY_NAME = {c.name: c for c in IMG_CASES}


def img_masks(H, W, g):
    """0: row 0, the last row, column 0 and the last column touched (in output coordinates) and
    not mirror-symmetric; 1: random; 2: all zero."""
    m = np.zeros((3, H, W), dtype=np.uint8)
    m[0, 0, :W // 2] = 1
    m[0, H - 1, W - 1] = 1
    m[0, 1:H // 2, 0] = 1
    m[0, H // 2, W - 2:] = 1
    m[1] = g.integers(0, 2, (H, W))
    return m


@functools.lru_cache(None)
def img_inputs(name):
    c = IMG_BY_NAME[name]
    g = _gen(2, c.G, c.B, c.H, c.W, c.C)
    n = 40
    src = g.integers(0, 256, (n, c.H, c.W, c.C)).astype(np.uint8)
    src[0, 0, 0, 0], src[1, 0, 0, 0] = 0, 255
    labels = g.integers(0, 10, n).astype(np.int32)
    if c.G == SMALL_G:
        idx, trig, pn = small_idx(g, n), np.array([0, 1, -1, 2, 1, 0], np.int32), np.array(SMALL_PN, np.int32)
    else:
        idx = big_idx(g, c.G, c.B, n)
        trig, pn = np.array([0, -1, 1][:c.G], np.int32), np.array([c.B, 5, c.B - 1][:c.G], np.int32)
    seeds = g.integers(-2 ** 31, 2 ** 31, c.G).astype(np.int32) if c.flip else None
    return {"src": src, "labels": labels, "idx": idx, "masks": img_masks(c.H, c.W, g), "trig": trig, "pn": pn,
            "seeds": seeds}


def flip_bits(seeds, B):
    ctr = torch.arange(B, dtype=torch.int64)[None, :]
    return (rng.hash2(torch.from_numpy(seeds).to(torch.int64)[:, None], ctr) & 1).numpy().astype(bool)


def images_oracle(src, labels, idx, masks, trig, pn, seeds):
    G, B = idx.shape
    _, H, W, C = src.shape
    x = np.zeros((G, B, H, W, C), dtype=np.float32)
    y = np.full((G, B), -1, dtype=np.int32)
    flip = flip_bits(seeds, B) if seeds is not None else np.zeros((G, B), dtype=bool)
    for g in range(G):
        for b in range(B):
            s = idx[g, b]
            if s < 0:
                continue
            img = src[s][:, ::-1] if flip[g, b] else src[s]
            v = img.astype(np.float32)
            pois = trig[g] >= 0 and b < pn[g]
            if pois:
                v[masks[trig[g]] != 0] = np.float32(255)      # the mask is in output coordinates
            x[g, b] = v * INV255
            y[g, b] = TARGET if pois else labels[s]
    return x, y


@functools.lru_cache(None)
def img_expected(name):
    return images_oracle(**img_inputs(name))


def run_images(fn, name, dev, who, sel=None):
    i = _sel(img_inputs(name), sel, ("idx", "trig", "pn", "seeds"))
    x, y = fn(_dev(i["src"], dev), _dev(i["labels"], dev), _dev(i["idx"], dev), _dev(i["masks"], dev),
              _dev(i["trig"], dev), _dev(i["pn"], dev), TARGET, _dev(i["seeds"], dev), torch.float32)
    wx, wy = img_expected(name)
    s = slice(None) if sel is None else slice(sel, sel + 1)
    K.check_exact(x, torch.from_numpy(wx[s]), f"gather_images[{name}]", "x", who)
    K.check_exact(y, torch.from_numpy(wy[s]), f"gather_images[{name}]", "y", who)
    return {"x": x, "y": y}


# ------------------------------------------------------------------ bn_fold
EPS = 1e-5
FoldCase = namedtuple("FoldCase", "name slots Cout K bias")
FOLD_CASES = [
    FoldCase("64x288-bias", 3, 64, 288, True),
    FoldCase("64x288", 3, 64, 288, False),
    FoldCase("K1-bias", 3, 37, 1, True),
    FoldCase("Cout1-bias", 3, 1, 50, True),
    FoldCase("Cout1", 3, 1, 50, False),
    FoldCase("over-cap-bias", 2, 257, 4099, True),     # 1 053 443 = cap + 4867 per slot: a second trip
]
FOLD_BY_NAME = {c.name: c for c in FOLD_CASES}
RV_EDGES = (0.0, 1e-12, 1e6)


def fold_state(slots, convs, key, dev=None):
    """One flat state [slots, S]; per conv (Cout, K): w, conv bias, gamma, beta, rm, rv as strided
    views of it.  rv is 0.5 .. 1.5 but for 0, 1e-12 and 1e6 on the first channels (Cout = 1: one
    per slot); gamma is of both signs, 0 on channel 3."""
    g = _gen(3, slots, key, *[a * 7919 + b for a, b in convs])
    S = sum(co * k + 5 * co for co, k in convs) + 7
    st = g.standard_normal((slots, S)).astype(np.float32)
    offs, o = [], 0
    for co, k in convs:
        offs.append(o)
        r = o + co * k + 4 * co
        st[:, r:r + co] = (0.5 + g.random((slots, co))).astype(np.float32)
        for j, e in enumerate(RV_EDGES):
            if co > j:
                st[:, r + j] = e
            elif co == 1 and j < slots:
                st[j, r] = e
        if co > 3:
            st[:, o + co * k + co + 3] = 0.0
        o += co * k + 5 * co
    t = torch.from_numpy(st)
    t = t if dev is None else t.to(dev)
    out = []
    for (co, k), o in zip(convs, offs):
        w = t[:, o:o + co * k].view(slots, co, 1, 1, k)
        cb, gamma, beta, rm, rv = (t[:, o + co * k + i * co:o + co * k + (i + 1) * co] for i in range(5))
        out.append({"w": w, "cb": cb, "gamma": gamma, "beta": beta, "rm": rm, "rv": rv})
    return out


def fold_oracle(p, bias):
    """numpy fp64: (wf, bf, bound of wf, bound of bf); eps as the fp32 the kernel receives."""
    d = {k: v.detach().cpu().double().numpy() for k, v in p.items()}
    s = d["gamma"] / np.sqrt(d["rv"] + K.f32(EPS))
    wf = d["w"] * s[:, :, None, None, None]
    b0 = d["cb"] if bias else np.zeros_like(s)
    bf = (b0 - d["rm"]) * s + d["beta"]
    return (torch.from_numpy(wf), torch.from_numpy(bf), torch.from_numpy(6 * K.U32 * np.abs(wf)),
            torch.from_numpy(8 * K.U32 * (np.abs(b0) * np.abs(s) + np.abs(d["rm"]) * np.abs(s) + np.abs(d["beta"]))))


def amax_value(am, slot):
    """The float a folded operand-max slot holds."""
    return struct.unpack("<f", struct.pack("<i", int(am[:, slot].max().item())))[0]


def run_fold(fn, name, dev, who):
    c = FOLD_BY_NAME[name]
    p = fold_state(c.slots, [(c.Cout, c.K)], 0, dev)[0]
    assert p["gamma"].stride(0) > c.Cout and not p["w"].is_contiguous() or c.slots == 1
    wf, bf = fn(p["w"], p["cb"] if c.bias else None, p["gamma"], p["beta"], p["rm"], p["rv"], EPS, torch.float32)
    wwf, wbf, bw, bb = fold_oracle(p, c.bias)
    assert wf.dtype == torch.float32 and tuple(wf.shape) == tuple(p["w"].shape) and tuple(bf.shape) == (c.slots, c.Cout)
    K.check_bound(wf, wwf, bw, "bn_fold", "wf", who)
    K.check_bound(bf, wbf, bb, "bn_fold", "bf", who)
    return wf, bf


# bn_fold_batch: 1, 24 and 25 descriptors (24 per launch); element counts around the 2048-element
# block chunk among them
BATCH_SHAPES = [(23, 89), (64, 32), (3, 683), (8, 5), (40, 129)]      # 2047, 2048, 2049, 40, 5160
BATCH_N = [1, 24, 25]


def batch_convs(n):
    return [BATCH_SHAPES[(i + (1 if n == 1 else 0)) % len(BATCH_SHAPES)] for i in range(n)]

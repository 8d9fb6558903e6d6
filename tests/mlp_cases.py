"""Case tables, seeded generators, the numpy oracle and the bounds of the persistent LoanNet
trainer's tests (csrc/kernels/mlp.hip): test_mlp_cases.py checks cases and oracle on the CPU,
test_gpu_mlp_kernel.py runs the kernel through ``ops.hip.mlp_train`` on hand-built step tables.

A case is a tuple of clients (the kernel runs one workgroup per client and clients never
interact, so the oracle runs one client at a time) plus the launch's scalars.  A client is a
tuple of active steps, contiguous from step 0 as ``pack_steps`` makes them.

The oracle (``run_client``) does literally what a LoanNet step is defined to do, in the dtype it
is given: fp64 is the reference; the fp32 run only measures what fp32 arithmetic costs on these
inputs (``E32``), which scales the kernel's bound:

    |kernel - oracle64| <= 32 E32 + 2^-24 max|p|

element-wise, per parameter tensor, for the parameter update (state after - state before), the
momentum and the FoolsGold sums.  ``E32`` is that tensor's max |oracle32 - oracle64| of the case;
32 = 6.4 (the loss kernel's measured dlogits error over the fp32 reference's, through ``__expf`` /
``__logf``: docs/ARCHITECTURE.md §6.2) x 5 (the MFMA's k order against numpy's); the last term is
the rounding of the stored fp32 parameter.

Conditions on the inputs (``build`` searches generator attempts until they hold, per client;
test_mlp_cases.py asserts them for every client of every case): every dropout-kept
pre-activation of a valid row and every valid row's top-two logit gap is at least
``max(1e-5, 16 max|z32 - z64|)`` in every step, so no ReLU decision and no argmax can differ
between an fp32 evaluation and the oracle: masks and correct counts are exact.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import step_kernel_cases as K
from dba_mod_amd.models.spec import get_spec
from dba_mod_amd.ops import rng

B, F, H1, H2, C = 64, 91, 46, 23, 9
P = 5760
TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3")
OFFS = {"w1": 0, "b1": 4224, "w2": 4288, "b2": 5376, "w3": 5440, "b3": 5696}
SHAPES = {"w1": (H1, F), "b1": (H1,), "w2": (H2, H1), "b2": (H2,), "w3": (C, H2), "b3": (C,)}
LAYERS = ("layer1.0.weight", "layer1.0.bias", "layer2.0.weight", "layer2.0.bias", "layer3.0.weight", "layer3.0.bias")
QUANT = ("update", "mom", "fg")
FACTOR = 32.0
SENT_STATE, SENT_MOM, SENT_FG, SENT_WIDE = -7.25, 3.5, -1.125, 9.75   # padding floats / columns >= P
WIDE = 64                                                               # extra state columns of a wide case

NROWS = 300            # clean source rows 1 .. NROWS
NAN_ROW = 0            # one NaN feature: indexed by the NaN test only, but it is the row a kernel loads for
                       # a clamped -1 index, so a padded row that is not zeroed puts a NaN into W1's gradient
TARGET = 7
# two feature triggers, K = 3: a -1 column (skipped), columns 0 and 90; a duplicated column (the
# last one wins); values far outside the rows' [0, 1)
TRIG_COLS = np.array([[0, -1, 90], [7, 7, 45]], dtype=np.int32)
TRIG_VALS = np.array([[10.0, 55.0, 80.0], [10.0, 80.0, 5.5]], dtype=np.float32)

ENTRY = np.zeros(P, dtype=bool)
for _n in TENSORS:
    ENTRY[OFFS[_n]:OFFS[_n] + int(np.prod(SHAPES[_n]))] = True


def sl(name):
    return slice(OFFS[name], OFFS[name] + int(np.prod(SHAPES[name])))


Step = namedtuple("Step", "nvalid poison_n trig first slot lr")
Client = namedtuple("Client", "steps mom0")
Case = namedtuple("Case", "name clients momentum wd max_slots T wide stats0")


def step(nvalid=B, poison_n=0, trig=-1, first=0, slot=0, lr=0.1):
    return Step(nvalid, poison_n, trig, first, slot, lr)


def client(*steps, mom0=False, first0=True):
    """Active steps of one client; ``first0`` sets the fresh-optimizer flag of step 0."""
    steps = list(steps)
    if steps and first0:
        steps[0] = steps[0]._replace(first=1)
    return Client(tuple(steps), mom0)


def case(name, clients, momentum=0.9, wd=5e-4, max_slots=1, T=None, wide=False, stats0=False):
    T = max(len(c.steps) for c in clients) if T is None else T
    return Case(name, tuple(clients), momentum, wd, max_slots, T, wide, stats0)


S4 = (step(),) * 4
CASES = [
    # (a) full batches, no poison, first at step 0
    case("full", [client(*S4), client(*S4), client(*S4)]),
    # (b) short batches with -1 tails, different per client in the same step
    case("nvalid", [client(step(63), step(1)), client(step(33), step(64)), client(step(32), step(33))]),
    # (c) poison_n 0 / 1 / 63 / 64 / beyond nvalid, trig = -1 with poison_n > 0, both trigger rows
    case("poison", [
        client(step(poison_n=0, trig=0, lr=0.01), step(poison_n=1, trig=0, lr=0.01), step(poison_n=63, trig=1, lr=0.01)),
        client(step(poison_n=64, trig=1, lr=0.01), step(33, poison_n=40, trig=0, lr=0.01),
               step(poison_n=10, trig=-1, lr=0.01)),
        client(step(poison_n=64, trig=0, lr=0.01), step(poison_n=1, trig=1, lr=0.01),
               step(poison_n=63, trig=-1, lr=0.01))]),
    # (d) a fresh optimizer again at step 2, on a non-zero buffer, for client 1 only
    case("first-again", [client(*S4), client(step(), step(), step(first=1), step()), client(*S4)]),
    # (e) non-zero momentum at the start without the first flag, wd = 0, lr per step and client
    case("mom0-wd0", [client(step(lr=0.1), step(lr=0.0), step(lr=0.03), mom0=True, first0=False),
                      client(step(lr=0.05), step(lr=0.2), step(lr=0.01), mom0=True, first0=False),
                      client(step(lr=0.0), step(lr=0.07), step(lr=0.1), mom0=True, first0=False)], wd=0.0),
    case("momentum0", [client(*S4[:3]), client(*S4[:3], mom0=True, first0=False), client(*S4[:3])], momentum=0.0),
    # (f) the statistics slot moves from step to step; stats non-zero before the launch
    case("slots", [client(step(slot=0), step(slot=2), step(slot=1), step(slot=1)),
                   client(step(slot=2), step(slot=2), step(slot=0), step(slot=1)),
                   client(step(40, slot=1), step(slot=0), step(7, slot=0), step(slot=2))], max_slots=3, stats0=True),
    # (g) / (h) clients of 4, 2 and 0 active steps; also run in two launches
    case("ragged", [client(*S4), client(step(), step(50)), client()], T=4),
    case("ragged6", [client(*(S4 + S4[:2])), client(step(), step()), client()], T=6),
    # (k) a state wider than P (sentinels beyond P); a poisoned short batch among full ones
    case("wide", [client(step(), step(20, poison_n=5, trig=1, lr=0.01)), client(step(), step()),
                  client(step(9), step())], wide=True),
]
BY_NAME = {c.name: c for c in CASES}
SPLIT_CASES = ("ragged", "ragged6")


def _mix(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(None)
def data():
    """Source rows uniform in [0, 1) and labels; row NAN_ROW has a NaN feature (never indexed by a case)."""
    g = np.random.default_rng(20240)
    rows = g.random((NROWS + 1, F), dtype=np.float32)
    rows[NAN_ROW, 5] = np.nan
    labels = g.integers(0, C, NROWS + 1).astype(np.int32)
    return rows, labels


def gather(rows, labels, idx, poison_n, trig, cols=TRIG_COLS, vals=TRIG_VALS, target=TARGET):
    """One client's batch: ``idx < 0`` gives a zero row with label -1; the first ``poison_n`` rows
    of a client with ``trig >= 0`` get every trigger column >= 0 overwritten in table order (the
    last duplicate wins) and the label ``target``."""
    x = np.zeros((len(idx), rows.shape[1]), dtype=np.float32)
    y = np.full(len(idx), -1, dtype=np.int64)
    for b, s in enumerate(idx):
        if s < 0:
            continue
        x[b] = rows[s]
        y[b] = labels[s]
        if trig >= 0 and b < poison_n:
            for c, v in zip(cols[trig], vals[trig]):
                if c >= 0:
                    x[b, c] = v
            y[b] = target
    return x, y


def keep_mask(seed, salt, width):
    """The dropout keep pattern of one step: element (b, j) has counter b * width + j."""
    ctr = torch.arange(B * width, dtype=torch.int64)
    u = rng.uniform01(rng.salted(int(seed), salt), ctr)
    return (u >= 0.5).numpy().reshape(B, width)


def _views(p):
    return {n: p[sl(n)].reshape(SHAPES[n]) for n in TENSORS}


def run_client(cl, cs, dtype, trace=None):
    """The client's steps in ``dtype``: final parameters, momentum, FoolsGold sums (on top of
    ``fg0``) and the statistics it adds, [3, max_slots] (loss, correct, count).  ``trace``: a list
    that receives each step's intermediates."""
    rows, labels = data()
    dt = np.dtype(dtype).type
    p = cl["state0"][:P].astype(dtype)
    m = cl["mom0"].astype(dtype)
    fg = cl["fg0"].astype(dtype)
    stats = np.zeros((3, cs.max_slots), dtype=np.float64)
    mu, wd = dt(np.float32(cs.momentum)), dt(np.float32(cs.wd))
    two = dt(2)
    for t, st in enumerate(cl["steps"]):
        x32, y = gather(rows, labels, cl["idx"][t], st.poison_n, st.trig)
        x = x32.astype(dtype)
        w = _views(p)
        valid = y >= 0
        k1, k2 = keep_mask(cl["seeds"][t], 0, H1), keep_mask(cl["seeds"][t], 1, H2)
        z1 = x @ w["w1"].T + w["b1"]
        a1 = np.where(k1, two * np.maximum(z1, 0), 0).astype(dtype)
        z2 = a1 @ w["w2"].T + w["b2"]
        a2 = np.where(k2, two * np.maximum(z2, 0), 0).astype(dtype)
        lg = a2 @ w["w3"].T + w["b3"]
        n = max(st.nvalid, 1)
        mx = lg.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(lg - mx).sum(1))
        onehot = np.zeros((B, C), dtype=dtype)
        onehot[np.arange(B)[valid], y[valid]] = 1
        rowloss = np.where(valid, lse - (lg * onehot).sum(1), 0)
        loss = rowloss.astype(np.float64).sum() / n if st.nvalid > 0 else 0.0
        correct = int(((lg.argmax(1) == y) & valid).sum())
        dl = ((np.exp(lg - lse[:, None]) - onehot) * (dt(1) / dt(n))).astype(dtype)
        dl[~valid] = 0
        d2 = np.where(a2 > 0, two * (dl @ w["w3"]), 0).astype(dtype)
        d1 = np.where(a1 > 0, two * (d2 @ w["w2"]), 0).astype(dtype)
        g = np.zeros(P, dtype=dtype)
        for name, v in (("w3", dl.T @ a2), ("b3", dl.sum(0)), ("w2", d2.T @ a1), ("b2", d2.sum(0)),
                        ("w1", d1.T @ x), ("b1", d1.sum(0))):
            g[sl(name)] = v.reshape(-1)
        if trace is not None:
            trace.append({"x": x, "y": y, "valid": valid, "k1": k1, "k2": k2, "z1": z1, "z2": z2, "lg": lg,
                          "g": g.copy(), "p": p.copy(), "n": n, "loss": loss})
        # SGD as ops.reference.sgd_step, on the entries only (the padding floats belong to nobody)
        fg = np.where(ENTRY, fg + g, fg)
        d = g + wd * p
        mn = d if st.first else mu * m + d
        m = np.where(ENTRY, mn, m)
        p = np.where(ENTRY, p - dt(np.float32(st.lr)) * m, p)
        stats[0, st.slot] += loss
        stats[1, st.slot] += correct
        stats[2, st.slot] += st.nvalid
    return {"p": p, "mom": m, "fg": fg, "stats": stats}


def margins(cl, cs):
    """(min |kept pre-activation| of valid rows, min top-two logit gap of valid rows, margin)."""
    t64, t32 = [], []
    run_client(cl, cs, np.float64, t64)
    run_client(cl, cs, np.float32, t32)
    dz, minz, gap = 0.0, np.inf, np.inf
    for a, b in zip(t64, t32):
        v = a["valid"]
        if not v.any():
            continue
        for k in ("z1", "z2", "lg"):
            dz = max(dz, float(np.abs(a[k][v] - b[k][v].astype(np.float64)).max()))
        for z, keep in ((a["z1"], a["k1"]), (a["z2"], a["k2"])):
            minz = min(minz, float(np.abs(z[v][keep[v]]).min()))
        top = np.sort(a["lg"][v], axis=1)
        gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
    return minz, gap, max(1e-5, 16.0 * dz)


def _init_flat(seed):
    with torch.random.fork_rng():
        return get_spec("loan").init_flat(seed).numpy().copy()


def _generate(cs, ci, attempt):
    cl = cs.clients[ci]
    key = _mix(sum(ord(ch) * (i + 1) for i, ch in enumerate(cs.name)), ci, attempt)
    g = np.random.default_rng(key)
    state0 = _init_flat(key)
    assert state0.shape == (P,)
    state0[~ENTRY] = SENT_STATE
    mom0 = np.zeros(P, dtype=np.float32)
    if cl.mom0:
        mom0[ENTRY] = (0.02 * g.standard_normal(int(ENTRY.sum()))).astype(np.float32)
    mom0[~ENTRY] = SENT_MOM
    fg0 = (0.1 * g.standard_normal(P)).astype(np.float32)     # it accumulates: non-zero before the launch
    fg0[~ENTRY] = SENT_FG
    n = len(cl.steps)
    idx = g.integers(1, NROWS + 1, size=(n, B)).astype(np.int32)
    for t, st in enumerate(cl.steps):
        idx[t, st.nvalid:] = -1
    seeds = g.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)   # the kernel reads them as uint32
    return {"steps": cl.steps, "state0": state0, "mom0": mom0, "fg0": fg0, "idx": idx, "seeds": seeds,
            "attempt": attempt}


@functools.lru_cache(None)
def build(name):
    """The case's clients, each from the first generator attempt that meets the conditions."""
    cs = BY_NAME[name]
    out = []
    for ci in range(len(cs.clients)):
        for attempt in range(400):
            cl = _generate(cs, ci, attempt)
            minz, gap, margin = margins(cl, cs)
            if minz >= margin and gap > margin:
                break
        else:
            raise AssertionError(f"{name} client {ci}: no attempt met the input conditions")
        out.append(cl)
    return tuple(out)


@functools.lru_cache(None)
def oracle(name):
    """Per client: the fp64 and fp32 runs."""
    cs = BY_NAME[name]
    return tuple((run_client(cl, cs, np.float64), run_client(cl, cs, np.float32)) for cl in build(name))


def quantities(cl, res):
    """update / mom / fg of one run, in fp64."""
    return {"update": res["p"].astype(np.float64) - cl["state0"][:P].astype(np.float64),
            "mom": res["mom"].astype(np.float64), "fg": res["fg"].astype(np.float64)}


@functools.lru_cache(None)
def e32(name):
    """{(tensor, quantity): max |oracle32 - oracle64| over the case's clients}."""
    out = {}
    for cl, (o64, o32) in zip(build(name), oracle(name)):
        q64, q32 = quantities(cl, o64), quantities(cl, o32)
        for q in QUANT:
            for n in TENSORS:
                out[(n, q)] = max(out.get((n, q), 0.0), float(np.abs(q64[q][sl(n)] - q32[q][sl(n)]).max()))
    return out


def bounds(name):
    """{(tensor, quantity): 32 E32 + 2^-24 max|p|}, p the oracle's final parameter tensor."""
    e = e32(name)
    out = {}
    for n in TENSORS:
        pmax = max(float(np.abs(o64["p"][sl(n)]).max()) for o64, _ in oracle(name))
        for q in QUANT:
            out[(n, q)] = FACTOR * e[(n, q)] + K.U32 * pmax
    return out


# ============================================================================ launch tables
def tables(name, sel=None):
    """Host tensors of a launch of the case (``sel``: that client alone, G = 1)."""
    cs = BY_NAME[name]
    cls = build(name)
    pick = list(range(len(cls))) if sel is None else [sel]
    G, T = len(pick), cs.T
    sched = np.zeros((T, G * B + 8 * G), dtype=np.int32)
    sched[:, :G * B] = -1
    f8 = sched[:, G * B:].reshape(T, 8, G)
    f8[:, 1] = -1
    S = P + (WIDE if cs.wide else 0)
    state = np.full((G, S), SENT_WIDE, dtype=np.float32)
    mom = np.zeros((G, P), dtype=np.float32)
    fg = np.zeros((G, P), dtype=np.float32)
    for g, ci in enumerate(pick):
        cl = cls[ci]
        state[g, :P], mom[g], fg[g] = cl["state0"], cl["mom0"], cl["fg0"]
        for t, st in enumerate(cl["steps"]):
            sched[t, g * B:(g + 1) * B] = cl["idx"][t]
            f8[t, :, g] = (st.poison_n, st.trig, st.first, 1, st.nvalid, st.slot, cl["seeds"][t],
                           np.float32(st.lr).view(np.int32))
    stats = np.zeros((3, G * cs.max_slots), dtype=np.float32)
    if cs.stats0:
        stats[0], stats[1], stats[2] = 1.5, 5.0, 100.0
    rows, labels = data()
    return {"sched": sched, "state": state, "mom": mom, "fg": fg, "stats": stats, "rows": rows, "labels": labels,
            "pick": pick}


def run_kernel(H, name, dev, segments=None, fg=True, sel=None, tab=None, spec=None, Bk=B):
    """The case through ``H.mlp_train`` (one launch per segment); everything back on the host."""
    cs = BY_NAME[name]
    tb = tables(name, sel) if tab is None else tab
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tb.items() if k != "pick"}
    state = t["state"]
    assert not cs.wide or state.stride(0) > P
    nan = torch.zeros(1, device=dev)
    fgt = t["fg"] if fg else None
    rcs = []
    for t0, t1 in (segments or [(0, cs.T)]):
        rcs.append(H.mlp_train(spec or get_spec("loan"), t["sched"], t0, t1, Bk, state, t["mom"], fgt, t["rows"],
                               t["labels"], torch.from_numpy(TRIG_COLS).to(dev), torch.from_numpy(TRIG_VALS).to(dev),
                               TARGET, t["stats"], cs.max_slots, nan, cs.momentum, cs.wd))
    torch.cuda.synchronize()
    return {"state": state.cpu(), "mom": t["mom"].cpu(), "fg": None if fgt is None else fgt.cpu(),
            "stats": t["stats"].cpu(), "nan": nan.cpu(), "rc": rcs}


def client_cols(out, g, max_slots):
    """Client ``g``'s share of a run's outputs (for bitwise comparisons between launches)."""
    return {"state": out["state"][g], "mom": out["mom"][g], "fg": None if out["fg"] is None else out["fg"][g],
            "stats": out["stats"][:, g * max_slots:(g + 1) * max_slots]}


MEASURED = {}   # (tensor, quantity) -> (kernel err, E32 of that case, err / E32, err / bound): the worst case each


def check_oracle(name, out, who="hip", sel=None):
    """A run's outputs against the fp64 oracle: parameters, momentum and FoolsGold sums within the
    bound; sentinels, counts and correct counts exact; the loss slot within 1e-4 (1 + |oracle|)."""
    cs = BY_NAME[name]
    cls, orc, bnd, e = build(name), oracle(name), bounds(name), e32(name)
    pick = list(range(len(cls))) if sel is None else [sel]
    tb = tables(name, sel)
    for g, ci in enumerate(pick):
        cl, o64 = cls[ci], orc[ci][0]
        want = quantities(cl, o64)
        got = {"update": out["state"][g, :P].double().numpy() - cl["state0"][:P].astype(np.float64),
               "mom": out["mom"][g].double().numpy()}
        if out["fg"] is not None:
            got["fg"] = out["fg"][g].double().numpy()
        for q, v in got.items():
            for n in TENSORS:
                err = float(np.abs(v[sl(n)] - want[q][sl(n)]).max())
                old = MEASURED.get((n, q, who), (-1.0, 0.0, 0.0, 0.0))
                if e[(n, q)] > 0 and err / e[(n, q)] > old[2]:
                    MEASURED[(n, q, who)] = (err, e[(n, q)], err / e[(n, q)], err / bnd[(n, q)])
                try:
                    K.check_bound(torch.from_numpy(v[sl(n)]), torch.from_numpy(want[q][sl(n)]), bnd[(n, q)],
                                  "mlp_train", f"{n} {q}", who)
                except AssertionError as ex:
                    raise AssertionError(f"case {name} client {ci} (E32 {e[(n, q)]:.3e}): {ex}") from None
        # padding floats and columns >= P keep their sentinels
        pad = torch.from_numpy(~ENTRY)
        for key, sent in (("state", SENT_STATE), ("mom", SENT_MOM), ("fg", SENT_FG)):
            if out[key] is not None:
                assert bool((out[key][g, :P][pad] == sent).all()), (name, ci, key, "padding floats")
        assert bool((out["state"][g, P:] == SENT_WIDE).all()), (name, ci, "columns >= P")
        ms = cs.max_slots
        st0 = torch.from_numpy(tb["stats"][:, g * ms:(g + 1) * ms]).double()
        st = out["stats"][:, g * ms:(g + 1) * ms].double()
        wst = st0 + torch.from_numpy(o64["stats"])
        K.check_exact(st[2], wst[2], f"mlp_train[{name}]", "stats count", who, bitwise=False)
        K.check_exact(st[1], wst[1], f"mlp_train[{name}]", "stats correct", who, bitwise=False)
        K.check_bound(st[0], wst[0], 1e-4 * (1 + wst[0].abs()), "mlp_train", "statistics loss slot", who)
        if not cl["steps"]:     # nothing to do: every byte as it was
            for key in ("state", "mom", "fg", "stats"):
                if out[key] is not None:
                    ref = tb[key][:, g * ms:(g + 1) * ms] if key == "stats" else tb[key][g]
                    got_b = out[key][:, g * ms:(g + 1) * ms] if key == "stats" else out[key][g]
                    K.check_exact(got_b, torch.from_numpy(np.ascontiguousarray(ref)), f"mlp_train[{name}]",
                                  f"idle client's {key}", who)
    assert float(out["nan"]) == 0.0, (name, "nan_flag on clean input")
    assert all(rc == 0 for rc in out["rc"]), out["rc"]


def report():
    lines = ["| tensor, quantity | kernel: max abs err | E32 | err / E32 | err / bound |", "|---|---|---|---|---|"]
    for n in TENSORS:
        for q in QUANT:
            for (n2, q2, who), (err, e, r, rb) in sorted(MEASURED.items()):
                if (n2, q2) == (n, q):
                    lines.append(f"| `mlp_train` {n} {q} [{who}] | {err:.2e} | {e:.2e} | {r:.2f} | {rb:.3f} |")
    return "\n".join(lines)

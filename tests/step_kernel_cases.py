"""Shared case tables, seeded generators, fp64 oracles and bounds of the per-step kernel tests
(loss.hip, optim.hip, elementwise.hip, flat.hip): the CPU reference ops in
test_step_kernel_cases.py and the HIP kernels in test_gpu_step_kernels.py run the same cases
against the same oracles with the same bounds.

Every oracle is plain torch-fp64 / numpy on the CPU and does literally what the op is defined to
do.  The ops take their scalar arguments (momentum, weight decay, alpha, gamma, coef, sigma, p) as
fp32, so the oracles round them to fp32 first (``f32``) and are exact from there.

Bounds (every comparison is element-wise, in fp64, never after a downcast):

* exact          integer / bitwise equality;
* ``bound32``    fp32-accumulating outputs: ``|got - oracle| <= (n + 2) 2^-24 A``.  ``n`` is the
                 longest chain of fp32 operations behind one output element (derived next to each
                 case table) and ``A`` the oracle's magnitude: the same expression over the
                 absolute values of its terms.  This is the a-priori bound of ANY evaluation order
                 of a chain of that length ((1 + u)^n - 1 <= (n + 2) u for the n used here; the 2
                 covers the fp32 rounding of a scalar argument and of the stored result), so it
                 needs no measurement;
* ``bound64``    fp64-accumulating outputs: ``1e-12 A``, more than ten times the a-priori fp64
                 bound at these lengths (n 2^-53 with n <= 4.2e6 / 256 terms per thread chain);
* through ``__expf`` / ``__logf``: the project's ceilings, loss ``1e-4 (1 + |oracle|)``, fp64
  loss ``1e-4 + 1e-6 |oracle|``, dlogits ``1e-6 + 1e-5 |oracle|`` (``E_DL``); the head's
  gradients take the dlogits bound propagated through the linear magnitude plus the ``bound32``
  of their own chain.

``check_*`` record the largest observed error and error / bound per (op, output, implementation)
in ``ERRORS`` (``report()`` formats the table of docs/ARCHITECTURE.md §6.2).
"""
import itertools
import math

import numpy as np
import torch

from dba_mod_amd.ops import rng

U32 = 2.0 ** -24
F64 = torch.float64
I32 = torch.int32

ERRORS = {}


def f32(v):
    """A Python scalar as the op sees it (rounded to fp32)."""
    return float(np.float32(v))


def gen(*key):
    """A generator seeded by the case's key (a fixed integer mix, the same in every process)."""
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def bound32(n, A):
    return (n + 2) * U32 * A


def bound64(A):
    return 1e-12 * A


def _note(op, what, who, err, ratio):
    e = ERRORS.setdefault((op, what), {})
    old = e.get(who, (0.0, 0.0))
    e[who] = (max(old[0], err), max(old[1], ratio))


def report():
    lines = ["| op | output | implementation | max abs err | max err / bound |", "|---|---|---|---|---|"]
    for (op, what), e in sorted(ERRORS.items()):
        for who, (err, ratio) in sorted(e.items()):
            lines.append(f"| {op} | {what} | {who} | {err:.3e} | {ratio:.3g} |")
    return "\n".join(lines)


def check_bound(got, want, bound, op, what, who):
    """|got - want| <= bound element-wise in fp64 (bound: tensor or scalar)."""
    g = got.detach().cpu().to(F64)
    w = want.to(F64)
    assert g.shape == w.shape, f"{op} {what} [{who}]: shape {tuple(g.shape)} != {tuple(w.shape)}"
    assert bool(torch.isfinite(g).all()), f"{op} {what} [{who}]: non-finite output"
    err = (g - w).abs()
    b = torch.as_tensor(bound, dtype=F64).expand_as(err)
    if err.numel() == 0:
        return
    ratio = torch.where(err > 0, err / b.clamp(min=1e-300), torch.zeros_like(err))
    _note(op, what, who, err.max().item(), ratio.max().item())
    bad = err > b
    if bool(bad.any()):
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(
            f"{op} {what} [{who}]: {int(bad.sum())}/{err.numel()} elements beyond the bound; worst at flat index "
            f"{i}: got {g.reshape(-1)[i].item():.9e} want {w.reshape(-1)[i].item():.9e} err "
            f"{err.reshape(-1)[i].item():.3e} bound {b.reshape(-1)[i].item():.3e}")


def bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def check_exact(got, want, op, what, who, bitwise=True):
    """Equality: of the bit patterns (``bitwise``) or of the values (-0.0 == 0.0)."""
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.shape == w.shape and g.dtype == w.dtype, (op, what, who, g.shape, w.shape, g.dtype, w.dtype)
    ne = (bits(g) != bits(w)) if bitwise else (g != w)
    if bool(ne.any()):
        i = int(ne.reshape(-1).nonzero()[0])
        raise AssertionError(f"{op} {what} [{who}]: {int(ne.sum())}/{g.numel()} elements differ; first at flat index "
                             f"{i}: got {g.reshape(-1)[i].item()!r} want {w.reshape(-1)[i].item()!r}")


def same_bits(a, b, what):
    """Two runs' outputs (dicts of tensors / None) agree bit for bit."""
    assert a.keys() == b.keys()
    for k in a:
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            check_exact(a[k], b[k], what, k, "invariant")


def pick(out, g):
    """Replica ``g`` of every per-replica output of a run."""
    return {k: (None if v is None else v[g:g + 1]) for k, v in out.items()}


# ===================================================================== softmax cross-entropy
# xent_kernel: L = 1 lane per row for C <= 16, 16 up to 512, 64 beyond; one slice for B <= 256,
# 32-row slices + the finish launch above.  Classes / rows on either side of each threshold; 257
# and 289 leave a last slice of one row.  Every C meets a B of each launch form and every B a C of
# each lane layout (a Latin arrangement of 27 of the 81 pairs); mean x want_grad cover all four
# combinations in both launch forms.
XENT_C = [[1, 2, 16], [17, 31, 200], [513, 577, 512]]
XENT_B = [[1, 15, 16], [17, 255, 256], [257, 288, 289]]
XENT_ROWS = ["randn3", "ties", "equal", "spread"]
XENT_SLICE, XENT_ONE_LAUNCH = 32, 256


def _xent_cases():
    out, idx = [], 0
    for a, r in itertools.product(range(3), range(3)):
        for t in range(3):
            C, B = XENT_C[a][r], XENT_B[t][(a + r + t) % 3]
            i = idx // 3
            out.append((C, B, bool(idx & 1), bool(idx & 2), XENT_ROWS[(i + 2 * t) % 4], ("none", "last")[(i // 2 + t) % 2]))
            idx += 1
    return out


XENT_CASES = _xent_cases()


def xent_id(c):
    C, B, mean, grad, rows, g2 = c
    return f"C{C}-B{B}-{'mean' if mean else 'sum'}-{'grad' if grad else 'nograd'}-{rows}-g2{g2}"


def xent_logits(kind, G, B, C, g):
    """fp32 logits [G, B, C], finite.  ``randn3``: N(0, 9).  ``ties``: the same rounded to
    integers (many exact ties; argmax takes the first maximum).  ``equal``: every row one value.
    ``spread``: one class per row near +3e4 and the others 15 .. 45 (exp partly underflows), 100,
    3e4 or 6e4 below it (exp underflows to zero): a finite spread of +-3e4.  (The row maximum is
    kept at least 13 above the rest: xent_kernel forms lse = max + log(sum) in fp32, so two near-
    equal maxima at |logit| ~ 3e4 would carry ulp(3e4) / 2 ~ 1e-3 of relative error into dlogits;
    training and evaluation logits are O(10), where that term is below 1e-6.)"""
    x = torch.randn(G, B, C, generator=g) * 3
    if kind == "ties":
        x = x.round()
    elif kind == "equal":
        x = (torch.randn(G, B, 1, generator=g) * 3).expand(G, B, C).contiguous()
    elif kind == "spread":
        top = 3e4 + torch.randn(G, B, 1, generator=g) * 3
        lvl = torch.randint(0, 4, (G, B, C), generator=g)
        drop = torch.where(lvl == 0, 15 + 30 * torch.rand(G, B, C, generator=g),
                           torch.where(lvl == 1, torch.full((G, B, C), 100.0),
                                       torch.where(lvl == 2, torch.full((G, B, C), 3e4), torch.full((G, B, C), 6e4))))
        x = top - drop + 0.1 * x
        pos = torch.randint(0, C, (G, B, 1), generator=g)
        x.scatter_(2, pos, top)
    return x.float()


def xent_inputs(case):
    """(logits [3, B, C], labels [3, B] int32, nvalid [3] int32, slot [3] int32, stats [3, 3 * 5]):
    group 0 full; group 1's valid rows end mid-slice (``n1``) and hold scattered -1 labels; group
    2 is all -1 or has its only valid row last.  ``stats`` holds non-zero contents: the loss row
    arbitrary, the count rows multiples of 0.25 (so their sums are exact in fp32)."""
    C, B, mean, grad, rows, g2 = case
    g = gen(1, C, B)
    G = 3
    logits = xent_logits(rows, G, B, C, g)
    labels = torch.randint(0, C, (G, B), generator=g).to(I32)
    n1 = max(1, B - B // 3 - 3)
    labels[1, n1:] = -1
    labels[1, 1:n1:5] = -1
    labels[2] = -1
    if g2 == "last":
        labels[2, B - 1] = int(torch.randint(0, C, (1,), generator=g))
    nvalid = torch.tensor([B, n1, 1 if g2 == "last" else 0], dtype=I32)
    slot = torch.tensor([0, 3, 4], dtype=I32)
    stats = torch.rand(3, G * 5, generator=g) + 0.5
    stats[1:] = torch.randint(1, 256, (2, G * 5), generator=g).float() * 0.25
    return logits, labels, nvalid, slot, stats


def xent_oracle(logits, labels, mean):
    """(loss [G], correct [G] int64, dlogits [G, B, C]) in fp64: log-sum-exp about the row
    maximum, rows with a label < 0 left out, the mean over the group's valid rows (0 for none),
    argmax the first maximum."""
    x = logits.double()
    lab = labels.long()
    valid = lab >= 0
    mx = x.max(-1, keepdim=True).values
    lse = mx.squeeze(-1) + torch.log(torch.exp(x - mx).sum(-1))
    xy = x.gather(-1, lab.clamp(min=0)[..., None]).squeeze(-1)
    nll = torch.where(valid, lse - xy, torch.zeros_like(lse))
    cnt = valid.sum(1)
    div = cnt.clamp(min=1).double()
    loss = nll.sum(1) / div if mean else nll.sum(1)
    pred = torch.from_numpy(np.argmax(x.numpy(), axis=-1))       # first occurrence of the maximum
    correct = ((pred == lab) & valid).sum(1)
    dl = torch.exp(x - lse[..., None])
    dl.scatter_add_(2, lab.clamp(min=0)[..., None], -torch.ones_like(dl[..., :1]))
    dl = torch.where(valid[..., None], dl, torch.zeros_like(dl))
    if mean:
        dl = dl / div[:, None, None]
    return loss, correct, dl


def stats_oracle(stats, slot, loss, correct, nvalid):
    out = stats.double().clone()
    ms = stats.shape[1] // loss.shape[0]
    for g in range(loss.shape[0]):
        col = g * ms + int(slot[g])
        out[0, col] += loss[g]
        out[1, col] += float(correct[g])
        out[2, col] += float(nvalid[g])
    return out


def loss_bound(want):
    return 1e-4 + 1e-4 * want.abs()


def loss64_bound(want):
    return 1e-4 + 1e-6 * want.abs()


def E_DL(want):
    return 1e-6 + 1e-5 * want.abs()


def check_stats(got, prior, want, lbound, loss, op, who):
    """The loss slots within the loss bound plus the fp32 rounding of the addition; the count
    slots exactly; every other column bit for bit as before."""
    touched = (want != prior.double()).any(0)
    b0 = lbound.max().item() + 2 * U32 * (prior[0].double().abs() + loss.abs().max().item())
    check_bound(got[0], want[0], b0, op, "stats loss slot", who)
    check_exact(got[1:].double(), want[1:], op, "stats count slots", who, bitwise=False)
    check_exact(got[:, ~touched], prior[:, ~touched], op, "stats other columns", who)


def run_xent(ops, case, dev, who, sel=None):
    C, B, mean, grad, rows, g2 = case
    logits, labels, nvalid, slot, stats = xent_inputs(case)
    if sel is not None:
        logits, labels, nvalid, slot = (t[sel:sel + 1].contiguous() for t in (logits, labels, nvalid, slot))
        slot = slot * 0 + 2
        stats = stats[:, :5].contiguous()
    loss_w, corr_w, dl_w = xent_oracle(logits, labels, mean)
    st = stats.clone().to(dev)
    loss, corr, dl = ops.softmax_xent(logits.to(dev), labels.to(dev), mean, grad, st, slot.to(dev), nvalid.to(dev),
                                      grad_dtype=torch.float32)
    assert loss.dtype == torch.float32 or who != "hip"        # (the reference returns its compute dtype)
    check_bound(loss, loss_w, loss_bound(loss_w), "softmax_xent", "loss", who)
    check_exact(corr.cpu().long(), corr_w, "softmax_xent", "correct", who)
    assert (dl is not None) == grad
    if grad:
        check_bound(dl, dl_w, E_DL(dl_w), "softmax_xent", "dlogits", who)
        pad = (labels < 0)[..., None].expand_as(dl_w)
        check_exact(dl.cpu()[pad], torch.zeros(int(pad.sum())), "softmax_xent", "dlogits of padding rows", who,
                    bitwise=False)
    check_stats(st.cpu(), stats, stats_oracle(stats, slot, loss_w, corr_w, nvalid), loss_bound(loss_w), loss_w,
                "softmax_xent", who)
    loss64, corr2, dl2 = ops.softmax_xent(logits.to(dev), labels.to(dev), mean, grad, grad_dtype=torch.float32,
                                          loss_dtype=torch.float64)
    assert loss64.dtype == torch.float64
    check_bound(loss64, loss_w, loss64_bound(loss_w), "softmax_xent", "loss fp64", who)
    check_exact(corr2.cpu().long(), corr_w, "softmax_xent", "correct (fp64 loss)", who)
    return {"loss": loss.cpu(), "correct": corr.cpu(), "dl": None if dl is None else dl.cpu(), "loss64": loss64.cpu(),
            "dl2": None if dl2 is None else dl2.cpu()}


# ================================================================== fused classifier head
# head_rows_kernel: row blocks of 4, pixel loads in batches of 16 up to HW = 64, K <= 16 classes,
# logits by 4 lanes x strided quarters; head_fin_kernel: weight-gradient column blocks of 64, row
# quarters stepping by 16, the bias gradient 16 rows per trip.
# (K, C, N, (H, W), nvalid of replica 1, mean): every K in {1, 2, 10, 16}, C in {4, 60, 64, 68,
# 512} (a partial single column block, exactly one, one + 4 columns, eight), N in {1, 3, 4, 5, 17,
# 64, 256}, HW in {1, 15, 16, 17, 64}; replica 1's nvalid off the row-block grid where N allows.
# nvalid = (N, that value, 0).
HEAD_CASES = [
    (1, 4, 1, (1, 1), 1, True), (2, 60, 3, (3, 5), 2, False), (10, 64, 4, (4, 4), 3, True),
    (16, 68, 5, (1, 17), 3, False), (10, 512, 17, (8, 8), 14, True), (16, 4, 64, (1, 1), 23, False),
    (1, 512, 256, (1, 1), 131, True), (2, 68, 256, (8, 8), 250, False), (10, 60, 64, (17, 1), 62, True),
    (16, 64, 17, (5, 3), 7, False), (2, 512, 4, (1, 17), 2, True), (10, 4, 5, (8, 8), 3, False),
    (16, 60, 256, (4, 4), 255, True), (1, 68, 3, (4, 4), 2, False), (10, 64, 256, (3, 5), 130, True),
]
HEAD_SENTINEL = 777.25


def head_id(c):
    K, C, N, (H, W), nv1, mean = c
    return f"K{K}-C{C}-N{N}-HW{H * W}-nv{nv1}-{'mean' if mean else 'sum'}"


def head_logit_n(HW, C):
    """fp32 chain of one logit: the pool (HW - 1 adds, a division), a quarter's C / 4 FMAs, two
    butterfly adds, the bias."""
    return HW + (C + 3) // 4 + 3


def head_oracle(x, W, b, labels, nvalid, mean):
    """fp64 head of the valid rows (row < nvalid, rows at and beyond it carry label -1):
    pooled = mean over pixels, logits = pooled W^T + b, cross-entropy (``xent_oracle``), dW =
    dl^T pooled, db = column sums of dl, dpool = dl W; plus the magnitudes and the bounds."""
    G, N, H, Wd, C = x.shape
    HW, K = H * Wd, W.shape[1]
    xd = x.double().reshape(G, N, HW, C)
    pooled, A_pool = xd.sum(2) / HW, xd.abs().sum(2) / HW
    Wd64, bd = W.double(), b.double()
    z = torch.einsum("gnc,gkc->gnk", pooled, Wd64) + bd[:, None, :]
    A_z = torch.einsum("gnc,gkc->gnk", A_pool, Wd64.abs()) + bd.abs()[:, None, :]
    rows = torch.arange(N)[None, :] < nvalid.long()[:, None]
    lab = torch.where(rows, labels.long(), torch.full_like(labels.long(), -1))
    loss, correct, dl = xent_oracle(z, lab, mean)
    e_dl = torch.where((lab >= 0)[..., None], E_DL(dl), torch.zeros_like(dl))
    adl = dl.abs()
    nvm = int(nvalid.max())
    o = {"pooled": pooled, "A_pool": A_pool, "z": z, "A_z": A_z, "rows": rows, "loss": loss, "correct": correct,
         "dl": dl, "dW": torch.einsum("gnk,gnc->gkc", dl, pooled), "db": dl.sum(1),
         "dpool": torch.einsum("gnk,gkc->gnc", dl, Wd64)}
    # chains: dW a quarter's rows (FMAs) + two adds over pooled values (HW); db the rows in order;
    # dpool the classes in order
    o["b_dW"] = torch.einsum("gnk,gnc->gkc", e_dl, pooled.abs()) + bound32(
        (nvm + 3) // 4 + 2 + HW, torch.einsum("gnk,gnc->gkc", adl, A_pool))
    o["b_db"] = e_dl.sum(1) + bound32(nvm, adl.sum(1))
    o["b_dpool"] = torch.einsum("gnk,gkc->gnc", e_dl, Wd64.abs()) + bound32(K, torch.einsum("gnk,gkc->gnc", adl, Wd64.abs()))
    o["b_z"] = bound32(head_logit_n(HW, C), A_z)
    return o


def head_gap(o, labels):
    """Smallest (top-2 logit gap) / (bound of the logits) over the valid rows (inf for K = 1)."""
    z = o["z"]
    if z.shape[-1] == 1:
        return math.inf
    top = z.topk(2, dim=-1)
    gap = top.values[..., 0] - top.values[..., 1]
    lim = o["b_z"].max(-1).values
    use = o["rows"] & (labels.long() >= 0)
    return (gap / lim)[use].min().item() if bool(use.any()) else math.inf


def head_inputs(case):
    """x a 16-byte-aligned [3, N, H, W, C] view whose stride(0) exceeds the tensor; W, bias
    slices of [3, S] flat parameter rows and dW, db of sentinel-filled gradient rows, as the
    trainer passes them; labels with -1 inside the valid range and beyond it.  Rows whose top-2
    logit gap is below 100 x the logits' bound are redrawn (so the correct count is compared
    exactly)."""
    K, C, N, (H, Wd), nv1, mean = case
    g = gen(2, K, C, N, H * Wd)
    G, per = 3, N * H * Wd * C
    xbig = torch.zeros(G, per + 12)
    x = xbig[:, 4:4 + per].view(G, N, H, Wd, C)
    x.copy_(torch.randn(G, N, H, Wd, C, generator=g))
    S = K * C + K + 7
    flat = torch.randn(G, S, generator=g)
    W = flat[:, 3:3 + K * C].view(G, K, C)
    W.mul_(2.0 / math.sqrt(C))
    b = flat[:, 4 + K * C:4 + K * C + K]
    nvalid = torch.tensor([N, nv1, 0], dtype=I32)
    labels = torch.randint(0, K, (G, N), generator=g).to(I32)
    labels[:, 2::4] = -1                                       # inside the valid range
    labels = torch.where(torch.arange(N)[None, :] < nvalid.long()[:, None], labels, torch.full_like(labels, -1))
    for _ in range(50):
        o = head_oracle(x, W, b, labels, nvalid, mean)
        if K == 1:
            break
        top = o["z"].topk(2, dim=-1).values
        close = (top[..., 0] - top[..., 1]) < 100 * o["b_z"].max(-1).values
        close &= o["rows"]
        if not bool(close.any()):
            break
        x[close] = torch.randn(int(close.sum()), H, Wd, C, generator=g)
    slot = torch.tensor([1, 0, 4], dtype=I32)
    stats = torch.rand(3, G * 5, generator=g) + 0.5
    stats[1:] = torch.randint(1, 256, (2, G * 5), generator=g).float() * 0.25
    return {"xbig": xbig, "flat": flat, "x": x, "W": W, "b": b, "labels": labels, "nvalid": nvalid, "slot": slot,
            "stats": stats, "S": S, "per": per}


def run_head(head_train, case, dev, who, sel=None):
    """``head_train``: ops.hip.head_train or a composition of reference ops with its signature."""
    K, C, N, (H, Wd), nv1, mean = case
    i = head_inputs(case)
    G, S, per = 3, i["S"], i["per"]
    o = head_oracle(i["x"], i["W"], i["b"], i["labels"], i["nvalid"], mean)
    s = slice(0, G) if sel is None else slice(sel, sel + 1)
    Gs = s.stop - s.start
    xbig, flat = i["xbig"][s].to(dev), i["flat"][s].to(dev)
    gflat = torch.full((Gs, S), HEAD_SENTINEL, device=dev)
    x = xbig[:, 4:4 + per].view(Gs, N, H, Wd, C)
    W, b = flat[:, 3:3 + K * C].view(Gs, K, C), flat[:, 4 + K * C:4 + K * C + K]
    dW, db = gflat[:, 3:3 + K * C].view(Gs, K, C), gflat[:, 4 + K * C:4 + K * C + K]
    labels, nvalid = i["labels"][s], i["nvalid"][s]
    slot = i["slot"][s] if sel is None else torch.tensor([2], dtype=I32)
    stats = i["stats"] if sel is None else i["stats"][:, :5].contiguous()
    st = stats.clone().to(dev)
    loss, correct, dpool = head_train(x, W, b, labels.to(dev), nvalid.to(dev), dW, db, st, slot.to(dev), mean)
    op = "head_train"
    check_bound(loss, o["loss"][s], loss_bound(o["loss"][s]), op, "loss", who)
    check_exact(correct.cpu().long(), o["correct"][s], op, "correct", who)
    check_stats(st.cpu(), stats, stats_oracle(stats, slot, o["loss"][s], o["correct"][s], nvalid),
                loss_bound(o["loss"][s]), o["loss"][s], op, who)
    rows = o["rows"][s]
    assert tuple(dpool.shape) == (Gs, N, 1, 1, C)
    dp = dpool.cpu().reshape(Gs, N, C)
    check_bound(dp[rows], o["dpool"][s][rows], o["b_dpool"][s][rows], op, "dpool (rows < nvalid)", who)
    # rows at and beyond nvalid: zero, as the unfused path's (avgpool_global_bwd copies every row)
    check_exact(dp[~rows], torch.zeros(int((~rows).sum()), C), op, "dpool (rows >= nvalid)", who, bitwise=False)
    gcpu = gflat.cpu()
    dWc, dbc = gcpu[:, 3:3 + K * C].view(Gs, K, C), gcpu[:, 4 + K * C:4 + K * C + K]
    act = nvalid > 0
    check_bound(dWc[act], o["dW"][s][act], o["b_dW"][s][act], op, "dW", who)
    check_bound(dbc[act], o["db"][s][act], o["b_db"][s][act], op, "db", who)
    # overwritten, not accumulated (the sentinel is far beyond every bound); the inactive
    # replica's rows and every element between the slices untouched
    keep = torch.ones(Gs, S, dtype=torch.bool)
    keep[act, 3:3 + K * C] = False
    keep[act, 4 + K * C:4 + K * C + K] = False
    check_exact(gcpu[keep], torch.full((int(keep.sum()),), HEAD_SENTINEL), op, "gradient rows outside dW / db", who)
    check_exact(flat.cpu(), i["flat"][s], op, "parameters", who)
    return {"loss": loss.cpu(), "correct": correct.cpu(), "grads": gcpu,
            "dpool": torch.where(rows[..., None], dp, torch.zeros_like(dp))}


# ================================================================================== SGD
# sgd_kernel: 4 parameters per thread, 256 threads, the grid capped at 1024 blocks: P = 4 one
# thread, 1020 / 1024 / 1028 around one block, 4 (1024 256 + 5) five quads past one sweep of the
# capped grid.  (P, fg_accum, wd)
SGD_WRAP = 4 * (1024 * 256 + 5)
SGD_CASES = [(4, True, 5e-4), (1020, False, 5e-4), (1024, True, 5e-4), (1028, False, 5e-4), (1028, True, 0.0),
             (SGD_WRAP, True, 5e-4), (SGD_WRAP, False, 5e-4)]
SGD_MOMENTUM = 0.9
# chains: d = g + wd p (2), m = momentum m + d (2), p = p - lr m (2); fg = fg + g (1)
SGD_N = {"mom": 4, "params": 6, "fg": 1}


def sgd_id(c):
    P, fg, wd = c
    return f"P{P}-{'fg' if fg else 'nofg'}-wd{wd:g}"


def sgd_inputs(case):
    P, use_fg, wd = case
    g = gen(3, P, use_fg)
    G = 3
    return {"st": torch.randn(G, P + 64, generator=g), "grads": torch.randn(G, P, generator=g),
            "mom": torch.randn(G, P, generator=g), "fg": torch.randn(G, P, generator=g) if use_fg else None,
            "lr": torch.tensor([0.1, 0.05, 0.2]), "first": torch.tensor([1, 0, 0], dtype=I32),
            "active": torch.tensor([1, 1, 0], dtype=I32)}


def sgd_oracle(p, gr, m, lr, first, active, momentum, wd, fg):
    """torch.optim.SGD(momentum, weight_decay) per active replica in fp64 and the magnitudes."""
    p, gr, m = p.double().clone(), gr.double(), m.double().clone()
    mu, wd = f32(momentum), f32(wd)
    A_p, A_m = p.abs(), m.abs()
    fgn = None if fg is None else fg.double().clone()
    A_f = None if fg is None else fg.double().abs()
    for g in range(p.shape[0]):
        if int(active[g]) == 0:
            continue
        l = float(lr[g])
        if fgn is not None:
            fgn[g] += gr[g]
            A_f[g] += gr[g].abs()
        d, A_d = gr[g] + wd * p[g], gr[g].abs() + wd * p[g].abs()
        if int(first[g]):
            m[g], A_m[g] = d, A_d
        else:
            m[g], A_m[g] = mu * m[g] + d, mu * m[g].abs() + A_d
        A_p[g] = p[g].abs() + l * A_m[g]
        p[g] = p[g] - l * m[g]
    return {"params": (p, A_p), "mom": (m, A_m), "fg": (fgn, A_f)}


def run_sgd(ops, case, dev, who, sel=None):
    P, use_fg, wd = case
    i = sgd_inputs(case)
    s = slice(0, 3) if sel is None else slice(sel, sel + 1)
    want = sgd_oracle(i["st"][s, :P], i["grads"][s], i["mom"][s], i["lr"][s], i["first"][s], i["active"][s],
                      SGD_MOMENTUM, wd, None if i["fg"] is None else i["fg"][s])
    st, gr, mom = i["st"][s].to(dev), i["grads"][s].to(dev), i["mom"][s].to(dev)
    fg = None if i["fg"] is None else i["fg"][s].to(dev)
    ops.sgd_step(st[:, :P], gr, mom, i["lr"][s].to(dev), i["first"][s].to(dev), i["active"][s].to(dev), SGD_MOMENTUM,
                 wd, fg_accum=fg)
    op = "sgd_step"
    check_bound(st[:, :P], want["params"][0], bound32(SGD_N["params"], want["params"][1]), op, "params", who)
    check_bound(mom, want["mom"][0], bound32(SGD_N["mom"], want["mom"][1]), op, "momentum", who)
    if fg is not None:
        check_bound(fg, want["fg"][0], bound32(SGD_N["fg"], want["fg"][1]), op, "fg_accum", who)
    check_exact(st[:, P:], i["st"][s, P:], op, "columns beyond P", who)
    check_exact(gr, i["grads"][s], op, "grads", who)
    off = i["active"][s] == 0
    check_exact(st.cpu()[off], i["st"][s][off], op, "inactive params", who)
    check_exact(mom.cpu()[off], i["mom"][s][off], op, "inactive momentum", who)
    if fg is not None:
        check_exact(fg.cpu()[off], i["fg"][s][off], op, "inactive fg_accum", who)
    return {"st": st.cpu(), "mom": mom.cpu(), "fg": None if fg is None else fg.cpu()}


# ====================================================================== dist_loss_grad
# distnorm_kernel / distgrad_kernel: 2048 elements per block, the grid capped at 256 blocks:
# P = 1, one block less one / exactly / plus one element, and 1029 elements past one sweep of the
# capped grid.  Replicas: (poison phase, benign: trig < 0, inactive, w == base).
DIST_CASES = [1, 2047, 2048, 2049, 256 * 2048 + 1029]
DIST_ALPHA = 0.7


def dist_norm_n(P):
    """fp32 chain of ||w - base||: the difference, a thread's FMAs, the wave butterfly (6), the
    block's four waves (3), the blocks in order, the square root."""
    bx = max(1, min(256, (P + 2047) // 2048))
    return 1 + -(-P // (bx * 256)) + 6 + 3 + bx + 1


def dist_inputs(P):
    g = gen(4, P)
    G = 4
    w = torch.randn(G, P + 37, generator=g)
    base = w + 0.01 * torch.randn(G, P + 37, generator=g)
    base[3] = w[3]
    return {"w": w, "base": base, "grads": torch.randn(G, P, generator=g),
            "trig": torch.tensor([0, -1, 2, 1], dtype=I32), "active": torch.tensor([1, 1, 0, 1], dtype=I32)}


def dist_oracle(w, base, grads, trig, active, alpha):
    G, P = grads.shape
    a = f32(alpha)
    out, A = grads.double().clone(), grads.double().abs()
    dist = torch.zeros(G, dtype=F64)
    for g in range(G):
        if int(trig[g]) < 0 or int(active[g]) == 0:
            continue
        d = w[g, :P].double() - base[g, :P].double()
        nr = math.sqrt(float((d * d).sum()))
        dist[g] = nr
        c = (1.0 - a) / nr if nr > 0 else 0.0
        out[g] = a * grads[g].double() + c * d
        A[g] = a * grads[g].double().abs() + c * d.abs()
    return dist, out, A


def run_dist(ops, P, dev, who):
    i = dist_inputs(P)
    dist_w, gr_w, A = dist_oracle(i["w"], i["base"], i["grads"], i["trig"], i["active"], DIST_ALPHA)
    gr = i["grads"].clone().to(dev)
    w, base = i["w"].to(dev), i["base"].to(dev)
    dist = ops.dist_loss_grad(w, base, gr, i["trig"].to(dev), i["active"].to(dev), DIST_ALPHA)
    n = dist_norm_n(P)
    op = "dist_loss_grad"
    check_bound(dist, dist_w, bound32(n, dist_w), op, "distance", who)
    check_bound(gr, gr_w, bound32(n + 5, A), op, "grads", who)     # + (1 - alpha), the division, w - base, c d, the FMA
    skip = (i["trig"] < 0) | (i["active"] == 0)
    check_exact(gr.cpu()[skip], i["grads"][skip], op, "grads of benign / inactive replicas", who)
    check_exact(w, i["w"], op, "w", who)
    check_exact(base, i["base"], op, "base", who)
    return {"dist": dist.cpu(), "grads": gr.cpu()}


# =============================================================================== pooling
# maxpool_kernel (any C) / maxpool_v4_kernel (C % 4 == 0) and their backward forms, both (k, s, p)
# the models use; H = W = 2 (one window), 5 (odd: (2, 2, 0) drops the last row and column), 24.
# Inputs pass through ReLU and round(), so most windows hold several equal maxima.
POOL_KSP = [(2, 2, 0), (3, 2, 1)]
POOL_CASES = [(ksp, C, H) for ksp in POOL_KSP for C in (1, 10, 20, 50) for H in (2, 5, 24)]
POOL_BWD_N = 4          # an input pixel lies in at most ceil(k / s)^2 = 4 windows
AVG_CASES = [(HW, C) for HW in ((1, 1), (4, 4), (8, 8)) for C in (1, 10, 64)]
RELU_CASES = [1, 7, 8, 9, 8 * 256 * 3 + 5]      # 8 elements per thread + a tail launch


def pool_id(c):
    (k, s, p), C, H = c
    return f"k{k}s{s}p{p}-C{C}-H{H}"


def maxpool_oracle(x, k, s, p):
    """(y, ind int32): the window scanned in row-major order, a value replacing the best only if
    greater (so the first maximum wins); ind = hi * W + wi."""
    xn = x.numpy()
    G, N, H, W, C = xn.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    best = np.full((G, N, Ho, Wo, C), -np.inf, dtype=np.float32)
    bi = np.full((G, N, Ho, Wo, C), -1, dtype=np.int32)
    ho, wo = np.arange(Ho), np.arange(Wo)
    for a in range(k):
        for b in range(k):
            hi, wi = ho * s - p + a, wo * s - p + b
            ok = ((hi >= 0) & (hi < H))[:, None] & ((wi >= 0) & (wi < W))[None, :]
            v = xn[:, :, np.clip(hi, 0, H - 1)][:, :, :, np.clip(wi, 0, W - 1)]
            take = ok[None, None, :, :, None] & ((v > best) | (bi < 0))
            idx = (hi[:, None] * W + wi[None, :]).astype(np.int32)[None, None, :, :, None]
            best = np.where(take, v, best)
            bi = np.where(take, idx, bi)
    return torch.from_numpy(best), torch.from_numpy(bi)


def maxpool_bwd_oracle(dy, ind, in_shape):
    """dx[.., ind, c] += dy in fp64 (and the same over |dy|)."""
    G, N, H, W, C = in_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx, A = np.zeros((G * N, H * W, C)), np.zeros((G * N, H * W, C))
    gn = np.arange(G * N)[:, None, None]
    c = np.arange(C)[None, None, :]
    idx = ind.numpy().reshape(G * N, Ho * Wo, C).astype(np.int64)
    d = dy.double().numpy().reshape(G * N, Ho * Wo, C)
    np.add.at(dx, (gn, idx, c), d)
    np.add.at(A, (gn, idx, c), np.abs(d))
    return torch.from_numpy(dx).reshape(G, N, H, W, C), torch.from_numpy(A).reshape(G, N, H, W, C)


def run_maxpool(ops, case, dev, who):
    (k, s, p), C, H = case
    g = gen(5, k, C, H)
    x = torch.relu(torch.randn(2, 2, H, H, C, generator=g) * 1.5).round()
    y_w, ind_w = maxpool_oracle(x, k, s, p)
    y, ind = ops.maxpool2d(x.to(dev), k, s, p)
    op = "maxpool2d"
    check_exact(y, y_w, op, "values", who)
    check_exact(ind, ind_w, op, "indices", who)
    y2, _ = ops.maxpool2d(x.to(dev), k, s, p, want_ind=False)
    check_exact(y2, y_w, op, "values (want_ind=False)", who)
    dy = torch.randn(y_w.shape, generator=g)
    dx_w, A = maxpool_bwd_oracle(dy, ind_w, tuple(x.shape))
    dx = ops.maxpool2d_bwd(dy.to(dev), ind, tuple(x.shape), k, s, p)        # the stored indices
    check_bound(dx, dx_w, bound32(POOL_BWD_N, A), "maxpool2d_bwd", "dx", who)
    return {"y": y.cpu(), "ind": ind.cpu(), "dx": dx.cpu()}


def run_avgpool(ops, case, dev, who):
    (H, W), C = case
    g = gen(6, H * W, C)
    x = torch.randn(2, 3, H, W, C, generator=g)
    xd = x.double().reshape(2, 3, H * W, C)
    y = ops.avgpool_global(x.to(dev))
    # HW - 1 adds and the division
    check_bound(y, (xd.sum(2) / (H * W)).reshape(2, 3, 1, 1, C), bound32(H * W, (xd.abs().sum(2) / (H * W)).reshape(
        2, 3, 1, 1, C)), "avgpool_global", "y", who)
    dy = torch.randn(2, 3, 1, 1, C, generator=g)
    dx = ops.avgpool_global_bwd(dy.to(dev), (H, W))
    want = (dy.double() / (H * W)).expand(2, 3, H, W, C)
    check_bound(dx, want, bound32(2, want.abs()), "avgpool_global_bwd", "dx", who)    # 1 / HW rounded, the product
    return {"y": y.cpu(), "dx": dx.cpu()}


def run_relu(ops, n, dev, who, bitwise=True):
    """din = dout where out > 0, else +0.0 (``bitwise``; the reference's multiply by the mask
    leaves -0.0 under a negative dout: compared by value)."""
    g = gen(7, n)
    out = torch.randn(n, generator=g)
    out[torch.rand(n, generator=g) < 0.3] = 0.0
    out[torch.rand(n, generator=g) < 0.2] = -0.0
    out[n - 1] = [0.0, -0.0, 1.0][n % 3]
    dout = torch.randn(n, generator=g)
    want = torch.where(out > 0, dout, torch.zeros_like(dout))
    din = ops.relu_mask_bwd(dout.to(dev), out.to(dev))
    check_exact(din, want, "relu_mask_bwd", "din", who, bitwise=bitwise)
    return {"din": din.cpu()}


# =============================================================================== dropout
# dropout_kernel: the egrid cap (16384 blocks x 256 threads); (elements per group, G, p)
EGRID_SWEEP = 16384 * 256
DROPOUT_CASES = [(1, 3, 0.5), (255, 3, 0.5), (257, 3, 0.3), (256, 1, 0.3), ((EGRID_SWEEP + 262) // 2, 2, 0.5)]
DROPOUT_N = 3           # 1 - p, the reciprocal, the product


def run_dropout(ops, case, dev, who):
    per, G, p = case
    g = gen(8, per, G)
    x = torch.randn(G, per, generator=g)
    seeds = torch.randint(0, 2 ** 31 - 1, (G,), generator=g).to(I32)
    salt = 3
    ctr = torch.arange(per, dtype=torch.int64)[None, :].expand(G, per)
    keep = rng.uniform01(rng.salted(seeds.to(torch.int64), salt)[:, None], ctr) >= torch.tensor(p, dtype=torch.float32)
    want = torch.where(keep, x.double() / (1.0 - f32(p)), torch.zeros(G, per, dtype=F64))
    y = ops.dropout(x.to(dev), p, seeds.to(dev), salt)
    yc = y.cpu()
    check_exact(yc != 0, keep & (x != 0), "dropout", "kept pattern", who)
    if p == 0.5:
        check_exact(yc, want.float(), "dropout", "values at p = 0.5", who, bitwise=False)
    else:
        check_bound(yc, want, bound32(DROPOUT_N, want.abs()), "dropout", "values", who)
    return {"y": yc}


# ================================================================================== flat
# the egrid kernels (scale, noise add, delta sum, weighted sums): one element per thread, 256
# threads, the grid capped at 16384 blocks; sqdist_kernel 1024 elements per block, capped at 512.
FLAT_WRAP = EGRID_SWEEP + 259
FLAT_L = [1, 255, 256, 257, FLAT_WRAP]
SQDIST_L = [1, 255, 256, 257, 1025, 512 * 1024 + 1029]
DELTA_CASES = [(1, 1), (10, 255), (10, 256), (1, 257), (10, 257), (1, FLAT_WRAP)]
WSUM_CASES = [(5, 1), (5, 255), (5, 256), (5, 257), (1, FLAT_WRAP)]
NOISE_CASES = [(L, dt) for L in FLAT_L for dt in ("f32", "f64")]
# (n, d): the 16-row MFMA tile edge, the 4-wide k step, the 1024-column chunk; "s" a strided view
# with unit inner stride, "t" a transposed view (inner stride != 1)
GRAM_CASES = [(1, 1, ""), (15, 3, ""), (16, 4, ""), (17, 5, "s"), (37, 1023, ""), (16, 1024, "s"), (17, 1025, ""),
              (15, 5000, ""), (1, 1024, ""), (37, 4, ""), (16, 1, "t"), (17, 5000, "s"), (37, 1025, "t")]
GRAM_CHUNK = 1024
SCALE_GAMMA, NOISE_COEF, NOISE_SIGMA, NOISE_SEED, FIXED_E = 100.0, 0.01, 0.01, 1234, 20


def rows_view(n, L, g, scale=1.0):
    """The [n, L] view big[:, 1:1 + L] of a [n, rstride] buffer with an odd rstride."""
    rstride = L + 2 if L % 2 else L + 3
    big = torch.randn(n, rstride, generator=g) * scale
    return big, slice(1, 1 + L)


def run_scale(ops, L, dev, who):
    g = gen(9, L)
    w, base = torch.randn(L, generator=g), torch.randn(L, generator=g)
    gm = f32(SCALE_GAMMA)
    d = w.double() - base.double()
    out = ops.scale_from_base(w.to(dev), base.to(dev), SCALE_GAMMA)
    # w - base, the product, the sum
    check_bound(out, base.double() + d * gm, bound32(3, base.double().abs() + d.abs() * gm), "scale_from_base", "out", who)
    return {"out": out.cpu()}


def noise_inputs(L, dt):
    """dst, upd of length L: a prefix of the wrap case's (so a short buffer's result must be the
    prefix of the long one's)."""
    g = gen(10, dt == "f64")
    dst, upd = torch.randn(FLAT_WRAP, generator=g), torch.randn(FLAT_WRAP, generator=g, dtype=F64) * 3
    return dst[:L].clone(), (upd if dt == "f64" else upd.float())[:L].clone()


def run_noise_add(ops, case, dev, who):
    L, dt = case
    dst, upd = noise_inputs(L, dt)
    c, sg = f32(NOISE_COEF), f32(NOISE_SIGMA)
    d0 = dst.clone().to(dev)
    ops.add_noise_scaled(d0, upd.to(dev), NOISE_COEF, NOISE_SIGMA, NOISE_SEED, False)
    u = upd.double() * c
    # the product rounded to fp32, the sum
    check_bound(d0, dst.double() + u, bound32(2, dst.double().abs() + u.abs()), "add_noise_scaled", f"no noise, {dt} upd", who)
    d1 = dst.clone().to(dev)
    ops.add_noise_scaled(d1, upd.to(dev), NOISE_COEF, NOISE_SIGMA, NOISE_SEED, True)
    resid = d1.cpu().double() - d0.cpu().double()
    want = sg * rng.normal(NOISE_SEED, torch.arange(L, dtype=torch.int64)).double()
    check_bound(resid, want, 1e-5 + 1e-4 * want.abs(), "add_noise_scaled", f"noise residual, {dt} upd", who)
    return {"plain": d0.cpu(), "noisy": d1.cpu()}


def run_delta_sum(ops, case, dev, who):
    nrows, L = case
    g = gen(11, nrows, L)
    big, cs = rows_view(nrows, L, g)
    base = torch.randn(L, generator=g)
    b = base.numpy().astype(np.float64)
    want = np.zeros(L)
    for r in range(nrows):                        # fp64 operations in row order
        want = want + (big[r, cs].numpy().astype(np.float64) - b)
    out = ops.delta_sum(big.to(dev)[:, cs], base.to(dev))
    assert out.dtype == F64
    check_exact(out, torch.from_numpy(want), "delta_sum", "out", who)
    return {"out": out.cpu()}


def run_sq_dists(ops, L, dev, who):
    g = gen(12, L)
    big, cs = rows_view(3, L, g)
    m = torch.randn(L, generator=g)
    d = big[:, cs].double() - m.double()[None]
    want = (d * d).sum(1)
    out = ops.sq_dists(big.to(dev)[:, cs], m.to(dev))
    assert out.dtype == F64
    check_bound(out, want, bound64(want), "sq_dists", "out", who)
    return {"out": out.cpu()}


def run_weighted_sum(ops, case, dev, who):
    n, L = case
    g = gen(13, n, L)
    big, cs = rows_view(n, L, g)
    wts = torch.rand(n, generator=g) + 0.1
    if n > 1:
        wts[2] = 0.0
    want, A = torch.zeros(L, dtype=F64), torch.zeros(L, dtype=F64)
    for i in range(n):
        t = wts[i].double() * big[i, cs].double()
        want, A = want + t, A + t.abs()
    o32 = ops.weighted_sum(big.to(dev)[:, cs], wts.to(dev))
    assert o32.dtype == torch.float32
    check_bound(o32, want, bound32(n, A), "weighted_sum", "fp32 out", who)        # an FMA per client
    o64 = ops.weighted_sum(big.to(dev)[:, cs], wts.to(dev), torch.float64)
    assert o64.dtype == F64
    check_bound(o64, want, bound64(A), "weighted_sum", "fp64 out", who)
    return {"o32": o32.cpu(), "o64": o64.cpu()}


def wsum_fixed_oracle(points, wts, E):
    """q = w p 2^E (exact in fp64), hi = floor(q), lo = floor((q - hi) 2^53), int64 sums."""
    q = wts.numpy().astype(np.float32).astype(np.float64)[:, None] * points.numpy().astype(np.float64) * 2.0 ** E
    hi = np.floor(q)
    lo = np.floor((q - hi) * 2.0 ** 53)
    return torch.from_numpy(np.stack([hi.astype(np.int64).sum(0), lo.astype(np.int64).sum(0)]))


def run_weighted_sum_fixed(ops, case, dev, who):
    """Rows: N(0, 1) under a positive weight, N(0, 1) under a negative weight (negative
    products), multiples of 2^(1 - E) under the weight 0.5 (products that are exact integers at
    scale 2^E), fp32 denormals of both signs."""
    n, L = case
    g = gen(14, n, L)
    big, cs = rows_view(n, L, g)
    wts = torch.rand(n, generator=g) + 0.1
    if n > 1:
        wts[1] = -0.37
        wts[2] = 0.5
        big[2] = torch.randint(-1000, 1000, (big.shape[1],), generator=g).float() * 2.0 ** (1 - FIXED_E)
        big[3] = torch.randint(-1000, 1000, (big.shape[1],), generator=g).float() * 2.0 ** -140
    out = ops.weighted_sum_fixed(big.to(dev)[:, cs], wts.to(dev), FIXED_E)
    check_exact(out, wsum_fixed_oracle(big[:, cs], wts, FIXED_E), "weighted_sum_fixed", "limbs", who)
    return {"out": out.cpu()}


def gram_id(c):
    return f"n{c[0]}-d{c[1]}" + (f"-{c[2]}" if c[2] else "")


def run_gram(ops, case, dev, who):
    n, d, view = case
    g = gen(15, n, d)
    if view == "s":
        big = torch.randn(n, d + 3, generator=g).to(dev)
        f = big[:, 1:1 + d]
    elif view == "t":
        f = torch.randn(d, n, generator=g).to(dev).t()
    else:
        f = torch.randn(n, d, generator=g).to(dev)
    fd = f.cpu().double()
    want, A = fd @ fd.t(), fd.abs() @ fd.abs().t()
    out = ops.gram(f)
    assert out.dtype == F64
    # a chunk's min(d, 1024) products accumulated in fp32, the chunks summed in fp64
    check_bound(out, want, bound32(min(d, GRAM_CHUNK), A) + bound64(A), "gram", "out", who)
    return {"out": out.cpu()}

"""Kernel microbenchmarks on the real ResNet-18 (CIFAR) layer shapes.

Times each HIP conv kernel family on the shapes the FL round actually runs — evaluation
(17 folded-BN client models x 1024 images) and grouped training (10 clients x 64 images) —
and prints achieved TFLOP/s, so kernel changes are judged on the chip, not guessed.

    python -m dba_mod_amd.tools.bench_kernels [--reps 20] [--json out.json]
"""
from __future__ import annotations

import argparse
import json

import torch

from dba_mod_amd.ops import hip as H

# name, G, N, H, Cin, Cout, k, stride, pad
SHAPES = [
    ("eval.layer1", 17, 1024, 32, 32, 32, 3, 1, 1),
    ("eval.layer2", 17, 1024, 16, 64, 64, 3, 1, 1),
    ("eval.layer3", 17, 1024, 8, 128, 128, 3, 1, 1),
    ("eval.layer4", 17, 1024, 4, 256, 256, 3, 1, 1),
    ("eval.l2.0.conv1", 17, 1024, 32, 32, 64, 3, 2, 1),
    ("eval.l3.0.conv1", 17, 1024, 16, 64, 128, 3, 2, 1),
    ("eval.l4.0.conv1", 17, 1024, 8, 128, 256, 3, 2, 1),
    ("eval.l2.0.sc", 17, 1024, 32, 32, 64, 1, 2, 0),
    ("eval.l3.0.sc", 17, 1024, 16, 64, 128, 1, 2, 0),
    ("eval.l4.0.sc", 17, 1024, 8, 128, 256, 1, 2, 0),
    ("eval.stem", 17, 1024, 32, 3, 32, 3, 1, 1),
    ("train.layer1", 10, 64, 32, 32, 32, 3, 1, 1),
    ("train.layer2", 10, 64, 16, 64, 64, 3, 1, 1),
    ("train.layer3", 10, 64, 8, 128, 128, 3, 1, 1),
    ("train.layer4", 10, 64, 4, 256, 256, 3, 1, 1),
    ("train.stem", 10, 64, 32, 3, 32, 3, 1, 1),
    ("train.l2.0.conv1", 10, 64, 32, 32, 64, 3, 2, 1),
    ("train.l2.0.sc", 10, 64, 32, 32, 64, 1, 2, 0),
    ("train.l3.0.conv1", 10, 64, 16, 64, 128, 3, 2, 1),
    ("train.l3.0.sc", 10, 64, 16, 64, 128, 1, 2, 0),
    ("train.l4.0.conv1", 10, 64, 8, 128, 256, 3, 2, 1),
    ("train.l4.0.sc", 10, 64, 8, 128, 256, 1, 2, 0),
    ("eval.tiny.stem", 1, 1024, 64, 3, 64, 7, 2, 3),  # Tiny-ImageNet 7x7/2 stem, an eval chunk
    ("tiny.stem", 1, 64, 64, 3, 64, 7, 2, 3),       # Tiny-ImageNet 7x7/2 stem, a lone client
    ("tiny.stem10", 10, 64, 64, 3, 64, 7, 2, 3),    # ... 10 clients
]


def _time(fn, reps, inner=10):
    """GPU time per call: `inner` calls are captured in one HIP graph and replayed (the FL
    round replays its kernels the same way), so host and graph-launch overhead do not count."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(inner):
            fn()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * inner) * 1e-3


def _time_eager(fn, reps):
    """GPU time per call of a torch composition that does not capture into a graph (``torch.sort``):
    device events around ``reps`` eager calls; at milliseconds per call the host does not count."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def _bench_fp32(name, G, N, Hh, Cin, Cout, k, s, p, reps, dev):
    """fwd / dgrad / wgrad of the fp16-pair fp32 family; TFLOP/s counts the real fp32 work."""
    torch.manual_seed(0)
    x = torch.randn(G, N, Hh, Hh, Cin, device=dev)
    w = torch.randn(G, Cout, k, k, Cin, device=dev) * 0.05
    Ho = (Hh + 2 * p - k) // s + 1
    dy = torch.randn(G, N, Ho, Ho, Cout, device=dev)
    flops = 2.0 * G * N * Ho * Ho * Cout * k * k * Cin
    rec = {"shape": name, "dtype": "fp32"}
    if name.startswith("eval"):
        # evaluation weights are static: split into fp16-pair planes once (as bn_fold does)
        per = Cout * k * k * Cin
        H.split_weights(w, per, per, H._amax_w(w, per, per))
    ops = [("fwd", lambda: H.conv2d(x, w, None, s, p, relu=True))]
    if name == "eval.tiny.stem":   # the exact-FMA stem kernel it replaces in evaluation

        def fma_fwd():
            prev, H._EVAL_STEM_MFMA = H._EVAL_STEM_MFMA, False
            try:
                return H.conv2d(x, w, None, s, p, relu=True)
            finally:
                H._EVAL_STEM_MFMA = prev
        ops.append(("fwd_fma", fma_fwd))

        def nopad_fwd():
            prev, H._EVAL_STEM_PAD = H._EVAL_STEM_PAD, False
            try:
                return H.conv2d(x, w, None, s, p, relu=True)
            finally:
                H._EVAL_STEM_PAD = prev
        ops.append(("fwd_nopad", nopad_fwd))
    block_flops = None
    if name.startswith("eval") and H.basic_block_ok(x, w, w):
        # the whole identity BasicBlock (two convs, the mid activation in LDS: xblock.hip); its
        # TFLOP/s counts both convs' fp32 work
        xb = torch.relu(x)
        w2 = torch.randn(G, Cout, k, k, Cin, device=dev) * 0.05
        H.split_weights(w2, per, per, H._amax_w(w2, per, per))
        b1, b2 = torch.randn(G, Cout, device=dev) * 0.1, torch.randn(G, Cout, device=dev) * 0.1
        xb._dba_amax = H._amax_act(xb, None)
        block_flops = 2 * flops
        ops.append(("block", lambda: H.basic_block_eval(xb, w, b1, w2, b2)))
    if name == "eval.stem":
        # the stem + layer1.0 (xblock.hip STEM variant) vs the stem launch + fused block; their
        # TFLOP/s count the stem's and both block convs' fp32 work
        wb = [torch.randn(G, 32, 3, 3, 32, device=dev) * 0.05 for _ in range(2)]
        for wi in wb:
            H.split_weights(wi, 9216, 9216, H._amax_w(wi, 9216, 9216))
        b0, b1, b2 = [torch.randn(G, 32, device=dev) * 0.1 for _ in range(3)]
        if H.stem_block_ok(x, w, *wb):
            block_flops = flops + 2 * 2.0 * G * N * 32 * 32 * 32 * 9 * 32
            ops += [("stem_then_block", lambda: H.basic_block_eval(H.conv2d(x, w, None, 1, 1, bias=b0, relu=True),
                                                                 wb[0], b1, wb[1], b2)),
                    ("stem_block", lambda: H.stem_block_eval(x, w, b0, wb[0], b1, wb[1], b2))]
    if name.startswith("train"):
        wt = H.prepare_dgrad_weights(w, [(w, None, s, p, (Hh, Hh), None, G)])[0]
        dw = torch.zeros(G, Cout, k, k, Cin, device=dev)
        ops += [("dgrad", lambda: H.conv2d_dgrad(dy, w, None, s, p, (Hh, Hh), wt=wt)),
                ("wgrad", lambda: H.conv2d_wgrad(dy, x, s, p, k, k, dw))]
    if name.startswith("tiny.stem"):   # the stem's weight gradient (the stem has no data gradient)
        dw = torch.zeros(G, Cout, k, k, Cin, device=dev)
        ops.append(("wgrad", lambda: H.conv2d_wgrad(dy, x, s, p, k, k, dw)))
    for tag, fn in ops:
        t = _time(fn, reps)
        rec[tag + "_us"] = round(t * 1e6, 1)
        rec[tag + "_tflops"] = round((block_flops if tag in ("block", "stem_block", "stem_then_block") else flops)
                                     / t / 1e12, 1)
    return rec


def _bench_down(name, G, N, W, C, C2, reps, dev):
    """A downsampling block's conv2 + 1x1 stride-2 shortcut: fused (one launch, xconv.hpp
    dba_xdown_fwd) vs the shortcut conv + conv2 with a residual epilogue; TFLOP/s counts both
    convs' fp32 work."""
    torch.manual_seed(0)
    a = torch.relu(torch.randn(G, N, W, W, C, device=dev))
    x2 = torch.relu(torch.randn(G, N, 2 * W, 2 * W, C2, device=dev))
    w2 = torch.randn(G, C, 3, 3, C, device=dev) * 0.03
    wsc = torch.randn(G, C, 1, 1, C2, device=dev) * 0.1
    for w in (w2, wsc):
        per = w[0].numel()
        H.split_weights(w, per, per, H._amax_w(w, per, per))
    b2, bsc = torch.randn(G, C, device=dev) * 0.1, torch.randn(G, C, device=dev) * 0.1
    a._dba_amax, x2._dba_amax = H._amax_act(a, None), H._amax_act(x2, None)
    flops = 2.0 * G * N * W * W * C * (9 * C + C2)
    rec = {"shape": name, "dtype": "fp32"}
    ops = [("fused", lambda: H.down_block_eval(a, w2, b2, x2, wsc, bsc)),
           ("two", lambda: H.conv2d(a, w2, None, 1, 1, bias=b2, relu=True,
                                    residual=H.conv2d(x2, wsc, None, 2, 0, bias=bsc)))]
    for tag, fn in ops:
        t = _time(fn, reps)
        rec[tag + "_us"] = round(t * 1e6, 1)
        rec[tag + "_tflops"] = round(flops / t / 1e12, 1)
    return rec


def _bench_eval_chunk(G, N, reps, dev):
    """The whole BN-folded CIFAR ResNet-18 evaluation forward of G models x N images (the
    evaluator's chunk: 17 x 1024), through the model program as the round runs it."""
    from dba_mod_amd.models import program as P
    from dba_mod_amd.models.spec import get_spec
    spec = get_spec("resnet18_cifar")
    torch.manual_seed(0)
    bank = torch.stack([spec.init_flat(i) for i in range(G)]).to(dev)
    bank[:, spec.P:] += 0.05 * torch.rand_like(bank[:, spec.P:])
    folded = P.fold_bank(spec, bank, torch.float32)
    x = torch.rand(G, N, 32, 32, 3, device=dev)
    x._dba_amax = H._unit_amax(G, dev)
    sel = torch.arange(G, dtype=torch.int32, device=dev)
    nval = torch.full((G,), N, dtype=torch.int32, device=dev)

    def fwd():
        ctx = P.Ctx(spec, None, None, sel, train=False, folded=folded, nvalid=nval, act_dtype=torch.float32)
        with H.amax_arena(G, dev):
            return P.forward(ctx, x)

    t = _time(fwd, reps, inner=1)
    return {"shape": f"eval.chunk.{G}x{N}", "dtype": "fp32", "fwd_ms": round(t * 1e3, 3),
            "fwd_tflops": round(G * N * 17.83e9 / 64 / t / 1e12, 1)}


DOWN = [("eval.l2.0.down", 17, 1024, 16, 64, 32)]

# softmax cross-entropy (loss.hip): G groups x B rows x C classes — Tiny-ImageNet's evaluation
# chunk and training step, CIFAR's evaluation chunk and training step
XENT = [("xent.tiny.eval", 1, 1024, 200), ("xent.tiny.train", 10, 64, 200), ("xent.cifar.eval", 17, 1024, 10),
        ("xent.cifar.train", 10, 64, 10)]


def _bench_xent(name, G, B, C, reps, dev):
    torch.manual_seed(0)
    logits = torch.randn(G, B, C, device=dev) * 3
    labels = torch.randint(0, C, (G, B), device=dev, dtype=torch.int32)
    t_grad = _time(lambda: H.softmax_xent(logits, labels, True, True, grad_dtype=torch.float32), reps)
    t_eval = _time(lambda: H.softmax_xent(logits, labels, False, False), reps)
    prev = H._L.dba_xent_r5_set(1)   # the round-5 kernel form (a thread per row, a block per group)
    try:
        t_grad5 = _time(lambda: H.softmax_xent(logits, labels, True, True, grad_dtype=torch.float32), reps)
        t_eval5 = _time(lambda: H.softmax_xent(logits, labels, False, False), reps)
    finally:
        H._L.dba_xent_r5_set(prev)
    return {"shape": name, "G": G, "B": B, "C": C, "train_us": round(t_grad * 1e6, 2),
            "eval_us": round(t_eval * 1e6, 2), "r5_train_us": round(t_grad5 * 1e6, 2),
            "r5_eval_us": round(t_eval5 * 1e6, 2)}


# norm-clipped FedAvg (clip.hip): n clients x S floats — a CIFAR round's 10 final states of the
# half-width ResNet-18 (S = 2,802,430; the rows are the [:, :S] view of the stacked states)
CLIP = [("clip.cifar", 10, 2_802_430)]


def _bench_clip(name, n, S, reps, dev):
    """The two fused passes against the composed path they replace: torch ``finals - global``
    materialised as [n, S], then sq_dists and weighted_sum_fixed over it.  GB/s counts the bytes
    each form must move (rows + base in; norms, or the [2, S] int64 limbs, out)."""
    from dba_mod_amd.fl import aggregate as agg
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    finals = base[None] + 0.01 * torch.randn(n, S, device=dev)
    finals[0] = base + 100.0 * (finals[0] - base)                 # a model-replacement client
    zero = torch.zeros(S, device=dev)
    sq, mx = H.delta_stats(finals, base)
    factors, _ = agg.clip_factors(sq, "median")
    scale = factors.float().to(dev)
    E = agg.fixed_exponent(agg.max_abs(mx), n)
    t_stats = _time(lambda: H.delta_stats(finals, base), reps)
    t_sum = _time(lambda: H.clipped_delta_sum_fixed(finals, base, scale, E), reps)
    t_sum64 = _time(lambda: H.clipped_delta_sum(finals, base, scale), reps)
    t_delta = _time(lambda: finals - base[None], reps)
    delta = finals - base[None]
    t_sqd = _time(lambda: H.sq_dists(delta, zero), reps)
    t_wsum = _time(lambda: H.weighted_sum_fixed(delta, scale, E), reps)
    b_in = (n + 1) * S * 4
    return {"shape": name, "n": n, "S": S, "delta_stats_us": round(t_stats * 1e6, 1),
            "delta_stats_GBps": round(b_in / t_stats / 1e9, 1),
            "clipped_sum_fixed_us": round(t_sum * 1e6, 1),
            "clipped_sum_fixed_GBps": round((b_in + 2 * S * 8) / t_sum / 1e9, 1),
            "clipped_sum_f64_us": round(t_sum64 * 1e6, 1),
            "fused_us": round((t_stats + t_sum) * 1e6, 1),
            "composed_delta_us": round(t_delta * 1e6, 1), "composed_sq_dists_us": round(t_sqd * 1e6, 1),
            "composed_wsum_fixed_us": round(t_wsum * 1e6, 1),
            "composed_us": round((t_delta + t_sqd + t_wsum) * 1e6, 1)}


# Multi-Krum (krum.hip): the [n, n] squared distances between a CIFAR round's 10 final states
KRUM = [("krum.cifar", 10, 2_802_430)]


def _bench_krum(name, n, S, reps, dev):
    """The fused pairwise-distance kernel, reading the final-state rows where they lie in a
    snapshot bank, against the composition it replaces: the [n, S] copy of those rows, then n
    calls of sq_dists(points, points[i]).  GB/s counts n * S * 4 bytes for both: the bytes a
    perfect kernel would move (the fused kernel fetches each row about twice, the composition
    n + 2 times)."""
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    bank = base[None] + 0.01 * torch.randn(2 * n + 1, S, device=dev)      # finals in the odd slots
    slots = torch.arange(1, 2 * n + 1, 2, device=dev)
    rows = bank[1::2]                                                     # the same rows as a strided view
    assert rows.shape[0] == n and torch.equal(rows, bank[slots])

    def composed():
        points = bank[slots]
        return torch.stack([H.sq_dists(points, points[i]) for i in range(n)])

    D = H.pairwise_sq_dists(rows)
    Dc = composed()
    rel = float(((D - Dc).abs() / Dc.clamp_min(1e-300)).max())
    t_fused = _time(lambda: H.pairwise_sq_dists(rows), reps)
    # (S is even but no multiple of 4: the bank's odd rows start 8 bytes off a 16-byte boundary
    # and take the scalar-load path; a padded copy has every row aligned)
    pad = torch.zeros(n, (S + 3) // 4 * 4, device=dev)
    pad[:, :S] = rows
    assert torch.equal(H.pairwise_sq_dists(pad[:, :S]), D)
    t_aligned = _time(lambda: H.pairwise_sq_dists(pad[:, :S]), reps)
    t_comp = _time(composed, reps)
    t_copy = _time(lambda: bank[slots], reps)
    b = n * S * 4
    return {"shape": name, "n": n, "S": S, "fused_us": round(t_fused * 1e6, 1),
            "fused_GBps": round(b / t_fused / 1e9, 1), "fused_aligned_us": round(t_aligned * 1e6, 1),
            "fused_aligned_GBps": round(b / t_aligned / 1e9, 1), "composed_us": round(t_comp * 1e6, 1),
            "composed_GBps": round(b / t_comp / 1e9, 1), "composed_copy_us": round(t_copy * 1e6, 1),
            "fused_vs_composed_max_rel": rel}


# coordinate-wise trimmed mean (trim.hip): a CIFAR round's 10 final states, k = 2 as in configs/cifar_trim.yaml
TRIM = [("trim.cifar", 10, 2_802_430, 2)]


def _bench_trim(name, n, S, k, reps, dev):
    """The fused trimmed-sum kernel, reading the final-state rows where they lie in a snapshot
    bank, against (a) the composition it replaces — the [n, S] copy of those rows, ``torch.sort``
    along the clients, the fp64 deltas of the kept ranks and their sum (the same total bits; no
    counts) — and (b) ``delta_sum`` over the same rows, plain FedAvg's pass: it moves the same
    bytes and does no sorting, so it is the floor.  GB/s counts n * S * 4 bytes for all three."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    bank = base[None] + 0.01 * torch.randn(2 * n + 1, S, device=dev)      # finals in the odd slots
    slots = torch.arange(1, 2 * n + 1, 2, device=dev)
    rows = bank[1::2]                                                     # the same rows as a strided view
    assert rows.shape[0] == n and torch.equal(rows, bank[slots])
    bd = base.double()

    def composed():
        s = torch.sort(bank[slots], dim=0).values
        return (s[k:n - k].double() - bd[None]).sum(0)

    total, kept, high = H.trimmed_delta_sum(rows, base, k)
    rt, rk, rh = R.trimmed_delta_sum(bank, base, k, slots)
    assert torch.equal(total, rt) and torch.equal(kept, rk) and torch.equal(high, rh)
    max_rel = float(((total - composed()).abs() / total.abs().clamp_min(1e-300)).max())
    t_fused = _time(lambda: H.trimmed_delta_sum(rows, base, k), reps)
    # (S is even but no multiple of 4: the bank's odd rows start 8 bytes off a 16-byte boundary
    # and take the scalar-load path; a padded copy has every row aligned)
    pad = torch.zeros(n, (S + 3) // 4 * 4, device=dev)
    pad[:, :S] = rows
    assert torch.equal(H.trimmed_delta_sum(pad[:, :S], base, k)[0], total)
    t_aligned = _time(lambda: H.trimmed_delta_sum(pad[:, :S], base, k), reps)
    t_comp = _time_eager(composed, reps)
    t_ref = _time_eager(lambda: R.trimmed_delta_sum(bank, base, k, slots), reps)
    t_dsum = _time(lambda: H.delta_sum(rows, base), reps)
    b = n * S * 4
    return {"shape": name, "n": n, "S": S, "k": k, "fused_us": round(t_fused * 1e6, 1),
            "fused_GBps": round(b / t_fused / 1e9, 1), "fused_aligned_us": round(t_aligned * 1e6, 1),
            "fused_aligned_GBps": round(b / t_aligned / 1e9, 1), "composed_us": round(t_comp * 1e6, 1),
            "composed_GBps": round(b / t_comp / 1e9, 1), "reference_op_us": round(t_ref * 1e6, 1),
            "delta_sum_us": round(t_dsum * 1e6, 1), "delta_sum_GBps": round(b / t_dsum / 1e9, 1),
            "fused_vs_composed_max_rel": max_rel}


# Bulyan's median window (bulyan.hip): the 8 clients iterated Krum selects of a CIFAR round's 10, f = 1 as in
# configs/cifar_bulyan.yaml
BULYAN = [("bulyan.cifar", 8, 2_802_430, 1)]


def _bench_bulyan(name, t, S, f, reps, dev, rounds=5):
    """The fused median-window kernel over t final-state rows read where they lie in a 21-row
    snapshot bank, against (a) ``trimmed_delta_sum`` over the same rows with k = f — the same loads
    and the same sort, a symmetric window: the yardstick — and (b) ``delta_sum`` over the same
    rows, the byte floor.  The three are timed in turn, ``rounds`` times over, in this process: the
    median of each and its min .. max (the spread a difference has to leave to mean anything).
    GB/s counts t * S * 4 bytes.  The bits are checked against the reference op first."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    bank = base[None] + 0.01 * torch.randn(21, S, device=dev)             # finals in the odd slots
    slots = torch.arange(1, 2 * t + 1, 2, device=dev)
    rows = bank[1:2 * t + 1:2]                                            # the same rows as a strided view
    assert rows.shape[0] == t and torch.equal(rows, bank[slots])
    total, kept, high = H.bulyan_delta_sum(rows, base, f)
    rt, rk, rh = R.bulyan_delta_sum(bank, base, f, slots)
    assert torch.equal(total, rt) and torch.equal(kept, rk) and torch.equal(high, rh)
    off_trim = float((total != H.trimmed_delta_sum(rows, base, f)[0]).double().mean())
    fns = {"bulyan": lambda: H.bulyan_delta_sum(rows, base, f), "trim": lambda: H.trimmed_delta_sum(rows, base, f),
           "delta_sum": lambda: H.delta_sum(rows, base)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(_time(fn, reps))
    b = t * S * 4
    out = {"shape": name, "t": t, "S": S, "f": f, "rounds": rounds, "totals_off_the_trimmed_sum": round(off_trim, 4)}
    for k, v in times.items():
        v = sorted(v)
        med = v[len(v) // 2]
        out.update({f"{k}_us": round(med * 1e6, 1), f"{k}_min_us": round(v[0] * 1e6, 1),
                    f"{k}_max_us": round(v[-1] * 1e6, 1), f"{k}_GBps": round(b / med / 1e9, 1)})
    return out


# FLAME's Gram matrix of the updates (dgram.hip): a CIFAR round's 10 final states against the global model
FLAME = [("flame.cifar", 10, 2_802_430)]


def _bench_flame(name, n, S, reps, dev, rounds=5):
    """The fused Gram kernel over n final-state rows read where they lie in a 21-row snapshot bank
    (every other row), against (a) ``pairwise_sq_dists`` over the same rows — Multi-Krum's pass: n
    rows where the Gram reads n + 1, 45 subtractions and 45 fma per coordinate where the Gram does
    55 fma: the yardstick is its time x (n + 1) / n — and (b) ``delta_sum`` over the same rows, the
    byte floor.  The three are timed in turn, ``rounds`` times over, in this process: the median
    of each and its min .. max (the spread a difference has to leave to mean anything).  GB/s counts
    (n + 1) * S * 4 bytes for the Gram and n * S * 4 for the others.  Before anything is timed the
    kernel is checked against the reference op on the device: G within the tests' bound (L + 2)
    2^-52 A, the same admitted set, the same median client and its norm S within (L + 4) 2^-53."""
    from dba_mod_amd.fl import aggregate as agg
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    common = torch.randn(S, device=dev)
    bank = base[None] + 0.01 * (common[None] + torch.randn(21, S, device=dev))   # finals in the odd slots
    bank[3] = base + 100.0 * (bank[3] - base)                             # a model-replacement client
    bank[7] = base + 0.01 * torch.randn(S, device=dev)                    # one with a direction of its own
    slots = torch.arange(1, 2 * n + 1, 2, device=dev)
    rows = bank[1:2 * n + 1:2]                                            # the same rows as a strided view
    assert rows.shape[0] == n and torch.equal(rows, bank[slots])
    G = H.delta_gram(rows, base)
    assert torch.equal(G, H.delta_gram(bank, base, slots)) and torch.equal(G, G.t())
    Gr = R.delta_gram(bank, base, slots)
    d = (rows.double() - base.double()[None]).abs()
    A = d @ d.t()
    del d
    assert bool(((G - Gr).abs() <= (S + 2) * 2.0 ** -52 * A).all())
    admitted = agg.flame_admit(agg.flame_distances(G))
    assert admitted == agg.flame_admit(agg.flame_distances(Gr))
    e, er = torch.diagonal(G).cpu().sqrt(), torch.diagonal(Gr).cpu().sqrt()
    med = int(torch.sort(e).indices[(n - 1) // 2])
    assert med == int(torch.sort(er).indices[(n - 1) // 2])
    bound, bound_r = agg.clip_bound(e, "median"), agg.clip_bound(er, "median")
    assert abs(bound - bound_r) <= (S + 4) * 2.0 ** -53 * bound_r
    fns = {"gram": lambda: H.delta_gram(rows, base), "krum": lambda: H.pairwise_sq_dists(rows),
           "delta_sum": lambda: H.delta_sum(rows, base)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(_time(fn, reps))
    out = {"shape": name, "n": n, "S": S, "rounds": rounds, "admitted": admitted, "median_norm": bound}
    for k, v in times.items():
        v = sorted(v)
        med_t = v[len(v) // 2]
        b = (n + 1 if k == "gram" else n) * S * 4
        out.update({f"{k}_us": round(med_t * 1e6, 1), f"{k}_min_us": round(v[0] * 1e6, 1),
                    f"{k}_max_us": round(v[-1] * 1e6, 1), f"{k}_GBps": round(b / med_t / 1e9, 1)})
    out["gram_vs_krum"] = round(out["gram_us"] / out["krum_us"], 3)
    out["yardstick"] = round((n + 1) / n, 3)
    return out


# robust learning rate (rlr.hip): a CIFAR round's 10 final states, theta = 4 as in configs/cifar_rlr.yaml
RLR = [("rlr.cifar", 10, 2_802_430, 4)]


def _bench_rlr(name, n, S, theta, reps, dev):
    """The three fused passes, reading the final states as the server holds them (the stacked
    [n, S] rows: S is even but no multiple of 4, so every odd row starts 8 bytes off a 16-byte
    boundary), each against the ``ops.reference`` composition on the same device (chunked torch
    ops, timed eagerly) and checked to give its bits.  The sum + votes pass must move n * S * 4
    (rows) + S * 4 (base) + S * 12 (fp64 total and int32 votes out) bytes: GB/s counts those; the
    agreement pass reads every row again with the base and the votes, the apply pass moves S * 20
    bytes."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    base = torch.randn(S, device=dev)
    finals = base[None] + 0.01 * torch.randn(n, S, device=dev)
    finals[0] = base + 100.0 * (finals[0] - base)                 # a model-replacement client
    finals[:, ::7] = base[::7]                                    # exact-zero deltas: abstentions
    coef, sigma, seed = 0.1 / n, 0.01, 12345
    total, votes = H.delta_sum_votes(finals, base)
    rt, rv = R.delta_sum_votes(finals, base)
    assert torch.equal(total, rt) and torch.equal(votes, rv) and torch.equal(total, H.delta_sum(finals, base))
    counts = H.vote_agreement(finals, base, votes, theta)
    assert torch.equal(counts, R.vote_agreement(finals, base, votes, theta))
    out = {"shape": name, "n": n, "S": S, "theta": theta}
    for noise in (False, True):
        a, b, c = base.clone(), base.clone(), base.clone()
        fa = H.rlr_apply(a, total, votes, theta, coef, sigma, seed, noise)
        H.add_noise_scaled(b, total, coef, sigma, seed, noise)
        H.add_noise_scaled(c, total, -coef, sigma, seed, noise)
        kept = votes.abs() >= theta
        assert torch.equal(a, torch.where(kept, b, c)) and int(fa) == int((~kept).sum())
    out["flipped_share"] = round(int(fa) / S, 4)
    dst = base.clone()
    t_votes = _time(lambda: H.delta_sum_votes(finals, base), reps)
    t_dsum = _time(lambda: H.delta_sum(finals, base), reps)
    t_agree = _time(lambda: H.vote_agreement(finals, base, votes, theta), reps)
    t_apply = _time(lambda: H.rlr_apply(dst, total, votes, theta, coef, sigma, seed, False), reps)
    t_apply_n = _time(lambda: H.rlr_apply(dst, total, votes, theta, coef, sigma, seed, True), reps)
    t_noise = _time(lambda: H.add_noise_scaled(dst, total, coef, sigma, seed, False), reps)
    r_votes = _time_eager(lambda: R.delta_sum_votes(finals, base), reps)
    r_agree = _time_eager(lambda: R.vote_agreement(finals, base, votes, theta), reps)
    r_apply = _time_eager(lambda: R.rlr_apply(dst, total, votes, theta, coef, sigma, seed, False), reps)
    r_apply_n = _time_eager(lambda: R.rlr_apply(dst, total, votes, theta, coef, sigma, seed, True), reps)
    b_votes = n * S * 4 + S * 4 + S * 12
    b_agree = n * S * 4 + S * 8
    out.update({"sum_votes_us": round(t_votes * 1e6, 1), "sum_votes_GBps": round(b_votes / t_votes / 1e9, 1),
                "sum_votes_composed_us": round(r_votes * 1e6, 1),
                "delta_sum_us": round(t_dsum * 1e6, 1),
                "delta_sum_GBps": round((n * S * 4 + S * 12) / t_dsum / 1e9, 1),
                "agreement_us": round(t_agree * 1e6, 1), "agreement_GBps": round(b_agree / t_agree / 1e9, 1),
                "agreement_composed_us": round(r_agree * 1e6, 1),
                "apply_us": round(t_apply * 1e6, 1), "apply_GBps": round(S * 20 / t_apply / 1e9, 1),
                "apply_composed_us": round(r_apply * 1e6, 1),
                "apply_noise_us": round(t_apply_n * 1e6, 1), "apply_noise_composed_us": round(r_apply_n * 1e6, 1),
                "add_noise_scaled_us": round(t_noise * 1e6, 1)})
    return out


# SparseFed (topk.hip): the CIFAR model's aggregated entries, k = 5 % as in configs/cifar_sparse.yaml
TOPK = [("topk.cifar", 2_802_430, 0.05)]


def _bench_topk(name, L, frac, reps, dev):
    """The radix select (with the residual addition in its first pass) and the sparse apply on a
    residual that a round's total is added into before every select, against the ``ops.reference``
    torch path on the same device (``torch.sort`` of the keys: timed eagerly) and checked to give
    its bits, and ``add_noise_scaled`` (plain FedAvg's dense update) at the same L for scale.  The
    apply's steady state needs the select before it (a second apply at the same threshold finds
    nothing to keep), so the pair is timed and ``apply_us`` is the pair minus the select.  The
    select must move L * 24 bytes in its first pass and L * 8 in each of the other seven: GB/s
    counts those L * 80."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    k = max(1, int(L * frac))
    total = 0.01 * torch.randn(L, device=dev, dtype=torch.float64)
    total[::7] = 0.0
    base = torch.randn(L, device=dev)
    coef = 0.1 / 10
    ra, rb = (torch.zeros(L, dtype=torch.float64, device=dev) for _ in range(2))
    da, db = base.clone(), base.clone()
    ws = H.topk_workspace(dev)
    for _ in range(3):                                            # three rounds: the residual carries over
        sa, sb = H.topk_threshold(ra, total, k, ws=ws), R.topk_threshold(rb, total, k)
        assert torch.equal(sa, sb) and torch.equal(ra, rb)
        H.topk_apply(da, ra, sa, coef)
        R.topk_apply(db, rb, sb, coef)
        assert torch.equal(sa, sb) and torch.equal(ra, rb) and torch.equal(da, db)
    out = {"shape": name, "L": L, "k": k, "kept": int(sa[1])}

    def pair(o, resid, dst):
        o.topk_apply(dst, resid, o.topk_threshold(resid, total, k), coef)

    resid, dst = ra.clone(), base.clone()
    t_pair = _time(lambda: pair(H, resid, dst), reps)
    t_select = _time(lambda: H.topk_threshold(resid, total, k, ws=ws), reps)
    t_noise = _time(lambda: H.add_noise_scaled(dst, total, coef, 0.0, 1, False), reps)
    resid, dst = ra.clone(), base.clone()
    r_pair = _time_eager(lambda: pair(R, resid, dst), reps)
    r_select = _time_eager(lambda: R.topk_threshold(resid, total, k), reps)
    out.update({"select_us": round(t_select * 1e6, 1), "select_GBps": round(L * 80 / t_select / 1e9, 1),
                "apply_us": round((t_pair - t_select) * 1e6, 1), "select_apply_us": round(t_pair * 1e6, 1),
                "select_reference_us": round(r_select * 1e6, 1),
                "apply_reference_us": round((r_pair - r_select) * 1e6, 1),
                "select_apply_reference_us": round(r_pair * 1e6, 1),
                "add_noise_scaled_us": round(t_noise * 1e6, 1)})
    return out


# the PGD attacker's per-step projection (flat.hip): the CIFAR model's aggregated entries, a lone
# attacker (the solo tail's G = 1 graph) and a full group of 10
PGD = [("pgd.cifar.g1", 1, 2_802_430), ("pgd.cifar.g10", 10, 2_802_430)]


def _bench_pgd(name, G, n, reps, dev, rounds=5, inner=10):
    """``project_to_ball`` with every replica projecting, against ``dist_loss_grad`` at the same n and
    G: the same two-launch shape (per-block partials of ||w - base||^2, then an element-wise pass that
    sums them).  Past the norm launch's w and base, dist_loss_grad's second launch moves 4 streams of n
    floats (w, base and grads in, grads out) and the projection's 3 (w and base in, w out): 6 to 5
    over the two launches (GB/s counts those), 4 to 3 in the element-wise pass alone.  A projected
    state does not project again, so one timed graph restores w (a copy, timed on its own and
    subtracted) and makes ``inner`` calls with radii shrinking by 1 % each: all of them project
    (checked on the counter).  The two are timed in turn, ``rounds`` times over: medians and
    min .. max.  The rows are [G, n] views of buffers 4-float aligned in width, so every row takes
    the float4 body.  dist_loss_grad is launched on preallocated outputs (its wrapper's zero fill and
    square root are not timed)."""
    torch.manual_seed(0)
    stride = (n + 3) // 4 * 4
    base = torch.randn(G, stride, device=dev)[:, :n]
    w0 = (base + 0.01 * torch.randn(G, n, device=dev))
    w = torch.zeros(G, stride, device=dev)[:, :n]
    grads = torch.randn(G, n, device=dev)
    trig = torch.zeros(G, dtype=torch.int32, device=dev)
    one = torch.ones(G, dtype=torch.int32, device=dev)
    norm = torch.zeros(G, dtype=torch.float64, device=dev)
    count = torch.zeros(G, dtype=torch.int32, device=dev)
    r0 = 0.5 * float(torch.linalg.vector_norm((w0[0] - base[0]).double()))

    def restore():
        w.copy_(w0)

    def projections():
        restore()
        for k in range(inner):
            H.project_to_ball(w, base, n, trig, one, r0 * 0.99 ** k, norm, count)

    projections()
    assert count.tolist() == [inner] * G, count.tolist()
    w.copy_(w0)
    nrm2 = torch.zeros(G, device=dev)
    part = torch.empty(G, 256, device=dev)

    def dist():
        H._call("dba_dist_loss_grad", w.data_ptr(), w.stride(0), base.data_ptr(), base.stride(0), grads.data_ptr(), n, G,
                trig.data_ptr(), one.data_ptr(), 0.7, nrm2.data_ptr(), part.data_ptr(), H._stream())

    fns = {"project": lambda: _time(projections, reps, inner=1), "restore": lambda: _time(restore, reps, inner=1),
           "dist_loss_grad": lambda: _time(dist, reps, inner=inner)}
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(fn())
    times["project"] = [(p - c) / inner for p, c in zip(times["project"], times["restore"])]
    out = {"shape": name, "G": G, "n": n, "rounds": rounds}
    for k, streams in (("project", 5), ("dist_loss_grad", 6)):
        v = sorted(times[k])
        med = v[len(v) // 2]
        out.update({f"{k}_us": round(med * 1e6, 2), f"{k}_min_us": round(v[0] * 1e6, 2),
                    f"{k}_max_us": round(v[-1] * 1e6, 2), f"{k}_GBps": round(streams * G * n * 4 / med / 1e9, 1)})
    out["restore_us"] = round(sorted(times["restore"])[rounds // 2] * 1e6, 2)
    out["project_vs_dist_loss_grad"] = round(out["project_us"] / out["dist_loss_grad_us"], 3)
    out["yardstick"] = 1.25
    return out


# the Neurotoxin attacker's two ops at the CIFAR model's P = 2,797,610 parameters: the per-step
# restore (flat.hip) for a lone attacker and a full group of 10, the server's mask build (nmask.hip)
NTX_P = 2_797_610
NTX_RESTORE = [("ntx.restore.cifar.g1", 1, NTX_P), ("ntx.restore.cifar.g10", 10, NTX_P)]
NTX_MASK = [("ntx.mask.cifar", NTX_P, 0.95)]


def _bench_ntx_restore(name, G, n, reps, dev, rho=0.95, rounds=5, inner=10):
    """``mask_restore`` with every replica gated in, under the rho = 0.95 mask of a random update,
    against ``project_to_ball`` at the same n and G in the same process (``_bench_pgd``'s row).  The
    op never reads w and copies a dropped entry whatever w holds, so repeated calls cost the same:
    ``inner`` calls per timed graph, ``rounds`` times over, the median and min .. max.  It must
    move the mask (n / 8 bytes per replica) and 8 bytes per dropped entry (base in, w out): GB/s
    counts those.  Rows are float4-aligned."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    stride = (n + 3) // 4 * 4
    base = torch.randn(G, stride, device=dev)[:, :n]
    w = (base + 0.01 * torch.randn(G, n, device=dev))
    w_old = torch.randn(n, device=dev)
    w_new = w_old + 0.01 * torch.randn(n, device=dev)
    k = max(1, int(rho * n))
    mask = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    kept = int(H.neurotoxin_mask(w_new, w_old, n, k, mask)[1])
    trig = torch.zeros(G, dtype=torch.int32, device=dev)
    one = torch.ones(G, dtype=torch.int32, device=dev)
    count = torch.zeros(G, dtype=torch.int32, device=dev)
    H.mask_restore(w, base, n, trig, one, mask, count)
    assert count.tolist() == [1] * G
    keep = R.neurotoxin_kept(mask, n).to(dev)
    assert bool((w[:, ~keep] == base[:, ~keep]).all()) and bool((w[:, keep] != base[:, keep]).any())
    v = sorted(_time(lambda: H.mask_restore(w, base, n, trig, one, mask, count), reps, inner=inner)
               for _ in range(rounds))
    med = v[len(v) // 2]
    moved = G * (n / 8 + 8 * (n - kept))
    pgd = _bench_pgd(name, G, n, reps, dev, rounds=rounds, inner=inner)
    return {"shape": name, "G": G, "n": n, "rho": rho, "k": k, "kept": kept, "rounds": rounds,
            "mask_restore_us": round(med * 1e6, 2), "mask_restore_min_us": round(v[0] * 1e6, 2),
            "mask_restore_max_us": round(v[-1] * 1e6, 2), "mask_restore_GBps": round(moved / med / 1e9, 1),
            "project_us": pgd["project_us"], "project_min_us": pgd["project_min_us"],
            "project_max_us": pgd["project_max_us"],
            "mask_restore_vs_project": round(med * 1e6 / pgd["project_us"], 3)}


def _bench_ntx_mask(name, P, rho, reps, dev, rounds=5):
    """``neurotoxin_mask`` (the memset, four histogram + scan passes and the ballot pass) on a random
    update, checked against the ``ops.reference`` form, ``rounds`` times over: the median and
    min .. max.  Each of its five passes over the coordinates reads w_new and w_old: GB/s counts P * 40
    bytes."""
    from dba_mod_amd.ops import reference as R
    torch.manual_seed(0)
    w_old = torch.randn(P, device=dev)
    w_new = w_old + 0.01 * torch.randn(P, device=dev)
    k = max(1, int(rho * P))
    nw = (P + 63) // 64
    mask = torch.empty(nw, dtype=torch.int64, device=dev)
    ws = H.neurotoxin_workspace(dev)
    sel = H.neurotoxin_mask(w_new, w_old, P, k, mask, ws)
    want = torch.empty(nw, dtype=torch.int64)
    sel_ref = R.neurotoxin_mask(w_new.cpu(), w_old.cpu(), P, k, want)
    assert sel.tolist() == sel_ref.tolist() and torch.equal(mask.cpu(), want)
    v = sorted(_time(lambda: H.neurotoxin_mask(w_new, w_old, P, k, mask, ws), reps) for _ in range(rounds))
    med = v[len(v) // 2]
    return {"shape": name, "P": P, "rho": rho, "k": k, "kept": int(sel[1]), "rounds": rounds,
            "mask_us": round(med * 1e6, 1), "mask_min_us": round(v[0] * 1e6, 1), "mask_max_us": round(v[-1] * 1e6, 1),
            "mask_GBps": round(P * 40 / med / 1e9, 1)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default="", help="substring filter on shape names")
    ap.add_argument("--ximg", type=int, default=-1, help="hip.set_ximg: 1 ximg2_kernel, 2 ximg_kernel, 0 implicit GEMM")
    ap.add_argument("--xstage", type=int, default=-1, help="hip.set_xstage: 1 LDS-DMA weight stages (each kernel's default), 2 the weight ring, 3 staged everywhere")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    H.set_ximg(args.ximg)
    H.set_xstage(args.xstage)
    rows = []
    for name, G, N, Hh, Cin, Cout, k, s, p in SHAPES:
        if args.only not in name:
            continue
        rows.append(_bench_fp32(name, G, N, Hh, Cin, Cout, k, s, p, args.reps, dev))
        print(json.dumps(rows[-1]), flush=True)
    for name, G, N, W, C, C2 in DOWN:
        if args.only in name:
            rows.append(_bench_down(name, G, N, W, C, C2, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, G, B, C in XENT:
        if args.only in name:
            rows.append(_bench_xent(name, G, B, C, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, n, S in CLIP:
        if args.only in name:
            rows.append(_bench_clip(name, n, S, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, n, S in KRUM:
        if args.only in name:
            rows.append(_bench_krum(name, n, S, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, n, S, k in TRIM:
        if args.only in name:
            rows.append(_bench_trim(name, n, S, k, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, t, S, f in BULYAN:
        if args.only in name:
            rows.append(_bench_bulyan(name, t, S, f, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, n, S in FLAME:
        if args.only in name:
            rows.append(_bench_flame(name, n, S, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, n, S, theta in RLR:
        if args.only in name:
            rows.append(_bench_rlr(name, n, S, theta, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, L, frac in TOPK:
        if args.only in name:
            rows.append(_bench_topk(name, L, frac, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, G, n in PGD:
        if args.only in name:
            rows.append(_bench_pgd(name, G, n, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, G, n in NTX_RESTORE:
        if args.only in name:
            rows.append(_bench_ntx_restore(name, G, n, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    for name, P, rho in NTX_MASK:
        if args.only in name:
            rows.append(_bench_ntx_mask(name, P, rho, args.reps, dev))
            print(json.dumps(rows[-1]), flush=True)
    if args.only in "eval.chunk":
        rows.append(_bench_eval_chunk(17, 1024, max(3, args.reps // 4), dev))
        print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())

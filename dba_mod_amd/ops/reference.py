"""Plain-PyTorch fp32 reference implementation of every framework op.

This is (a) the implementation used for CPU tensors (the world_size=1 plumbing config and
the unit tests) and (b) the numerics oracle the HIP kernels are tested against.  Layouts
are the device layouts: activations ``[G, N, H, W, C]`` (group = client replica / eval job),
conv weights ``[Gm, Cout, KH, KW, Cin]`` (possibly a strided view into a flat parameter
buffer), per-group model selection ``wsel`` (group -> weight slot).

Semantics follow the reference's stock-PyTorch ops: BatchNorm2d in
train mode (biased var to normalise, unbiased var into running stats, momentum 0.1),
cross-entropy mean/sum reductions, ``torch.optim.SGD`` with momentum + weight decay.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import bnstate as bs
from . import rng

Tensor = torch.Tensor


def _sel(w: Tensor, wsel: Optional[Tensor], g: int) -> Tensor:
    return w[int(wsel[g])] if wsel is not None else w[g]


def _nchw(x: Tensor) -> Tensor:
    return x.permute(0, 3, 1, 2)


def _nhwc(x: Tensor) -> Tensor:
    return x.permute(0, 2, 3, 1)


# Compute dtype of the reference implementation: fp32 (the kernels' accumulation dtype);
# tests switch it to fp64 to get an oracle free of fp32 ReLU-mask flips.
COMPUTE_DTYPE = torch.float32


def _cdt() -> torch.dtype:
    return COMPUTE_DTYPE


def _rows_valid(nvalid: Optional[Tensor], g: int, n: int) -> int:
    return n if nvalid is None else int(nvalid[g])


# ------------------------------------------------------------------------- data ingest
def gather_images(src: Tensor, labels: Tensor, idx: Tensor, trig_masks: Tensor, trig_id: Tensor,
                  poison_n: Tensor, target: int, flip_seeds: Optional[Tensor], out_dtype: torch.dtype
                  ) -> Tuple[Tensor, Tensor]:
    """uint8 NHWC gather + /255 + optional h-flip + pixel trigger + relabel (K17/K19).

    Row ``b`` of group ``g`` is flipped iff ``hash2(flip_seeds[g], b) & 1`` (per-client
    seeds keep the result independent of how clients are placed on ranks/groups).
    """
    G, B = idx.shape
    _, H, W, C = src.shape
    valid = idx >= 0
    safe = idx.clamp(min=0).long()
    x = src[safe.reshape(-1)].reshape(G, B, H, W, C).to(torch.float32)
    y = labels.long()[safe.reshape(-1)].reshape(G, B)
    if flip_seeds is not None:
        ctr = torch.arange(B, dtype=torch.int64, device=src.device)[None, :].expand(G, B)
        flip = (rng.hash2(flip_seeds.to(torch.int64)[:, None], ctr) & 1).bool()
        x = torch.where(flip[..., None, None, None], x.flip(3), x)
    b_ar = torch.arange(B, device=src.device)[None, :]
    tid = trig_id.long()
    pois = (b_ar < poison_n.long()[:, None]) & (tid[:, None] >= 0) & valid
    if trig_masks.numel() > 0:
        m = trig_masks[tid.clamp(min=0)].bool()  # [G, H, W]
        pm = pois[:, :, None, None] & m[:, None, :, :]
        x = torch.where(pm[..., None], torch.full_like(x, 255.0), x)
    y = torch.where(pois, torch.full_like(y, int(target)), y)
    x = x * (1.0 / 255.0)
    x = torch.where(valid[..., None, None, None], x, torch.zeros_like(x))
    y = torch.where(valid, y, torch.full_like(y, -1))
    return x.to(out_dtype), y.to(torch.int32)


def gather_rows(src: Tensor, labels: Tensor, idx: Tensor, trig_cols: Tensor, trig_vals: Tensor,
                trig_id: Tensor, poison_n: Tensor, target: int, out_dtype: torch.dtype
                ) -> Tuple[Tensor, Tensor]:
    """Tabular (LOAN) gather + feature trigger (K18): x[:, col] = value for poisoned rows."""
    G, B = idx.shape
    Fd = src.shape[1]
    valid = idx >= 0
    safe = idx.clamp(min=0).long()
    x = src[safe.reshape(-1)].reshape(G, B, Fd).to(torch.float32).clone()
    y = labels.long()[safe.reshape(-1)].reshape(G, B)
    b_ar = torch.arange(B, device=src.device)[None, :]
    tid = trig_id.long()
    pois = (b_ar < poison_n.long()[:, None]) & (tid[:, None] >= 0) & valid
    for g in range(G):
        if int(tid[g]) < 0:
            continue
        cols = trig_cols[int(tid[g])]
        vals = trig_vals[int(tid[g])]
        rows = pois[g].nonzero().flatten()
        for k in range(cols.shape[0]):
            c = int(cols[k])
            if c >= 0:
                x[g, rows, c] = float(vals[k])
    y = torch.where(pois, torch.full_like(y, int(target)), y)
    x = torch.where(valid[..., None], x, torch.zeros_like(x))
    y = torch.where(valid, y, torch.full_like(y, -1))
    return x.to(out_dtype), y.to(torch.int32)


# ------------------------------------------------------------------------------ conv
def conv2d(x: Tensor, w: Tensor, wsel: Optional[Tensor], stride: int, pad: int,
           bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
           relu: bool = False, nvalid: Optional[Tensor] = None,
           out_dtype: Optional[torch.dtype] = None, bn_stats: bool = False) -> Tensor:
    """y = act(conv(x, w) + bias + residual); NHWC in/out (K1, K3, K4, K8).  ``bn_stats`` (a
    hint that y feeds a training BN) only matters to the HIP backend."""
    G = x.shape[0]
    outs = []
    for g in range(G):
        wg = _sel(w, wsel, g).to(_cdt()).permute(0, 3, 1, 2)  # [Cout, Cin, KH, KW]
        bg = _sel(bias, wsel, g).to(_cdt()) if bias is not None else None
        yg = F.conv2d(_nchw(x[g].to(_cdt())), wg, bg, stride=stride, padding=pad)
        yg = _nhwc(yg)
        if residual is not None:
            yg = yg + residual[g].to(_cdt())
        if relu:
            yg = torch.relu(yg)
        outs.append(yg)
    if out_dtype == torch.float32 and _cdt() == torch.float64:
        out_dtype = torch.float64
    return torch.stack(outs).to(out_dtype or x.dtype)


def basic_block_ok(x: Tensor, w1: Tensor, w2: Tensor) -> bool:
    """Whether the backend runs an evaluation BasicBlock as one fused op (HIP: xblock.hip);
    the reference runs the two convs."""
    return False


def basic_block_eval(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                     wsel: Optional[Tensor] = None, nvalid: Optional[Tensor] = None) -> Tensor:
    """relu(conv2(relu(conv1(x) + b1)) + b2 + x), 3x3 stride-1 convs with BN folded into w / b
    (the identity BasicBlock of the reference models/resnet_cifar.py:14-37, evaluated)."""
    h = conv2d(x, w1, wsel, 1, 1, bias=b1, relu=True, nvalid=nvalid)
    return conv2d(h, w2, wsel, 1, 1, bias=b2, residual=x, relu=True, nvalid=nvalid)


def stem_block_ok(x: Tensor, w0: Tensor, w1: Tensor, w2: Tensor) -> bool:
    """Whether the backend runs the stem + first BasicBlock as one fused op (HIP: xblock.hip
    STEM variant); the reference runs the three convs."""
    return False


def stem_block_eval(x: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                    wsel: Optional[Tensor] = None, nvalid: Optional[Tensor] = None) -> Tensor:
    """The CIFAR ResNet stem relu(conv(x) + b0) (3x3, pad 1) followed by the identity
    BasicBlock of :func:`basic_block_eval`, BN folded (reference models/resnet_cifar.py:80-88)."""
    s = conv2d(x, w0, wsel, 1, 1, bias=b0, relu=True, nvalid=nvalid)
    return basic_block_eval(s, w1, b1, w2, b2, wsel, nvalid)


def down_block_ok(a: Tensor, w2: Tensor, x2: Tensor, wsc: Tensor) -> bool:
    """Whether the backend runs a downsampling block's conv2 with its 1x1 stride-2 shortcut as
    one fused op (HIP: xconv_fwd.hip dba_xdown_fwd); the reference runs the two convs."""
    return False


def down_block_eval(a: Tensor, w2: Tensor, b2: Tensor, x2: Tensor, wsc: Tensor, bsc: Tensor,
                    wsel: Optional[Tensor] = None, nvalid: Optional[Tensor] = None) -> Tensor:
    """relu(conv3x3(a, w2) + b2 + conv1x1_s2(x2, wsc) + bsc), BN folded: the second half of a
    downsampling BasicBlock with its shortcut (reference models/resnet_cifar.py:24-36), evaluated."""
    sc = conv2d(x2, wsc, wsel, 2, 0, bias=bsc, nvalid=nvalid)
    return conv2d(a, w2, wsel, 1, 1, bias=b2, residual=sc, relu=True, nvalid=nvalid)


def _valid_mask(t: Tensor, nvalid: Optional[Tensor]) -> Tensor:
    """[G, N, 1, 1, 1] (bool) of the valid images of each replica."""
    G, N = t.shape[:2]
    n = torch.full((G,), N, dtype=torch.int64) if nvalid is None else nvalid.long().cpu()
    v = torch.arange(N)[None, :] < n[:, None]
    return v.view(G, N, *([1] * (t.dim() - 2))).to(t.device)


def _coef(st: "bs.BnStat", row: int, t: Tensor) -> Tensor:
    """Row ``row`` of a BN's coefficients broadcast over ``t`` [G, N, H, W, C]."""
    return st.coef[:, row].view(t.shape[0], *([1] * (t.dim() - 2)), t.shape[-1]).to(t.dtype)


def lazy_value(a: "bs.LazyBN", nvalid: Optional[Tensor] = None) -> Tensor:
    """relu?(y * scale + shift) of a lazy training-BN output (zero on invalid images).  A
    replayed ReLU decision (``ops.branches``) is taken from ``a.stat.relu_mask``."""
    v = a.y * _coef(a.stat, bs.SCALE, a.y) + _coef(a.stat, bs.SHIFT, a.y)
    if a.relu:
        m = getattr(a.stat, "relu_mask", None)   # replayed decisions (ops.branches)
        tiny = 1e-300 if v.dtype == torch.float64 else 1e-30
        v = torch.relu(v) if m is None else torch.where(m.to(v.device), v.clamp(min=tiny), torch.zeros_like(v))
    return torch.where(_valid_mask(v, nvalid), v, torch.zeros_like(v))


def lazy_grad_value(lg: "bs.LazyGrad", nvalid: Optional[Tensor] = None) -> Tensor:
    """dy = A * d + B * y + K of a training BN's input gradient (zero on invalid images)."""
    st = lg.stat
    v = _coef(st, bs.A, lg.d) * lg.d + _coef(st, bs.B, lg.y) * lg.y + _coef(st, bs.K, lg.d)
    return torch.where(_valid_mask(v, nvalid), v, torch.zeros_like(v)).to(lg.d.dtype)


def conv_bn_stats(x, w: Tensor, wsel: Optional[Tensor], stride: int, pad: int, nvalid: Optional[Tensor],
                  p: "bs.BnParams", relu: bool):
    """y = conv(x, w) and the training-BN statistics of y (running stats updated in place);
    x may be a lazy BN output.  Returns (y, BnStat) — the fused conv + BN forward
    (csrc/kernels/bnfuse.hpp); the BN output is :func:`lazy_value` of ``LazyBN(y, stat, relu)``."""
    xv = lazy_value(x, nvalid) if isinstance(x, bs.LazyBN) else x
    y = conv2d(xv, w, wsel, stride, pad, nvalid=nvalid)
    G, N = y.shape[:2]
    C = y.shape[-1]
    coef = torch.zeros(G, bs.ROWS, C, dtype=_cdt(), device=y.device)
    for g in range(G):
        n = _rows_valid(nvalid, g, N)
        if n == 0:
            continue
        flat = y[g, :n].to(_cdt()).reshape(-1, C)
        cnt = flat.shape[0]
        mean = flat.mean(0)
        var = flat.var(0, unbiased=False)
        invstd = torch.rsqrt(var + p.eps)
        unbiased = var * (cnt / max(cnt - 1, 1))
        p.rmean[g] = (1 - p.momentum) * p.rmean[g] + p.momentum * mean
        p.rvar[g] = (1 - p.momentum) * p.rvar[g] + p.momentum * unbiased
        sc = invstd * p.gamma[g].to(_cdt())
        coef[g, bs.MEAN], coef[g, bs.INV] = mean, invstd
        coef[g, bs.SCALE], coef[g, bs.SHIFT] = sc, p.beta[g].to(_cdt()) - mean * sc
        coef[g, bs.YMAX], coef[g, bs.YMIN] = flat.max(0).values, flat.min(0).values
    return y, bs.BnStat(coef, p)


def bn_apply(a: "bs.LazyBN", residual, relu: bool, nvalid: Optional[Tensor] = None) -> Tensor:
    """out = relu?(lazy BN value of ``a`` (its own ReLU not applied) + residual), residual a
    tensor, a lazy BN output or None: the stored output of a BasicBlock / the stem."""
    v = a.y * _coef(a.stat, bs.SCALE, a.y) + _coef(a.stat, bs.SHIFT, a.y)
    if isinstance(residual, bs.LazyBN):
        v = v + lazy_value(residual, nvalid)
    elif residual is not None:
        v = v + residual.to(v.dtype)
    if relu:
        v = torch.relu(v)
    return torch.where(_valid_mask(v, nvalid), v, torch.zeros_like(v)).to(a.y.dtype)


def bn_finish(g: Optional[Tensor], fin: "bs.Finish", nvalid: Optional[Tensor] = None,
              pool: Optional[Tensor] = None, hw: Optional[Tuple[int, int]] = None) -> "bs.Fin":
    """Finish the gradient of a BN output: d = g where the output is > 0, then the backward
    sums of BN a (and BN b) -> dbeta += sum d, dgamma += sum d * xhat and the coefficients A, B,
    K of dy = A d + B y + K (bn_train_bwd's arithmetic).  ``pool`` ([G, N, 1, 1, C]): g is the
    global average pool's gradient of it (``avgpool_global_bwd``)."""
    if pool is not None:
        g = avgpool_global_bwd(pool, hw)
    ya = fin.ya
    d = g.to(_cdt())
    if fin.mask_out is not None:
        d = d * (fin.mask_out.to(_cdt()) > 0)
    elif fin.lazy:
        m = getattr(fin.sa, "relu_mask", None)
        pre = ya.to(_cdt()) * _coef(fin.sa, bs.SCALE, ya).to(_cdt()) + _coef(fin.sa, bs.SHIFT, ya).to(_cdt())
        d = d * ((pre > 0) if m is None else m.to(d.device))
    d = torch.where(_valid_mask(d, nvalid), d, torch.zeros_like(d))
    G, N = d.shape[:2]
    C = d.shape[-1]
    for y, st in ((ya, fin.sa), (fin.yb, fin.sb)):
        if st is None:
            continue
        p = st.params
        for gg in range(G):
            n = _rows_valid(nvalid, gg, N)
            if n == 0:
                continue
            dg = d[gg, :n].reshape(-1, C)
            mean, inv = st.coef[gg, bs.MEAN].to(_cdt()), st.coef[gg, bs.INV].to(_cdt())
            xhat = (y[gg, :n].to(_cdt()).reshape(-1, C) - mean) * inv
            cnt = dg.shape[0]
            sd, sdx = dg.sum(0), (dg * xhat).sum(0)
            p.dbeta[gg] += sd.to(p.dbeta.dtype)
            p.dgamma[gg] += sdx.to(p.dgamma.dtype)
            A = p.gamma[gg].to(_cdt()) * inv
            B = -A * inv * sdx / cnt
            st.coef[gg, bs.A], st.coef[gg, bs.B] = A, B
            st.coef[gg, bs.K] = -A * sd / cnt - B * mean
    return bs.Fin(d.to(g.dtype), fin.stats())


def wgrad_prepare(dy, x, nvalid=None):
    """HIP backend: attaches the operands' fp16-pair maxima before the weight gradient moves to
    a side stream.  Nothing to prepare here."""
    return None


def wgrad_flush(defer: list) -> None:
    """Backend hook for deferred weight-gradient reductions; the reference has none."""
    if defer:
        defer.clear()


def prepare_dgrad_weights(ref: Tensor, items: list) -> dict:
    """Backend hook for pre-transposed data-gradient weights; the reference needs none."""
    return {}


def conv2d_dgrad(dy: Tensor, w: Tensor, wsel: Optional[Tensor], stride: int, pad: int,
                 in_hw: Tuple[int, int], nvalid: Optional[Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None, accum: Optional[Tensor] = None,
                 wt: Optional[Tensor] = None, finish: Optional["bs.Finish"] = None):
    """dX of a conv; ``accum`` (the input's gradient from another branch) is added in.
    ``wt`` (a backend's pre-transposed weights) is ignored here.  ``finish``: dX is the complete
    gradient of a training-BN output — return it finished (:func:`bn_finish`, a ``Fin``)."""
    if finish is not None:
        dx = conv2d_dgrad(dy, w, wsel, stride, pad, in_hw, nvalid, out_dtype, accum, wt)
        return bn_finish(dx, finish, nvalid)
    G, N = dy.shape[:2]
    cin = w.shape[-1]
    outs = []
    for g in range(G):
        wg = _sel(w, wsel, g).to(_cdt()).permute(0, 3, 1, 2)
        dx = torch.nn.grad.conv2d_input((N, cin, in_hw[0], in_hw[1]), wg, _nchw(dy[g].to(_cdt())),
                                        stride=stride, padding=pad)
        outs.append(_nhwc(dx))
    dx = torch.stack(outs)
    if accum is not None:
        dx = dx + accum.to(dx.dtype)
    return dx.to(out_dtype or dy.dtype)


def conv2d_wgrad(dy, x, stride: int, pad: int, kh: int, kw: int,
                 dw: Tensor, dbias: Optional[Tensor] = None, nvalid: Optional[Tensor] = None,
                 defer: Optional[list] = None) -> Optional[Tensor]:
    """dw[g] += sum_rows dy (x) x  (fp32 accumulate into the flat grad buffer view).
    ``defer`` (a backend's batched-reduction queue) is unused here: the sum is immediate.
    ``dy`` may be a :class:`LazyGrad` (its value is returned, for the data gradient) and ``x`` a
    :class:`LazyBN`."""
    out = None
    if isinstance(dy, bs.LazyGrad):
        dy = out = lazy_grad_value(dy, nvalid)
    if isinstance(x, bs.LazyBN):
        x = lazy_value(x, nvalid)
    G = dy.shape[0]
    cout = dy.shape[-1]
    cin = x.shape[-1]
    for g in range(G):
        gw = torch.nn.grad.conv2d_weight(_nchw(x[g].to(_cdt())), (cout, cin, kh, kw),
                                         _nchw(dy[g].to(_cdt())), stride=stride, padding=pad)
        dw[g] += gw.permute(0, 2, 3, 1)
        if dbias is not None:
            dbias[g] += dy[g].to(_cdt()).sum(dim=(0, 1, 2))
    return out


# ------------------------------------------------------------------------ batch norm
def relu_mask_bwd(dout: Tensor, out: Tensor) -> Tensor:
    return (dout.to(_cdt()) * (out.to(_cdt()) > 0)).to(dout.dtype)


def bn_fold(w: Tensor, conv_bias: Optional[Tensor], gamma: Tensor, beta: Tensor,
            rmean: Tensor, rvar: Tensor, eps: float, out_dtype: torch.dtype,
            amax_slot: Optional[Tensor] = None, split: bool = True) -> Tuple[Tensor, Tensor]:
    """Eval-mode BN folded into the preceding conv: w' = w*s, b' = (b - mean)*s + beta.
    (``amax_slot`` / ``split``: the HIP backend's operand-max slot and fp16-pair split; unused here.)"""
    s = gamma.to(_cdt()) * torch.rsqrt(rvar.to(_cdt()) + eps)  # [Gm, Cout]
    wf = w.to(_cdt()) * s[:, :, None, None, None]
    b0 = conv_bias.to(_cdt()) if conv_bias is not None else torch.zeros_like(s)
    bf = (b0 - rmean.to(_cdt())) * s + beta.to(_cdt())
    return wf.to(out_dtype), bf.contiguous()


# --------------------------------------------------------------------------- pooling
def maxpool2d(x: Tensor, k: int, s: int, p: int, want_ind: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """K7 max-pool; ``want_ind`` is a HIP hint (evaluation stores no indices): the reference
    always returns them."""
    G, N, H, W, C = x.shape
    y, ind = F.max_pool2d(_nchw(x.to(_cdt()).reshape(G * N, H, W, C)), k, s, p, return_indices=True)
    return (_nhwc(y).reshape(G, N, y.shape[2], y.shape[3], C).to(x.dtype),
            _nhwc(ind).reshape(G, N, y.shape[2], y.shape[3], C).to(torch.int32))


def maxpool2d_bwd(dy: Tensor, ind: Tensor, in_shape: Sequence[int], k: int, s: int, p: int) -> Tensor:
    G, N, H, W, C = in_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    dyn = _nchw(dy.to(_cdt()).reshape(G * N, Ho, Wo, C)).contiguous()
    indn = _nchw(ind.long().reshape(G * N, Ho, Wo, C)).contiguous()
    dx = torch.zeros(G * N, C, H * W, dtype=_cdt(), device=dy.device)
    dx.scatter_add_(2, indn.reshape(G * N, C, -1), dyn.reshape(G * N, C, -1))
    return _nhwc(dx.reshape(G * N, C, H, W)).reshape(G, N, H, W, C).to(dy.dtype)


def avgpool_global(x: Tensor) -> Tensor:
    return x.to(_cdt()).mean(dim=(2, 3), keepdim=True).to(x.dtype)


def avgpool_global_bwd(dy: Tensor, hw: Tuple[int, int]) -> Tensor:
    H, W = hw
    return (dy.to(_cdt()).expand(-1, -1, H, W, -1) / (H * W)).to(dy.dtype).contiguous()


# --------------------------------------------------------------------------- dropout
def dropout(x: Tensor, p: float, seeds: Tensor, salt: int) -> Tensor:
    """Inverted dropout; element i of group g kept iff uniform(salted(seeds[g]), i) >= p."""
    G = x.shape[0]
    per = x[0].numel()
    ctr = torch.arange(per, dtype=torch.int64, device=x.device)[None, :].expand(G, per)
    s = rng.salted(seeds.to(torch.int64), salt)[:, None]
    keep = (rng.uniform01(s, ctr) >= p).reshape(x.shape)
    return (x.to(_cdt()) * keep / (1.0 - p)).to(x.dtype)


def dropout_bwd(dy: Tensor, p: float, seeds: Tensor, salt: int) -> Tensor:
    return dropout(dy, p, seeds, salt)


# ---------------------------------------------------------------------------- loss
def softmax_xent(logits: Tensor, labels: Tensor, mean: bool, want_grad: bool,
                 stats: Optional[Tensor] = None, slot: Optional[Tensor] = None,
                 nvalid: Optional[Tensor] = None, grad_dtype: Optional[torch.dtype] = None,
                 loss_dtype: Optional[torch.dtype] = None) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """Per-group CE (mean over valid rows or sum) + correct count + dlogits (K9).

    ``grad_dtype``: dtype of dlogits (default: the logits' dtype).  ``loss_dtype`` fp64: the
    per-row losses are summed in fp64 (the sum then does not depend on how rows are grouped
    into chunks or sharded over ranks).

    Rows with label < 0 are padding.  dlogits corresponds to the *mean* loss when
    ``mean`` (training) and to the sum otherwise.  With ``stats`` ([3, G*max_slots] fp32),
    also accumulates (loss, correct, nvalid) of group g into column g*max_slots + slot[g]
    (the per-client per-internal-epoch training statistics).
    """
    G, B, C = logits.shape
    lf = logits.to(_cdt())
    lab = labels.long()
    valid = lab >= 0
    logp = torch.log_softmax(lf, dim=-1)
    nll = -logp.gather(-1, lab.clamp(min=0)[..., None]).squeeze(-1)
    nll = torch.where(valid, nll, torch.zeros_like(nll))
    cnt = valid.sum(1).clamp(min=1).to(_cdt())
    if loss_dtype == torch.float64:
        nll = nll.to(torch.float64)
        cnt = cnt.to(torch.float64)
    loss = nll.sum(1) / cnt if mean else nll.sum(1)
    pred = lf.argmax(-1)
    correct = ((pred == lab) & valid).sum(1).to(_cdt())
    dl = None
    if want_grad:
        dl = torch.softmax(lf, -1)
        dl = dl - F.one_hot(lab.clamp(min=0), C).to(_cdt())
        dl = torch.where(valid[..., None], dl, torch.zeros_like(dl))
        if mean:
            dl = dl / cnt[:, None, None]
        dl = dl.to(grad_dtype or logits.dtype)
    if stats is not None:
        accumulate_step_stats(stats, slot, loss, correct, nvalid)
    return loss, correct, dl


def accumulate_step_stats(stats: Tensor, slot: Tensor, loss: Tensor, correct: Tensor, nvalid: Tensor) -> None:
    """stats[:, g*max_slots + slot[g]] += (loss[g], correct[g], nvalid[g])."""
    G = loss.shape[0]
    ms = stats.shape[1] // G
    col = torch.arange(G, device=stats.device, dtype=torch.int64) * ms + slot.long()
    stats[0].index_add_(0, col, loss.to(stats.dtype))
    stats[1].index_add_(0, col, correct.to(stats.dtype))
    stats[2].index_add_(0, col, nvalid.to(stats.dtype))


# ------------------------------------------------------------------------- optimizer
def sgd_step(params: Tensor, grads: Tensor, mom: Tensor, lr: Tensor, first: Tensor, active: Tensor,
             momentum: float, wd: float, fg_accum: Optional[Tensor] = None) -> None:
    """torch.optim.SGD(momentum, weight_decay) on [G, P] flat buffers (K10).

    ``first[g]`` marks the first step of a freshly created optimizer (buffer := d_p).
    ``fg_accum`` (FoolsGold) accumulates the raw per-batch gradients (image_train.py:94-100).
    """
    for g in range(params.shape[0]):
        if int(active[g]) == 0:
            continue
        gr = grads[g]
        if fg_accum is not None:
            fg_accum[g] += gr
        dp = gr + wd * params[g]
        if int(first[g]):
            mom[g] = dp
        else:
            mom[g] = momentum * mom[g] + dp
        params[g] -= float(lr[g]) * mom[g]


def dist_loss_grad(w: Tensor, base: Tensor, grads: Tensor, trig: Tensor, active: Tensor,
                   alpha: float) -> Tensor:
    """Anomaly-evasion loss a*CE + (1-a)*||w - w_g||_2 (helper.py:111-123, image_train.py:87-90).

    For replicas in a poison phase (``trig >= 0``) rewrites ``grads`` (the CE gradient) to
    ``a*g + (1-a)(w - base)/||w - base||`` (0 where w == base, torch's norm subgradient);
    returns the per-replica distance ``||w - base||`` over the parameter region.
    """
    G, P = grads.shape
    out = torch.zeros(G, dtype=torch.float32, device=grads.device)
    for g in range(G):
        if int(trig[g]) < 0 or int(active[g]) == 0:
            continue
        d = w[g, :P] - base[g, :P]
        nr = torch.linalg.vector_norm(d.double()).float()
        out[g] = nr
        c = (1.0 - alpha) / nr if float(nr) > 0 else 0.0
        grads[g] = alpha * grads[g] + c * d
    return out


def project_to_ball(w: Tensor, base: Tensor, n: int, trig: Tensor, active: Tensor, radius: float,
                    norm_out: Tensor, count: Tensor) -> None:
    """The norm-bounded (PGD) attacker's per-step projection (Sun et al. 2019; Wang et al. 2020).

    For replicas training with a trigger (``trig >= 0`` and active): ``norm_out[g]`` (fp64) :=
    ``||w[g, :n] - base[g, :n]||`` in fp64; where that norm is finite and ``> radius`` (strict),
    ``w[g, :n] := base + (radius / norm)(w - base)`` computed in fp64 and rounded once, and
    ``count[g] += 1``.  Nothing else is written: other replicas, a replica whose norm is within
    the radius or not finite, and entries at and past ``n`` keep their bits.
    """
    for g in range(w.shape[0]):
        if int(trig[g]) < 0 or int(active[g]) == 0:
            continue
        b = base[g, :n].double()
        d = w[g, :n].double() - b
        nr = torch.sqrt((d * d).sum())
        norm_out[g] = nr
        nrf = float(nr)
        if math.isfinite(nrf) and nrf > radius:
            w[g, :n] = (b + (radius / nrf) * d).float()
            count[g] += 1


def neurotoxin_all_kept(P: int, device=None) -> Tensor:
    """The mask that keeps every one of P coordinates: int64 [ceil(P / 64)], bits at and past P zero."""
    nw = (int(P) + 63) // 64
    m = torch.full((nw,), -1, dtype=torch.int64)
    if P % 64:
        m[-1] = (1 << (P % 64)) - 1
    return m.to(device) if device is not None else m


def neurotoxin_keys(w_new: Tensor, w_old: Tensor, P: int) -> Tensor:
    """The select keys of the Neurotoxin mask: the bits of ``u = w_new[:P] - w_old[:P]`` (one fp32
    subtraction) with the sign bit cleared, as (non-negative) int32.  Integer order is magnitude
    order: -0 and +0 are 0, denormals order, inf ranks above every finite value and a NaN above inf."""
    return (w_new[:P] - w_old[:P]).view(torch.int32) & 0x7FFFFFFF


def neurotoxin_check(w_new: Tensor, w_old: Tensor, P, k, mask_words: Tensor) -> Tuple[int, int]:
    """(P, k) of :func:`neurotoxin_mask`, checked the same way on every backend: contiguous fp32
    vectors of at least P entries, int64 mask words, ``k`` an integer with 1 <= k <= P."""
    P = int(P)
    assert w_new.dim() == 1 and w_old.dim() == 1 and w_new.dtype == torch.float32 and w_old.dtype == torch.float32
    assert w_new.is_contiguous() and w_old.is_contiguous()
    assert 1 <= P <= w_new.numel() and P <= w_old.numel(), (P, w_new.numel(), w_old.numel())
    assert mask_words.dtype == torch.int64 and mask_words.is_contiguous() and mask_words.numel() >= (P + 63) // 64
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"neurotoxin_mask: k {k!r}: expected an integer")
    if not 1 <= k <= P:
        raise ValueError(f"neurotoxin_mask: k {k} needs 1 <= k <= P = {P}")
    return P, k


def _pack_bits(keep: Tensor) -> Tensor:
    """bool [P] -> int64 [ceil(P / 64)], bit j % 64 of word j / 64 = keep[j], the tail bits 0."""
    P = keep.numel()
    nw = (P + 63) // 64
    bits = np.zeros(nw * 64, dtype=np.uint8)
    bits[:P] = keep.cpu().numpy()
    return torch.from_numpy(np.packbits(bits, bitorder="little").view("<i8").copy())


def neurotoxin_kept(mask_words: Tensor, P: int) -> Tensor:
    """bool [P] on the CPU: coordinate j's bit of the keep mask (:func:`neurotoxin_mask`)."""
    by = mask_words.detach().cpu().contiguous().numpy().view(np.uint8)
    return torch.from_numpy(np.unpackbits(by, bitorder="little")[:P].astype(np.bool_))


def neurotoxin_mask(w_new: Tensor, w_old: Tensor, P: int, k: int, mask_words: Tensor,
                    ws: Optional[Tensor] = None) -> Tensor:
    """The Neurotoxin attacker's coordinate mask (Zhang et al., ICML 2022; nmask.hip is the GPU form),
    from the update the server applied: with T the k-th smallest of :func:`neurotoxin_keys`,
    coordinate j < P is kept iff ``key[j] <= T`` (ties at T all kept, so m >= k are).  The first
    ``ceil(P / 64)`` of ``mask_words`` (int64) are rewritten in place: bit ``j % 64`` of word ``j //
    64`` is 1 when j is kept, bits at and past P are 0.  Returns ``sel`` int64 [2] on the vectors'
    device = (T, m).  1 <= k <= P or a ValueError.  ``ws``: a workspace the GPU form can reuse."""
    P, k = neurotoxin_check(w_new, w_old, P, k, mask_words)
    keys = neurotoxin_keys(w_new, w_old, P)
    T = torch.kthvalue(keys.cpu(), k).values
    keep = keys.cpu() <= T
    mask_words[:(P + 63) // 64] = _pack_bits(keep).to(mask_words.device)
    return torch.stack([T.to(torch.int64), keep.sum()]).to(w_new.device)


def mask_restore(w: Tensor, base: Tensor, P: int, trig: Tensor, active: Tensor, mask_words: Tensor,
                 count: Tensor) -> None:
    """The Neurotoxin attacker's per-step restore.  For replicas training with a trigger (``trig >=
    0`` and active): every entry ``j < P`` whose bit in ``mask_words`` (:func:`neurotoxin_mask`) is 0
    is set back to ``base[g, j]``, a copy, and ``count[g] += 1``.  Nothing else is written: kept
    entries, entries at and past ``P`` and the other replicas keep their bits."""
    keep = None
    for g in range(w.shape[0]):
        if int(trig[g]) < 0 or int(active[g]) == 0:
            continue
        if keep is None:
            keep = neurotoxin_kept(mask_words, P).to(w.device)
        w[g, :P] = torch.where(keep, w[g, :P], base[g, :P])
        count[g] += 1


# ---------------------------------------------------------------- flat / aggregation
def scale_from_base(w: Tensor, base: Tensor, gamma: float) -> Tensor:
    """Model-replacement scaling w' = base + gamma (w - base) (K11, image_train.py:166-171)."""
    return base + (w - base) * gamma


def add_noise_scaled(dst: Tensor, upd: Tensor, coef: float, sigma: float, seed: int,
                     noise: bool) -> None:
    """dst += coef*upd (+ N(0, sigma) per element if noise)  (K12, helper.py:240-257).
    ``upd`` may be fp64 (the FedAvg delta sum): the product is rounded to fp32 once."""
    u = (upd * coef).to(dst.dtype)
    if noise:
        ctr = torch.arange(u.numel(), dtype=torch.int64, device=u.device).reshape(u.shape)
        u = u + sigma * rng.normal(seed, ctr)
    dst += u


def delta_sum(rows: Tensor, base: Tensor) -> Tensor:
    """sum_r (rows[r] - base) in fp64 (FedAvg's per-rank Σ-delta, K12; helper.py:218-222).
    fp32 deltas summed in fp64 are exact, so a cross-rank all-reduce of the partial sums
    gives the same total as one rank summing all clients."""
    n = base.numel()
    if rows.shape[0] == 0:
        return torch.zeros(n, dtype=torch.float64, device=base.device)
    return (rows[:, :n].double() - base.double()[None]).sum(0)


def sq_dists(points: Tensor, m: Tensor) -> Tensor:
    """||points[i] - m||^2 for all i in one pass (K13)."""
    d = points.double() - m.double()[None]
    return (d * d).sum(1)


def weighted_sum(points: Tensor, wts: Tensor, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """sum_i wts[i] * points[i] (K14/K16); ``out_dtype`` fp64 keeps a partial sum unrounded."""
    return (wts.double()[:, None] * points.double()).sum(0).to(out_dtype or points.dtype)


def weighted_sum_fixed(points: Tensor, wts: Tensor, E: int) -> Tensor:
    """[2, L] int64 limb sums of sum_i wts[i] * points[i] on the fixed grid 2^-(E + 53): each
    product (exact in fp64) quantised on its own, hi = floor(q), lo = floor((q - hi) 2^53), q =
    w p 2^E, then summed exactly (order-free; flat.hip wsum_fixed_kernel is the GPU form)."""
    q = (wts.float().double()[:, None] * points.double()) * (2.0 ** E)
    hi = torch.floor(q)
    lo = torch.floor((q - hi) * 2.0 ** 53)
    return torch.stack([hi.to(torch.int64).sum(0), lo.to(torch.int64).sum(0)])


def delta_stats(rows: Tensor, base: Tensor) -> Tuple[Tensor, Tensor]:
    """(||rows_i - base||^2 in fp64 [n], max |rows_i - base| in fp32 [n]) of the client updates,
    without keeping the [n, L] deltas (clip.hip delta_stats_kernel is the GPU form).  The delta is
    the fp64 difference; the max is taken over its fp32 rounding, a NaN mapped to +inf (so no
    later max can swallow it); a NaN delta makes its client's squared norm NaN.  Each row is
    summed on its own, so a client's bits do not depend on which other rows share the call."""
    n = rows.shape[0]
    sq = torch.zeros(n, dtype=torch.float64, device=base.device)
    mx = torch.zeros(n, dtype=torch.float32, device=base.device)
    if base.numel() == 0:
        return sq, mx
    b = base.double()
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=base.device)
    for i in range(n):
        d = rows[i].double() - b
        sq[i] = (d * d).sum()
        a = d.float().abs()
        mx[i] = torch.where(a.isnan(), inf, a).max()
    return sq, mx


def clipped_delta_sum_fixed(rows: Tensor, base: Tensor, scale: Tensor, E: int) -> Tensor:
    """[2, L] int64 limb sums of sum_i scale[i] * (rows[i] - base) on the fixed grid 2^-(E + 53):
    q = scale * (rows - base) * 2^E evaluated in fp64 in exactly this order, hi = floor(q), lo =
    floor((q - hi) 2^53), each product quantised on its own, then summed exactly (order-free;
    clip.hip clipped_sum_kernel computes the same limbs bit for bit)."""
    L = base.numel()
    if rows.shape[0] == 0:
        return torch.zeros(2, L, dtype=torch.int64, device=base.device)
    d = rows.double() - base.double()[None]
    q = (scale.float().double()[:, None] * d) * (2.0 ** E)
    hi = torch.floor(q)
    lo = torch.floor((q - hi) * 2.0 ** 53)
    return torch.stack([hi.to(torch.int64).sum(0), lo.to(torch.int64).sum(0)])


def clipped_delta_sum(rows: Tensor, base: Tensor, scale: Tensor) -> Tensor:
    """fp64 [L] sum_i scale[i] * (rows[i] - base): the clipped sum off the fixed grid (a NaN / Inf
    delta is carried into it)."""
    L = base.numel()
    if rows.shape[0] == 0:
        return torch.zeros(L, dtype=torch.float64, device=base.device)
    return (scale.float().double()[:, None] * (rows.double() - base.double()[None])).sum(0)


PAIRWISE_CHUNK = 1 << 18


def _picked_rows(buf: Tensor, row_idx) -> Tuple[Optional[Tensor], int]:
    """(row numbers as an int64 tensor or None, n) of the ops over n rows of ``buf`` [R, L]: the rows
    ``row_idx`` (repeats allowed) or all R."""
    assert buf.dim() == 2
    if row_idx is None:
        return None, buf.shape[0]
    idx = torch.as_tensor(row_idx, dtype=torch.int64, device=buf.device).reshape(-1)
    return idx, idx.numel()


def pairwise_sq_dists(buf: Tensor, row_idx=None) -> Tensor:
    """fp64 [n, n] squared L2 distances between the rows of ``buf`` [R, L] fp32 (Multi-Krum;
    krum.hip pairwise_sqdist_kernel is the GPU form): rows ``row_idx`` (n row numbers, repeats
    allowed) or all of them.  The pair difference is taken in fp64 (exact for fp32 rows: the
    Gram formula g_ii + g_jj - 2 g_ij would cancel the digits that carry the distance between
    nearly equal client states).  Chunked over L, so no [n, n, L] temporary; each unordered pair
    is summed once and mirrored: symmetric, zero diagonal.  A NaN / Inf element makes its row's
    off-diagonal distances non-finite and leaves the others alone."""
    idx, n = _picked_rows(buf, row_idx)
    L = buf.shape[1]
    D = torch.zeros(n, n, dtype=torch.float64, device=buf.device)
    if n < 2:
        return D
    for c0 in range(0, L, PAIRWISE_CHUNK):
        x = buf[:, c0:c0 + PAIRWISE_CHUNK]
        x = (x if idx is None else x.index_select(0, idx)).double()
        for i in range(n - 1):
            d = x[i + 1:] - x[i][None]
            D[i, i + 1:] += (d * d).sum(1)
    return D + D.t()


def delta_gram(buf: Tensor, base: Tensor, row_idx=None) -> Tensor:
    """fp64 [n, n] Gram matrix of the client updates (FLAME's cosine stage; dgram.hip is the GPU
    form): ``G[i][j] = sum_k d_i[k] d_j[k]`` with ``d_i = (double)buf[row_i] - (double)base`` (exact
    for fp32 operands), rows ``row_idx`` (n row numbers, repeats allowed) or all of ``buf`` [R, L]
    fp32, ``base`` [L] fp32.  Pair by pair and chunked over L, so no [n, n, L] temporary; each
    unordered pair i <= j is summed once, the diagonal by the same expression, and mirrored:
    bitwise symmetric, and a pair's bits do not depend on the other rows of the call.  A NaN / Inf
    element makes its row's entries non-finite and leaves the others alone."""
    idx, n = _picked_rows(buf, row_idx)
    L = buf.shape[1]
    assert base.numel() == L, (tuple(buf.shape), base.numel())
    G = torch.zeros(n, n, dtype=torch.float64, device=buf.device)
    b = base.reshape(-1).double()
    for c0 in range(0, L, PAIRWISE_CHUNK):
        x = buf[:, c0:c0 + PAIRWISE_CHUNK]
        d = (x if idx is None else x.index_select(0, idx)).double() - b[None, c0:c0 + PAIRWISE_CHUNK]
        for i in range(n):
            for j in range(i, n):
                G[i, j] += (d[i] * d[j]).sum()
    return torch.triu(G) + torch.triu(G, 1).t()


TRIM_CHUNK = 1 << 18


def check_trim(n: int, k: int) -> int:
    """The trim count of n rows: an integer with 0 <= k and 2 k + 1 <= n (k = 0 when n = 0)."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 0 or (2 * k + 1 > n and not (n == 0 and k == 0)):
        raise ValueError(f"trimmed_delta_sum: k = {k!r} needs 0 <= k <= (n - 1) // 2 (n = {n})")
    return k


def trimmed_delta_sum(buf: Tensor, base: Tensor, k: int, row_idx=None) -> Tuple[Tensor, Tensor, Tensor]:
    """Coordinate-wise trimmed sum of the client deltas (trimmed mean / median, Yin et al., ICML
    2018; trim.hip is the GPU form): rows ``row_idx`` (n row numbers, repeats allowed) or all of
    ``buf`` [R, L] fp32, ``base`` [L] fp32, ``0 <= k <= (n - 1) // 2``.  Per coordinate the n values
    are sorted ascending (-inf first, +inf last among the numbers, every NaN after +inf, -0 == +0),
    ``d_r = (double)s_r - (double)base`` and ``total = ((d_k + d_{k+1}) + ...) + d_{n-1-k}``, one
    fp64 rounding per addition, in ascending rank.  With ``lo = s_k`` and ``hi = s_{n-1-k}``
    (comparisons in which NaN compares false) a client is low at a coordinate if ``v < lo``, high
    if ``v > hi`` or v is NaN and hi is not, kept otherwise; clients tied with a threshold are all
    kept.  Returns (total fp64 [L], kept int64 [n], high int64 [n]): the coordinates each client
    was kept / cut as high at (low is L - kept - high).  Chunked over L: no [n, L] fp64."""
    idx, n = _picked_rows(buf, row_idx)
    L = buf.shape[1]
    k = check_trim(n, k)
    total = torch.zeros(L, dtype=torch.float64, device=buf.device)
    kept = torch.zeros(n, dtype=torch.int64, device=buf.device)
    high = torch.zeros(n, dtype=torch.int64, device=buf.device)
    if n == 0:
        return total, kept, high
    b = base.double()
    for c0 in range(0, L, TRIM_CHUNK):
        x = buf[:, c0:c0 + TRIM_CHUNK]
        x = x if idx is None else x.index_select(0, idx)
        s = torch.sort(x, dim=0).values                       # (NaN last)
        bc = b[c0:c0 + TRIM_CHUNK]
        t = s[k].double() - bc
        for r in range(k + 1, n - k):
            t = t + (s[r].double() - bc)
        total[c0:c0 + TRIM_CHUNK] = t
        lo, hi = s[k][None], s[n - 1 - k][None]
        is_low = x < lo
        is_high = (x > hi) | (x.isnan() & ~hi.isnan())
        kept += (~is_low & ~is_high).sum(1)
        high += is_high.sum(1)
    return total, kept, high


def check_bulyan(t: int, f: int) -> int:
    """Bulyan's f for t selected rows: an integer with 0 <= f and 2 f + 1 <= t (f = 0 when t = 0)."""
    if isinstance(f, bool) or not isinstance(f, int) or f < 0 or (2 * f + 1 > t and not (t == 0 and f == 0)):
        raise ValueError(f"bulyan_delta_sum: f = {f!r} needs 0 <= f <= (t - 1) // 2 (t = {t})")
    return f


def bulyan_delta_sum(buf: Tensor, base: Tensor, f: int, row_idx=None) -> Tuple[Tensor, Tensor, Tensor]:
    """Bulyan's second stage (El Mhamdi, Guerraoui and Rouault, ICML 2018; bulyan.hip is the GPU
    form): the coordinate-wise median window over the rows ``row_idx`` (t row numbers, repeats
    allowed) or all of ``buf`` [R, L] fp32, ``base`` [L] fp32, ``0 <= f <= (t - 1) // 2``.  Per
    coordinate the t values are sorted ascending in :func:`trimmed_delta_sum`'s order (every NaN
    after +inf, -0 == +0): s_0 .. s_{t-1}.  With ``beta = t - 2 f``, ``m = (t - 1) // 2`` and ``med =
    (double)s_m`` (the lower median) the window is the ranks ``a .. a + beta - 1``, where ``a`` is
    the number of j in ``0 .. 2 f - 1`` with ``(double)s_{j+beta} - med < med - (double)s_j`` (fp64,
    false when a side is NaN): the beta values closest to the median, ties to the lower one.
    ``d_r = (double)s_r - (double)base`` and ``total = ((d_a + d_{a+1}) + ...) + d_{a+beta-1}``, one
    fp64 rounding per addition, in ascending rank.  With ``lo = s_a`` and ``hi = s_{a+beta-1}`` a row
    is low at a coordinate if ``v < lo``, high if ``v > hi`` or v is NaN and hi is not, kept
    otherwise (rows tied with a threshold are all kept).  Returns (total fp64 [L], kept int64
    [t], high int64 [t]).  Chunked over L: no [t, L] fp64."""
    idx, t = _picked_rows(buf, row_idx)
    L = buf.shape[1]
    f = check_bulyan(t, f)
    total = torch.zeros(L, dtype=torch.float64, device=buf.device)
    kept = torch.zeros(t, dtype=torch.int64, device=buf.device)
    high = torch.zeros(t, dtype=torch.int64, device=buf.device)
    if t == 0:
        return total, kept, high
    beta, m = t - 2 * f, (t - 1) // 2
    b = base.double()
    for c0 in range(0, L, TRIM_CHUNK):
        x = buf[:, c0:c0 + TRIM_CHUNK]
        x = x if idx is None else x.index_select(0, idx)
        s = torch.sort(x, dim=0).values                       # (NaN last)
        med = s[m].double()
        a = torch.zeros(s.shape[1], dtype=torch.int64, device=buf.device)
        for j in range(2 * f):
            a += (s[j + beta].double() - med) < (med - s[j].double())
        bc = b[c0:c0 + TRIM_CHUNK]
        lo = s.gather(0, a[None])
        tot = lo[0].double() - bc
        hi = lo
        for r in range(1, beta):
            hi = s.gather(0, (a + r)[None])
            tot = tot + (hi[0].double() - bc)
        total[c0:c0 + TRIM_CHUNK] = tot
        is_low = x < lo
        is_high = (x > hi) | (x.isnan() & ~hi.isnan())
        kept += (~is_low & ~is_high).sum(1)
        high += is_high.sum(1)
    return total, kept, high


RLR_CHUNK = 1 << 18


def _rlr_rows(rows: Tensor, base: Tensor) -> Tuple[int, int]:
    assert rows.dim() == 2 and rows.dtype == torch.float32 and base.dtype == torch.float32
    assert rows.shape[1] == base.numel(), (tuple(rows.shape), base.numel())
    return rows.shape[0], rows.shape[1]


def delta_sum_votes(rows: Tensor, base: Tensor) -> Tuple[Tensor, Tensor]:
    """(total fp64 [L], votes int32 [L]) of the robust learning rate's sign vote (rlr.hip is the GPU
    form): ``total = sum_i ((double)rows_i - (double)base)`` added in row order, one fp64 rounding
    per addition (the bits of :func:`delta_sum`), and ``votes = sum_i s_i`` with ``s_i`` = +1 where
    ``rows_i > base``, -1 where ``rows_i < base``, 0 otherwise: fp32 comparisons, so a NaN on either
    side and -0 against +0 vote 0 (a non-finite value still enters ``total``).  Chunked over L: no
    full [n, L] temporary."""
    n, L = _rlr_rows(rows, base)
    total = torch.zeros(L, dtype=torch.float64, device=base.device)
    votes = torch.zeros(L, dtype=torch.int32, device=base.device)
    for c0 in range(0, L if n else 0, RLR_CHUNK):
        b = base[c0:c0 + RLR_CHUNK]
        bd = b.double()
        t = total[c0:c0 + RLR_CHUNK]
        v = votes[c0:c0 + RLR_CHUNK]
        for i in range(n):
            x = rows[i, c0:c0 + RLR_CHUNK]
            t += x.double() - bd
            v += (x > b).to(torch.int32) - (x < b).to(torch.int32)
    return total, votes


def vote_agreement(rows: Tensor, base: Tensor, votes: Tensor, theta: int) -> Tensor:
    """int64 [n, 2] (agree, dissent) of each row against the reduced ``votes`` [L] at threshold
    ``theta``: over the kept coordinates (``|votes| >= theta``) only, with ``m = sign(votes)``, the
    coordinates at which the row's sign (as in :func:`delta_sum_votes`) is non-zero and equals m /
    equals -m.  Chunked over L."""
    n, L = _rlr_rows(rows, base)
    assert votes.numel() == L
    votes = votes.reshape(-1)
    counts = torch.zeros(n, 2, dtype=torch.int64, device=base.device)
    for c0 in range(0, L if n else 0, RLR_CHUNK):
        b = base[c0:c0 + RLR_CHUNK][None]
        x = rows[:, c0:c0 + RLR_CHUNK]
        V = votes[c0:c0 + RLR_CHUNK].to(torch.int64)
        s = (x > b).to(torch.int64) - (x < b).to(torch.int64)
        m = torch.sign(V)[None]
        live = ((V.abs() >= int(theta))[None]) & (s != 0)
        counts[:, 0] += (live & (s == m)).sum(1)
        counts[:, 1] += (live & (s == -m)).sum(1)
    return counts


def rlr_apply(dst: Tensor, total: Tensor, votes: Tensor, theta: int, coef: float, sigma: float, seed: int,
              noise: bool) -> Tensor:
    """The robust-learning-rate update, in place: ``dst += (float)(total * (double)(kept ? coef :
    -coef))`` (+ N(0, sigma) per element if ``noise``: the hash RNG and counters of
    :func:`add_noise_scaled`) with ``kept = |votes| >= theta``; a kept coordinate gets the bits of
    :func:`add_noise_scaled` with ``coef``, a flipped one those with ``-coef``.  ``total`` fp64 [L],
    ``votes`` int32 [L].  Returns the number of flipped coordinates (an int64 scalar tensor).
    Chunked over L."""
    L = dst.numel()
    assert dst.dim() == 1 and total.numel() == L and votes.numel() == L and total.dtype == torch.float64
    total, votes = total.reshape(-1), votes.reshape(-1)
    flipped = torch.zeros((), dtype=torch.int64, device=dst.device)
    cpos = torch.tensor(float(coef), dtype=torch.float64, device=dst.device)     # (as add_noise_scaled multiplies)
    for c0 in range(0, L, RLR_CHUNK):
        t = total[c0:c0 + RLR_CHUNK]
        kept = votes[c0:c0 + RLR_CHUNK].to(torch.int64).abs() >= int(theta)
        u = (t * torch.where(kept, cpos, -cpos)).to(dst.dtype)
        if noise:
            ctr = torch.arange(c0, c0 + u.numel(), dtype=torch.int64, device=u.device)
            u = u + sigma * rng.normal(seed, ctr)
        dst[c0:c0 + RLR_CHUNK] += u
        flipped += (~kept).sum()
    return flipped


TOPK_ABS_MASK = 0x7FFFFFFFFFFFFFFF


def topk_keys(resid: Tensor) -> Tensor:
    """The select keys of SparseFed: the bits of the fp64 ``resid`` with the sign bit cleared, as
    (non-negative) int64.  Integer order is magnitude order: -0 and +0 are 0, denormals order, inf
    ranks above every finite value and a NaN above inf, by payload."""
    return resid.view(torch.int64) & TOPK_ABS_MASK


def topk_check(resid: Tensor, total: Tensor, k) -> Tuple[int, int]:
    """(L, k) of :func:`topk_threshold`, checked the same way on every backend: fp64 vectors of one
    length, ``k`` an integer (a bool or a float is a ValueError) with 1 <= k <= L unless L = 0."""
    assert resid.dim() == 1 and resid.dtype == torch.float64 and total.dtype == torch.float64
    assert total.numel() == resid.numel(), (total.numel(), resid.numel())
    L = resid.numel()
    if isinstance(k, bool) or not isinstance(k, int):
        raise ValueError(f"topk: k {k!r}: expected an integer")
    if L and not 1 <= k <= L:
        raise ValueError(f"topk: k {k} needs 1 <= k <= L = {L}")
    return L, k


def topk_apply_check(dst: Tensor, resid: Tensor, sel: Tensor) -> int:
    assert dst.dim() == 1 and dst.dtype == torch.float32 and resid.dim() == 1 and resid.dtype == torch.float64
    assert resid.numel() == dst.numel(), (resid.numel(), dst.numel())
    assert sel.dtype == torch.int64 and sel.numel() == 2
    return dst.numel()


def topk_threshold(resid: Tensor, total: Tensor, k: int, ws: Optional[Tensor] = None) -> Tensor:
    """SparseFed's select (topk.hip is the GPU form): ``resid += total`` in place (fp64 [L]), then
    ``sel`` int64 [2] on the vectors' device = (T, m) with T the k-th largest of :func:`topk_keys`
    and m the number of keys >= T (m >= k, more only on ties at T; T = 0 and m = L when fewer than k
    keys are non-zero).  Both entries are filled here, without a host sync; :func:`topk_apply`
    rewrites ``sel[1]`` with the number of coordinates it applied, which is the same m.  1 <= k <=
    L or a ValueError; L = 0 gives (0, 0).  ``ws``: a workspace the GPU form can reuse (unused
    here)."""
    L, k = topk_check(resid, total, k)
    if L == 0:
        return torch.zeros(2, dtype=torch.int64, device=resid.device)
    resid += total.reshape(-1)
    keys = topk_keys(resid)
    T = torch.sort(keys).values[L - k]
    return torch.stack([T, (keys >= T).sum()])


def topk_apply(dst: Tensor, resid: Tensor, sel: Tensor, coef: float) -> None:
    """SparseFed's sparse update, in place: where ``topk_keys(resid) >= sel[0]``, ``dst +=
    (float)(resid * (double)(float)coef)`` (the update of :func:`add_noise_scaled` with noise off,
    at the fp32 coefficient the kernels take) and ``resid = +0.0``; elsewhere ``dst`` keeps its
    bits (a ``-0.0f`` stays ``-0.0f``) and ``resid`` its value.  ``sel[1]`` is rewritten with the
    number of coordinates applied."""
    if topk_apply_check(dst, resid, sel) == 0:
        return
    kept = topk_keys(resid) >= sel[0]
    c = torch.tensor(float(coef), dtype=torch.float32, device=dst.device).double()
    dst.copy_(torch.where(kept, dst + (resid * c).to(dst.dtype), dst))
    resid.masked_fill_(kept, 0.0)
    sel[1] = kept.sum()


def gram(feats: Tensor) -> Tensor:
    """F F^T in float64 (K15)."""
    f = feats.double()
    return f @ f.t()

"""Server-side aggregation over flat client buffers.

Each rule is ONE function, used by ``Server._aggregate`` and on a single rank alike.  Where the
round's n client rows live is an argument: the rules whose sums decompose over clients (FedAvg,
``clip_norm``, ``rlr_threshold``, distributed RFA) take this rank's rows ``finals [len(idx), S]`` and
a :class:`Shard` (the positions ``idx`` of those rows among the n, a sum and a max over the ranks;
default: every row here, identity reductions); the rules that read every row (``krum_f``,
``krum_bulyan``, ``trim_k``, ``clip_flame``) take the server's gathered snapshot bank and the clients' slots ``row_idx`` and read
the rows in place.  Every rank applies the identical update redundantly, so no broadcast is
needed and every rank ends the round with a bit-identical global model.  A rule returns what the
server records: the two ``weight_result.csv`` columns (and what its log line needs).

* :func:`fedavg` — reference ``helper.py:240-257``: ``w += (eta/no_models)
  * sum_i delta_i`` (+ N(0, sigma) per element with ``diff_privacy``); unweighted; applied to
  the BN running stats too (D2).  The delta sum is an fp64 HIP reduction, per rank then
  summed over the ranks.  The int64 ``num_batches_tracked`` counters are not part of the float
  bucket (D1: the reference's float→int64 add crashes on modern torch).
* :func:`fedavg_clipped` / :func:`clip_factors` — norm-clipped FedAvg (config ``clip_norm``, not in
  the reference): each client's update is scaled to an L2 norm of at most C (fixed, or the round's
  lower-median norm) before the average, which bounds what one model-replacement client can
  move and gives ``diff_privacy``'s noise a sensitivity bound.  Norms and the clipped sum are
  fused HIP passes over the strided client rows (``ops.delta_stats``,
  ``ops.clipped_delta_sum_fixed``); the products ``s_i delta_i`` are not exactly summable in
  fp64, so the sum goes through the same fixed-point limbs as RFA / FoolsGold.
* :func:`fedavg_flame` / :func:`flame_distances` / :func:`flame_admit` — FLAME (config ``clip_norm:
  median`` with ``clip_flame``; Nguyen et al., USENIX Security 2022; not in the reference): the
  clients are filtered by the direction of their updates, then clipped and noised.  The fp64 Gram
  matrix of the n updates comes from one fused HIP pass over the final states where they lie
  (``ops.delta_gram``: exact deltas, one fma per product, no atomics, a pair's bits independent of
  the other rows); the cosine distances and the clustering are host fp64 arithmetic (single
  linkage up to the first component of n // 2 + 1 clients: the closed form of HDBSCAN with the
  paper's parameters); the admitted updates are clipped to the lower-median norm S with
  :func:`clip_factors`, summed through :func:`clipped_part` and noised with sigma = lambda S.
  Like Krum it reads every row on every rank and reduces nothing.
* :func:`fedavg_krum` / :func:`krum_scores` / :func:`krum_select` — Multi-Krum (config ``krum_f``,
  ``krum_m``; Blanchard et al., NeurIPS 2017; not in the reference): the clients farthest from the
  crowd are dropped and the rest averaged.  The [n, n] squared distances between the final states
  come from one fused HIP pass (``ops.pairwise_sq_dists``: fp64 differences, no atomics, a pair's
  bits independent of the other rows); scores and selection are host fp64 arithmetic.
* :func:`fedavg_bulyan` / :func:`bulyan_select` — Bulyan (config ``krum_f`` with ``krum_bulyan``;
  El Mhamdi, Guerraoui and Rouault, ICML 2018; not in the reference): Krum iterated on the same
  distance matrix picks theta = n - 2 f clients one at a time (host fp64 arithmetic), then per
  coordinate the beta = theta - 2 f of their values closest to the coordinate's lower median are
  averaged.  The second stage is one fused HIP pass over the selected rows where they lie
  (``ops.bulyan_delta_sum``: the sort in registers, the window found without a dynamic index, its
  ranks added in ascending order in fp64), which also counts, per selected client, the
  coordinates at which it was kept.
* :func:`fedavg_trimmed` / :func:`trim_count` — coordinate-wise trimmed mean / median (config
  ``trim_k``; Yin et al., ICML 2018; not in the reference): per coordinate the k smallest and k
  largest client values are dropped and the rest averaged; no per-client decision.  One fused HIP
  pass over the strided final states (``ops.trimmed_delta_sum``: each coordinate sorted in
  registers, the kept ranks added in ascending order in fp64, so every bit is fixed by IEEE
  arithmetic) also counts, per client, the coordinates at which it was kept or cut.
* :func:`fedavg_rlr` / :func:`rlr_theta` — robust learning rate (config
  ``rlr_threshold``; Ozdayi, Kantarcioglu and Gel, AAAI 2021; not in the reference): per coordinate
  the signs of the clients' updates are summed and the averaged update is applied with a negative
  rate wherever the vote's |sum| is below theta; magnitudes play no part.  The fp64 delta sum and the
  int32 votes come from one fused HIP pass over the strided final states (``ops.delta_sum_votes``),
  the per-client agreement counts from a second (``ops.vote_agreement``) and the signed update from
  ``ops.rlr_apply`` (``add_noise_scaled``'s bits with ``+coef`` / ``-coef``).  Sums over clients
  decompose, so the clients stay on their owner ranks and every quantity is an integer or an fp64
  sum in client order.
* :func:`fedavg_sparse` / :func:`sparse_count` — SparseFed (config ``sparse_topk``,
  ``sparse_clip``; Panda et al., AISTATS 2022; not in the reference): the (optionally clipped)
  total is added into a server-side fp64 error-feedback residual and only the k largest-magnitude
  coordinates of the residual are applied and cleared; the rest wait in the residual.  The k-th
  largest magnitude is an exact radix select on the device (``ops.topk_threshold``: integer
  histograms, no host read inside) and the sparse update one pass (``ops.topk_apply``:
  ``add_noise_scaled``'s bits at the kept coordinates, nothing written elsewhere).  The residual is
  the one piece of server state besides FoolsGold's: every rank holds it, checkpoints carry it.
* :func:`geometric_median` — RFA / Weiszfeld, ``helper.py:295-373`` (on the gathered rows, or
  with the points resident on their owner ranks): one batched distance kernel (all n clients in
  one pass) and one weighted-sum kernel per iteration; weights and the stopping test stay on the device (one host read per aggregation).  Quirk D5 (``wv`` undefined if
  converged at iteration 0) resolves to the current weights.
* The weighted sums of RFA and FoolsGold are REPRODUCIBLE: every product is quantised on its own
  onto a fixed two-limb int64 grid (:func:`fixed_exponent`, ``ops.weighted_sum_fixed``) and the
  limbs are summed exactly — over a rank's clients, then over ranks by an int64 all-reduce — so
  the global model's bits do not depend on the world size or on which rank holds which client.
* :class:`FoolsGold` — ``helper.py:527-607``: cosine similarity of the clients' final-FC
  gradient features (history-summed with ``fg_use_memory``), pardoning, logit weights,
  weighted gradient sum, then one fresh-SGD server step (BN buffers untouched).
"""
from __future__ import annotations

import dataclasses
import logging
import math
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import config as C
from .. import ops

log = logging.getLogger("logger")


@dataclasses.dataclass
class Shard:
    """Where a round's ``n`` client rows live: this rank holds the rows of the clients at positions
    ``idx`` (in that order); ``reduce(t)`` sums a tensor over the ranks and ``reduce_max(v)`` takes
    the max of a host float over them.  The default is the single-rank case: every row here,
    identity reductions.  ``Server`` passes its own ``_reduce`` / ``_reduce_max``."""
    n: int
    idx: Optional[Sequence[int]] = None
    reduce: Callable[[torch.Tensor], torch.Tensor] = lambda t: t
    reduce_max: Callable[[float], float] = lambda v: v

    def __post_init__(self) -> None:
        self.idx = list(range(self.n) if self.idx is None else self.idx)
        self._idx_t: Optional[torch.Tensor] = None

    def index(self, device) -> torch.Tensor:
        """``idx`` as an int64 tensor on ``device``."""
        if self._idx_t is None or self._idx_t.device != torch.device(device):
            self._idx_t = torch.tensor(self.idx, dtype=torch.int64, device=device)
        return self._idx_t

    def sum_rows(self, vals: Optional[torch.Tensor], tail: Tuple[int, ...], dtype, device) -> torch.Tensor:
        """The [n, *tail] tensor of a per-client quantity from this rank's rows' ``vals``
        [len(idx), *tail] (None on a rank without clients): zeros at the other ranks' clients,
        summed over the ranks (each row owned by one rank, zero elsewhere: exact)."""
        full = torch.zeros((self.n,) + tuple(tail), dtype=dtype, device=device)
        if self.idx:
            full[self.index(device)] = vals
        return self.reduce(full)


def fedavg(global_state: torch.Tensor, finals: torch.Tensor, eta: float, no_models: int,
           dp: bool, sigma: float, seed: int, n_update: int, where: Optional[Shard] = None) -> None:
    """In-place FedAvg of this rank's ``finals`` [len(idx), S]: ``w += (eta / no_models) * sum_i
    delta_i (+ noise)``; ``n_update`` = leading entries aggregated (S or P).  Each rank sums its
    own clients' deltas in fp64 (``ops.delta_sum``: fused HIP kernel on GPU), one reduction of
    ``n_update`` values."""
    where = where or Shard(finals.shape[0])
    total = delta_total(finals[:, :n_update], global_state[:n_update], where)
    ops.add_noise_scaled(global_state[:n_update], total, eta / no_models, sigma, seed, dp)


def delta_total(rows: torch.Tensor, base: torch.Tensor, where: Shard) -> torch.Tensor:
    """Plain FedAvg's fp64 total sum_i (rows_i - base) over every rank's clients: this rank's
    ``ops.delta_sum`` (zeros without clients), ONE reduction."""
    return where.reduce(ops.delta_sum(rows, base))


FIXED_MAX_TERMS = 512


def fixed_exponent(maxabs: float, n: int) -> Optional[int]:
    """E of the fixed-point weighted sums: with weights <= 1 and |points| <= ``maxabs`` (the max
    over ALL clients, every rank the same), each scaled product |w p 2^E| < 2^52 / n, so neither
    limb sum of n <= 512 products overflows int64.  The grid step is 2^-(E + 53): ~105 bits below
    the largest product.  None when the grid cannot hold the sum — a non-finite ``maxabs`` (a NaN /
    Inf client update: the fp64 sum carries it into the global model, as the reference's torch
    aggregation does, instead of quantising it into finite garbage) or more than 512 terms; the
    callers then take the plain fp64 weighted sum (:func:`wsum_part`)."""
    if n > FIXED_MAX_TERMS or not math.isfinite(maxabs):
        return None
    if not maxabs > 0.0:
        return 0
    n2 = max(0, math.ceil(math.log2(max(1, n))))
    _, ex = math.frexp(maxabs)          # maxabs < 2**ex
    return max(-1000, min(1000, 52 - n2 - ex))


def max_abs(t: Optional[torch.Tensor]) -> float:
    """Host max |t| for :func:`fixed_exponent`, NaN mapped to +inf (so a max-all-reduce over ranks
    sees it whatever the backend does with NaN)."""
    if t is None or t.numel() == 0:
        return 0.0
    v = float(t.abs().max().item())
    return math.inf if math.isnan(v) else v


def wsum_part(points: torch.Tensor, w: torch.Tensor, E: Optional[int]) -> torch.Tensor:
    """A rank's partial of sum_i w_i points_i: [2, L] int64 fixed-point limbs on the 2^E grid
    (exact, order-free), or an fp64 [L] vector when ``E`` is None."""
    if E is None:
        return ops.weighted_sum(points, w.float(), torch.float64)
    return ops.weighted_sum_fixed(points, w.float(), E)


def wsum_zero(L: int, E: Optional[int], device) -> torch.Tensor:
    """The partial of a rank without clients (same shape / dtype as :func:`wsum_part`)."""
    if E is None:
        return torch.zeros(L, dtype=torch.float64, device=device)
    return torch.zeros(2, L, dtype=torch.int64, device=device)


def wsum_decode(part: torch.Tensor, E: Optional[int]) -> torch.Tensor:
    """fp32 value of a (reduced) :func:`wsum_part`."""
    return (part if E is None else fixed_decode(part, E)).float()


def fixed_decode(limbs: torch.Tensor, E: int) -> torch.Tensor:
    """fp64 value of [2, L] int64 limb sums on the 2^-(E + 53) grid (elementwise, exact up to the
    final rounding: the same bits for the same limbs)."""
    return limbs[0].double() * (2.0 ** -E) + limbs[1].double() * (2.0 ** -(E + 53))


def clip_factors(sqnorms: torch.Tensor, clip) -> Tuple[torch.Tensor, float]:
    """Per-client clip factors of norm-clipped FedAvg from the squared update norms (fp64 [n]):
    ``s_i = 1`` if ``norm_i <= C`` else ``C / norm_i`` (a zero-norm client gets 1).  ``clip`` is
    the bound C, or ``"median"``: the lower median of this round's norms (the sorted fp64 norms
    at index (n - 1) // 2).  Host fp64 arithmetic on the all-reduced norms, so every rank computes
    the same factors; the kernels take ``factors.float()``.  Returns (factors fp64 [n] on the
    host, C).  A NaN norm (a NaN client update) gives a NaN factor, which carries the NaN into the
    aggregate."""
    norms = sqnorms.detach().double().cpu().sqrt()
    bound = clip_bound(norms, clip)
    factors = torch.where(norms <= bound, torch.ones_like(norms), bound / norms)
    return factors, bound


def clip_bound(norms: Sequence[float], clip) -> float:
    """The bound C of a round with the update ``norms`` (fp64, on the host): ``clip`` itself, or
    their lower median for ``"median"``."""
    if not isinstance(clip, str):
        return float(clip)
    if clip != "median":
        raise ValueError(f"clip {clip!r}: expected a bound or 'median'")
    norms = torch.as_tensor(norms, dtype=torch.float64)
    n = norms.numel()
    return float(torch.sort(norms).values[(n - 1) // 2]) if n else 0.0


def clipped_part(rows: torch.Tensor, base: torch.Tensor, scale: torch.Tensor, E: Optional[int]) -> torch.Tensor:
    """A rank's partial of sum_i scale_i (rows_i - base), fused over the strided rows: [2, L] int64
    limbs on the 2^E grid, or an fp64 [L] vector when ``E`` is None (shapes of :func:`wsum_part`)."""
    if E is None:
        return ops.clipped_delta_sum(rows, base, scale.float())
    return ops.clipped_delta_sum_fixed(rows, base, scale.float(), E)


def fedavg_clipped(global_state: torch.Tensor, finals: torch.Tensor, clip, eta: float, no_models: int,
                   dp: bool, sigma: float, seed: int, n_update: int, where: Optional[Shard] = None
                   ) -> Tuple[List[float], List[float]]:
    """In-place norm-clipped FedAvg of this rank's ``finals`` [len(idx), S]: ``w += (eta /
    no_models) * sum_i s_i delta_i (+ noise)`` with the factors of :func:`clip_factors`.  The norm
    is taken over the ``n_update`` leading entries, exactly the entries aggregated.  Every rank
    takes the norms and max |delta| of its own clients in one fused pass; ONE reduction of the [n]
    fp64 squared norms and ONE max of a host float; every rank then computes the same factors and
    forms its partial clipped sum as fixed-point limbs; ONE reduction of the [2, n_update] int64
    limbs (exact, so the global model's bits do not depend on the world size or on which rank
    holds which client; fp64 partials if an update is not finite: the NaN reaches the model).
    Returns (factors [n], norms [n])."""
    where = where or Shard(finals.shape[0])
    rows, base = finals[:, :n_update], global_state[:n_update]
    sq, mx_l = delta_norms(rows, base, where)
    factors, _ = clip_factors(sq, clip)
    total = clipped_total(rows, base, factors, mx_l, where)
    ops.add_noise_scaled(base, total, eta / no_models, sigma, seed, dp)
    return [float(x) for x in factors], [float(x) for x in sq.double().cpu().sqrt()]


def delta_norms(rows: torch.Tensor, base: torch.Tensor, where: Shard) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(squared update norms of all n clients, fp64 [n]; max |delta| of this rank's clients, None
    without any): one fused pass over this rank's rows (``ops.delta_stats``), ONE reduction."""
    sq_l, mx_l = ops.delta_stats(rows, base) if where.idx else (None, None)
    return where.sum_rows(sq_l, (), torch.float64, base.device), mx_l


def clipped_total(rows: torch.Tensor, base: torch.Tensor, factors: torch.Tensor, mx_l: Optional[torch.Tensor],
                  where: Shard) -> torch.Tensor:
    """The fp64 total sum_i factors_i (rows_i - base) over every rank's clients, through the
    fixed-point limbs (ONE max of a host float for the grid, ONE reduction of the [2, L] int64
    limbs, decoded; fp64 partials if an update is not finite).  ``factors``: fp64 [n] on the host;
    ``mx_l``: :func:`delta_norms`'s."""
    dev, idx, L = base.device, where.idx, base.numel()
    E = fixed_exponent(where.reduce_max(max_abs(mx_l)), where.n)
    part = clipped_part(rows, base, factors[idx].to(dev), E) if idx else wsum_zero(L, E, dev)
    total = where.reduce(part)
    return total if E is None else fixed_decode(total, E)


def flame_distances(G: torch.Tensor) -> torch.Tensor:
    """FLAME's cosine distances (fp64 [n, n], on the host) from the Gram matrix of the clients'
    updates: ``c = G[i][j] / sqrt(G[i][i] * G[j][j])`` clamped to [-1, 1], ``D[i][j] = 1 - c``,
    ``D[i][i] = 0``.  A client with ``G[i][i] == 0`` (it returned the global model) is at distance 1
    from every other client (FoolsGold's zero-row convention).  A client whose ``G[i][i]`` is not
    finite is unusable: its row and column, the diagonal included, are NaN, which is how
    :func:`flame_admit` knows it.  A cosine between two usable clients that is not finite (the
    product of two finite squared norms overflowed) says nothing about the angle and reads as
    distance 1.  Host fp64 arithmetic in this order on a matrix every rank holds with the same
    bits: every rank computes the same distances."""
    g = G.detach().double().cpu().tolist()
    n = len(g)
    D = [[0.0] * n for _ in range(n)]
    usable = [math.isfinite(g[i][i]) for i in range(n)]
    for i in range(n):
        for j in range(i, n):
            if not (usable[i] and usable[j]):
                d = math.nan
            elif i == j:
                d = 0.0
            elif g[i][i] == 0.0 or g[j][j] == 0.0:
                d = 1.0
            else:
                den = math.sqrt(g[i][i] * g[j][j])
                c = g[i][j] / den if den > 0.0 else math.nan
                d = 1.0 - min(1.0, max(-1.0, c)) if math.isfinite(c) else 1.0
            D[i][j] = D[j][i] = d
    return torch.tensor(D, dtype=torch.float64).reshape(n, n)


def flame_admit(D: torch.Tensor) -> List[int]:
    """FLAME's admitted clients (sorted) from the [n, n] cosine distances of
    :func:`flame_distances`: with m = n // 2 + 1, the unordered pairs of usable clients (finite
    ``D[i][i]``) are sorted by ``(D[i][j], i, j)`` and merged in that order (single linkage,
    Kruskal); the first component to reach m members is admitted, whole (so at least m clients).
    This is what HDBSCAN returns with the paper's ``min_cluster_size = n // 2 + 1``,
    ``min_samples = 1``, ``allow_single_cluster = True``: no split of the hierarchy can leave two
    clusters of more than half the clients, and mutual reachability with one sample is the plain
    distance.  Fewer than m usable clients is an error.  Host arithmetic on a matrix every rank
    holds with the same bits."""
    d = D.detach().double().cpu().tolist()
    n = len(d)
    m = n // 2 + 1
    usable = [i for i in range(n) if math.isfinite(d[i][i])]
    if len(usable) < m:
        raise RuntimeError(f"flame: only {len(usable)} of {n} clients have a finite update, fewer than the majority "
                           f"m = n // 2 + 1 = {m}")
    if m <= 1:
        return usable[:1]
    parent = list(range(n))
    size = [1] * n

    def find(i: int) -> int:
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    pairs = sorted((d[i][j], i, j) for a, i in enumerate(usable) for j in usable[a + 1:])
    for _, i, j in pairs:
        ri, rj = find(i), find(j)
        if ri == rj:
            continue
        parent[rj] = ri
        size[ri] += size[rj]
        if size[ri] >= m:
            return [k for k in usable if find(k) == ri]
    raise RuntimeError(f"flame: no component of {m} clients among {len(usable)} usable ones (a distance is not "
                       "comparable)")


def fedavg_flame(global_state: torch.Tensor, finals: torch.Tensor, lam: float, eta: float, seed: int,
                 n_update: int, row_idx: Optional[Sequence[int]] = None
                 ) -> Tuple[List[float], List[float], List[int]]:
    """In-place FLAME of the n clients' final states: the rows ``row_idx`` of ``finals`` (the
    server's gathered snapshot bank, read in place) or all of ``finals`` [n, S]; n >= 3.  The Gram
    matrix of the updates over the ``n_update`` leading entries (exactly the entries aggregated;
    ``ops.delta_gram``: one fused HIP pass), :func:`flame_distances`, :func:`flame_admit` (the
    admitted set A, L = |A|); S = the lower median of all n update norms sqrt(G[i][i]) (a
    non-finite norm ranks as +inf) and the factors of :func:`clip_factors` against it; then ``w +=
    (eta / L) * sum_{i in A} gamma_i delta_i`` over the admitted rows (the only ones gathered) in
    client order, through the fixed-point limbs of :func:`clipped_part` (their grid from the
    largest admitted norm, which bounds every |delta|), and N(0, (lam S)^2) noise per entry
    (``lam`` = 0: none).  Every rank holds every row and computes the same bits redundantly: no
    reduction.  Returns (factor applied [n]: gamma_i, 0.0 for a client not admitted; update norms
    [n]; the admitted clients, sorted)."""
    n = finals.shape[0] if row_idx is None else len(row_idx)
    C.check_flame_sizes(n, "the round's clients")
    base = global_state[:n_update]
    G = ops.delta_gram(finals[:, :n_update], base, row_idx)
    admitted = flame_admit(flame_distances(G))
    sq = torch.diagonal(G).detach().double().cpu()
    sq = torch.where(torch.isfinite(sq), sq, torch.full_like(sq, math.inf))
    gamma, S = clip_factors(sq, C.CLIP_MEDIAN)
    norms = sq.sqrt()
    rows = finals[admitted if row_idx is None else [row_idx[i] for i in admitted]][:, :n_update]
    E = fixed_exponent(float(norms[admitted].max()), len(admitted))
    part = clipped_part(rows, base, gamma[admitted].to(base.device), E)
    total = part if E is None else fixed_decode(part, E)
    sigma = float(lam) * S
    ops.add_noise_scaled(base, total, eta / len(admitted), sigma, seed, sigma > 0.0)
    factors = [0.0] * n
    for i in admitted:
        factors[i] = float(gamma[i])
    return factors, [float(x) for x in norms], admitted


def krum_scores(D: torch.Tensor, f: int) -> torch.Tensor:
    """Krum scores (fp64 [n], on the host) from the [n, n] squared-distance matrix: score_i is
    the sum, in ascending order, of the n - f - 2 smallest D[i][j], j != i.  Non-finite entries
    of D (a NaN / Inf client state) count as +inf, so such a client scores +inf and pushes nobody
    else's score up unless fewer than n - f - 2 finite neighbours remain.  Host fp64 arithmetic on
    a matrix every rank holds with the same bits: every rank computes the same scores."""
    D = D.detach().double().cpu()
    n = D.shape[0]
    k = n - f - 2
    if k < 1:
        raise ValueError(f"krum: n = {n} clients need n >= f + 3 (f = {f}) to score")
    inf = torch.full_like(D, math.inf)
    D = torch.where(torch.isfinite(D), D, inf)
    scores = torch.empty(n, dtype=torch.float64)
    for i in range(n):
        row = torch.sort(torch.cat([D[i, :i], D[i, i + 1:]])).values[:k]
        s = 0.0
        for v in row.tolist():
            s += v
        scores[i] = s
    return scores


def krum_select(scores: torch.Tensor, m: int) -> List[int]:
    """The (sorted) indices of the ``m`` smallest scores, ties to the lower index; a client with
    an infinite score is never selected, so fewer than ``m`` come back when fewer are finite, and
    none finite is an error."""
    s = scores.detach().double().cpu()
    order = torch.sort(s, stable=True).indices.tolist()
    sel = [i for i in order if math.isfinite(float(s[i]))][:m]
    if not sel:
        raise RuntimeError("krum: no client has a finite score (every client state is non-finite)")
    return sorted(sel)


def fedavg_krum(global_state: torch.Tensor, finals: torch.Tensor, f: int, m: Optional[int], eta: float,
                dp: bool, sigma: float, seed: int, n_update: int, row_idx: Optional[Sequence[int]] = None
                ) -> Tuple[List[float], List[float]]:
    """In-place Multi-Krum of the n clients' final states: the rows ``row_idx`` of ``finals`` (the
    server's gathered snapshot bank, read in place) or all of ``finals`` [n, S].  The squared
    distances between the states over the ``n_update`` leading entries (exactly the entries
    aggregated; ``ops.pairwise_sq_dists``: one fused HIP pass), the scores, the ``m`` (default n -
    f) best, then ``w += (eta / m_sel) * sum_{i selected} (finals_i - w) (+ noise)`` with the plain
    FedAvg delta sum over the selected rows (the only ones gathered) in client order.  Every rank
    holds every row and computes the same bits redundantly: no reduction.  Returns (selected mask
    [n], scores [n])."""
    n = finals.shape[0] if row_idx is None else len(row_idx)
    D = ops.pairwise_sq_dists(finals[:, :n_update], row_idx)
    scores = krum_scores(D, f)
    sel = krum_select(scores, n - f if m is None else m)
    selected = finals[sel if row_idx is None else [row_idx[i] for i in sel]]
    total = ops.delta_sum(selected[:, :n_update], global_state[:n_update])
    ops.add_noise_scaled(global_state[:n_update], total, eta / len(sel), sigma, seed, dp)
    return [1.0 if i in sel else 0.0 for i in range(n)], [float(x) for x in scores]


def bulyan_select(D: torch.Tensor, f: int) -> Tuple[List[int], List[float]]:
    """Bulyan's first stage, iterated Krum on the [n, n] squared-distance matrix: (the selected
    clients in selection order, scores [n]).  Non-finite entries of D count as +inf, as in
    :func:`krum_scores`.  With the remaining set R = all n clients, until theta = n - 2 f are
    selected: r = |R|, k = max(1, r - f - 2) (the clamp serves the last iterations, where r - f - 2 <
    1; a lone last client has no neighbour and scores 0); score_i, i in R, is the sum in ascending
    order of the k smallest D[i][j], j in R, j != i; the smallest score wins, ties to the lower
    index; a winner whose score is not finite stops the selection; otherwise it leaves R, joins
    the selection and keeps its score of that moment.  A client never selected reports its score
    from the last iteration that ran.  Fewer than 2 f + 1 selected (the second stage's minimum) is
    an error.  Host fp64 arithmetic on a matrix every rank holds with the same bits."""
    D = D.detach().double().cpu()
    n = D.shape[0]
    if isinstance(f, bool) or not isinstance(f, int) or f < 0:
        raise ValueError(f"bulyan: f = {f!r} is not an integer >= 0")
    theta = n - 2 * f
    if theta < 2 * f + 1:
        raise ValueError(f"bulyan: n = {n} clients need n >= 4 f + 1 (f = {f}) to select 2 f + 1")
    rows = torch.where(torch.isfinite(D), D, torch.full_like(D, math.inf)).tolist()
    remaining = list(range(n))
    scores = [math.inf] * n
    selected: List[int] = []
    while len(selected) < theta:
        k = max(1, len(remaining) - f - 2)
        for i in remaining:
            s = 0.0
            for v in sorted(rows[i][j] for j in remaining if j != i)[:k]:
                s += v
            scores[i] = s
        win = min(remaining, key=lambda i: (scores[i], i))
        if not math.isfinite(scores[win]):
            break
        remaining.remove(win)
        selected.append(win)
    if len(selected) < 2 * f + 1:
        raise RuntimeError(f"bulyan: only {len(selected)} of {n} clients have a finite score, fewer than "
                           f"2 f + 1 = {2 * f + 1} (the other client states are non-finite)")
    return selected, scores


def fedavg_bulyan(global_state: torch.Tensor, finals: torch.Tensor, f: int, eta: float, dp: bool, sigma: float,
                  seed: int, n_update: int, row_idx: Optional[Sequence[int]] = None
                  ) -> Tuple[List[float], List[float], List[int]]:
    """In-place Bulyan of the n clients' final states: the rows ``row_idx`` of ``finals`` (the
    server's gathered snapshot bank, read in place) or all of ``finals`` [n, S]; n >= 4 f + 3.  The
    squared distances between the states over the ``n_update`` leading entries
    (``ops.pairwise_sq_dists``), :func:`bulyan_select` (t clients, normally n - 2 f), then over the
    selected rows in client order, per coordinate, the beta = t - 2 f values closest to the lower
    median (``ops.bulyan_delta_sum``: one fused HIP pass) and ``w += (eta / beta) * total (+
    noise)``.  Every rank holds every row and computes the same bits redundantly: no reduction.
    Returns (kept share [n], scores [n], the selected clients in selection order): the fraction of
    the aggregated coordinates at which each client's value was inside the window, 0.0 for a
    client the first stage dropped."""
    n = finals.shape[0] if row_idx is None else len(row_idx)
    C.check_bulyan_sizes(n, f, "the round's clients")
    D = ops.pairwise_sq_dists(finals[:, :n_update], row_idx)
    order, scores = bulyan_select(D, f)
    sel = sorted(order)
    total, kept, _ = ops.bulyan_delta_sum(finals[:, :n_update], global_state[:n_update], f,
                                          sel if row_idx is None else [row_idx[i] for i in sel])
    ops.add_noise_scaled(global_state[:n_update], total, eta / (len(sel) - 2 * f), sigma, seed, dp)
    den = float(max(1, n_update))
    share = [0.0] * n
    for i, v in zip(sel, kept.tolist()):
        share[i] = float(v) / den
    return share, [float(x) for x in scores], order


def trim_count(n: int, trim_k) -> int:
    """The trim count k of a round of n clients: ``trim_k`` itself, or (n - 1) // 2 for
    ``"median"`` (the coordinate-wise median: the middle value for odd n, the mean of the two
    middle values for even n); n >= 2 k + 1 or a ValueError."""
    t = C.check_trim_k(trim_k)
    if t is None:
        raise ValueError("trim_count: trim_k is not set")
    return C.check_trim_sizes(n, t, "the round's clients")


def fedavg_trimmed(global_state: torch.Tensor, finals: torch.Tensor, k_or_median, eta: float, dp: bool,
                   sigma: float, seed: int, n_update: int, row_idx: Optional[Sequence[int]] = None
                   ) -> Tuple[List[float], List[float]]:
    """In-place coordinate-wise trimmed mean of the n clients' final states: the rows ``row_idx``
    of ``finals`` (the server's gathered snapshot bank, read in place) or all of ``finals`` [n, S].
    Per coordinate of the ``n_update`` leading entries the k smallest and k largest client values
    are dropped (``ops.trimmed_delta_sum``: one fused HIP pass, the sort in registers) and ``w +=
    (eta / (n - 2 k)) * total (+ noise)``.  Every rank holds every row and computes the same bits
    redundantly: no reduction.  (Sharding the coordinates over the ranks and all-gathering the
    totals would move fewer bytes.)  Returns (kept share [n], high share [n]): the fraction of the
    aggregated coordinates at which each client's value was kept / cut as too high."""
    n = finals.shape[0] if row_idx is None else len(row_idx)
    k = trim_count(n, k_or_median)
    total, kept, high = ops.trimmed_delta_sum(finals[:, :n_update], global_state[:n_update], k, row_idx)
    ops.add_noise_scaled(global_state[:n_update], total, eta / (n - 2 * k), sigma, seed, dp)
    den = float(max(1, n_update))
    return [float(v) / den for v in kept.tolist()], [float(v) / den for v in high.tolist()]


def rlr_theta(n: int, theta) -> int:
    """The vote threshold of a round of n clients: ``rlr_threshold`` itself, checked again against
    the round's actual client count (1 <= theta <= n) or a ValueError."""
    t = C.check_rlr_threshold(theta)
    if t is None:
        raise ValueError("rlr_theta: rlr_threshold is not set")
    return C.check_rlr_sizes(n, t, "the round's clients")


def fedavg_rlr(global_state: torch.Tensor, finals: torch.Tensor, theta: int, eta: float, no_models: int,
               dp: bool, sigma: float, seed: int, n_update: int, where: Optional[Shard] = None
               ) -> Tuple[List[float], List[float], int]:
    """In-place robust-learning-rate FedAvg of this rank's ``finals`` [len(idx), S]: per coordinate
    of the ``n_update`` leading entries the clients' signs are summed (``ops.delta_sum_votes``: one
    fused HIP pass that also gives plain FedAvg's fp64 delta sum) and ``w += (eta / no_models) *
    total (+ noise)`` where ``|V| >= theta``, ``w -= ...`` where it is not (``ops.rlr_apply``).  Sign
    sums and delta sums decompose over clients: every rank takes those of its own clients (zeros on
    a rank without clients); ONE reduction of the fp64 total (the one plain FedAvg does) and ONE of
    the int32 votes (integer addition: exact); every rank then counts its own clients' agreement
    with the reduced votes, against the old ``w`` (``ops.vote_agreement``); ONE reduction of the
    [n, 2] int64 counts; every rank applies the signed update redundantly.  Returns (agree share
    [n], dissent share [n], flipped): the fraction of the aggregated coordinates that were kept
    and at which each client's non-zero sign agreed with / opposed the vote, and the number of
    flipped coordinates."""
    where = where or Shard(finals.shape[0])
    theta = rlr_theta(where.n, theta)
    rows, base = finals[:, :n_update], global_state[:n_update]
    dev = base.device
    if where.idx:
        total, votes = ops.delta_sum_votes(rows, base)
    else:
        total = torch.zeros(n_update, dtype=torch.float64, device=dev)
        votes = torch.zeros(n_update, dtype=torch.int32, device=dev)
    total = where.reduce(total)
    votes = where.reduce(votes)
    agreement = ops.vote_agreement(rows, base, votes, theta) if where.idx else None
    counts = where.sum_rows(agreement, (2,), torch.int64, dev)
    flipped = ops.rlr_apply(base, total, votes, theta, eta / no_models, sigma, seed, dp)
    den = float(max(1, n_update))
    c = counts.cpu().tolist()
    return [float(a) / den for a, _ in c], [float(d) / den for _, d in c], int(flipped)


def sparse_count(n_update: int, frac) -> int:
    """The number k of coordinates a SparseFed round keeps: ``max(1, floor(sparse_topk *
    n_update))`` (never more than ``n_update``), on the host, the same on every rank."""
    f = C.check_sparse_topk(frac)
    if f is None:
        raise ValueError("sparse_count: sparse_topk is not set")
    return min(int(n_update), max(1, int(math.floor(f * n_update))))


def key_value(T: int) -> float:
    """The magnitude whose select key (``ops.topk_threshold``) is ``T``."""
    return float(torch.tensor(int(T), dtype=torch.int64).view(torch.float64))


def fedavg_sparse(global_state: torch.Tensor, finals: torch.Tensor, k: int, clip, resid: torch.Tensor, eta: float,
                  no_models: int, n_update: int, where: Optional[Shard] = None
                  ) -> Tuple[List[float], List[float], int, float]:
    """In-place SparseFed round over this rank's ``finals`` [len(idx), S]: the fp64 total of the
    clients' updates (``clip`` None: plain FedAvg's, :func:`delta_total`; else each update clipped
    as in :func:`fedavg_clipped`, :func:`clipped_total`) is added into the error-feedback residual
    ``resid`` (fp64 [n_update], in place); the ``k`` largest-magnitude coordinates of the residual
    (and every tie at the k-th) are applied, ``w += (eta / no_models) * resid``, and zeroed there;
    every other coordinate of ``w`` is left untouched and stays in ``resid`` (``ops.topk_threshold``,
    ``ops.topk_apply``).  The per-client norms always come from ``ops.delta_stats`` (ONE reduction
    of [n] fp64); the total costs what the rule it borrows costs.  Every rank holds ``resid``
    redundantly and selects and applies redundantly on the reduced total: no further collective,
    the same bits at any world size.  ONE host read, after the apply is enqueued.  Returns (factors
    [n], norms [n], kept m, the threshold magnitude)."""
    where = where or Shard(finals.shape[0])
    rows, base = finals[:, :n_update], global_state[:n_update]
    sq, mx_l = delta_norms(rows, base, where)
    if clip is None:
        factors = torch.ones(where.n, dtype=torch.float64)
        total = delta_total(rows, base, where)
    else:
        factors, _ = clip_factors(sq, clip)
        total = clipped_total(rows, base, factors, mx_l, where)
    sel = ops.topk_threshold(resid, total, k)
    ops.topk_apply(base, resid, sel, eta / no_models)
    T, m = sel.tolist()
    return [float(x) for x in factors], [float(x) for x in sq.double().cpu().sqrt()], int(m), key_value(T)


def _weiszfeld(avg, dists, alphas: torch.Tensor, maxiter: int, eps: float, ftol: float, poll: int = 0):
    """Weiszfeld iteration control on the DEVICE (reference ``helper.py:320-352``, SURVEY
    §7.4.4): ``maxiter`` iterations are always enqueued; the stopping test
    ``|f_prev - f| < ftol * f`` clears a device flag that freezes the median, distances and
    weights from the converging iteration on (exactly the values the reference's ``break``
    leaves).  No host sync inside the loop: one read of the per-iteration objectives at the
    end (for the reference's log lines).  ``avg(w)``: weighted sum of the points for the
    normalised fp64 weights ``w`` (device); ``dists(m)``: fp64 distances of the points to m.
    ``poll`` > 0: read the flag every ``poll`` iterations and stop enqueueing once converged
    (the distributed form: each further iteration is two all-reduces; every rank reads the
    same all-reduced objective, so all stop at the same iteration).  Returns (median,
    distances, weights, iterations run = the reference's num_oracle_calls - 1)."""
    dev = alphas.device
    median = avg(alphas)
    d = dists(median)
    obj = (alphas * d).sum()
    active = torch.ones((), dtype=torch.bool, device=dev)
    weights = alphas.clone()
    wv = None
    hist = torch.zeros(maxiter, 3, dtype=torch.float64, device=dev)   # prev_obj, obj, logged
    for i in range(maxiter):
        w = alphas / torch.clamp(d, min=eps)
        w = w / w.sum()
        m_new = avg(w)
        d_new = dists(m_new)
        o_new = (alphas * d_new).sum()
        conv = (obj - o_new).abs() < ftol * o_new
        hist[i, 0], hist[i, 1] = obj, o_new
        hist[i, 2] = (active & ~conv).double()
        weights = torch.where(active, w, weights)
        median = torch.where(active, m_new, median)
        d = torch.where(active, d_new, d)
        obj = torch.where(active, o_new, obj)
        # wv = the weights of the last iteration that did NOT converge (D5: the current ones)
        upd = active & ~conv
        wv = torch.where(upd, w, wv) if wv is not None else torch.where(upd, w, torch.full_like(w, float("nan")))
        active = active & ~conv
        if poll > 0 and (i + 1) % poll == 0 and i + 1 < maxiter and not bool(active.item()):
            break
    h = hist.cpu().numpy()                       # the one host read of the aggregation
    for i in range(maxiter):
        if h[i, 2] > 0:
            log.info(f"[rfa agg] iter:  {i}, prev_obj_val: {h[i, 0]}, obj_val: {h[i, 1]}, "
                     f"abs dis: {abs(h[i, 0] - h[i, 1])}")
    wv_h = wv.cpu().numpy() if wv is not None else None
    if wv_h is None or np.isnan(wv_h).any():      # D5: converged at iteration 0
        wv_h = weights.cpu().numpy()
    # iterations the reference runs: up to and including the converging one (its break)
    iters = min(int((h[:, 2] > 0).sum()) + 1, maxiter)
    return median, d, wv_h, iters


def geometric_median(global_state: torch.Tensor, finals: torch.Tensor, num_samples: Sequence[int],
                     eta: float, maxiter: int, dp: bool, sigma: float, seed: int, n_update: int,
                     eps: float = 1e-5, ftol: float = 1e-6, max_update_norm: Optional[float] = None,
                     where: Optional[Shard] = None) -> Tuple[bool, List[float], List[float], int]:
    """Weiszfeld geometric median of the client deltas (reference ``helper.py:320-352``) over this
    rank's ``finals`` [len(idx), S]; returns (updated, wv, alphas, oracle calls).  Per iteration each
    rank forms its partial weighted sum of its own points as fixed-point limbs (one reduction of
    the [2, n_update] int64 limbs: exact, so the median's bits are the same at any world size) and
    its points' distances to the median (one reduction of an n-vector with zeros for other ranks'
    clients: exact); the fixed grid's exponent comes from the max |delta| over all clients (one max
    of a host float).  ``where`` None: every row is here (a single rank, or the server's gather
    mode) and nothing is reduced; with the points resident on their owner ranks the convergence
    flag is polled every second iteration (each further one is two reductions)."""
    poll = 0 if where is None else 2
    where = where or Shard(finals.shape[0])
    n, idx, dev = len(num_samples), where.idx, global_state.device
    points = finals[:, :n_update] - global_state[None, :n_update] if idx else None
    a = torch.tensor(num_samples, dtype=torch.float64, device=dev)
    alphas = a / a.sum()
    E = fixed_exponent(where.reduce_max(max_abs(points)), n)

    def avg(w: torch.Tensor) -> torch.Tensor:
        # exact fixed-point sum of the products (each quantised on its own)
        wn = w / w.sum()
        part = wsum_part(points, wn[where.index(dev)], E) if idx else wsum_zero(n_update, E, dev)
        return wsum_decode(where.reduce(part), E)

    def dists(m: torch.Tensor) -> torch.Tensor:
        sq = ops.sq_dists(points, m).double() if idx else None
        return where.sum_rows(sq, (), torch.float64, dev).clamp(min=0.0).sqrt()

    median, d, wv, iters = _weiszfeld(avg, dists, alphas, maxiter, eps, ftol, poll)
    return _rfa_apply(global_state, median, d, wv, eta, dp, sigma, seed, n_update, max_update_norm, iters)


def _rfa_apply(global_state, median, d, wv, eta, dp, sigma, seed, n_update, max_update_norm, iters):
    upd_norm = float(torch.linalg.vector_norm(median.double()).item())
    if max_update_norm is None or upd_norm < max_update_norm:
        ops.add_noise_scaled(global_state[:n_update], median, eta, sigma, seed, dp)
        updated = True
    else:
        log.info(f"\t\t\tUpdate norm = {upd_norm} is too large. Update rejected")
        updated = False
    return updated, [float(x) for x in wv], [float(x) for x in d.cpu().tolist()], 1 + iters


class FoolsGold:
    """FoolsGold with per-client history (reference helper.py:527-607)."""

    def __init__(self, use_memory: bool) -> None:
        self.use_memory = use_memory
        self.memory_dict: Dict[str, np.ndarray] = {}
        self.wv_history: List[np.ndarray] = []

    @staticmethod
    def weights(feats: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
        """FoolsGold weighting from the [n, d] feature matrix; the cosine Gram F F^T runs on
        the features' device (the MFMA Gram kernel on GPU), the n x n logic on the host."""
        n = feats.shape[0]
        g = ops.gram(feats).double().cpu()
        nrm = torch.sqrt(torch.clamp(torch.diagonal(g), min=0.0))
        nrm = torch.where(nrm == 0, torch.ones_like(nrm), nrm)   # sklearn normalises zero rows to 0
        cs = (g / nrm[:, None] / nrm[None, :]).numpy() - np.eye(n)
        return FoolsGold._from_cs(cs)

    @staticmethod
    def _from_cs(cs: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        n = cs.shape[0]
        cs = cs.copy()
        maxcs = np.max(cs, axis=1)
        for i in range(n):                      # pardoning
            for j in range(n):
                if i == j:
                    continue
                if maxcs[i] < maxcs[j]:
                    cs[i][j] = cs[i][j] * maxcs[i] / maxcs[j]
        wv = 1 - (np.max(cs, axis=1))
        wv[wv > 1] = 1
        wv[wv < 0] = 0
        alpha = np.max(cs, axis=1)
        wv = wv / np.max(wv)
        wv[(wv == 1)] = .99
        with np.errstate(divide="ignore", invalid="ignore"):
            wv = (np.log(wv / (1 - wv)) + 0.5)
        wv[(np.isinf(wv) + wv > 1)] = 1
        wv[(wv < 0)] = 0
        return wv, alpha

    def aggregate(self, grads: torch.Tensor, names: Sequence[Any], feat_slice: Tuple[int, int]
                  ) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
        """grads [n, P] summed client gradients -> (aggregated [P], wv, alpha)."""
        lo, hi = feat_slice
        wv, alpha = self.weights_from(grads[:, lo:hi], names)
        wts = torch.tensor(wv / len(names), dtype=torch.float32, device=grads.device)
        E = fixed_exponent(max_abs(grads), len(names))
        agg = wsum_decode(wsum_part(grads, wts, E), E)
        return agg, wv, alpha

    def weights_from(self, feat_rows: torch.Tensor, names: Sequence[Any]) -> Tuple[np.ndarray, np.ndarray]:
        """FoolsGold weights from this round's [n, d] final-layer gradient features (the
        reference's ``client_grads[i][-2]``, ``helper.py:544``): history update, cosine Gram,
        pardoning, logit.  Deterministic, so every rank computes the same weights."""
        feats = feat_rows.double().cpu().numpy()
        mem = np.zeros_like(feats)
        for i, nm in enumerate(names):
            key = str(nm)
            if key in self.memory_dict:
                self.memory_dict[key] = self.memory_dict[key] + feats[i]
            else:
                self.memory_dict[key] = feats[i].copy()
            mem[i] = self.memory_dict[key]
        use = mem if self.use_memory else feats
        wv, alpha = self.weights(torch.from_numpy(use).to(feat_rows.device, torch.float32))
        self.wv_history.append(wv)
        return wv, alpha

    def state(self) -> Dict[str, Any]:
        return {"memory": {k: torch.from_numpy(v) for k, v in self.memory_dict.items()}}

    def load_state(self, st: Dict[str, Any]) -> None:
        self.memory_dict = {k: v.double().numpy() for k, v in st.get("memory", {}).items()}


def foolsgold_server_step(global_state: torch.Tensor, agg: torch.Tensor, P: int, eta: float, lr: float,
                          wd: float) -> None:
    """Fresh ``SGD(lr, momentum, wd)`` single step with ``p.grad = eta * agg``
    (helper.py:280-290): first momentum step means buf = d_p, so p -= lr (eta*agg + wd*p)."""
    p = global_state[:P]
    p -= lr * (eta * agg + wd * p)

"""Experiment configuration: the reference's YAML schema, loaded into a typed dict.

The reference drives everything from one YAML file passed as ``--params`` and read into
a plain dict (reference ``main.py:88-92``); it mutates the dict at run time
(``helper.py:44-48``, ``image_helper.py:63``) and reads dynamic per-trigger keys such as
``{i}_poison_pattern`` / ``{i}_poison_epochs``.  ``Params`` keeps that
exact dict behaviour (so reference YAML files load unchanged, unknown/dead keys are kept
and ignored), adds the new framework's own keys with defaults that reproduce reference
behaviour, and exposes typed helpers for the dynamic keys.

Constants mirror reference ``config.py:4-13``.
"""
from __future__ import annotations

import copy
import math
import os
from typing import Any, Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import yaml

AGGR_MEAN = "mean"
AGGR_GEO_MED = "geom_median"
AGGR_FOOLSGOLD = "foolsgold"
AGGREGATIONS = (AGGR_MEAN, AGGR_GEO_MED, AGGR_FOOLSGOLD)

TYPE_LOAN = "loan"
TYPE_CIFAR = "cifar"
TYPE_MNIST = "mnist"
TYPE_TINYIMAGENET = "tiny-imagenet-200"
TYPES = (TYPE_LOAN, TYPE_CIFAR, TYPE_MNIST, TYPE_TINYIMAGENET)

# reference config.py:7-8 (declared but unused there; kept for API parity)
MAX_UPDATE_NORM = 1000
PATIENCE_ITER = 20

# Defaults of keys the reference reads (so partial YAMLs work) and of the new keys this
# framework adds.  Reference keys default to the values of utils/cifar_params.yaml.
_DEFAULTS: Dict[str, Any] = {
    # --- reference keys --------------------------------------------------------------
    "test_batch_size": 64,
    "batch_size": 64,
    "lr": 0.1,
    "poison_lr": 0.05,
    "momentum": 0.9,
    "decay": 0.0005,
    "epochs": 1,
    "internal_epochs": 1,
    "internal_poison_epochs": 6,
    "poisoning_per_batch": 5,
    "aggr_epoch_interval": 1,
    "aggregation_methods": AGGR_MEAN,
    "geom_median_maxiter": 10,
    "fg_use_memory": True,
    "participants_namelist": list(range(10)),
    "no_models": 10,
    "number_of_total_participants": 100,
    "is_random_namelist": True,
    "is_random_adversary": False,
    "is_poison": False,
    "baseline": False,
    "scale_weights_poison": 100,
    "eta": 0.1,
    "sampling_dirichlet": True,
    "dirichlet_alpha": 0.5,
    "poison_label_swap": 2,
    "adversary_list": [],
    "centralized_test_trigger": True,
    "trigger_num": 0,
    "poison_epochs": [],
    "poison_step_lr": True,
    "alpha_loss": 1.0,
    "diff_privacy": False,
    "sigma": 0.01,
    "save_model": False,
    "save_on_epochs": [],
    "resumed_model": False,
    "resumed_model_name": "",
    "vis_train": False,
    "vis_train_batch_loss": False,
    "vis_trigger_split_test": False,
    "batch_track_distance": False,
    "tied": False,
    # --- new keys (this framework) -----------------------------------------------------
    "seed": 1,                    # reference seeds python/torch with 1 (main.py:36-38,86)
    "data_dir": "./data",         # torchvision root in the reference (image_helper.py:175)
    "save_dir": "saved_models",   # run-dir parent (helper.py:35)
    "synthetic_data": "auto",     # auto: real files if present under data_dir, else synthetic
    "synthetic_train_size": None,  # override synthetic dataset sizes (tests / smoke runs)
    "synthetic_test_size": None,
    # synthetic LOAN rows over all 51 states (default: the LendingClub dump's 2,260,668 loans,
    # split by approximate LendingClub state shares; tests pass a small value)
    "synthetic_loan_rows": None,
    "synthetic_noise": None,       # synthetic image pixel-noise sigma (None: per-dataset default)
    "synthetic_shared": None,      # fraction of the class template shared by all classes
    "synthetic_clutter": None,     # weight of the per-image random background field
    "synthetic_sky": None,         # fraction of images with a saturated bright top band (None: per dataset)
    "synthetic_margin": None,      # exactly black border width in pixels (None: per dataset)
    "synthetic_sky_rows": None,    # rows of the bright band (row 0 saturated; None: 3)
    "synthetic_contrast": None,    # [lo, hi] per-image contrast range (None: [0.6, 1.2])
    "compute_dtype": "fp32",      # fp32 = reference precision (split fp32 operands on the 16-bit MFMA)
    "eval_batch_size": 1024,      # per-model eval chunk (reference: 64; a free parameter, D13)
    "aggregate_bn_buffers": True,  # D2: deltas/aggregation include BN running stats
    "best_on_clean_loss": False,   # D6: reference keys .best on the poison-test loss
    "visdom": False,               # live plots need a visdom server; JSONL stream always on
    "metrics_jsonl": True,
    "max_rounds": None,            # stop after this many rounds (bench / smoke)
    "local_eval": True,            # per-client local tests (reference behaviour)
    "graph_capture": True,         # HIP-graph the grouped training step on GPU
    "overlap_eval": True,          # evaluate round r on a side stream under round r+1's training
    "early_local_eval": True,      # enqueue a client's local tests as soon as it finishes training
    # N > 1 ranks: image-sharded tests split by water-filling over each rank's load in the
    # window (training of the next round + its local tests), in eval image-forward units:
    # one grouped training step costs balance_step_latency + balance_step_per_client * active.
    # The constants are calibrated for fp32 CIFAR ResNets on MI355X
    # (profiles/balance_sweep_r3/); None = on for CIFAR only, the strided even split elsewhere
    # (MNIST / LOAN / Tiny have other step-to-forward cost ratios: set both constants with it)
    "eval_balance": None,
    "balance_step_latency": 2400.0,
    "balance_step_per_client": 420.0,
    "rfa_mode": "auto",            # RFA across ranks: gather | distributed | auto (fewer bytes)
    "pretrain_rounds": 0,          # benign FedAvg warm start when not resuming (Server.pretrain)
    "pretrain_central_epochs": 0,  # centralised warm start epochs, before any FedAvg warm start
    "nan_check": True,             # abort the run if the aggregated global model is not finite
    "max_update_norm": None,       # RFA update-norm rejection (helper.py:360-369; never enabled there)
    # norm-clipped FedAvg (aggregation "mean" only): each client's update is scaled to an L2 norm
    # of at most C before averaging.  None = off; a finite number > 0 = C; "median" = the lower
    # median of the round's client update norms.  With diff_privacy the noise then sits on a sum
    # of bounded sensitivity
    "clip_norm": None,
    # FLAME (with clip_norm: median only; Nguyen et al., USENIX Security 2022): the cosine distances
    # between the clients' updates are clustered, the majority cluster (at least n // 2 + 1 clients,
    # single linkage: what HDBSCAN returns with the paper's parameters) is admitted, the admitted
    # updates are clipped to the round's median update norm S and averaged, and N(0, (lambda S)^2)
    # noise is added.  clip_flame: None / false = off (plain clipping); true = FLAME (needs
    # no_models >= 3; not with diff_privacy: FLAME sets its own noise level).  clip_flame_lambda
    # (with clip_flame: true only): None = 0.001, the paper's value for image models; a finite
    # float >= 0 = lambda (0 adds no noise)
    "clip_flame": None,
    "clip_flame_lambda": None,
    # Multi-Krum (aggregation "mean" only; Blanchard et al., NeurIPS 2017): each client is scored
    # by the sum of its n - f - 2 smallest squared distances to the other clients' final states and
    # the m best-scored clients are averaged.  krum_f: None = off; an integer >= 0 = f, the number
    # of Byzantine clients tolerated per round (needs n >= 2 f + 3).  krum_m: None = n - f
    # (Multi-Krum); an integer in 1 .. n - f = m (1 is the original Krum).  krum_bulyan: None / false =
    # Multi-Krum; true = Bulyan (El Mhamdi, Guerraoui and Rouault, ICML 2018) with f = krum_f: Krum
    # iterated n - 2 f times picks the clients, then per coordinate the n - 4 f of their values closest
    # to the median are averaged (needs n >= 4 f + 3; not with krum_m)
    "krum_f": None,
    "krum_m": None,
    "krum_bulyan": None,
    # coordinate-wise trimmed mean / median (aggregation "mean" only; Yin et al., ICML 2018): per
    # coordinate the k smallest and k largest of the n client values are dropped and the rest
    # averaged.  None = off; an integer k >= 1 (needs n >= 2 k + 1); "median" = k = (n - 1) // 2,
    # the coordinate-wise median (the mean of the two middle values for even n)
    "trim_k": None,
    # robust learning rate (aggregation "mean" only; Ozdayi, Kantarcioglu and Gel, AAAI 2021): the
    # server takes a sign vote per coordinate over the clients' updates and applies the averaged
    # update with a negative rate where the vote's |sum| is below theta.  None = off; an integer
    # theta with 1 <= theta <= no_models
    "rlr_threshold": None,
    # SparseFed (aggregation "mean" only; Panda et al., AISTATS 2022): the round's aggregate is added
    # into a server-side error-feedback residual and only the k largest-magnitude coordinates of the
    # residual reach the model (and leave the residual); the rest wait there for later rounds.
    # sparse_topk: None = off; a float fraction with 0 < frac <= 1, k = max(1, floor(frac * entries
    # aggregated)) (an integer is an error: YAML 1 must not mean one coordinate).  Not with
    # diff_privacy: noise on every coordinate undoes the sparsity, noise on the kept ones only
    # publishes the support
    "sparse_topk": None,
    # sparse_clip (with sparse_topk only): each client's update is clipped before it enters the
    # aggregate, with clip_norm's grammar: None = off; a finite number > 0 = C; "median" = the lower
    # median of the round's client update norms
    "sparse_clip": None,
    # norm-bounded (PGD) attacker (Sun et al. 2019; Wang et al., NeurIPS 2020): while a client trains
    # with a trigger its state is projected, after every SGD step, onto the L2 ball of radius
    # delta / gamma around its phase-start state, over the entries the server aggregates; gamma =
    # scale_weights_poison when the phase is scaled afterwards (not baseline), else 1, so the update
    # it submits has norm at most delta.  None = off; a finite number > 0 = delta.  Needs is_poison
    # and aggr_epoch_interval == 1; not with foolsgold (which aggregates gradient sums).  LOAN then
    # trains on the per-step graph (the persistent launch has no per-step hook)
    "poison_pgd_norm": None,
    # Neurotoxin attacker (Zhang et al., ICML 2022): while a client trains with a trigger, every
    # parameter outside a coordinate mask is set back, after every SGD step, to its phase-start
    # value, so the update it submits is exactly 0 there.  The server rebuilds the mask each round
    # from the update it just applied: the k = max(1, floor(rho * P)) parameters that moved least
    # (ties at the threshold all kept), ranked globally.  None = off; a float 0 < rho <= 1 = the kept
    # fraction (an int is an error, as for sparse_topk).  Needs is_poison and aggr_epoch_interval ==
    # 1; not with foolsgold (which aggregates gradient sums).  LOAN then trains on the per-step graph
    "poison_neurotoxin_ratio": None,
    "pretrain_eta": 1.0,
    "pretrain_lr": None,           # client lr of the warm start (None: the config's lr)
    "model_arch": None,            # cifar only: resnet{18,34,50,101,152}_cifar (resnet_cifar.py:106-116);
                                   # None = ResNet-18 as in image_helper.py:33-38
}

# keys whose value may legitimately be a python list of ints/strings
_CLIENT_ID_KEYS = ("adversary_list", "participants_namelist")


class Params(dict):
    """dict with typed accessors; behaves exactly like the reference's params dict."""

    def __init__(self, data: Optional[Dict[str, Any]] = None, **kw: Any) -> None:
        super().__init__()
        merged = copy.deepcopy(_DEFAULTS)
        if data:
            merged.update(data)
        merged.update(kw)
        super().update(merged)
        self._validate()

    # ------------------------------------------------------------------ helpers
    def _validate(self) -> None:
        t = self.get("type")
        if t is not None and t not in TYPES:
            raise ValueError(f"unknown workload type {t!r}; expected one of {TYPES}")
        if self["aggregation_methods"] not in AGGREGATIONS:
            raise ValueError(f"unknown aggregation {self['aggregation_methods']!r}")
        if self["aggregation_methods"] == AGGR_FOOLSGOLD and self["aggr_epoch_interval"] != 1:
            # reference image_train.py:24 'only works for aggr_epoch_interval=1'
            raise ValueError("foolsgold requires aggr_epoch_interval == 1")
        # the options of "mean" (MEAN_OPTIONS): each on its own, and with "mean" only
        earlier: List[str] = []
        earlier_on = False
        for opt in MEAN_OPTIONS:
            on = getattr(self, opt.key) is not None
            for k in opt.companions:
                if getattr(self, k) is not None and not on:
                    raise ValueError(f"{k} is set without {opt.key}")
            if on:
                if self["aggregation_methods"] != AGGR_MEAN:
                    raise ValueError(f"{opt.key} is an option of aggregation {AGGR_MEAN!r} "
                                     f"(got {self['aggregation_methods']!r})")
                if earlier_on:
                    others = (f"and {earlier[0]} cannot be combined" if len(earlier) == 1 else
                              f"cannot be combined with {', '.join(earlier[:-1])} or {earlier[-1]}")
                    raise ValueError(f"{opt.key} {others}")
                if opt.sizes is not None:
                    opt.sizes(self, int(self["no_models"]), "no_models")
            earlier.append(opt.key)
            earlier_on = earlier_on or on
        if self.clip_flame:
            if self.clip_norm != CLIP_MEDIAN:
                raise ValueError(f"clip_flame needs clip_norm: {CLIP_MEDIAN!r} (got {self.clip_norm!r}): FLAME clips "
                                 "to the round's median update norm")
            if self["diff_privacy"]:
                raise ValueError("clip_flame cannot be combined with diff_privacy (FLAME sets its own noise "
                                 "level, clip_flame_lambda times the median update norm)")
            check_flame_sizes(int(self["no_models"]), "no_models")
        elif self.clip_flame_lambda is not None:
            raise ValueError("clip_flame_lambda is set without clip_flame: true")
        if self.sparse_topk is not None and self["diff_privacy"]:
            raise ValueError("sparse_topk cannot be combined with diff_privacy (noise on the dropped "
                             "coordinates undoes the sparsity, noise on the kept ones publishes the support)")
        if self.poison_pgd_norm is not None:
            if self["aggregation_methods"] == AGGR_FOOLSGOLD:
                raise ValueError("poison_pgd_norm cannot be combined with aggregation 'foolsgold' (it aggregates "
                                 "gradient sums, not state deltas)")
            if self["aggr_epoch_interval"] != 1:
                raise ValueError("poison_pgd_norm requires aggr_epoch_interval == 1 (the ball's centre moves at "
                                 "every phase end: the bound would hold per phase only)")
            if not self["is_poison"]:
                raise ValueError("poison_pgd_norm is set without is_poison: true")

        if self.poison_neurotoxin_ratio is not None:
            if self["aggregation_methods"] == AGGR_FOOLSGOLD:
                raise ValueError("poison_neurotoxin_ratio cannot be combined with aggregation 'foolsgold' (it "
                                 "aggregates gradient sums, not state deltas)")
            if self["aggr_epoch_interval"] != 1:
                raise ValueError("poison_neurotoxin_ratio requires aggr_epoch_interval == 1 (the restore's base "
                                 "moves at every phase end: the update would be masked per phase only)")
            if not self["is_poison"]:
                raise ValueError("poison_neurotoxin_ratio is set without is_poison: true")

    @property
    def poison_neurotoxin_ratio(self) -> Optional[float]:
        """The checked ``poison_neurotoxin_ratio``: None (off) or the kept fraction rho."""
        return check_neurotoxin_ratio(self.get("poison_neurotoxin_ratio"))

    @property
    def poison_pgd_norm(self) -> Optional[float]:
        """The checked ``poison_pgd_norm``: None (off) or the bound delta as a float."""
        return check_pgd_norm(self.get("poison_pgd_norm"))

    @property
    def type(self) -> str:
        return self["type"]

    @property
    def clip_norm(self) -> Any:
        """The checked ``clip_norm``: None (off), the bound C as a float, or ``"median"``."""
        return check_clip_norm(self.get("clip_norm"))

    @property
    def clip_flame(self) -> Optional[bool]:
        """The checked ``clip_flame``: None (plain clipping; ``false`` reads as None) or True (FLAME)."""
        return check_clip_flame(self.get("clip_flame"))

    @property
    def clip_flame_lambda(self) -> Optional[float]:
        """The checked ``clip_flame_lambda``: None (the default, ``FLAME_LAMBDA``) or lambda >= 0."""
        return check_flame_lambda(self.get("clip_flame_lambda"))

    @property
    def flame_lambda(self) -> float:
        """FLAME's noise factor lambda: ``clip_flame_lambda``, or ``FLAME_LAMBDA`` when it is None."""
        v = self.clip_flame_lambda
        return FLAME_LAMBDA if v is None else v

    @property
    def krum_f(self) -> Optional[int]:
        """The checked ``krum_f``: None (Multi-Krum off) or f >= 0."""
        return check_krum_int("krum_f", self.get("krum_f"), 0)

    @property
    def krum_m(self) -> Optional[int]:
        """The checked ``krum_m``: None (m = n - f) or m >= 1."""
        return check_krum_int("krum_m", self.get("krum_m"), 1)

    @property
    def krum_bulyan(self) -> Optional[bool]:
        """The checked ``krum_bulyan``: None (Multi-Krum; ``false`` reads as None) or True (Bulyan)."""
        return check_krum_bulyan(self.get("krum_bulyan"))

    @property
    def trim_k(self) -> Any:
        """The checked ``trim_k``: None (off), k >= 1 or ``"median"``."""
        return check_trim_k(self.get("trim_k"))

    @property
    def rlr_threshold(self) -> Optional[int]:
        """The checked ``rlr_threshold``: None (off) or theta >= 1."""
        return check_rlr_threshold(self.get("rlr_threshold"))

    @property
    def sparse_topk(self) -> Optional[float]:
        """The checked ``sparse_topk``: None (SparseFed off) or the kept fraction in (0, 1]."""
        return check_sparse_topk(self.get("sparse_topk"))

    @property
    def sparse_clip(self) -> Any:
        """The checked ``sparse_clip``: None (off), the bound C as a float, or ``"median"``."""
        return check_clip_norm(self.get("sparse_clip"), "sparse_clip")

    @property
    def adversary_list(self) -> List[Any]:
        return list(self.get("adversary_list") or [])

    def poison_pattern(self, idx: int) -> List[List[int]]:
        """Pixel (row, col) list of local trigger ``idx``; ``-1`` = union of all (global).

        reference image_helper.py:328-335
        """
        if idx == -1:
            out: List[List[int]] = []
            for i in range(int(self["trigger_num"])):
                out.extend(self.get(f"{i}_poison_pattern", []))
            return out
        return list(self.get(f"{idx}_poison_pattern", []))

    def poison_epochs_of(self, adv_index: int) -> List[int]:
        """Rounds in which adversary ``adv_index`` poisons (reference image_train.py:38-43)."""
        key = f"{adv_index}_poison_epochs"
        if key in self:
            return list(self[key])
        return list(self.get("poison_epochs") or [])

    def trigger_features(self, idx: int) -> List[tuple]:
        """LOAN trigger (feature name, value) pairs; ``-1`` = all triggers (test.py:62-67)."""
        if idx == -1:
            out: List[tuple] = []
            for j in range(int(self["trigger_num"])):
                out.extend(zip(self.get(f"{j}_poison_trigger_names", []),
                               self.get(f"{j}_poison_trigger_values", [])))
            return out
        return list(zip(self.get(f"{idx}_poison_trigger_names", []),
                        self.get(f"{idx}_poison_trigger_values", [])))

    def adversary_index(self, name: Any) -> int:
        """Index of ``name`` in adversary_list or -1 (reference image_train.py:40-46)."""
        for i, a in enumerate(self.adversary_list):
            if _same_client(a, name):
                return i
        return -1

    def is_adversary(self, name: Any) -> bool:
        return self.adversary_index(name) >= 0

    def to_plain(self) -> Dict[str, Any]:
        return {k: v for k, v in self.items()}


CLIP_MEDIAN = "median"


def check_clip_norm(v: Any, key: str = "clip_norm") -> Any:
    """None, a finite bound > 0 (returned as float) or ``"median"``; anything else is an error
    (``key``: the config key in the message; ``sparse_clip`` has the same grammar)."""
    if v is None or (isinstance(v, str) and v == CLIP_MEDIAN):
        return v
    if isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0:
        return float(v)
    raise ValueError(f"{key} {v!r}: expected None, a finite number > 0 or {CLIP_MEDIAN!r}")


FLAME_LAMBDA = 0.001     # the paper's noise factor for image models (sigma = lambda * median norm)


def check_clip_flame(v: Any) -> Optional[bool]:
    """None for None / False (plain clipping), True for True (FLAME); anything else is an error."""
    if v is None or v is False:
        return None
    if v is True:
        return True
    raise ValueError(f"clip_flame {v!r}: expected None, false or true")


def check_flame_lambda(v: Any) -> Optional[float]:
    """None or a finite number >= 0 (returned as float; a bool, a string or a list is an error)."""
    if v is None:
        return None
    if isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v >= 0:
        return float(v)
    raise ValueError(f"clip_flame_lambda {v!r}: expected None or a finite number >= 0")


def check_flame_sizes(n: int, what: str = "n") -> int:
    """FLAME's inequality for n clients: n >= 3 (with two clients the majority m = n // 2 + 1 is
    both of them and nothing can be filtered).  Returns m."""
    if n < 3:
        raise ValueError(f"clip_flame needs {what} >= 3 (got {n})")
    return n // 2 + 1


def check_krum_int(key: str, v: Any, lo: int) -> Optional[int]:
    """None or an integer >= ``lo`` (a bool, a float or a string is an error)."""
    if v is None:
        return None
    if isinstance(v, int) and not isinstance(v, bool) and v >= lo:
        return v
    raise ValueError(f"{key} {v!r}: expected None or an integer >= {lo}")


def check_krum_sizes(n: int, f: int, m: Optional[int], what: str = "n") -> int:
    """Multi-Krum's two inequalities for n clients: n >= 2 f + 3 (so every score sums n - f - 2 >=
    f + 1 >= 1 distances) and m <= n - f.  Returns m (``n - f`` when None)."""
    if n < 2 * f + 3:
        raise ValueError(f"krum_f {f} needs {what} >= 2 f + 3 = {2 * f + 3} (got {n})")
    if m is None:
        return n - f
    if m > n - f:
        raise ValueError(f"krum_m {m} exceeds {what} - krum_f = {n - f}")
    return m


def check_krum_bulyan(v: Any) -> Optional[bool]:
    """None for None / False (Multi-Krum), True for True (Bulyan); anything else is an error."""
    if v is None or v is False:
        return None
    if v is True:
        return True
    raise ValueError(f"krum_bulyan {v!r}: expected None, false or true")


def check_bulyan_sizes(n: int, f: int, what: str = "n") -> int:
    """Bulyan's inequality for n clients: n >= 4 f + 3 (so the n - 2 f clients that iterated Krum
    selects leave beta = n - 4 f >= 3 values per coordinate, and every Krum iteration but the
    clamped last ones scores at least one neighbour).  Returns theta = n - 2 f."""
    if n < 4 * f + 3:
        raise ValueError(f"krum_bulyan with krum_f {f} needs {what} >= 4 f + 3 = {4 * f + 3} (got {n})")
    return n - 2 * f


def krum_option_sizes(p: "Params", n: int, what: str = "n") -> int:
    """The Krum option's inequalities for n clients: Multi-Krum's (returns m) or, with
    ``krum_bulyan``, Bulyan's (returns theta; ``krum_m`` has no meaning there)."""
    if p.krum_bulyan:
        if p.krum_m is not None:
            raise ValueError("krum_bulyan cannot be combined with krum_m (Bulyan selects n - 2 f clients)")
        return check_bulyan_sizes(n, p.krum_f, what)
    return check_krum_sizes(n, p.krum_f, p.krum_m, what)


TRIM_MEDIAN = "median"


def check_trim_k(v: Any) -> Any:
    """None, an integer k >= 1 or ``"median"`` (a bool, a float or another string is an error)."""
    if v is None or (isinstance(v, str) and v == TRIM_MEDIAN):
        return v
    if isinstance(v, int) and not isinstance(v, bool) and v >= 1:
        return v
    raise ValueError(f"trim_k {v!r}: expected None, an integer >= 1 or {TRIM_MEDIAN!r}")


def check_trim_sizes(n: int, trim_k: Any, what: str = "n") -> int:
    """The trim count k for n clients: ``trim_k``, or (n - 1) // 2 for ``"median"``; n >= 2 k + 1
    (so at least one value per coordinate is kept) and n >= 1."""
    k = (n - 1) // 2 if trim_k == TRIM_MEDIAN else int(trim_k)
    if n < 1 or n < 2 * k + 1:
        raise ValueError(f"trim_k {trim_k} needs {what} >= 2 k + 1 = {2 * max(k, 0) + 1} (got {n})")
    return k


def check_rlr_threshold(v: Any) -> Optional[int]:
    """None or an integer theta >= 1 (a bool, a float, a string or a list is an error)."""
    if v is None:
        return None
    if isinstance(v, int) and not isinstance(v, bool) and v >= 1:
        return v
    raise ValueError(f"rlr_threshold {v!r}: expected None or an integer >= 1")


def check_rlr_sizes(n: int, theta: int, what: str = "n") -> int:
    """The vote threshold for n clients: 1 <= theta <= n (|V| <= n, so a larger theta would flip
    every coordinate)."""
    if theta < 1 or theta > n:
        raise ValueError(f"rlr_threshold {theta} needs 1 <= theta <= {what} (got {n})")
    return theta


def check_sparse_topk(v: Any) -> Optional[float]:
    """None or a float fraction with 0 < frac <= 1 (a bool, an int, a string or a list is an error:
    an int is rejected so that 1 cannot be read as one coordinate)."""
    if v is None:
        return None
    if isinstance(v, float) and 0.0 < v <= 1.0:
        return v
    raise ValueError(f"sparse_topk {v!r}: expected None or a float fraction with 0 < frac <= 1")


def check_pgd_norm(v: Any) -> Optional[float]:
    """None or a finite bound > 0 (returned as float; a bool, a string or a list is an error)."""
    if v is None:
        return None
    if isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0:
        return float(v)
    raise ValueError(f"poison_pgd_norm {v!r}: expected None or a finite number > 0")


def check_neurotoxin_ratio(v: Any) -> Optional[float]:
    """None or a float fraction with 0 < rho <= 1 (a bool, an int, a string or a list is an error: an
    int is rejected so that YAML ``1`` cannot be read as the ratio 1.0)."""
    if v is None:
        return None
    if isinstance(v, float) and 0.0 < v <= 1.0:
        return v
    raise ValueError(f"poison_neurotoxin_ratio {v!r}: expected None or a float fraction with 0 < rho <= 1")


class MeanOption(NamedTuple):
    """One option of aggregation ``"mean"``.  ``Params.<key>`` is its checked value (None: off)."""
    key: str
    companions: Tuple[str, ...]     # keys that mean nothing without it
    gathers: bool                   # the rule reads every client's final row on every rank
    sizes: Optional[Callable[["Params", int, str], Any]]   # the rule's inequalities for n clients


# in the order ``Server._aggregate`` looks for them; at most one is set
MEAN_OPTIONS = (
    MeanOption("clip_norm", ("clip_flame", "clip_flame_lambda"), False, None),
    MeanOption("krum_f", ("krum_m", "krum_bulyan"), True, krum_option_sizes),
    MeanOption("trim_k", (), True, lambda p, n, what: check_trim_sizes(n, p.trim_k, what)),
    MeanOption("rlr_threshold", (), False, lambda p, n, what: check_rlr_sizes(n, p.rlr_threshold, what)),
    MeanOption("sparse_topk", ("sparse_clip",), False, None),
)
MEAN_OPTION_KEYS = tuple(k for opt in MEAN_OPTIONS for k in (opt.key,) + opt.companions)


def mean_option(p: Params) -> Optional[MeanOption]:
    """The option of aggregation ``"mean"`` that ``p`` sets (None: plain FedAvg)."""
    for opt in MEAN_OPTIONS:
        if getattr(p, opt.key) is not None:
            return opt
    return None


def _same_client(a: Any, b: Any) -> bool:
    if a == b:
        return True
    try:
        return int(a) == int(b)
    except (TypeError, ValueError):
        return str(a) == str(b)


def load_params(path: str, overrides: Optional[Dict[str, Any]] = None) -> Params:
    """Load a reference-style YAML file (``yaml.safe_load``: reference used the PyYAML<6
    ``yaml.load(f)`` API, quirk D8)."""
    with open(path, "r") as f:
        data = yaml.safe_load(f) or {}
    if not isinstance(data, dict):
        raise ValueError(f"{path}: top level must be a mapping")
    if overrides:
        data.update(overrides)
    return Params(data)


def parse_override(items: Iterable[str]) -> Dict[str, Any]:
    """``key=value`` CLI overrides; values are parsed as YAML scalars/lists."""
    out: Dict[str, Any] = {}
    for it in items:
        if "=" not in it:
            raise ValueError(f"override {it!r} is not key=value")
        k, v = it.split("=", 1)
        out[k.strip()] = yaml.safe_load(v)
    return out


def default_dataset_name(t: str) -> str:
    """Run-name default per workload (reference main.py:96-108)."""
    return {TYPE_LOAN: "loan", TYPE_CIFAR: "cifar", TYPE_MNIST: "mnist",
            TYPE_TINYIMAGENET: "tiny"}[t]

"""The collectives ``Server._aggregate`` issues, per aggregation rule: one round through ``Server`` on
CPU with ``Server._reduce`` / ``Server._reduce_max`` wrapped to record (kind, dtype, shape) while
``_aggregate`` runs.  The sequence (order, dtype and shape) is what every rank of a multi-rank run
puts on the wire, so it must not move when the aggregation code is reorganised."""
import pytest
import torch

import test_trim_aggregation as trim_cpu

F64, F32, I64, I32 = torch.float64, torch.float32, torch.int64, torch.int32
MAX = ("max", float, ())


def record_round(tmp, **kw):
    """Round 12 of the small MNIST config: (the recorded sequence, the server)."""
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    s = Server(trim_cpu.mnist_params(tmp, **kw), DistCtx(), write_outputs=False)
    seen, live = [], []
    reduce, reduce_max, aggregate = s._reduce, s._reduce_max, s._aggregate

    def rec_reduce(t):
        if live:
            seen.append(("sum", t.dtype, tuple(t.shape)))
        return reduce(t)

    def rec_max(v):
        assert isinstance(v, float)
        if live:
            seen.append(MAX)
        return reduce_max(v)

    def rec_aggregate(*a):
        live.append(True)
        try:
            return aggregate(*a)
        finally:
            live.pop()
    s._reduce, s._reduce_max, s._aggregate = rec_reduce, rec_max, rec_aggregate
    s.run_round(12)
    return seen, s


def sizes(s):
    p = s.params
    return int(p["no_models"]), (s.spec.S if p["aggregate_bn_buffers"] else s.spec.P)


def test_plain_mean(tmp_path):
    seen, s = record_round(tmp_path)
    n, n_upd = sizes(s)
    assert seen == [("sum", F64, (n_upd,))]


def test_clip_norm(tmp_path):
    seen, s = record_round(tmp_path, clip_norm="median")
    n, n_upd = sizes(s)
    assert seen == [("sum", F64, (n,)), MAX, ("sum", I64, (2, n_upd))]


def test_krum(tmp_path):
    seen, _ = record_round(tmp_path, krum_f=1)
    assert seen == []


def test_trim(tmp_path):
    seen, _ = record_round(tmp_path, trim_k=2)
    assert seen == []


def test_rlr(tmp_path):
    seen, s = record_round(tmp_path, rlr_threshold=4)
    n, n_upd = sizes(s)
    assert seen == [("sum", F64, (n_upd,)), ("sum", I32, (n_upd,)), ("sum", I64, (n, 2))]


def test_foolsgold(tmp_path):
    seen, s = record_round(tmp_path, aggregation_methods="foolsgold")
    n, _ = sizes(s)
    lo, hi = s.spec.fg_feature_slice()
    assert seen == [("sum", F32, (n, hi - lo)), MAX, ("sum", I64, (2, s.spec.P))]


def test_rfa_gather_mode(tmp_path):
    seen, _ = record_round(tmp_path, aggregation_methods="geom_median")
    assert seen == []

"""Norm-clipped FedAvg on the GPU: the fused HIP passes of csrc/kernels/clip.hip (delta stats,
clipped delta sum on the fixed-point limbs, fp64 fallback) against the CPU reference ops and the
numpy fp64 oracle of clip_cases.py, and one model-replacement round through ``Server``."""
import functools
import os

import pytest
import torch

import clip_cases as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = cc.SMALL_CASES + [cc.WRAP_CASE]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs and the CPU reference of a case, computed once: (rows, base, scale, E, limbs)."""
    from dba_mod_amd.ops import reference as R
    rows, base, scale = cc.make_case(*case)
    _, mx = R.delta_stats(rows, base)
    E = cc.exponent(mx.numpy(), rows.shape[0])
    return rows, base, scale, E, R.clipped_delta_sum_fixed(rows, base, scale, E)


def _on_device(case, dev):
    """The same strided view on the device: big[:, off:off + L] of a [n, rstride] buffer."""
    n, L, rstride, off = case
    rows, base, scale, _, _ = _case(case)
    big = torch.zeros(n, rstride, device=dev)
    big[:, off:off + L] = rows.to(dev)
    view = big[:, off:off + L]
    assert view.stride(0) == rstride or n == 1
    return view, base.to(dev), scale.to(dev)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernels_match_reference(dev, case):
    from dba_mod_amd import ops
    rows, base, scale, E, limbs_ref = _case(case)
    n = rows.shape[0]
    d_rows, d_base, d_scale = _on_device(case, dev)
    sq, mx = ops.delta_stats(d_rows, d_base)
    cc.check_stats(sq, mx, rows, base, scale)
    sq2, mx2 = ops.delta_stats(d_rows, d_base)
    assert torch.equal(sq, sq2) and torch.equal(mx, mx2)          # bitwise run to run
    assert cc.exponent(mx.cpu().numpy(), n) == E
    limbs = ops.clipped_delta_sum_fixed(d_rows, d_base, d_scale, E)
    assert limbs.dtype == torch.int64 and tuple(limbs.shape) == (2, base.numel())
    assert torch.equal(limbs.cpu(), limbs_ref)                    # bit for bit the CPU reference's
    cc.check_decoded(limbs, E, rows, base, scale)
    cc.check_fp64(ops.clipped_delta_sum(d_rows, d_base, d_scale), rows, base, scale)


def test_aligned_copy_and_misaligned_view_agree(dev):
    """The offset-1 view (every row misaligned: scalar loads) and a 16-byte aligned copy of it
    (vector loads) give the same bits, squared norms included."""
    from dba_mod_amd import ops
    case = cc.SMALL_CASES[3]
    _, _, _, E, _ = _case(case)
    view, base, scale = _on_device(case, dev)
    assert view.data_ptr() % 16 != 0
    L = view.shape[1]
    pad = torch.zeros(view.shape[0], (L + 3) // 4 * 4, device=dev)
    pad[:, :L] = view
    copy = pad[:, :L]
    assert copy.data_ptr() % 16 == 0 and copy.stride(0) % 4 == 0
    a, b = ops.delta_stats(view, base), ops.delta_stats(copy, base)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.clipped_delta_sum_fixed(view, base, scale, E),
                       ops.clipped_delta_sum_fixed(copy, base, scale, E))
    assert torch.equal(ops.clipped_delta_sum(view, base, scale), ops.clipped_delta_sum(copy, base, scale))


def test_no_rows_returns_zeros(dev):
    from dba_mod_amd import ops
    base = torch.randn(37, device=dev)
    rows = torch.zeros(0, 37, device=dev)
    sq, mx = ops.delta_stats(rows, base)
    assert sq.shape == (0,) and mx.shape == (0,) and sq.dtype == torch.float64 and mx.dtype == torch.float32
    scale = torch.zeros(0, device=dev)
    assert torch.equal(ops.clipped_delta_sum_fixed(rows, base, scale, 5), torch.zeros(2, 37, dtype=torch.int64, device=dev))
    assert torch.equal(ops.clipped_delta_sum(rows, base, scale), torch.zeros(37, dtype=torch.float64, device=dev))


def test_nan_surfaces_in_stats_and_fallback(dev):
    """A NaN delta: NaN squared norm, max |delta| = +inf (not swallowed by the max), and the fp64
    fallback carries it into the sum."""
    from dba_mod_amd import ops
    base = torch.zeros(3000, device=dev)
    rows = torch.randn(3, 3000, device=dev)
    rows[1, 2047] = float("nan")
    sq, mx = ops.delta_stats(rows, base)
    assert torch.isnan(sq[1]) and torch.isfinite(sq[[0, 2]]).all()
    assert float(mx[1]) == float("inf") and torch.isfinite(mx[[0, 2]]).all()
    out = ops.clipped_delta_sum(rows, base, torch.ones(3, device=dev))
    assert torch.isnan(out[2047]) and int(torch.isnan(out).sum()) == 1


def test_server_round_clips_the_attacker(dev, tmp_path):
    """The CPU invariant test's round (MNIST synthetic, attacker 41 poisons in round 12 with scale
    100) on the GPU with clip_norm = median: the update-norm bound holds, the attacker's factor is
    < 0.1 x the smallest benign one, and a second identical run gives the same bits."""
    from dba_mod_amd import config as C
    from dba_mod_amd.fl.server import Server
    from dba_mod_amd.parallel.dist import DistCtx
    outs = []
    for rep in range(2):
        p = C.load_params(os.path.join(ROOT, "configs", "mnist_params.yaml"),
                          {"resumed_model": False, "start_epoch": 11, "synthetic_data": True,
                           "synthetic_train_size": 4000, "synthetic_test_size": 600,
                           "save_dir": str(tmp_path / f"r{rep}"), "eval_batch_size": 300, "clip_norm": "median"})
        s = Server(p, DistCtx(device=dev), write_outputs=False)
        before = s.global_state.clone()
        s.run_round(12)
        outs.append(s.global_state.clone())
        if rep == 0:
            names, factors, norms = s.csv.weight_result
            n = len(names)
            bound_c = sorted(norms)[(n - 1) // 2]
            n_upd = s.spec.S if p["aggregate_bn_buffers"] else s.spec.P
            got = float((s.global_state.double() - before.double())[:n_upd].norm())
            bound = float(p["eta"]) * (n / int(p["no_models"])) * bound_c * (1 + 1e-6)
            print(f"update norm {got:.6g}, bound {bound:.6g}, C {bound_c:.6g}; factors {factors}; norms {norms}")
            assert got <= bound
            i = names.index(41)
            others = [f for j, f in enumerate(factors) if j != i]
            assert factors[i] < 0.1 * min(others), (factors[i], others)
            assert not torch.equal(outs[0], before)
    assert torch.equal(outs[0], outs[1])

"""The persistent LoanNet trainer kernel (csrc/kernels/mlp.hip) called directly through
``ops.hip.mlp_train`` on the hand-built step tables of mlp_cases.py (GPU only): element-wise
against the fp64 oracle within ``32 E32 + 2^-24 max|p|`` per parameter tensor (update, momentum,
FoolsGold sums), counts and correct counts exact, and bit for bit run to run, split into two
launches, alone against in the group, and with the FoolsGold sums on and off."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mlp_cases as M
import step_kernel_cases as K

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in M.CASES]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dba_mod_amd.ops import hip
    return hip


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _same(a, b, what):
    K.same_bits({k: v for k, v in a.items() if k != "rc"}, {k: v for k, v in b.items() if k != "rc"}, what)


@pytest.mark.parametrize("name", NAMES)
def test_against_oracle(H, dev, name):
    a = M.run_kernel(H, name, dev)
    _same(a, M.run_kernel(H, name, dev), "run to run")
    M.check_oracle(name, a)


@pytest.mark.parametrize("name", NAMES)
def test_client_alone_and_in_the_group(H, dev, name):
    """A client's state, momentum, FoolsGold sums and statistics columns: the same bits with the
    client alone in the launch (G = 1) as at position 0 and at position 2 of the group."""
    ms = M.BY_NAME[name].max_slots
    grp = M.run_kernel(H, name, dev)
    for g in (0, 2):
        alone = M.run_kernel(H, name, dev, sel=g)
        K.same_bits(M.client_cols(grp, g, ms), M.client_cols(alone, 0, ms), f"client {g} alone vs in the group")
        M.check_oracle(name, alone, sel=g)


@pytest.mark.parametrize("name", M.SPLIT_CASES)
def test_two_launches(H, dev, name):
    """[0, T) in one launch == [0, k), [k, T) in two, k = 1 and T - 1: the 2-step client is
    inactive at the second segment's first step for k = T - 1 (the early return), and the first
    segment must not prefetch past its own end."""
    T = M.BY_NAME[name].T
    one = M.run_kernel(H, name, dev)
    for k in (1, T - 1):
        two = M.run_kernel(H, name, dev, segments=[(0, k), (k, T)])
        assert two["rc"] == [0, 0]
        _same(one, two, f"one launch vs split at {k}")


@pytest.mark.parametrize("name", ["full", "poison", "ragged"])
def test_fg_off_changes_no_parameter_bit(H, dev, name):
    on, off = M.run_kernel(H, name, dev), M.run_kernel(H, name, dev, fg=False)
    assert off["fg"] is None
    for k in ("state", "mom", "stats"):
        K.check_exact(off[k], on[k], "mlp_train", f"{k} without fg", "invariant")
    M.check_oracle(name, off)


def test_nan_feature_raises_the_flag(H, dev):
    """One source row with a NaN feature in client 1's second batch: the launch returns 0 and
    nan_flag counts it; the other clients' bits are those of the clean run."""
    tb = M.tables("full")
    tb["sched"] = tb["sched"].copy()
    tb["sched"][1, 1 * M.B + 3] = M.NAN_ROW
    out = M.run_kernel(H, "full", dev, tab=tb)
    assert out["rc"] == [0] and float(out["nan"]) >= 1.0
    clean = M.run_kernel(H, "full", dev)
    for g in (0, 2):
        K.same_bits(M.client_cols(out, g, 1), M.client_cols(clean, g, 1), f"client {g} beside the NaN client")


def test_refused_shapes_write_nothing(H, dev):
    """B = 32, a step table of another width and P > 6144: -100 and no byte written."""
    tb = M.tables("full")
    before = {k: torch.from_numpy(tb[k]) for k in ("state", "mom", "fg", "stats")}
    narrow = dict(tb, sched=np.ascontiguousarray(tb["sched"][:, :-1]))
    spec = M.get_spec("loan")
    big = SimpleNamespace(P=6144 + 64, by_name=spec.by_name)
    for kw in ({"Bk": 32}, {"tab": narrow}, {"spec": big}):
        out = M.run_kernel(H, "full", dev, **{"tab": tb, **kw})
        assert out["rc"] == [-100], kw
        for k, v in before.items():
            K.check_exact(out[k], v, "mlp_train refused", k, "invariant")
        assert float(out["nan"]) == 0.0


def test_zz_report_measured_errors(H, capsys):
    """Prints the kernel's largest error against the oracle, E32 and their ratio per tensor (shown
    with ``-s``)."""
    with capsys.disabled():
        print("\n" + M.report())

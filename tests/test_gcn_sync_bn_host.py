"""CPU tests of gcnx.GCN's sync-BN training over graph shards: the C ABI of the new entry points, the sharded float64 oracle
(tests/gcn_sync_bn_ref.py) against the whole-batch oracle, and which communicators the constructor accepts."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gcn_bn_ref as R
import gcn_sync_bn_ref as S
from test_gcn_bn_host import _graphs

NEW = ("gcnx_bn_act_pool_bwd_stats", "gcnx_bn_act_pool_bwd_apply", "gcnx_bce_head_phase_scratch_floats",
       "gcnx_bce_head_phase_red_floats", "gcnx_bce_head_phase")


def test_new_entry_points_are_declared_listed_and_exported():
    from gcnx import _lib
    header = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for name in NEW:
        assert re.search(r"GCNX_API\s+[\w\s\*]+\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name
    lib = _lib.load()
    assert lib.gcnx_version() >= 402


@pytest.mark.parametrize("b,h", [(1, 1), (7, 64), (50, 256)])
def test_phase_sizes_are_the_documented_ones(b, h):
    from gcnx import _lib, device as D
    lib = _lib.load()
    assert lib.gcnx_bce_head_phase_scratch_floats(b, h) == lib.gcnx_bce_head_scratch_floats(b, h) + 2 * h + 2
    assert lib.gcnx_bce_head_scratch_floats(b, h) == 2 * b * h + h * h + 2 * b
    assert lib.gcnx_bce_head_phase_red_floats(h) == 4 * h + 4
    # the slices the model all-reduces tile red exactly once
    cover = np.zeros(4 * h + 4, int)
    for k in range(7):
        sl = D.bce_head_phase_slice(k, h)
        if sl is not None:
            cover[sl[0]:sl[0] + sl[1]] += 1
    assert np.all(cover == 1)


def _cmp(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64).reshape(np.shape(got))
    assert float(np.max(np.abs(got - ref))) <= tol * max(1.0, float(np.max(np.abs(ref)))), what


@pytest.mark.parametrize("bounds", [[0, 8, 16], [0, 1, 9, 16], [0, 4, 5, 11, 16], [0, 15, 16]])
def test_sharded_oracle_equals_the_whole_batch(bounds):
    x, a, gp, y = _graphs(16, 16, seed=31)
    p = R.init_params(16, 24, seed=5)
    whole = R.model(x, a, gp, p, y)
    sh = S.model(x, a, gp, p, y, bounds)
    _cmp(sh["out"], whole["out"], 1e-12, "out")
    assert abs(sh["loss"] - whole["loss"]) <= 1e-12 * max(1.0, abs(whole["loss"])) and sh["hits"] == whole["hits"]
    assert np.array_equal(sh["argmax"], whole["argmax"])
    for k in R.KEYS:
        _cmp(sh["grads"][k], whole["grads"][k], 1e-12, k)
    # the parts really are partial: a shard's own gradient is not the whole batch's
    assert not np.allclose(sh["parts"][0]["grads"]["linear_1.weight"], whole["grads"]["linear_1.weight"])


def test_sharded_oracle_with_empty_graphs_and_kink_sides():
    import scipy.sparse as sp
    x, a, gp, y = _graphs(6, 8, seed=2)
    # insert two empty graphs (after graph 1 and at the end)
    gp = np.concatenate([gp[:2], [gp[1]], gp[2:], [gp[-1]]])
    y = np.concatenate([y[:1], [[1.0, 0.0]], y[1:], [[0.0, 1.0]]])
    p = R.init_params(8, 16, seed=1)
    whole = R.model(x, sp.csr_matrix(a), gp, p, y)
    masks = {k: whole[k] for k in ("m1", "m2", "m3", "m4")}
    sh = S.model(x, a, gp, p, y, [0, 2, 5, 8], masks=masks, argmax=whole["argmax"])
    _cmp(sh["out"], whole["out"], 1e-12, "out")
    for k in R.KEYS:
        _cmp(sh["grads"][k], whole["grads"][k], 1e-12, k)


def test_sharded_head_oracle_with_a_one_row_shard():
    rng = np.random.default_rng(3)
    p = R.init_params(8, 32, seed=2)
    P = rng.normal(size=(9, 32))
    lab = np.eye(2)[rng.integers(0, 2, 9)]
    whole = R.head(P, p, lab)
    parts = S.head([P[:1], P[1:5], P[5:]], p, [lab[:1], lab[1:5], lab[5:]])
    _cmp(np.concatenate([r["dP"] for r in parts]), whole["dP"], 1e-12, "dP")
    for k, v in whole["grads"].items():
        _cmp(sum(r["grads"][k] for r in parts), v, 1e-12, k)
    assert abs(sum(r["loss"] for r in parts) - whole["loss"]) < 1e-12


class _FakeComm:
    """Has the gcnx.comm.Communicator interface; never called (construction only)."""
    rank, world_size = 0, 2

    def allreduce_sum(self, arr, n=None):
        raise AssertionError("not called")

    def allreduce_host(self, values, op="max"):
        raise AssertionError("not called")


def test_gcn_constructor_accepts_a_communicator():
    from gcnx.models import GCN
    ctx = object()                    # never touched before the first batch
    m = GCN(ctx=ctx, hidden_channels=64, comm=_FakeComm())
    assert m.comm is not None and m._multi()
    with pytest.raises(NotImplementedError):
        GCN(ctx=ctx, hidden_channels=64, comm=object())
    with pytest.raises(NotImplementedError):
        GCN(ctx=ctx, num_classes=2, comm=_FakeComm())

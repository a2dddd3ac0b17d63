"""CPU tests of the TopKPool feature (gcnx.TopKPool, gcnx.TopKNet): the float64 oracle (tests/topk_ref.py) pinned against a
plain-torch autograd restatement and an adjoint identity, the k_g arithmetic, the tie rule, the C ABI of the new entry
points, and what the layer and the model promise without a device.  torch is imported inside the tests only."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import topk_ref as TR


def _batch(sizes=(9, 1, 14, 6), f=8, seed=0):
    rng = np.random.default_rng(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rng.standard_normal((int(gp[-1]), f)), gp, rng.standard_normal(f)


@pytest.mark.parametrize("sigmoid", [False, True])
def test_oracle_matches_torch_autograd(sigmoid):
    import torch
    x, gp, p = _batch()
    r = TR.pool_fwd(x, p, gp, 0.5, sigmoid)
    assert TR.threshold_gap(r["y"], gp, 0.5) > 1e-6
    dout = np.random.default_rng(1).standard_normal(r["out"].shape)
    dx, dp = TR.pool_bwd(x, p, r["y"], r["idx"], dout, sigmoid)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    yt = xt @ pt / pt.norm()
    idx = torch.tensor(r["idx"], dtype=torch.long)
    out = xt[idx] * (torch.sigmoid(yt[idx]) if sigmoid else torch.tanh(yt[idx]))[:, None]
    (out * torch.tensor(dout)).sum().backward()
    # the selection itself, restated with torch.topk per graph (scores are distinct here)
    want = torch.cat([gp[g] + torch.sort(torch.topk(yt[gp[g]:gp[g + 1]], int(TR.kept_counts(gp, 0.5)[g])).indices).values
                      for g in range(len(gp) - 1)])
    assert np.array_equal(want.numpy(), r["idx"])
    for got, ref in ((r["y"], yt.detach().numpy()), (r["out"], out.detach().numpy()), (dx, xt.grad.numpy()), (dp, pt.grad.numpy())):
        assert np.max(np.abs(got - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))
    assert (r["pos"] < 0).any() and not dx[r["pos"] < 0].any()


@pytest.mark.parametrize("sigmoid", [False, True])
def test_oracle_pool_pair_is_consistent(sigmoid):
    """pool_bwd is the adjoint of the forward's derivative at a fixed selection: <dout, J v> = <J^T dout, v> in x and in p,
    with J v taken by central differences."""
    x, gp, p = _batch(seed=3)
    r = TR.pool_fwd(x, p, gp, 0.5, sigmoid)
    rng = np.random.default_rng(4)
    dout, vx, vp = rng.standard_normal(r["out"].shape), rng.standard_normal(x.shape), rng.standard_normal(p.shape)
    dx, dp = TR.pool_bwd(x, p, r["y"], r["idx"], dout, sigmoid)
    h = 1e-6
    f = lambda xx, pp: TR.pool_fwd(xx, pp, gp, 0.5, sigmoid, idx=r["idx"])["out"]
    jx = (f(x + h * vx, p) - f(x - h * vx, p)) / (2 * h)
    jp = (f(x, p + h * vp) - f(x, p - h * vp)) / (2 * h)
    assert abs(np.sum(dout * jx) - np.sum(dx * vx)) <= 1e-7 * max(1.0, abs(np.sum(dx * vx)))
    assert abs(np.sum(dout * jp) - np.sum(dp * vp)) <= 1e-7 * max(1.0, abs(np.sum(dp * vp)))
    assert abs(dp @ p) <= 1e-12 * np.linalg.norm(dp) * np.linalg.norm(p) + 1e-14      # y does not depend on |p|


def test_kept_counts():
    from gcnx.device import topk_kept_ptr
    gp = np.concatenate([[0], np.cumsum([0, 1, 2, 3, 7])])
    want = {0.25: [0, 1, 1, 1, 2], 0.5: [0, 1, 1, 2, 4], 0.8: [0, 1, 2, 3, 6], 1.0: [0, 1, 2, 3, 7]}
    for ratio, k in want.items():
        assert TR.kept_counts(gp, ratio).tolist() == k, ratio
        assert np.diff(topk_kept_ptr(gp, ratio)).tolist() == k and topk_kept_ptr(gp, ratio).dtype == np.int32
    assert TR.kept_counts([0, 3], 1 / 3).tolist() == [1] and np.diff(topk_kept_ptr([0, 3], 1 / 3)).tolist() == [1]
    assert np.array_equal(TR.kept_ptr(gp, 0.5), topk_kept_ptr(gp, 0.5))


def test_oracle_tie_rule_and_negative_zero():
    gp = np.array([0, 5, 9])
    # all equal: the first k rows of every graph
    idx, pos, kp = TR.select(np.zeros(9), gp, 0.5)
    assert idx.tolist() == [0, 1, 2, 5, 6] and kp.tolist() == [0, 3, 5] and pos.tolist() == [0, 1, 2, -1, -1, 3, 4, -1, -1]
    # duplicates straddling the threshold: 2.0 twice above, then 1.0 three times of which one fits -> the lowest row
    idx, _, _ = TR.select(np.array([1.0, 2.0, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0]), gp, 0.5)
    assert idx.tolist() == [0, 1, 3, 5, 6]
    # -0.0 equals +0.0: the lower row wins whatever the sign
    y = np.array([-1.0, -0.0, 0.0, -2.0, -3.0, 0.0, -0.0, -1.0, -1.0])
    assert TR.select(y, gp, 0.2)[0].tolist() == [1, 5]
    y[[1, 2, 5, 6]] = [0.0, -0.0, -0.0, 0.0]
    assert TR.select(y, gp, 0.2)[0].tolist() == [1, 5]
    assert TR.threshold_gap(np.zeros(9), gp, 0.5) == 0.0 and TR.threshold_gap(np.arange(9.0), gp, 1.0) == np.inf
    # rows come back in row order, not in score order
    assert TR.select(np.array([1.0, 5.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0]), gp, 0.5)[0][:3].tolist() == [1, 2, 3]


def test_oracle_induce_is_scipy_slicing():
    import scipy.sparse as sp
    rng = np.random.default_rng(2)
    a = sp.random(30, 30, 0.2, format="csr", random_state=3)
    idx = np.sort(rng.choice(30, 17, replace=False))
    got, ref = TR.induce(a, idx), a[idx][:, idx].tocsr()
    ref.sort_indices()
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices) and np.array_equal(got.data, ref.data)


def test_abi_declares_and_exports_the_topk_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    names = ("gcnx_topk_select_ok", "gcnx_topk_select", "gcnx_topk_gather", "gcnx_topk_bwd", "gcnx_csr_induce")
    for nm in names:
        assert re.search(r"GCNX_API\s+int\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert hdr.count("gcn.py:10") >= len(names)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 405
    ok = lib.gcnx_topk_select_ok                             # answers without a context
    assert ok(8192, 16) == 1 and ok(1, 1) == 1 and ok(0, 64) == 1 and ok(16384, 128) == 1
    assert ok(16385, 16) == 0 and ok(2 ** 40, 16) == 0 and ok(-1, 16) == 0
    assert ok(8192, 0) == 0 and ok(8192, -4) == 0


def test_package_exports_and_constructor_refusals():
    import gcnx
    from gcnx.layers import TopKPool
    from gcnx.models import TopKNet, _GraphRunner
    assert "TopKPool" in gcnx.__all__ and "TopKNet" in gcnx.__all__
    assert gcnx.TopKPool is TopKPool and gcnx.TopKNet is TopKNet
    for bad in (0, 0.0, -0.5, 1.5, "half", None):
        with pytest.raises(ValueError):
            TopKPool(bad)
    with pytest.raises(NotImplementedError):
        TopKPool(0.5, kernel_initializer="he_normal")
    lay = TopKPool(1, seed=1)
    assert lay.ratio == 1.0 and not lay.sigmoid_gating and not lay.return_selection and not lay.return_score
    spec = TopKPool(0.5, sigmoid_gating=True, seed=1)._param_spec(64)
    assert [(n, s) for n, s, _ in spec] == [("kernel", (64, 1))] and np.max(np.abs(spec[0][2])) <= np.sqrt(6.0 / 65)
    assert str(inspect.signature(TopKPool.__init__)) == ("(self, ratio, return_selection=False, return_score=False, sigmoid_gating=False, "
                                                         "kernel_initializer='glorot_uniform', **kw)")
    assert "original relative order" in TopKPool.__doc__.replace("ORIGINAL", "original") and "lower row index" in TopKPool.__doc__.replace("LOWER", "lower")
    assert issubclass(TopKNet, _GraphRunner) and TopKNet.uses_edge_features is False
    with pytest.raises(NotImplementedError):
        TopKNet(ctx=None, comm=object())
    for prec in ("bf16", "bf16x3"):
        with pytest.raises(NotImplementedError):
            TopKNet(ctx=None, prec=prec)
    with pytest.raises(NotImplementedError):
        TopKNet(ctx=None, pool="max")
    with pytest.raises(ValueError):
        TopKNet(ctx=None, ratio=0.0)
    m = TopKNet(ctx=None, ratio=0.8, pool="avg", sigmoid_gating=True)
    assert m.use_graph is False and m.ratio == 0.8 and m.sigmoid_gating and m.hidden == 64 and m.n_labels == 2


_CALL = "(self, inputs, training=False)"
_EVAL = "(self, inputs, target)"
_STEP = "(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None)"
_GRADS = "(self, inputs, target=None, global_batch=None, _lr=None)"


def test_topknet_signatures_are_eccnets_without_the_edge_argument():
    from gcnx.models import ECCNet, TopKNet
    want = {"__call__": _CALL, "loss_and_grads": _GRADS, "train_step": _STEP, "fetch_metrics": "(self, n_graphs)", "evaluate_batch": _EVAL,
            "get_weights": "(self, as_dict=False)", "set_weights": "(self, weights)", "build": "(self, f_in)", "gradients": "(self)"}
    for name, sig in want.items():
        assert str(inspect.signature(getattr(TopKNet, name))) == sig, name
        if name != "build":
            assert str(inspect.signature(getattr(ECCNet, name))) == sig, name
    assert str(inspect.signature(TopKNet.__init__)).startswith("(self, ctx, n_labels=2, hidden=64, ratio=0.5, pool='sum', sigmoid_gating=False, seed=0")


class _View:
    def __init__(self, shape):
        self.shape = shape

    def copy_from_host(self, host, wait=True):
        assert host.shape == tuple(self.shape)


class _Buffer:
    def __init__(self, size):
        self.size, self.views = size, []

    def flat(self, off, n, shape=None):
        assert off + n <= self.size
        self.views.append((off, n, shape or (n,)))
        return _View(shape or (n,))


class _RecordingContext:
    """Stands in for gcnx.Context in build(): records zeros(n) and every flat(off, n, shape) of what it hands back
    (the pattern of tests/test_model_protocol_host.py)."""

    def __init__(self):
        self.buffers = []

    def zeros(self, n):
        self.buffers.append(_Buffer(n))
        return self.buffers[-1]


def test_topknet_flat_buffer_starts_every_tensor_on_four_floats():
    from gcnx.models import TopKNet
    ctx = _RecordingContext()
    m = TopKNet(ctx=ctx, n_labels=2, hidden=3, ratio=0.5)
    m.build(5)
    order = TopKNet.PARAM_ORDER
    assert order == TR.KEYS
    shapes = {"conv1_kernel": (5, 3), "conv1_bias": (3,), "pool_kernel": (3, 1), "conv2_kernel": (3, 3), "conv2_bias": (3,),
              "dense_kernel": (3, 2), "dense_bias": (2,)}
    # 15 -> 16, 3 -> 4, 9 -> 12, 6 -> 8, 2 -> 4 floats per tensor
    offsets = {"conv1_kernel": 0, "conv1_bias": 16, "pool_kernel": 20, "conv2_kernel": 24, "conv2_bias": 36, "dense_kernel": 40,
               "dense_bias": 48}
    n_params = 52
    assert [b.size for b in ctx.buffers] == [n_params, n_params + 2]
    assert m.flat_p is ctx.buffers[0] and m.flat_g is ctx.buffers[1] and m.n_params == n_params
    want = [(offsets[k], int(np.prod(shapes[k])), shapes[k]) for k in order]
    assert sorted(m.flat_p.views) == want
    assert sorted(m.flat_g.views) == want + [(n_params, 2, (2,))]
    assert set(m.p) == set(m.g) == set(order) and all(m.p[k].shape == shapes[k] == m.g[k].shape for k in order)
    assert all(o % 4 == 0 for o in offsets.values()) and m.loss_acc.shape == (2,)
    # the layers hold the same views
    assert m.conv1.params["kernel"] is m.p["conv1_kernel"] and m.topk.grads["kernel"] is m.g["pool_kernel"]
    assert m.conv2.params["bias"] is m.p["conv2_bias"] and m.conv1.in_dim == 5 and m.topk.in_dim == m.conv2.in_dim == 3


def test_oracle_model_gradients_match_torch_autograd():
    """The whole TopKNet step of the oracle against torch autograd at the oracle's selection (float64, 1e-10)."""
    import scipy.sparse as sp
    import torch
    rng = np.random.default_rng(5)
    sizes = [7, 12, 1, 9]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    blocks = []
    for s in sizes:
        mm = np.triu(rng.random((s, s)) < 0.4, 1)
        blocks.append(sp.csr_matrix((mm | mm.T | np.eye(s, dtype=bool)) * rng.uniform(0.2, 1.0, (s, s))))
    a = sp.block_diag(blocks, format="csr")
    x = rng.standard_normal((gp[-1], 6))
    yl = np.eye(2)[rng.integers(0, 2, len(sizes))]
    p = TR.init_params(6, 8, 2, seed=1)
    for pool, sigmoid in (("sum", False), ("avg", True)):
        r = TR.model(x, a, gp, p, 0.5, yl, pool=pool, sigmoid=sigmoid)
        assert r["gap"] > 1e-6
        t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
        at = torch.tensor(a.toarray())
        idx = torch.tensor(r["pool"]["idx"], dtype=torch.long)
        y1 = torch.relu(at @ (torch.tensor(x) @ t["conv1_kernel"]) + t["conv1_bias"])
        sc = (y1 @ t["pool_kernel"])[:, 0] / t["pool_kernel"].norm()
        x2 = y1[idx] * (torch.sigmoid(sc[idx]) if sigmoid else torch.tanh(sc[idx]))[:, None]
        y2 = torch.relu(at[idx][:, idx] @ (x2 @ t["conv2_kernel"]) + t["conv2_bias"])
        kp = r["pool"]["kept_ptr"]
        pooled = torch.stack([y2[kp[g]:kp[g + 1]].sum(0) if pool == "sum" else y2[kp[g]:kp[g + 1]].mean(0) for g in range(len(sizes))])
        logits = pooled @ t["dense_kernel"] + t["dense_bias"]
        loss = -(torch.tensor(yl) * torch.log_softmax(logits, 1)).sum() / len(sizes)
        loss.backward()
        assert abs(float(loss.detach()) - r["loss"]) <= 1e-10
        assert np.max(np.abs(torch.softmax(logits, 1).detach().numpy() - r["probs"])) <= 1e-10
        for k in TR.KEYS:
            ref = t[k].grad.numpy().reshape(np.shape(r["grads"][k]))
            assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), (pool, k)


def test_model_seed_table_holds_the_first_qualifying_seeds():
    """tests/test_gpu_topk.py hard-codes, per (ratio, pool), the first weight seed whose loss_and_grads and three SGD steps keep
    the oracle's threshold gap on the hidden scores >= 1e-4 max|y|: recomputed here, so that a change to synth or to
    init_params cannot leave the GPU test with a stale table."""
    import test_gpu_topk as G
    for (ratio, pool), seed in G.MODEL_SEED.items():
        gaps = [G._model_track(ratio, pool, s) for s in range(seed + 1)]
        assert gaps[-1] >= 1e-4 and all(g < 1e-4 for g in gaps[:-1]), (ratio, pool, gaps)

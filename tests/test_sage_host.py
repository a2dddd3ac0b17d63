"""CPU tests of the SAGEConv feature (gcnx.SAGEConv, gcnx.SAGE): the float64 oracle (tests/sage_ref.py) pinned against a
plain-torch autograd restatement, the C ABI of the new entry points, and what the model class promises without a device.
torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import sage_ref as SR


def _graphs(kind, n_graphs=16, f=16, seed=0):
    """One disjoint batch of random graphs of 8-64 nodes: x, scipy adjacency (row = target), graph_ptr, y.
    "symmetric": an undirected pattern, most rows with a stored self-loop.  "directed": a directed pattern without loops,
    one node without any stored entry in its row or its column, and one graph of a single (isolated) node."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    sizes = rng.integers(8, 65, n_graphs)
    if kind == "directed":
        sizes[3] = 1
    gp = np.concatenate([[0], np.cumsum(sizes)])
    blocks = []
    for s in sizes:
        m = np.triu(rng.random((s, s)) < 0.15, 1)
        m = m | (np.tril(rng.random((s, s)) < 0.15, -1) if kind == "directed" else m.T)
        if kind == "symmetric":
            m[np.diag_indices(s)] = rng.random(s) < 0.7
        elif s > 2:
            m[1, :] = False                                   # an isolated node inside a graph
            m[:, 1] = False
        blocks.append(sp.csr_matrix(m.astype(np.float64) * rng.uniform(0.5, 2.0, (s, s))))   # values are ignored
    a = sp.block_diag(blocks, format="csr")
    x = rng.normal(size=(gp[-1], f))
    y = np.eye(2)[rng.integers(0, 2, n_graphs)]
    return x, a, gp, y


def _torch_model(x, a, gp, y, p):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, a, gp, y, p)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, a, gp, y, p):
    """The model from torch.nn modules + a hand-written PyG SAGEConv(aggr="mean"): lin_l(mean of the sources' rows by
    index_add_ and a clamped count) + lin_r(x); scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.lin_l.bias"].shape[0]
    coo = a.tocoo()
    src, dst = torch.tensor(coo.col, dtype=torch.long), torch.tensor(coo.row, dtype=torch.long)   # row = target

    class Conv(torch.nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.lin_l = torch.nn.Linear(fi, fo, bias=True)
            self.lin_r = torch.nn.Linear(fi, fo, bias=False)

        def forward(self, xx):
            cnt = torch.zeros(n).index_add_(0, dst, torch.ones(dst.numel())).clamp(min=1)
            mean = torch.zeros(n, xx.shape[1]).index_add_(0, dst, xx[src]) / cnt[:, None]
            return F.linear(mean, self.lin_l.weight, self.lin_l.bias) + F.linear(xx, self.lin_r.weight)

    mods = {"conv1": Conv(f, h), "conv2": Conv(h, h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    assert set(named) == set(SR.KEYS)
    with torch.no_grad():
        for k, v in p.items():
            named[k].copy_(torch.tensor(v))
    batch = torch.tensor(np.repeat(np.arange(len(gp) - 1), np.diff(gp)), dtype=torch.long)
    t = net["prelu_1"](net["batch_norm_1"](net["conv1"](torch.tensor(x))))
    t = net["prelu_2"](net["batch_norm_2"](net["conv2"](t)))
    pooled = torch.full((len(gp) - 1, h), -torch.inf).scatter_reduce(0, batch[:, None].expand(-1, h), t, "amax", include_self=True)
    t = net["prelu_3"](net["batch_norm_3"](net["linear_1"](pooled)))
    out = net["prelu_4"](net["batch_norm_4"](net["linear_2"](t)))
    loss = F.binary_cross_entropy_with_logits(out[:, 0], torch.tensor(y[:, 1]))
    loss.backward()
    return out.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in net.named_parameters()}


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind):
    x, a, gp, y = _graphs(kind, seed=2 if kind == "directed" else 0)
    pat = a != 0
    if kind == "symmetric":
        assert (pat != pat.T).nnz == 0 and a.diagonal().any()
    else:
        deg_in, deg_out = np.diff(a.indptr), np.diff(a.tocsc().indptr)
        assert (pat != pat.T).nnz > 0 and not a.diagonal().any() and np.any((deg_in == 0) & (deg_out == 0)) and 1 in np.diff(gp)
    p = SR.init_params(16, 64, seed=3)
    out_t, loss_t, g_t = _torch_model(x, a, gp, y, p)
    r = SR.model(x, a, gp, p, y)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(SR.KEYS) == set(r["grads"])
    for k in SR.KEYS:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


def test_oracle_conv_pair_is_consistent():
    """sage_conv_bwd is the adjoint of sage_conv_fwd (with and without the root weight): <dz, J v> = <J^T dz, v>."""
    x, a, gp, _ = _graphs("directed", n_graphs=4, seed=5)
    rng = np.random.default_rng(0)
    A = SR.mean_operator(a, x.shape[0])
    wl, wr, b = rng.normal(size=(8, 16)), rng.normal(size=(8, 16)), rng.normal(size=8)
    for root in (wr, None):
        out, s = SR.sage_conv_fwd(A, x, wl, root, b)
        empty = np.diff(A.indptr) == 0
        assert empty.any() and not s[empty].any()
        dz, v = rng.normal(size=out.shape), rng.normal(size=x.shape)
        dx, dwl, dwr, db = SR.sage_conv_bwd(A, x, s, wl, root, dz)
        jv = SR.sage_conv_fwd(A, v, wl, root, None)[0]
        assert abs(np.sum(dz * jv) - np.sum(dx * v)) <= 1e-10 * abs(np.sum(dz * jv))
        assert np.allclose(dwl, dz.T @ (A @ x)) and np.allclose(db, dz.sum(0)) and (dwr is None) == (root is None)


def test_abi_declares_and_exports_the_sage_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    names = ("gcnx_sage_conv", "gcnx_sage_conv_ok")
    for nm in names:
        assert re.search(r"GCNX_API\s+int\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert "gcn_utills.py:804-806" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 404
    ok = lib.gcnx_sage_conv_ok                               # answers without a context
    assert ok(1000, 16, 64, 16) == 1 and ok(1000, 128, 128, 256) == 1 and ok(1000, 32, 16, 32) == 1
    assert ok(1000, 96, 64, 96) == 0 and ok(1000, 16, 256, 16) == 0 and ok(1000, 16, 64, 18) == 0
    assert ok(1000, 64, 64, 32) == 0 and ok(1000, 16, 24, 16) == 0 and ok(-1, 16, 64, 16) == 0
    assert ok(2 ** 26, 16, 64, 16) == 0 and ok(2 ** 26 - 8, 16, 64, 16) == 1     # n * ldx * 4 reaches 2^32 / stays below


def test_sage_constructor_refusals_keys_and_edge_features():
    from gcnx.models import GCN, SAGE
    with pytest.raises(NotImplementedError):
        SAGE(num_classes=2)
    with pytest.raises(NotImplementedError):
        SAGE(hidden_channels=64, comm=object())
    assert issubclass(SAGE, GCN) and SAGE.uses_edge_features is False
    keys = [k for k, _, _ in SAGE.TORCH_KEYS]
    assert keys == list(SR.KEYS)
    assert keys[:6] == ["conv1.lin_l.weight", "conv1.lin_l.bias", "conv1.lin_r.weight",
                        "conv2.lin_l.weight", "conv2.lin_l.bias", "conv2.lin_r.weight"]
    assert keys[6:] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
    assert {k: tr for k, _, tr in SAGE.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in SR.CONV_KEYS}
    assert sorted(k for _, k, _ in SAGE.TORCH_KEYS) == sorted(SAGE.PARAM_ORDER)


def test_package_exports_the_new_names():
    import gcnx
    assert "SAGEConv" in gcnx.__all__ and "SAGE" in gcnx.__all__
    from gcnx.layers import SAGEConv
    with pytest.raises(NotImplementedError):
        SAGEConv(64, activation="relu")
    lay = SAGEConv(64, root_weight=False, seed=1)
    assert [n for n, _, _ in lay._param_spec(16)] == ["lin_l.weight", "lin_l.bias"]
    spec = SAGEConv(64, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("lin_l.weight", (16, 64)), ("lin_l.bias", (64,)), ("lin_r.weight", (16, 64))]
    assert all(np.max(np.abs(v)) <= 0.25 for _, _, v in spec)          # U(+-1/sqrt(16))

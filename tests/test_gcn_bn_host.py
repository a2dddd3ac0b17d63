"""CPU tests of the torch-GCN feature (gcnx.GCN): the float64 oracle (tests/gcn_bn_ref.py) pinned against torch autograd,
the C ABI of the new entry points, and the NumPy binary_acc.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gcn_bn_ref as R


def _graphs(n_graphs=16, f=16, seed=0, self_loops=True, directed=False):
    """Random undirected (or directed) graphs of 8-64 nodes, as one disjoint batch: x, scipy adjacency (row = target),
    graph_ptr, y."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    sizes = rng.integers(8, 65, n_graphs)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    blocks = []
    for s in sizes:
        m = np.triu(rng.random((s, s)) < 0.15, 1)
        m = m | (np.tril(rng.random((s, s)) < 0.15, -1) if directed else m.T)
        if self_loops:
            m[np.diag_indices(s)] = rng.random(s) < 0.7        # some rows with a stored loop, some without
        blocks.append(sp.csr_matrix(m.astype(np.float64) * rng.uniform(0.5, 2.0, (s, s))))   # values are ignored
    a = sp.block_diag(blocks, format="csr")
    x = rng.normal(size=(gp[-1], f))
    lab = rng.integers(0, 2, n_graphs)
    y = np.eye(2)[lab]
    return x, a, gp, y


def _torch_model(x, a, gp, y, p):
    """The reference's torch GCN composed from torch.nn modules + a hand-written PyG GCNConv (add_remaining_self_loops,
    symmetric normalisation via index_add_), scatter_reduce("amax") for global_max_pool, BCEWithLogitsLoss."""
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, a, gp, y, p)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, a, gp, y, p):
    n, f = x.shape
    h = p["conv1.bias"].shape[0]
    coo = a.tocoo()
    src, dst = torch.tensor(coo.col, dtype=torch.long), torch.tensor(coo.row, dtype=torch.long)   # row = target

    class Conv(torch.nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(fo))
            self.lin = torch.nn.Linear(fi, fo, bias=False)

        def forward(self, xx):
            loop = torch.zeros(n, dtype=torch.bool)
            loop[src[src == dst]] = True
            miss = torch.nonzero(~loop).ravel()
            s, d = torch.cat([src, miss]), torch.cat([dst, miss])
            deg = torch.zeros(n).index_add_(0, d, torch.ones(d.numel()))
            dinv = deg.pow(-0.5)
            norm = dinv[s] * dinv[d]
            hh = self.lin(xx)
            return torch.zeros(n, hh.shape[1]).index_add_(0, d, norm[:, None] * hh[s]) + self.bias

    mods = {"conv1": Conv(f, h), "conv2": Conv(h, h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    with torch.no_grad():
        for k, v in p.items():
            dict(net.named_parameters())[k].copy_(torch.tensor(v))
    batch = torch.tensor(np.repeat(np.arange(len(gp) - 1), np.diff(gp)), dtype=torch.long)
    t = net["conv1"](torch.tensor(x))
    t = net["prelu_1"](net["batch_norm_1"](t))
    t = net["prelu_2"](net["batch_norm_2"](net["conv2"](t)))
    pooled = torch.full((len(gp) - 1, h), -torch.inf).scatter_reduce(0, batch[:, None].expand(-1, h), t, "amax", include_self=True)
    t = net["prelu_3"](net["batch_norm_3"](net["linear_1"](pooled)))
    out = net["prelu_4"](net["batch_norm_4"](net["linear_2"](t)))
    loss = torch.nn.BCEWithLogitsLoss()(out[:, 0], torch.tensor(y[:, 1]))
    loss.backward()
    return out.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in net.named_parameters()}


@pytest.mark.parametrize("self_loops", [True, False])
def test_oracle_matches_torch_autograd(self_loops):
    _check_oracle_against_torch(*_graphs(self_loops=self_loops))


@pytest.mark.parametrize("self_loops", [True, False])
def test_oracle_matches_torch_autograd_directed(self_loops):
    """A directed adjacency (as gcnx.GCN.forward's edge_index allows): A^ != A^T, so the oracle's backward must aggregate
    with the transpose, and PyG's degrees are in-degrees of the targets (the rows)."""
    x, a, gp, y = _graphs(self_loops=self_loops, directed=True, seed=1)
    pat = a != 0
    assert (pat != pat.T).nnz > 0
    _check_oracle_against_torch(x, a, gp, y)


def _check_oracle_against_torch(x, a, gp, y):
    p = R.init_params(16, 64, seed=3)
    out_t, loss_t, g_t = _torch_model(x, a, gp, y, p)
    r = R.model(x, a, gp, p, y)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(R.KEYS) == set(r["grads"])
    for k in R.KEYS:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    # accuracy: tags round(sigmoid(z)) against the labels, as binary_acc
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


def test_oracle_batchnorm_refuses_one_row():
    import torch
    bn = torch.nn.BatchNorm1d(4, track_running_stats=False, momentum=None)
    for training in (True, False):
        bn.train(training)
        with pytest.raises(ValueError):
            bn(torch.zeros(1, 4))
        with pytest.raises(ValueError):
            R.bn_fwd(np.zeros((1, 4)), np.ones(4), np.zeros(4))
    x, a, gp, y = _graphs(n_graphs=1)
    with pytest.raises(ValueError):
        R.model(x, a, gp, R.init_params(16), y)        # BN3 / BN4 see one row


def test_abi_declares_and_exports_the_torch_gcn_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    names = ("gcnx_bn_act_pool", "gcnx_bn_act_pool_bwd", "gcnx_bn_prelu_bce_head", "gcnx_bce_head_scratch_floats")
    for nm in names:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert re.search(r"GCNX_ACT_PRELU_SHARED\s*=\s*3", hdr) and _lib.ACT_PRELU_SHARED == 3
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gcnx_\w+)", out))
    assert set(names) <= exported
    lib = _lib.load()
    assert lib.gcnx_version() > 400
    assert lib.gcnx_bce_head_scratch_floats(50, 64) >= 2 * 50 * 64


def test_bce_head_args_mirror_matches_the_c_layout(tmp_path):
    import ctypes as C
    from gcnx import _lib
    fields = [f for f, _ in _lib.BceHeadArgs._fields_]
    body = '  printf("%zu", sizeof(gcnx_bce_head_args));\n' + "".join(
        f'  printf(" %zu", offsetof(gcnx_bce_head_args, {f}));\n' for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gcnx.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    size, *offs = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert int(size) == C.sizeof(_lib.BceHeadArgs)
    assert [int(o) for o in offs] == [getattr(_lib.BceHeadArgs, f).offset for f in fields]


def test_binary_acc_matches_the_reference_formula():
    import gcnx
    z = np.array([[-2.0], [0.0], [1e-3], [3.0], [-1e-3], [0.5]])
    y = np.array([[0.0], [0.0], [1.0], [0.0], [1.0], [1.0]])
    acc, tags, probas = gcnx.binary_acc(z, y)
    assert tags[1, 0] == 0.0                            # sigmoid(0) = 0.5 rounds to even: tag 0
    np.testing.assert_array_equal(tags.ravel(), [0, 0, 1, 1, 0, 1])
    np.testing.assert_allclose(probas, 1 / (1 + np.exp(-z)))
    assert acc == np.round(100 * 4 / 6)
    # against torch's own round / sigmoid
    import torch
    tt = torch.round(torch.sigmoid(torch.tensor(z)))
    np.testing.assert_array_equal(tt.numpy(), tags)


def test_gcn_constructor_refuses_what_it_does_not_implement():
    from gcnx.models import GCN
    with pytest.raises(NotImplementedError):
        GCN(num_classes=2)
    with pytest.raises(NotImplementedError):
        GCN(hidden_channels=64, comm=object())

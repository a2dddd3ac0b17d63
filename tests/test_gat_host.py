"""CPU tests of the GATConv feature (gcnx.GATConv, gcnx.GAT): the float64 oracle (tests/gat_ref.py) pinned against a
plain-torch autograd restatement and against its own Jacobian, the C ABI of the new entry points, and what the model and
layer classes promise without a device.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gat_ref as GR


def _graphs(kind, n_graphs=16, f=16, seed=0):
    """One disjoint batch of random graphs of 8-64 nodes: x, scipy adjacency (row = target), graph_ptr, y (the batches of
    test_sage_host).  "symmetric": an undirected pattern, most rows with a stored self-loop.  "directed": a directed pattern
    without loops, one node without any stored entry in its row or its column, and one graph of a single (isolated) node."""
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


def _torch_model(x, a, gp, y, p, heads):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, a, gp, y, p, heads)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, a, gp, y, p, heads):
    """The model from torch.nn modules + a hand-written PyG GATConv(heads, concat=True, negative_slope=0.2) on the pattern
    with remaining self-loops: the softmax over a target's entries from scatter_reduce("amax") and index_add_;
    scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.bias"].shape[0]
    c = h // heads
    rp, ci = GR.pattern(a, n)
    src = torch.tensor(ci, dtype=torch.long)                                                   # row = target
    dst = torch.tensor(np.repeat(np.arange(n), np.diff(rp)), dtype=torch.long)

    class Conv(torch.nn.Module):
        def __init__(self, fi):
            super().__init__()
            self.att_src = torch.nn.Parameter(torch.zeros(1, heads, c))
            self.att_dst = torch.nn.Parameter(torch.zeros(1, heads, c))
            self.bias = torch.nn.Parameter(torch.zeros(h))
            self.lin = torch.nn.Linear(fi, h, bias=False)

        def forward(self, xx):
            hf = self.lin(xx).view(n, heads, c)
            a_s, a_d = (hf * self.att_src).sum(-1), (hf * self.att_dst).sum(-1)
            e = F.leaky_relu(a_s[src] + a_d[dst], 0.2)
            m = torch.full((n, heads), -torch.inf).scatter_reduce(0, dst[:, None].expand(-1, heads), e.detach(), "amax", include_self=True)
            w = torch.exp(e - m[dst])
            alpha = w / torch.zeros(n, heads).index_add_(0, dst, w)[dst]
            out = torch.zeros(n, heads, c).index_add_(0, dst, alpha[:, :, None] * hf[src])
            return out.reshape(n, h) + self.bias

    mods = {"conv1": Conv(f), "conv2": Conv(h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    assert set(named) == set(GR.KEYS)
    assert [k for k in named if k.startswith("conv")] == list(GR.CONV_KEYS)            # att_src, att_dst, bias, lin.weight
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


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind, heads):
    x, a, gp, y = _graphs(kind, seed=2 if kind == "directed" else 0)
    pat = a != 0
    if kind == "symmetric":
        assert (pat != pat.T).nnz == 0 and a.diagonal().any()
    else:
        deg_in, deg_out = np.diff(a.indptr), np.diff(a.tocsc().indptr)
        assert (pat != pat.T).nnz > 0 and not a.diagonal().any() and np.any((deg_in == 0) & (deg_out == 0)) and 1 in np.diff(gp)
    p = GR.init_params(16, 64, heads, seed=3)
    assert p["conv1.att_src"].shape == (1, heads, 64 // heads) and p["conv1.lin.weight"].shape == (64, 16)
    out_t, loss_t, g_t = _torch_model(x, a, gp, y, p, heads)
    r = GR.model(x, a, gp, p, y, heads=heads)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(GR.KEYS) == set(r["grads"])
    for k in GR.KEYS:
        assert r["grads"][k].shape == g_t[k].shape or r["grads"][k].size == g_t[k].size, k
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


@pytest.mark.parametrize("heads", [1, 4])
def test_oracle_conv_pair_is_consistent(heads):
    """gat_conv_bwd is the adjoint of the Jacobian of gat_conv_fwd: <dz, J v> = <J^T dz, v>, J v by a central difference in
    float64 (step 1e-6, on the base point's side of every score), agreement 1e-6 relative.  The pattern has an empty row,
    which must give out = bias exactly."""
    x, a, gp, _ = _graphs("directed", n_graphs=4, seed=5)
    rp, ci = GR.pattern(a, x.shape[0], loops=False)
    empty = np.diff(rp) == 0
    assert empty.any()
    rng = np.random.default_rng(heads)
    c = 8
    base = [x, rng.normal(size=(16, heads * c)) / 4, rng.normal(size=(heads, c)) / np.sqrt(c), rng.normal(size=(heads, c)) / np.sqrt(c),
            rng.normal(size=heads * c)]
    out, cache = GR.gat_conv_fwd(rp, ci, *base)
    assert np.array_equal(out[empty], np.broadcast_to(base[4], out[empty].shape))
    assert np.allclose(np.add.reduceat(cache["alpha"], rp[:-1][~empty]), 1.0, rtol=0, atol=1e-12)    # every row's softmax sums to 1
    sides = cache["pos"]
    dz = rng.normal(size=out.shape)
    grads = GR.gat_conv_bwd(cache, dz)
    v = [rng.normal(size=t.shape) for t in base]
    step = 1e-6
    plus = GR.gat_conv_fwd(rp, ci, *[t + step * d for t, d in zip(base, v)], sides=sides)[0]
    minus = GR.gat_conv_fwd(rp, ci, *[t - step * d for t, d in zip(base, v)], sides=sides)[0]
    lhs = np.sum(dz * (plus - minus) / (2 * step))
    rhs = sum(np.sum(g * d) for g, d in zip(grads, v))
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), (lhs, rhs)
    # and one operand at a time (a cancellation between two wrong gradients would pass the sum)
    for i in range(5):
        vi = [d if j == i else np.zeros_like(d) for j, d in enumerate(v)]
        plus = GR.gat_conv_fwd(rp, ci, *[t + step * d for t, d in zip(base, vi)], sides=sides)[0]
        minus = GR.gat_conv_fwd(rp, ci, *[t - step * d for t, d in zip(base, vi)], sides=sides)[0]
        lhs, rhs = np.sum(dz * (plus - minus) / (2 * step)), np.sum(grads[i] * v[i])
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (i, lhs, rhs)


def test_device_score_sides_is_the_float32_comparison():
    a_src = np.array([[1e-8], [-1.0], [1.0]], np.float32)
    a_dst = np.array([[1.0], [1.0], [-1.0]], np.float32)
    rp, ci = np.array([0, 2, 3, 5]), np.array([0, 1, 1, 0, 2])
    # row 0: 1e-8 + 1 (> 0), -1 + 1 (= 0: not positive); row 1: -1 + 1; row 2: 1e-8 - 1 (< 0), 1 - 1
    assert GR.device_score_sides(a_src, a_dst, rp, ci).ravel().tolist() == [True, False, False, False, False]
    assert GR.device_score_sides(a_src.astype(np.float64), a_dst, rp, ci).shape == (5, 1)      # float64 input is narrowed first


NAMES = ("gcnx_gat_conv_ok", "gcnx_gat_scores", "gcnx_gat_aggregate", "gcnx_gat_bwd_edges", "gcnx_gat_bwd_nodes",
         "gcnx_gat_bwd_scratch_floats")


def test_abi_declares_and_exports_the_gat_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert "gcn_utills.py:804-806" in hdr
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 406
    assert lib.gcnx_gat_bwd_scratch_floats(1659, 4, 16) >= 2 * 64 * -(-1659 // 32)


def test_gat_conv_ok_truth_table():
    from gcnx import _lib
    ok = _lib.load().gcnx_gat_conv_ok                        # answers without a context
    for n, heads, c, ld in ((1000, 1, 64, 64), (1000, 4, 16, 64), (1000, 8, 16, 128), (1000, 8, 4, 32), (1000, 2, 8, 16),
                            (1000, 1, 16, 32)):
        assert ok(n, heads, c, ld) == 1, (n, heads, c, ld)
    for n, heads, c, ld in ((1000, 3, 16, 48),               # heads 3
                            (1000, 4, 24, 96), (1000, 1, 96, 96),      # HC 96
                            (1000, 8, 32, 256), (1000, 1, 256, 256),   # HC 256
                            (1000, 8, 2, 16),                # c 2
                            (1000, 1, 16, 18),               # ld % 4
                            (1000, 1, 64, 32),               # ld < HC
                            (-1, 1, 64, 64)):
        assert ok(n, heads, c, ld) == 0, (n, heads, c, ld)
    assert ok(2 ** 26, 1, 16, 16) == 0 and ok(2 ** 26 - 8, 1, 16, 16) == 1       # n * ld * 4 reaches 2^32 / stays below


def test_gat_constructor_refusals_and_keys():
    from gcnx.models import GAT, GCN
    with pytest.raises(NotImplementedError):
        GAT(num_classes=2)
    with pytest.raises(NotImplementedError):
        GAT(hidden_channels=64, comm=object())
    for kw in (dict(hidden_channels=96), dict(hidden_channels=256), dict(hidden_channels=64, heads=3)):
        with pytest.raises(NotImplementedError):
            GAT(**kw)
    assert issubclass(GAT, GCN) and GAT.uses_edge_features is False
    keys = [k for k, _, _ in GAT.TORCH_KEYS]
    assert keys == list(GR.KEYS)
    assert keys[:8] == [f"conv{k}.{t}" for k in (1, 2) for t in ("att_src", "att_dst", "bias", "lin.weight")]
    assert keys[8:] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
    assert GAT.PROBE_KEY == "conv1.lin.weight"
    assert {k: tr for k, _, tr in GAT.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in GR.CONV_KEYS}
    assert sorted(k for _, k, _ in GAT.TORCH_KEYS) == sorted(GAT.PARAM_ORDER)
    assert list(GAT.PARAM_ORDER[:8]) == [k for _, k, _ in GAT.TORCH_KEYS[:8]]
    for phrase in ("confirm", "named dicts", "duplicate"):      # the caveats GCN's docstring states, and the deviation
        assert phrase in GAT.__doc__


def test_package_exports_the_new_names_and_the_layer_refuses_what_is_missing():
    import gcnx
    assert "GATConv" in gcnx.__all__ and "GAT" in gcnx.__all__
    from gcnx.layers import GATConv
    for kw, word in ((dict(concat=False), "concat"), (dict(dropout=0.5), "dropout"), (dict(activation="relu"), "activation"),
                     (dict(edge_dim=3), "edge")):
        with pytest.raises(NotImplementedError) as e:
            GATConv(16, heads=4, **kw)
        assert word in str(e.value)
    spec = GATConv(16, heads=4, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("att_src", (4, 16)), ("att_dst", (4, 16)), ("bias", (64,)), ("lin.weight", (16, 64))]
    assert not spec[2][2].any()                                                               # the bias starts at zero
    assert np.max(np.abs(spec[0][2])) <= np.sqrt(6 / 20) and np.max(np.abs(spec[3][2])) <= np.sqrt(6 / 80)   # glorot-uniform
    assert [n for n, _, _ in GATConv(16, use_bias=False, seed=1)._param_spec(16)] == ["att_src", "att_dst", "lin.weight"]

"""CPU tests of the TransformerConv feature (gcnx.TransformerConv, gcnx.Transformer): the float64 oracle
(tests/transformer_ref.py) pinned against a plain-torch autograd restatement of PyG's message() / forward() and against its own
Jacobian, the two properties of dot-product attention the kernels lean on, the C ABI of the new entry points, and what the model
and layer classes promise without a device.  torch is imported inside the tests only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import transformer_ref as TR
from test_gat_host import _graphs

# heads x edge_dim x (beta, root_weight); beta only with the root connection
OPTIONS = [(False, True), (True, True), (False, False)]


def _edge_features(nnz, d, seed):
    return np.random.default_rng(seed).normal(size=(nnz, d)) if d else None


def _torch_model(x, rp, ci, e, gp, y, p, heads, beta, root):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, rp, ci, e, gp, y, p, heads, beta, root)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, rp, ci, e, gp, y, p, heads, beta, root):
    """The model from torch.nn modules + a hand-written PyG TransformerConv(heads, concat=True, beta, dropout=0, edge_dim,
    bias=True, root_weight) on the stored pattern, statement by statement its forward() / message(): separate Linears, the
    softmax over a target's entries from scatter_reduce("amax") and index_add_; scatter_reduce("amax") for global_max_pool;
    BCEWithLogitsLoss."""
    import math
    F = torch.nn.functional
    n, f = x.shape
    h = p["batch_norm_1.weight"].shape[0]
    c = h // heads
    src = torch.tensor(ci, dtype=torch.long)                                                   # row = target
    dst = torch.tensor(np.repeat(np.arange(n), np.diff(rp)), dtype=torch.long)
    et = None if e is None else torch.tensor(e)

    class Conv(torch.nn.Module):
        def __init__(self, fi):
            super().__init__()
            self.lin_key = torch.nn.Linear(fi, h)
            self.lin_query = torch.nn.Linear(fi, h)
            self.lin_value = torch.nn.Linear(fi, h)
            if et is not None:
                self.lin_edge = torch.nn.Linear(et.shape[1], h, bias=False)
            if root:
                self.lin_skip = torch.nn.Linear(fi, h)
                if beta:
                    self.lin_beta = torch.nn.Linear(3 * h, 1, bias=False)

        def forward(self, xx):
            query = self.lin_query(xx).view(-1, heads, c)
            key = self.lin_key(xx).view(-1, heads, c)
            value = self.lin_value(xx).view(-1, heads, c)
            # message(query_i, key_j, value_j, edge_attr, index)
            query_i, key_j, value_j = query[dst], key[src], value[src]
            if et is not None:
                edge_attr = self.lin_edge(et).view(-1, heads, c)
                key_j = key_j + edge_attr
            alpha = (query_i * key_j).sum(dim=-1) / math.sqrt(c)
            m = torch.full((n, heads), -torch.inf).scatter_reduce(0, dst[:, None].expand(-1, heads), alpha.detach(), "amax",
                                                                  include_self=True)
            w = torch.exp(alpha - m[dst])
            alpha = w / torch.zeros(n, heads).index_add_(0, dst, w)[dst]
            out = value_j
            if et is not None:
                out = out + edge_attr
            out = out * alpha.view(-1, heads, 1)
            out = torch.zeros(n, heads, c).index_add_(0, dst, out).view(-1, heads * c)         # aggr = add, concat
            if root:
                x_r = self.lin_skip(xx)
                if beta:
                    b = self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)).sigmoid()
                    out = b * x_r + (1 - b) * out
                else:
                    out = out + x_r
            return out

    mods = {"conv1": Conv(f), "conv2": Conv(h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    want = TR.keys(None if e is None else e.shape[1], beta, root)
    assert set(named) == set(want)
    assert [k for k in named if k.startswith("conv")] == [k for k in want if k.startswith("conv")]    # key, query, value, edge, skip, beta
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


@pytest.mark.parametrize("beta,root", OPTIONS)
@pytest.mark.parametrize("edge_dim", [0, 2])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind, heads, edge_dim, beta, root):
    x, a, gp, y = _graphs(kind, seed=2 if kind == "directed" else 0)
    pat = a != 0
    if kind == "symmetric":
        assert (pat != pat.T).nnz == 0 and a.diagonal().any()
    else:
        assert (pat != pat.T).nnz > 0 and (np.diff(a.indptr) == 0).any()                      # rows without entries: O = 0
    rp, ci, _ = TR.stored_pattern(a)
    e = _edge_features(len(ci), edge_dim, 11)
    p = TR.init_params(16, 64, edge_dim or None, beta, root, seed=3)
    assert p["conv1.lin_key.weight"].shape == (64, 16) and p["conv2.lin_query.bias"].shape == (64,)
    assert ("conv2.lin_edge.weight" in p) == bool(edge_dim) and ("conv1.lin_beta.weight" in p) == beta and ("conv1.lin_skip.bias" in p) == root
    out_t, loss_t, g_t = _torch_model(x, rp, ci, e, gp, y, p, heads, beta, root)
    r = TR.model(x, rp, ci, e, gp, p, heads=heads, y=y)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(TR.keys(edge_dim or None, beta, root)) == set(r["grads"])
    for k in g_t:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


@pytest.mark.parametrize("beta,root", OPTIONS)
@pytest.mark.parametrize("edge_dim", [0, 2])
@pytest.mark.parametrize("heads", [1, 4])
def test_oracle_conv_pair_is_consistent(heads, edge_dim, beta, root):
    """conv_bwd is the adjoint of the Jacobian of conv_fwd: <dz, J v> = <J^T dz, v>, J v by a central difference in float64
    (step 1e-6), agreement 1e-6 relative.  Softmax, dot and sigmoid are smooth: no side to pin.  The pattern has an empty row,
    which must give O = 0 exactly."""
    x, a, _, _ = _graphs("directed", n_graphs=4, seed=5)
    rp, ci, _ = TR.stored_pattern(a)
    empty = np.diff(rp) == 0
    assert empty.any()
    rng = np.random.default_rng(heads + 10 * edge_dim + 100 * beta + 1000 * root)
    c, step = 8, 1e-6
    hc, n = heads * c, x.shape[0]
    e = _edge_features(len(ci), edge_dim, 13)
    names = ["P"] + (["We"] if edge_dim else []) + (["w_beta"] if beta else [])
    base = [rng.normal(size=(n, (4 if root else 3) * hc))] + ([rng.normal(size=(edge_dim, hc)) / 2] if edge_dim else []) + \
        ([rng.normal(size=3 * hc) / np.sqrt(hc)] if beta else [])

    def fwd(ops):
        ops = dict(zip(names, ops))
        P = ops["P"]
        return TR.conv_fwd(rp, ci, P, heads, c, e, ops.get("We"), P[:, 3 * hc:] if root else None, ops.get("w_beta"))

    out, cache = fwd(base)
    assert np.array_equal(cache["O"][empty], np.zeros_like(cache["O"][empty]))
    assert np.allclose(np.add.reduceat(cache["alpha"], rp[:-1][~empty]), 1.0, rtol=0, atol=1e-12)    # every row's softmax sums to 1
    dz = rng.normal(size=out.shape)
    r = TR.conv_bwd(cache, dz)
    grads = {"P": np.hstack([r["dQ"], r["dK"], r["dV"]] + ([r["dS"]] if root else [])), "We": r["dWe"], "w_beta": r["dw_beta"]}
    v = [rng.normal(size=t.shape) for t in base]

    def directional(vs):
        (plus, _), (minus, _) = fwd([t + step * d for t, d in zip(base, vs)]), fwd([t - step * d for t, d in zip(base, vs)])
        return np.sum(dz * (plus - minus) / (2 * step))

    lhs, rhs = directional(v), sum(np.sum(grads[k] * d) for k, d in zip(names, v))
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), (lhs, rhs)
    # and one operand at a time, the blocks of P separately (a cancellation between two wrong gradients would pass the sum)
    for i, k in enumerate(names):
        lhs, rhs = directional([d if j == i else np.zeros_like(d) for j, d in enumerate(v)]), np.sum(grads[k] * v[i])
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)
    for blk in range(4 if root else 3):
        vb = np.zeros_like(v[0])
        vb[:, blk * hc:(blk + 1) * hc] = v[0][:, blk * hc:(blk + 1) * hc]
        lhs, rhs = directional([vb] + [np.zeros_like(d) for d in v[1:]]), np.sum(grads["P"] * vb)
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (blk, lhs, rhs)


@pytest.mark.parametrize("edge_dim", [0, 2])
def test_a_common_key_shift_changes_nothing_and_the_key_bias_has_no_gradient(edge_dim):
    """Adding one vector to every row of K moves every score of a row by the same amount: out is unchanged (1e-12) and the
    column sums of dK -- the gradient of lin_key.bias -- vanish."""
    x, a, _, _ = _graphs("directed", n_graphs=4, seed=6)
    rp, ci, _ = TR.stored_pattern(a)
    heads, c = 4, 8
    hc, n = heads * c, x.shape[0]
    rng = np.random.default_rng(7 + edge_dim)
    P = rng.normal(size=(n, 4 * hc))
    e = _edge_features(len(ci), edge_dim, 17)
    We = rng.normal(size=(edge_dim, hc)) / 2 if edge_dim else None
    wb = rng.normal(size=3 * hc) / np.sqrt(hc)
    out, cache = TR.conv_fwd(rp, ci, P, heads, c, e, We, P[:, 3 * hc:], wb)
    P2 = P.copy()
    P2[:, hc:2 * hc] += 3.0 * rng.normal(size=hc)
    out2, _ = TR.conv_fwd(rp, ci, P2, heads, c, e, We, P2[:, 3 * hc:], wb)
    assert np.max(np.abs(out2 - out)) <= 1e-12 * max(1.0, np.max(np.abs(out)))
    r = TR.conv_bwd(cache, rng.normal(size=out.shape))
    assert np.max(np.abs(r["dK"].sum(0))) <= 1e-12 * np.max(np.abs(r["dK"]))
    assert np.max(np.abs(r["dK"])) > 1e-3                                                    # (the rows themselves are not zero)


@pytest.mark.parametrize("edge_dim", [0, 2])
def test_zero_queries_average_the_values(edge_dim):
    """Q = 0: every score is 0, alpha = 1 / degree, O[i] = the mean of v_ij over the row."""
    x, a, _, _ = _graphs("directed", n_graphs=4, seed=6)
    rp, ci, _ = TR.stored_pattern(a)
    heads, c = 2, 8
    hc, n = heads * c, x.shape[0]
    rng = np.random.default_rng(9 + edge_dim)
    P = rng.normal(size=(n, 3 * hc))
    P[:, :hc] = 0.0
    e = _edge_features(len(ci), edge_dim, 19)
    We = rng.normal(size=(edge_dim, hc)) / 2 if edge_dim else None
    out, cache = TR.conv_fwd(rp, ci, P, heads, c, e, We)
    v = P[ci, 2 * hc:] + (e @ We if edge_dim else 0.0)
    deg = np.diff(rp)
    want = np.zeros((n, hc))
    np.add.at(want, np.repeat(np.arange(n), deg), v)
    want[deg > 0] /= deg[deg > 0, None]
    assert np.max(np.abs(out - want)) <= 1e-12 * np.max(np.abs(want))
    assert np.array_equal(cache["alpha"], np.repeat(1.0 / deg[deg > 0], deg[deg > 0])[:, None] * np.ones((1, heads)))


def test_oracle_sigmoid_stays_finite():
    g = TR.sigmoid(np.array([-800.0, -200.0, 0.0, 200.0, 800.0]))
    assert np.isfinite(g).all() and g[0] == 0.0 and g[2] == 0.5 and g[4] == 1.0 and np.isfinite(g * (1 - g)).all()


ERR_INVALID = 1                       # GCNX_ERR_INVALID (include/gcnx.h)
NAMES = ("gcnx_transformer_conv_ok", "gcnx_transformer_aggregate", "gcnx_transformer_bwd_scratch_floats", "gcnx_transformer_beta_bwd",
         "gcnx_transformer_bwd_targets", "gcnx_transformer_bwd_sources")


def test_abi_declares_and_exports_the_transformer_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+int\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert hdr.count("gcn.py:71") >= 6
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    assert _lib.load().gcnx_version() >= 420


def test_bwd_scratch_floats_answers_without_a_device():
    from gcnx import _lib
    fn = _lib.load().gcnx_transformer_bwd_scratch_floats
    out = ctypes.c_int64(-1)
    tiles = -(-1659 // 32)
    assert fn(1659, 4, 16, 2, 0, ctypes.byref(out)) == _lib.OK and out.value >= 2 * 64 * tiles        # dw_e: edge_dim HC per workgroup
    assert fn(1659, 4, 16, 0, 1, ctypes.byref(out)) == _lib.OK and out.value >= 3 * 64 * tiles        # dw_beta: 3 HC per workgroup
    assert fn(1659, 4, 16, 8, 1, ctypes.byref(out)) == _lib.OK and out.value >= 8 * 64 * tiles
    assert fn(1659, 1, 128, 2, 0, ctypes.byref(out)) == _lib.OK and out.value >= 2 * 128 * -(-1659 // 16)   # 16 rows per workgroup
    assert fn(1659, 4, 16, 0, 0, ctypes.byref(out)) == _lib.OK and out.value == 0                    # nothing to reduce
    assert fn(0, 4, 16, 2, 1, ctypes.byref(out)) == _lib.OK and out.value == 0
    out.value = -7
    for args in ((10, 0, 16, 2, 0), (10, 4, 0, 2, 0), (10, -4, 16, 2, 0), (-1, 4, 16, 2, 0), (10, 4, 16, -1, 1)):
        assert fn(*args, ctypes.byref(out)) == ERR_INVALID and out.value == -7, args
    assert fn(10, 4, 16, 2, 1, None) == ERR_INVALID


def test_calls_without_a_context_are_invalid():
    from gcnx import _lib
    lib = _lib.load()
    for nm in NAMES:
        if nm.endswith("conv_ok") or nm.endswith("scratch_floats"):
            continue
        args = [None if t is ctypes.c_void_p else 0 for t in _lib.SIGNATURES[nm]]
        assert getattr(lib, nm)(*args) == ERR_INVALID, nm


def test_transformer_conv_ok_truth_table():
    from gcnx import _lib
    ok = _lib.load().gcnx_transformer_conv_ok                # answers without a context
    for n, heads, c, ld, d in ((1000, 1, 64, 192, 0), (1000, 4, 16, 256, 2), (1000, 8, 16, 512, 8), (1000, 8, 4, 96, 1), (1000, 2, 8, 48, 0),
                               (1000, 1, 16, 52, 2), (1000, 1, 128, 384, 0), (0, 1, 16, 48, 0)):
        assert ok(n, heads, c, ld, d) == 1, (n, heads, c, ld, d)
    for n, heads, c, ld, d in ((1000, 4, 16, 256, 9), (1000, 4, 16, 256, -1),   # edge_dim 9, negative
                               (1000, 3, 16, 192, 0),            # heads 3
                               (1000, 16, 4, 256, 0),            # heads 16
                               (1000, 4, 24, 384, 0), (1000, 1, 96, 384, 0),      # HC 96
                               (1000, 8, 32, 1024, 0), (1000, 1, 256, 1024, 0),   # HC 256
                               (1000, 8, 2, 64, 0),              # c 2
                               (1000, 1, 64, 128, 0), (1000, 1, 64, 188, 0),      # ldp < 3 HC
                               (1000, 1, 16, 50, 0),             # ldp % 4
                               (-1, 1, 64, 256, 0)):
        assert ok(n, heads, c, ld, d) == 0, (n, heads, c, ld, d)
    assert ok(2 ** 24, 1, 16, 64, 0) == 0 and ok(2 ** 24 - 8, 1, 16, 64, 0) == 1      # n * ldp * 4 reaches 2^32 / stays below


def _model_options():
    return [dict(edge_dim=d, beta=b, root_weight=r) for d in (None, 2) for b, r in OPTIONS]


def test_transformer_constructor_refusals_and_keys():
    from gcnx.models import GATv2, GCN, Transformer
    with pytest.raises(NotImplementedError):
        Transformer(num_classes=2)
    with pytest.raises(NotImplementedError):
        Transformer(hidden_channels=64, comm=object())
    for kw in (dict(hidden_channels=96), dict(hidden_channels=256), dict(hidden_channels=64, heads=3), dict(hidden_channels=16, heads=8),
               dict(edge_dim=9), dict(edge_dim=0), dict(beta=True, root_weight=False)):
        with pytest.raises(NotImplementedError):
            Transformer(**kw)
    assert issubclass(Transformer, GCN) and not issubclass(Transformer, GATv2)
    nodev = object()                                            # stands in for the context: nothing here touches a device
    assert Transformer(ctx=nodev, edge_dim=2).uses_edge_features is True and Transformer(ctx=nodev).uses_edge_features is False
    for opt in _model_options():
        m = Transformer(ctx=nodev, hidden_channels=64, heads=4, **opt)
        d, beta, root = opt["edge_dim"], opt["beta"], opt["root_weight"]
        keys = [k for k, _, _ in m.TORCH_KEYS]
        assert keys == list(TR.keys(d, beta, root)), opt
        parts = TR.conv_keys(d, beta, root)
        assert keys[:2 * len(parts)] == [f"conv{k}.{t}" for k in (1, 2) for t in parts]
        assert keys[2 * len(parts):] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
        assert ("conv1.lin_edge.weight" in keys) == bool(d) and ("conv2.lin_beta.weight" in keys) == beta and ("conv2.lin_skip.bias" in keys) == root
        assert {k: tr for k, _, tr in m.TORCH_KEYS if k.startswith("conv")} == \
            {k: k.endswith("weight") and "lin_beta" not in k for k in keys if k.startswith("conv")}
        assert m.PROBE_KEY == "conv1.lin_key.weight"
        # one stacked weight and one stacked bias per convolution
        assert [k for k in m.PARAM_ORDER if k.endswith("1")][:2] == ["w1", "lb1"]
        assert ("we1" in m.PARAM_ORDER) == bool(d) and ("wb2" in m.PARAM_ORDER) == beta
        s, w = m._shapes(16), (256 if root else 192)
        assert s["w1"] == (16, w) and s["w2"] == (64, w) and s["lb1"] == (w,) and s["we2"][1] == 64 and s["wb1"] == (192,)
    for phrase in ("named dicts", "add_self_loops", "lin_key.bias"):
        assert phrase in Transformer.__doc__


def test_package_exports_the_new_names_and_the_layer_refuses_what_is_missing():
    import gcnx
    assert "TransformerConv" in gcnx.__all__ and "Transformer" in gcnx.__all__
    assert gcnx.TransformerConv is gcnx.layers.TransformerConv and gcnx.Transformer is gcnx.models.Transformer
    from gcnx.layers import TransformerConv
    for kw, word in ((dict(concat=False), "concat"), (dict(dropout=0.5), "dropout"), (dict(activation="relu"), "activation"),
                     (dict(beta=True, root_weight=False), "root_weight"), (dict(edge_dim=9), "edge_dim"), (dict(heads=3), "heads")):
        with pytest.raises(NotImplementedError) as e:
            TransformerConv(16, **{"heads": 4, **kw})
        assert word in str(e.value)
    with pytest.raises(NotImplementedError):
        TransformerConv(24, heads=4)                                                         # HC 96
    with pytest.raises(NotImplementedError):
        TransformerConv(16, heads=4)([(object(), object()), object()])                       # bipartite
    for d in (None, 2):
        for beta, root in OPTIONS:
            for bias in (True, False):
                layer = TransformerConv(16, heads=4, edge_dim=d, beta=beta, root_weight=root, use_bias=bias, seed=1)
                spec = layer._param_spec(8)
                want = [k for k in TR.conv_keys(d, beta, root) if bias or not k.endswith(".bias")]
                assert [n for n, _, _ in spec] == want == layer._names()
                shapes = {n: s for n, s, _ in spec}
                assert shapes["lin_key.weight"] == (8, 64) and (not bias or shapes["lin_query.bias"] == (64,))
                assert (not d or shapes["lin_edge.weight"] == (2, 64)) and (not beta or shapes["lin_beta.weight"] == (192,))
                assert layer.n_params(8) == sum(int(np.prod(s)) for s in shapes.values())
    init = {n: v for n, _, v in TransformerConv(16, heads=4, edge_dim=2, beta=True, seed=1)._param_spec(8)}
    lim = {"lin_key.weight": 8, "lin_key.bias": 8, "lin_skip.weight": 8, "lin_edge.weight": 2, "lin_beta.weight": 192}
    for k, fan_in in lim.items():                                                            # torch's Linear: U(+-1 / sqrt(fan_in))
        assert 0.5 / np.sqrt(fan_in) < np.max(np.abs(init[k])) <= 1 / np.sqrt(fan_in), k
    assert not np.array_equal(init["lin_key.weight"], init["lin_query.weight"])
    assert "use_bias=False" in TransformerConv.__doc__ and "2.5" in TransformerConv.__doc__

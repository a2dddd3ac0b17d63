"""CPU tests of the GATv2Conv feature (gcnx.GATv2Conv, gcnx.GATv2): the float64 oracle (tests/gatv2_ref.py) pinned against a
plain-torch autograd restatement and against its own Jacobian, the property that separates the layer from GATConv, the host
self-loop rule, the C ABI of the new entry points, and what the model and layer classes promise without a device.  torch is
imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gatv2_ref as GV
from test_gat_host import _graphs


def _edge_features(nnz, d, seed):
    return np.random.default_rng(seed).normal(size=(nnz, d)) if d else None


def _torch_model(x, rp, ci, e, gp, y, p, heads):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, rp, ci, e, gp, y, p, heads)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, rp, ci, e, gp, y, p, heads):
    """The model from torch.nn modules + a hand-written PyG GATv2Conv(heads, concat=True, negative_slope=0.2,
    add_self_loops=False, edge_dim, share_weights=False) on the stored pattern: the softmax over a target's entries from
    scatter_reduce("amax") and index_add_; scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.bias"].shape[0]
    c = h // heads
    src = torch.tensor(ci, dtype=torch.long)                                                   # row = target
    dst = torch.tensor(np.repeat(np.arange(n), np.diff(rp)), dtype=torch.long)
    et = None if e is None else torch.tensor(e)

    class Conv(torch.nn.Module):
        def __init__(self, fi):
            super().__init__()
            self.att = torch.nn.Parameter(torch.zeros(1, heads, c))
            self.bias = torch.nn.Parameter(torch.zeros(h))
            self.lin_l = torch.nn.Linear(fi, h)
            self.lin_r = torch.nn.Linear(fi, h)
            if et is not None:
                self.lin_edge = torch.nn.Linear(et.shape[1], h, bias=False)

        def forward(self, xx):
            xl, xr = self.lin_l(xx).view(n, heads, c), self.lin_r(xx).view(n, heads, c)
            s = xl[src] + xr[dst]
            if et is not None:
                s = s + self.lin_edge(et).view(-1, heads, c)
            score = (F.leaky_relu(s, 0.2) * self.att).sum(-1)
            m = torch.full((n, heads), -torch.inf).scatter_reduce(0, dst[:, None].expand(-1, heads), score.detach(), "amax",
                                                                  include_self=True)
            w = torch.exp(score - m[dst])
            alpha = w / torch.zeros(n, heads).index_add_(0, dst, w)[dst]
            out = torch.zeros(n, heads, c).index_add_(0, dst, alpha[:, :, None] * xl[src])
            return out.reshape(n, h) + self.bias

    mods = {"conv1": Conv(f), "conv2": Conv(h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    want = GV.keys(None if e is None else e.shape[1])
    assert set(named) == set(want)
    assert [k for k in named if k.startswith("conv")] == [k for k in want if k.startswith("conv")]    # att, bias, lin_l, lin_r, lin_edge
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


@pytest.mark.parametrize("edge_dim", [0, 2])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind, heads, edge_dim):
    x, a, gp, y = _graphs(kind, seed=2 if kind == "directed" else 0)
    pat = a != 0
    if kind == "symmetric":
        assert (pat != pat.T).nnz == 0 and a.diagonal().any()
    else:
        assert (pat != pat.T).nnz > 0 and (np.diff(a.indptr) == 0).any()                      # rows without entries: out = bias
    rp, ci, _ = GV.stored_pattern(a)
    e = _edge_features(len(ci), edge_dim, 11)
    p = GV.init_params(16, 64, heads, edge_dim or None, seed=3)
    assert p["conv1.att"].shape == (1, heads, 64 // heads) and p["conv1.lin_r.weight"].shape == (64, 16)
    assert ("conv2.lin_edge.weight" in p) == bool(edge_dim)
    out_t, loss_t, g_t = _torch_model(x, rp, ci, e, gp, y, p, heads)
    r = GV.model(x, rp, ci, e, gp, p, y, heads=heads)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(GV.keys(edge_dim or None)) == set(r["grads"])
    for k in g_t:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


@pytest.mark.parametrize("edge_dim", [0, 2])
@pytest.mark.parametrize("heads", [1, 4])
def test_oracle_conv_pair_is_consistent(heads, edge_dim):
    """conv_bwd is the adjoint of the Jacobian of conv_fwd: <dz, J v> = <J^T dz, v>, J v by a central difference in float64
    (step 1e-6), agreement 1e-6 relative.  No side is pinned: every |s| of the base point exceeds the step (asserted over all
    nnz H C of them, none left out) and both displaced points sit on the base point's sides (asserted).  The pattern has an
    empty row, which must give out = bias exactly."""
    x, a, _, _ = _graphs("directed", n_graphs=4, seed=5)
    rp, ci, _ = GV.stored_pattern(a)
    empty = np.diff(rp) == 0
    assert empty.any()
    rng = np.random.default_rng(heads + 10 * edge_dim)
    c, step = 8, 1e-6
    hc = heads * c
    names = ["x", "Wl", "bl", "Wr", "br", "att", "bias"] + (["We"] if edge_dim else [])
    base = [x, rng.normal(size=(16, hc)) / 4, rng.normal(size=hc), rng.normal(size=(16, hc)) / 4, rng.normal(size=hc),
            rng.normal(size=(heads, c)) / np.sqrt(c), rng.normal(size=hc)]
    e = _edge_features(len(ci), edge_dim, 13)
    if edge_dim:
        base.append(rng.normal(size=(edge_dim, hc)) / 2)

    def fwd(ops):
        return GV.conv_fwd(rp, ci, *ops[:7], e=e, We=ops[7] if edge_dim else None)

    out, cache = fwd(base)
    assert cache["s"].size == len(ci) * hc and np.min(np.abs(cache["s"])) > step, np.min(np.abs(cache["s"]))
    assert np.array_equal(out[empty], np.broadcast_to(base[6], out[empty].shape))
    assert np.allclose(np.add.reduceat(cache["alpha"], rp[:-1][~empty]), 1.0, rtol=0, atol=1e-12)    # every row's softmax sums to 1
    dz = rng.normal(size=out.shape)
    grads = GV.conv_bwd(cache, dz)
    v = [rng.normal(size=t.shape) for t in base]

    def directional(vs):
        (plus, cp), (minus, cm) = fwd([t + step * d for t, d in zip(base, vs)]), fwd([t - step * d for t, d in zip(base, vs)])
        assert np.array_equal(cp["pos"], cache["pos"]) and np.array_equal(cm["pos"], cache["pos"])
        return np.sum(dz * (plus - minus) / (2 * step))

    lhs, rhs = directional(v), sum(np.sum(grads[k] * d) for k, d in zip(names, v))
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs), (lhs, rhs)
    # and one operand at a time (a cancellation between two wrong gradients would pass the sum)
    for i, k in enumerate(names):
        lhs, rhs = directional([d if j == i else np.zeros_like(d) for j, d in enumerate(v)]), np.sum(grads[k] * v[i])
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)


def test_attention_is_dynamic_only_through_the_target_term():
    """What separates GATv2 from GAT.  Without edge features and with W_r = 0, b_r = 0 the score of an entry is a function of
    its source alone, so every target orders its sources the same way (GAT's static attention); with W_r != 0 two targets
    order the same two sources differently."""
    n, f, heads, c = 12, 8, 2, 8
    hc = heads * c
    rng = np.random.default_rng(4)
    rp, ci = np.arange(0, n * n + 1, n), np.tile(np.arange(n), n)                              # complete pattern, loops included
    x, Wl, bl = rng.normal(size=(n, f)), rng.normal(size=(f, hc)), rng.normal(size=hc)
    att = rng.normal(size=(heads, c))
    _, k0 = GV.conv_fwd(rp, ci, x, Wl, bl, np.zeros((f, hc)), np.zeros(hc), att, None)
    s0 = k0["score"].reshape(n, n, heads)                                                      # [target, source, head]
    assert np.array_equal(s0, np.broadcast_to(s0[0], s0.shape))                                # the same row of scores for every target
    _, k1 = GV.conv_fwd(rp, ci, x, Wl, bl, rng.normal(size=(f, hc)), np.zeros(hc), att, None)
    s1 = k1["score"].reshape(n, n, heads)
    order = np.argsort(s1, axis=1)
    assert any(not np.array_equal(order[i], order[0]) for i in range(1, n))                   # some target ranks the sources differently
    flips = [(i, j1, j2) for i in range(1, n) for j1 in range(n) for j2 in range(j1)
             if (s1[0, j1, 0] - s1[0, j2, 0]) * (s1[i, j1, 0] - s1[i, j2, 0]) < 0]
    assert flips                                                                               # a pair of sources two targets order oppositely


def test_mean_self_loop_rule_of_the_host_route():
    """Nodes: 0 has a stored loop (feature 9, 9: replaced) and entries from 1 and 2; 1 has no loop and one entry from 0; 2 has
    only its loop; 3 is isolated (no entry in its row)."""
    import scipy.sparse as sp
    from gcnx.models import _with_mean_self_loops
    rows, cols = np.array([0, 0, 0, 1, 2]), np.array([0, 1, 2, 0, 2])
    e = np.array([[9.0, 9.0], [1.0, 2.0], [3.0, 6.0], [5.0, 7.0], [4.0, 4.0]])
    want_cols = [0, 1, 2, 0, 1, 2, 3]
    want_e = np.array([[2.0, 4.0], [1.0, 2.0], [3.0, 6.0], [5.0, 7.0], [5.0, 7.0], [0.0, 0.0], [0.0, 0.0]])
    rp, ci, e2 = GV.mean_self_loops(np.array([0, 3, 4, 5, 5]), cols, e)
    assert rp.tolist() == [0, 3, 5, 6, 7] and ci.tolist() == want_cols and np.array_equal(e2, want_e)
    a = sp.coo_matrix((np.full(5, 0.5), (rows, cols)), shape=(4, 4))
    st, e3 = _with_mean_self_loops(a, e, 4)
    assert np.asarray(st.indices)[:, 0].tolist() == [0, 0, 0, 1, 1, 2, 3] and np.asarray(st.indices)[:, 1].tolist() == want_cols
    assert e3.dtype == np.float32 and np.array_equal(e3, want_e) and np.all(np.asarray(st.values) == 1.0)
    st0, none = _with_mean_self_loops(a, None, 4)
    assert none is None and np.array_equal(np.asarray(st0.indices), np.asarray(st.indices))
    with pytest.raises(ValueError):
        _with_mean_self_loops(a, e[:4], 4)


def test_device_sides_is_the_float32_expression_of_the_contract():
    rp, ci = np.array([0, 2, 3]), np.array([0, 1, 0])
    # one channel per half: Xl = [1e-8, -1], Xr = [1, 1]
    xlr = np.array([[1e-8, 1.0], [-1.0, 1.0]], np.float32)
    assert GV.device_sides(xlr, None, None, rp, ci).ravel().tolist() == [True, False, True]   # 1e-8 + 1 > 0; -1 + 1 = 0: not positive
    # the products are rounded separately and added in the order d = 0, 1, 2: (2^24 + 1) - 2^24 vanishes in float32 only in this order
    e = np.array([[2.0 ** 24, 1.0, -2.0 ** 24]] * 3, np.float32)
    w = np.ones((3, 1), np.float32)
    zero = np.zeros((2, 2), np.float32)
    assert GV.device_sides(zero, e, w, rp, ci).ravel().tolist() == [False] * 3
    assert GV.device_sides(zero, e[:, [0, 2, 1]], w, rp, ci).ravel().tolist() == [True] * 3
    assert GV.device_sides(zero.astype(np.float64), e.astype(np.float64), w, rp, ci).shape == (3, 1)   # float64 input is narrowed first


NAMES = ("gcnx_gatv2_conv_ok", "gcnx_gatv2_aggregate", "gcnx_gatv2_bwd_edges", "gcnx_gatv2_bwd_nodes", "gcnx_gatv2_bwd_scratch_floats")


def test_abi_declares_and_exports_the_gatv2_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 407
    assert lib.gcnx_gatv2_bwd_scratch_floats(1659, 4, 16, 2) >= 3 * 64 * -(-1659 // 32)
    assert lib.gcnx_gatv2_bwd_scratch_floats(1659, 4, 16, 0) >= 64 * -(-1659 // 32)
    assert lib.gcnx_gatv2_bwd_scratch_floats(-1, 4, 16, 0) == 0


def test_gatv2_conv_ok_truth_table():
    from gcnx import _lib
    ok = _lib.load().gcnx_gatv2_conv_ok                      # answers without a context
    for n, heads, c, ld, d in ((1000, 1, 64, 128, 0), (1000, 4, 16, 128, 2), (1000, 8, 16, 256, 8), (1000, 8, 4, 64, 1), (1000, 2, 8, 32, 0),
                               (1000, 1, 16, 40, 2), (0, 1, 16, 32, 0)):
        assert ok(n, heads, c, ld, d) == 1, (n, heads, c, ld, d)
    for n, heads, c, ld, d in ((1000, 4, 16, 128, 9), (1000, 4, 16, 128, -1),   # edge_dim 9, negative
                               (1000, 3, 16, 96, 0),             # heads 3
                               (1000, 4, 24, 192, 0), (1000, 1, 96, 192, 0),      # HC 96
                               (1000, 8, 32, 512, 0), (1000, 1, 256, 512, 0),     # HC 256
                               (1000, 8, 2, 32, 0),              # c 2
                               (1000, 1, 64, 64, 0), (1000, 1, 64, 124, 0),       # ldx < 2 HC
                               (1000, 1, 16, 34, 0),             # ldx % 4
                               (-1, 1, 64, 128, 0)):
        assert ok(n, heads, c, ld, d) == 0, (n, heads, c, ld, d)
    assert ok(2 ** 25, 1, 16, 32, 0) == 0 and ok(2 ** 25 - 8, 1, 16, 32, 0) == 1      # n * ldx * 4 reaches 2^32 / stays below


def test_gatv2_constructor_refusals_and_keys():
    from gcnx.models import GAT, GATv2, GCN
    with pytest.raises(NotImplementedError):
        GATv2(num_classes=2)
    with pytest.raises(NotImplementedError):
        GATv2(hidden_channels=64, comm=object())
    for kw in (dict(hidden_channels=96), dict(hidden_channels=256), dict(hidden_channels=64, heads=3), dict(hidden_channels=16, heads=8),
               dict(edge_dim=9), dict(edge_dim=0)):
        with pytest.raises(NotImplementedError):
            GATv2(**kw)
    assert issubclass(GATv2, GCN) and not issubclass(GATv2, GAT)
    nodev = object()                                            # stands in for the context: nothing here touches a device
    assert GATv2(ctx=nodev, edge_dim=2).uses_edge_features is True and GATv2(ctx=nodev).uses_edge_features is False
    assert GAT.uses_edge_features is False                                                   # (an instance attribute: nothing leaks)
    for d in (None, 2):
        m = GATv2(ctx=nodev, hidden_channels=64, heads=4, edge_dim=d)
        keys = [k for k, _, _ in m.TORCH_KEYS]
        assert keys == list(GV.keys(d))
        parts = GV.CONV_PARTS if d else GV.CONV_PARTS[:-1]
        assert keys[:2 * len(parts)] == [f"conv{k}.{t}" for k in (1, 2) for t in parts]
        assert keys[2 * len(parts):] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
        assert {k: tr for k, _, tr in m.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in keys if k.startswith("conv")}
        assert m.PROBE_KEY == "conv1.lin_l.weight"
        # one stacked weight and one stacked bias per convolution
        assert [k for k in m.PARAM_ORDER if k.endswith("1")][:4] == ["att1", "b1", "w1", "lb1"] and ("we1" in m.PARAM_ORDER) == bool(d)
        s = m._shapes(16)
        assert s["w1"] == (16, 128) and s["w2"] == (64, 128) and s["lb1"] == (128,) and s["att2"] == (4, 16) and s["we2"][1] == 64
    for phrase in ("named dicts", "add_self_loops", "fill_value"):
        assert phrase in GATv2.__doc__


def test_package_exports_the_new_names_and_the_layer_refuses_what_is_missing():
    import gcnx
    assert "GATv2Conv" in gcnx.__all__ and "GATv2" in gcnx.__all__
    assert gcnx.GATv2Conv is gcnx.layers.GATv2Conv and gcnx.GATv2 is gcnx.models.GATv2
    from gcnx.layers import GATv2Conv
    for kw, word in ((dict(concat=False), "concat"), (dict(dropout=0.5), "dropout"), (dict(activation="relu"), "activation"),
                     (dict(share_weights=True), "share_weights"), (dict(edge_dim=9), "edge_dim")):
        with pytest.raises(NotImplementedError) as e:
            GATv2Conv(16, heads=4, **kw)
        assert word in str(e.value)
    spec = GATv2Conv(16, heads=4, edge_dim=2, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("att", (4, 16)), ("bias", (64,)), ("lin_l.weight", (16, 64)), ("lin_l.bias", (64,)),
                                            ("lin_r.weight", (16, 64)), ("lin_r.bias", (64,)), ("lin_edge.weight", (2, 64))]
    init = {n: v for n, _, v in spec}
    assert not init["bias"].any() and not init["lin_l.bias"].any() and not init["lin_r.bias"].any()      # the biases start at zero
    assert np.max(np.abs(init["att"])) <= np.sqrt(6 / 20) and np.max(np.abs(init["lin_l.weight"])) <= np.sqrt(6 / 80)   # glorot-uniform
    assert np.max(np.abs(init["lin_edge.weight"])) <= np.sqrt(6 / 66) and not np.array_equal(init["lin_l.weight"], init["lin_r.weight"])
    assert [n for n, _, _ in GATv2Conv(16, use_bias=False, seed=1)._param_spec(16)] == ["att", "lin_l.weight", "lin_l.bias", "lin_r.weight",
                                                                                        "lin_r.bias"]
    assert GATv2Conv(16, heads=2, edge_dim=3).n_params(8) == 32 + 32 + 2 * 8 * 32 + 64 + 3 * 32

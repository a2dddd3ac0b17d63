"""CPU tests of the GINEConv feature (gcnx.GINEConv, gcnx.GINE): the float64 oracle (tests/gine_ref.py) pinned against a
plain-torch autograd restatement, the float32 contract restatement on exact kinks, the C ABI of the new entry points, the launch
sequences of gcnx.convs.gine_forward / gine_backward, and what the layer and model classes promise without a device.
torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gine_ref as ER
from host_fakes import HostContext as _HostContext
from test_sage_host import _graphs

NAMES = ("gcnx_gine_conv_ok", "gcnx_gine_conv", "gcnx_gine_aggregate", "gcnx_gine_bwd_scratch_floats", "gcnx_gine_bwd_edges",
         "gcnx_gine_bwd_nodes")


# ---- 1. the oracle against torch autograd ---------------------------------------------------------------------------------
def _torch_model(x, rowptr, colidx, e, gp, y, p):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, rowptr, colidx, e, gp, y, p)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, rowptr, colidx, e, gp, y, p):
    """The model from torch.nn modules + a hand-written PyG GINEConv(Sequential(Linear, ReLU, Linear), train_eps=True, edge_dim):
    nn((1 + eps) x + index_add_ of relu(x_j + lin(e))); scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h, d = p["conv1.nn.0.bias"].shape[0], e.shape[1]
    src, dst = torch.tensor(colidx, dtype=torch.long), torch.tensor(ER.rows_of(rowptr), dtype=torch.long)   # row = target
    et = torch.tensor(e)

    class Conv(torch.nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.eps = torch.nn.Parameter(torch.zeros(1))
            self.nn = torch.nn.Sequential(torch.nn.Linear(fi, fo), torch.nn.ReLU(), torch.nn.Linear(fo, fo))
            self.lin = torch.nn.Linear(d, fi)

        def forward(self, xx):
            agg = torch.zeros(n, xx.shape[1]).index_add_(0, dst, torch.relu(xx[src] + self.lin(et)))
            return self.nn((1 + self.eps) * xx + agg)

    mods = {"conv1": Conv(f, h), "conv2": Conv(h, h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    assert list(named)[:14] == list(ER.CONV_KEYS) and set(named) == set(ER.KEYS)     # eps, nn.*, lin.*: a module's own order
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


def _batch(kind):
    """x, rowptr, colidx, e (float32 values held as float64), graph_ptr, y."""
    import scipy.sparse as sp
    if kind == "symmetric":
        from gcnx import synth
        raw = synth.tiny_graphs(12, 16, seed=2)
        a = sp.block_diag([g[1] for g in raw], format="csr")
        gp = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in raw])])
        x = np.concatenate([g[0] for g in raw]).astype(np.float32).astype(np.float64)
        y = np.stack([g[2] for g in raw]).astype(np.float64)
        a.sort_indices()
        assert ((a != 0) != (a != 0).T).nnz == 0
    else:
        x, a, gp, y = _graphs("directed", seed=2)
        x = x.astype(np.float32).astype(np.float64)
        a = a.tolil()
        a[5, 5] = 1.0                                        # one stored self-loop: a neighbour like any other, with its own features
        a = a.tocsr()
        a.sort_indices()
        assert ((a != 0) != (a != 0).T).nnz > 0 and np.any(np.diff(a.indptr) == 0) and a.diagonal().sum() == 1.0
    e = np.random.default_rng(11).uniform(0, 1, (a.nnz, 2)).astype(np.float32).astype(np.float64)
    return x, a.indptr.astype(np.int64), a.indices.astype(np.int64), e, gp, y


@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind):
    x, rowptr, colidx, e, gp, y = _batch(kind)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in ER.init_params(16, 64, 2, seed=3, eps=(-0.3, 0.2)).items()}
    out_t, loss_t, g_t = _torch_model(x, rowptr, colidx, e, gp, y, p)
    r = ER.model(x, rowptr, colidx, e, gp, p, y)
    # no message within 1e-6 of its kink: the float64 and the float32 (contract) masks coincide
    for c, xin in (("conv1", x), ("conv2", r["y1"])):
        m64 = xin[colidx] + e @ p[f"{c}.lin.weight"].T + p[f"{c}.lin.bias"]
        assert np.min(np.abs(m64)) >= 1e-6, (c, np.min(np.abs(m64)))
        m32 = ER.contract_m(colidx, xin, e, p[f"{c}.lin.weight"], p[f"{c}.lin.bias"])
        assert np.array_equal(m32 > 0, m64 > 0) and np.array_equal(m64 > 0, r["msg" + c[-1]]) and (m64 > 0).any() and not (m64 > 0).all()
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(ER.KEYS) == set(r["grads"])
    for k in ER.KEYS:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    for k in ER.EPS_KEYS + ("conv1.lin.weight", "conv1.lin.bias", "conv2.lin.weight", "conv2.lin.bias"):
        assert np.max(np.abs(r["grads"][k])) > 1e-6, k                   # the new gradients are exercised
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


def test_oracle_conv_pair_is_consistent():
    """gine_conv_bwd is the adjoint of gine_conv_fwd's linearisation at fixed masks; a row without entries has T = (1 + eps) x;
    d lin.weight / d lin.bias / d eps are the directional derivatives."""
    x, rowptr, colidx, e, _, _ = _batch("directed")
    rng = np.random.default_rng(0)
    lw, lb = rng.normal(size=(16, 2)), rng.normal(size=16)
    wa, ba, wb, bb, eps = rng.normal(size=(24, 16)), rng.normal(size=24), rng.normal(size=(8, 24)), rng.normal(size=8), np.array([-0.3])
    out, t, u, mm, rm = ER.gine_conv_fwd(rowptr, colidx, x, e, eps, lw, lb, wa, ba, wb, bb)
    empty = np.diff(rowptr) == 0
    assert empty.any() and np.array_equal(t[empty], 0.7 * x[empty]) and mm.any() and not mm.all()
    dz = rng.normal(size=out.shape)
    dx, deps, dwa, dba, dwb, dbb, dlw, dlb = ER.gine_conv_bwd(rowptr, colidx, x, e, eps, t, u, mm, rm, wa, wb, dz)
    f = lambda xx, ee, w, b: np.sum(dz * ER.gine_conv_fwd(rowptr, colidx, xx, e, ee, w, b, wa, ba, wb, bb, msg_mask=mm, relu_mask=rm)[0])
    base = f(x, eps, lw, lb)
    for got, (vx, ve, vw, vb) in ((dx, (rng.normal(size=x.shape), 0, 0, 0)), (deps, (0, np.ones(1), 0, 0)),
                                  (dlw, (0, 0, rng.normal(size=lw.shape), 0)), (dlb, (0, 0, 0, rng.normal(size=16)))):
        v = vx if np.ndim(vx) else ve if np.ndim(ve) else vw if np.ndim(vw) else vb
        want = f(x + vx, eps + ve, lw + vw, lb + vb) - base                  # the map is affine at fixed masks
        assert abs(np.sum(got * v) - want) <= 1e-9 * max(1.0, abs(want)), (np.sum(got * v), want)
    assert np.allclose(dwb, dz.T @ u) and np.allclose(dbb, dz.sum(0)) and np.allclose(dwa, ((dz @ wb) * rm).T @ t)


# ---- 2. the contract restatement on exact kinks --------------------------------------------------------------------------
def test_contract_restatement_on_exact_kinks():
    """e = 0 and lin.bias = -x_j: m == 0 exactly -> message 0, gradient 0 (the zero side); one ulp above passes, one below not.
    The products and sums are rounded one by one, in the stated order: a fused or reordered evaluation gives another m."""
    x = np.array([[1.5, -0.75], [0.3, 2.0], [np.float32(0.1), 1.0]], np.float32)
    b = -x[1]                                                   # the kink of source 1
    rowptr, colidx = np.array([0, 3, 3, 3]), np.array([1, 1, 1])
    up, dn = np.nextafter(x[1], np.float32(np.inf)), np.nextafter(x[1], np.float32(-np.inf))
    for which, (xs, side) in enumerate(((x[1], False), (up, True), (dn, False))):
        xx = x.copy()
        xx[1] = xs
        e = np.zeros((3, 2), np.float32)
        m = ER.contract_m(colidx, xx, e, np.ones((2, 2), np.float32), b)
        assert m.dtype == np.float32 and ((m == 0).all() if which == 0 else (m != 0).all())
        mask = ER.contract_mask(colidx, xx, e, np.ones((2, 2), np.float32), b)
        assert (mask == side).all()
        t, _ = ER.gine_aggregate(rowptr, colidx, xx, e, 0.0, np.ones((2, 2)), b, msg_mask=mask)
        dx, _, dlw, dlb = ER.gine_edge_bwd(rowptr, colidx, xx, e, 0.0, mask, np.ones((3, 2)))
        if side:
            assert (t[0] > xx[0]).all() and (dlb == 3).all() and (dx[1] == 4).all()
        else:
            assert np.array_equal(t, xx.astype(np.float64)) and not dlb.any() and not dlw.any() and np.array_equal(dx, np.ones((3, 2)))
    # order and rounding: t = rn(rn(e0 w0) + rn(e1 w1)), then + b, then + x
    e = np.array([[3.0, 1.0]], np.float32)
    w = np.array([[np.float32(1) / 3, np.float32(2.0 ** -26)]], np.float32)                  # lin.weight [in = 1, D = 2]
    p0 = np.float32(e[0, 0] * w[0, 0])
    t = np.float32(p0 + np.float32(e[0, 1] * w[0, 1]))
    want = np.float32(np.float32(-1.0) + np.float32(t + np.float32(0.0)))
    got = ER.contract_m(np.array([0]), np.array([[-1.0]], np.float32), e, w, np.zeros(1, np.float32))
    assert got[0, 0] == want
    exact = -1.0 + (3.0 * float(w[0, 0]) + float(w[0, 1]))
    assert float(got[0, 0]) != exact                                                     # float64 (or an FMA chain) lands elsewhere


# ---- 3. the C ABI --------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_gine_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(?:int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
        assert re.search(r"/\*(?:(?!\*/).)*gcn\.py:71(?:(?!\*/).)*\*/\s*GCNX_API\s+\w+\s+" + nm + r"\s*\(", hdr, re.S), nm   # cites its source
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 423
    assert len(_lib.SIGNATURES["gcnx_gine_conv"]) == 25 and len(_lib.SIGNATURES["gcnx_gine_aggregate"]) == 15
    assert len(_lib.SIGNATURES["gcnx_gine_bwd_edges"]) == 17 and len(_lib.SIGNATURES["gcnx_gine_bwd_nodes"]) == 18
    sf = lib.gcnx_gine_bwd_scratch_floats
    assert sf(0, 64, 2) == 0 and sf(1, 64, 2) == 3 * 64 and sf(32, 5, 8) == 45 and sf(33, 5, 8) == 90 and sf(20000, 64, 2) == 625 * 192
    assert sf(10, 64, 0) == 0 and sf(10, 64, 9) == 0 and sf(-1, 64, 2) == 0


def test_gine_conv_ok_over_the_shape_grid():
    from gcnx import _lib
    ok = _lib.load().gcnx_gine_conv_ok                      # answers without a context: (n, k0, k1, k2, ldx, edge_dim)
    for k0 in range(0, 161, 4):
        for k1 in (0, 8, 16, 24, 48, 112, 128, 144):
            for k2 in (0, 8, 16, 24, 48, 112, 128, 144):
                for d in (0, 1, 2, 8, 9):
                    want = k0 in (16, 32, 64, 128) and k1 % 16 == 0 and 16 <= k1 <= 128 and k2 % 16 == 0 and 16 <= k2 <= 128 and 1 <= d <= 8
                    assert ok(1000, k0, k1, k2, max(k0, 4), d) == int(want), (k0, k1, k2, d)
    assert ok(1000, 64, 64, 0, 64, 2) == 0                                      # no single-stage form
    assert ok(1000, 16, 64, 64, 20, 2) == 1 and ok(1000, 16, 64, 64, 18, 2) == 0 and ok(1000, 64, 64, 64, 32, 2) == 0
    assert ok(0, 16, 64, 64, 16, 2) == 1 and ok(-1, 16, 64, 64, 16, 2) == 0 and ok(1000, 16, 64, 64, 16, -1) == 0
    assert ok(2 ** 26, 16, 64, 64, 16, 2) == 0 and ok(2 ** 26 - 8, 16, 64, 64, 16, 2) == 1    # n * ldx * 4 reaches 2^32 / stays below


def test_package_exports_the_new_names():
    import gcnx
    from gcnx import device as D
    assert "GINEConv" in gcnx.__all__ and "GINE" in gcnx.__all__
    from gcnx.layers import GINConv, GINEConv
    from gcnx.models import GCN, GIN, GINE
    assert gcnx.GINEConv is GINEConv and gcnx.GINE is GINE and issubclass(GINE, GCN) and GINE.uses_edge_features is True
    assert GIN.uses_edge_features is False and GINE.OPERATOR == "perm" and GINE.SELF_LOOPS is False and GINE.KERNELS == "GINEConv"
    for nm in ("gine_conv_ok", "gine_conv", "gine_aggregate", "gine_bwd_scratch_floats", "gine_bwd_edges", "gine_bwd_nodes"):
        assert callable(getattr(D, nm)), nm
    for bad in (None, 0, 9):
        with pytest.raises(NotImplementedError):
            GINEConv(64, bad)
    with pytest.raises(NotImplementedError):
        GINEConv(64, 2, activation="relu")
    lay = GINEConv(64, 2, seed=1)
    assert isinstance(lay, GINConv) and lay.mlp_hidden == 64 and lay.edge_dim == 2 and not lay.train_eps and lay.eps == 0.0
    spec = lay._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("nn.0.weight", (16, 64)), ("nn.0.bias", (64,)), ("nn.2.weight", (64, 64)), ("nn.2.bias", (64,)),
                                            ("lin.weight", (2, 16)), ("lin.bias", (16,))]
    lim = 1 / np.sqrt(2)                                                        # lin: fan_in = edge_dim
    assert 0.25 < np.max(np.abs(spec[4][2])) <= lim and np.max(np.abs(spec[5][2])) <= lim and np.max(np.abs(spec[0][2])) <= 0.25
    spec = GINEConv(32, 8, mlp_hidden=48, eps=-0.3, train_eps=True, use_bias=False, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("eps", (1,)), ("nn.0.weight", (16, 48)), ("nn.2.weight", (48, 32)), ("lin.weight", (8, 16))]


# ---- 4. the launch sequences ------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for gcnx.device inside gcnx.convs: records (name, args, kwargs) of every call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args, **kw):
            self.calls.append((name, args, kw))
        return call


@pytest.mark.parametrize("train_eps", [False, True])
@pytest.mark.parametrize("need_dx", [False, True])
@pytest.mark.parametrize("one_launch", [False, True])
def test_launch_sequences_of_gine_forward_and_backward(monkeypatch, one_launch, need_dx, train_eps):
    from gcnx import convs
    rec = _Recorder()
    monkeypatch.setattr(convs, "D", rec)
    o = {k: object() for k in ("ctx", "a", "x", "e", "eps", "w_e", "b_e", "w_a", "b_a", "w_b", "b_b", "t", "u", "out", "dz", "g_eps",
                               "g_w_e", "g_b_e", "g_w_a", "g_b_a", "g_w_b", "g_b_b", "du", "dt", "scratch", "parts", "dx")}
    fwd = lambda keep: convs.gine_forward(o["ctx"], o["a"], o["x"], o["e"], o["eps"], o["w_e"], o["b_e"], o["w_a"], o["b_a"], o["w_b"],
                                          o["b_b"], o["t"], o["u"], o["out"], one_launch, keep)
    for keep in (True, False):
        rec.calls.clear()
        fwd(keep)
        if one_launch:
            kept = dict(t=o["t"], u=o["u"]) if keep else dict(t=None, u=None)
            assert rec.calls == [("gine_conv", (o["ctx"], o["a"], o["x"], o["eps"], o["e"], o["w_e"], o["b_e"], o["w_a"], o["b_a"], o["w_b"],
                                                o["b_b"], o["out"]), kept)]
        else:
            assert rec.calls == [("gine_aggregate", (o["ctx"], o["a"], o["x"], o["eps"], o["e"], o["w_e"], o["b_e"], o["t"]), {}),
                                 ("gemm", (o["ctx"], o["t"], o["w_a"], o["b_a"], o["u"]), {"act": "relu"}),
                                 ("gemm", (o["ctx"], o["u"], o["w_b"], o["b_b"], o["out"]), {})]
    rec.calls.clear()
    convs.gine_backward(o["ctx"], o["a"], o["x"], o["e"], o["eps"], o["t"], o["u"], o["dz"], o["w_e"], o["b_e"], o["w_a"], o["w_b"],
                        o["g_eps"] if train_eps else None, o["g_w_e"], o["g_b_e"], o["g_w_a"], o["g_b_a"], o["g_w_b"], o["g_b_b"],
                        o["du"], o["dt"], o["scratch"], o["parts"] if train_eps else None, o["dx"] if need_dx else None)
    want = [("act_bias_grad", (o["ctx"], o["dz"], None, o["dz"], None), {"db": o["g_b_b"]}),
            ("gemm_dx", (o["ctx"], o["dz"], o["w_b"], o["du"]), {"y_mask": o["u"], "db": o["g_b_a"]}),
            ("gemm_dw2", (o["ctx"], o["u"], o["dz"], o["g_w_b"], o["t"], o["du"], o["g_w_a"]), {}),
            ("gemm_dx", (o["ctx"], o["du"], o["w_a"], o["dt"]), {}),
            ("gine_bwd_edges", (o["ctx"], o["a"], o["x"], o["e"], o["w_e"], o["b_e"], o["dt"], o["g_w_e"], o["g_b_e"], o["scratch"]), {})]
    if train_eps:
        want.append(("gin_eps_grad", (o["ctx"], o["x"], o["dt"], o["parts"], o["g_eps"]), {}))
    if need_dx:
        want.append(("gine_bwd_nodes", (o["ctx"], o["a"], o["x"], o["eps"], o["e"], o["w_e"], o["b_e"], o["dt"], o["dx"]), {}))
    assert rec.calls == want


# ---- 5. the model without a device ---------------------------------------------------------------------------------------
def test_gine_constructor_refusals():
    from gcnx.models import GINE
    for bad in (None, 0, 9):
        with pytest.raises(NotImplementedError):
            GINE(ctx=_HostContext(), edge_dim=bad)
    with pytest.raises(NotImplementedError):
        GINE(ctx=_HostContext(), comm=object())
    with pytest.raises(NotImplementedError):
        GINE(ctx=_HostContext(), num_classes=2)
    with pytest.raises(NotImplementedError):
        GINE(ctx=_HostContext(), readout="mean")
    with pytest.raises(NotImplementedError):
        GINE(ctx=_HostContext(), hidden_channels=512).build(16)
    m = GINE(ctx=_HostContext())
    assert m.edge_dim == 2 and m.hidden == 64 and not m.train_eps and m.uses_edge_features
    with pytest.raises(ValueError):
        m.forward(np.zeros((4, 16), np.float32), np.zeros((2, 0), np.int64), np.zeros(4, np.int64))   # (x, a, i) for a model that reads e


def test_gine_reads_its_route_knob_at_construction(monkeypatch):
    from gcnx.models import GINE
    monkeypatch.setenv("GCNX_GINE_FUSED", "0")
    monkeypatch.setenv("GCNX_GIN_FUSED", "1")
    m = GINE(ctx=_HostContext())
    monkeypatch.setenv("GCNX_GINE_FUSED", "1")
    assert m._fused is False and GINE(ctx=_HostContext())._fused is True


@pytest.mark.parametrize("train_eps", [False, True])
@pytest.mark.parametrize("readout,norm", [("max", "batch"), ("attention", "graph")])
def test_gine_state_dict_keys_shapes_and_round_trip(train_eps, readout, norm):
    from gcnx.models import GINE
    ctx = _HostContext()
    m = GINE(ctx=ctx, hidden_channels=32, edge_dim=3, train_eps=train_eps, seed=4, readout=readout, norm=norm)
    m.build(5)
    want = list(ER.keys(readout, norm))
    assert [k for k, _, _ in m.TORCH_KEYS] == [k for k in want if train_eps or k not in ER.EPS_KEYS]
    sd = m.state_dict()
    assert list(sd) == want                                              # eps is listed although it is not trained
    shapes = {"eps": (1,), "nn.0.weight": (32, None), "nn.0.bias": (32,), "nn.2.weight": (32, 32), "nn.2.bias": (32,),
              "lin.weight": (None, 3), "lin.bias": (None,)}
    for k, f in ((1, 5), (2, 32)):
        for s, shp in shapes.items():
            assert sd[f"conv{k}.{s}"].shape == tuple(f if v is None else v for v in shp), (k, s)
    assert np.max(np.abs(sd["conv1.lin.weight"])) <= 1 / np.sqrt(3) and np.max(np.abs(sd["conv1.lin.bias"])) <= 1 / np.sqrt(3)
    assert np.max(np.abs(sd["conv1.lin.weight"])) > 1 / np.sqrt(5) or np.max(np.abs(sd["conv2.lin.weight"])) > 1 / np.sqrt(5)
    assert sd["conv1.eps"][0] == 0 and sd["conv2.eps"][0] == 0
    # every tensor of the flat buffer starts on four floats; without train_eps the two constants live outside it
    assert all(off % 4 == 0 for off, _, _ in m.flat_p.views) and len(ctx.buffers) == (2 if train_eps else 3)
    assert ("e1" in m.PARAM_ORDER) == ("e2" in m.PARAM_ORDER) == train_eps
    assert len(m.get_weights()) == len(want) - (0 if train_eps else 2)
    # round trip through another model, eps included (a checkpoint's eps is honoured, trained or not)
    rng = np.random.default_rng(0)
    new = {k: rng.normal(size=v.shape).astype(np.float32) for k, v in sd.items()}
    m2 = GINE(ctx=_HostContext(), hidden_channels=32, edge_dim=3, train_eps=train_eps, seed=9, readout=readout, norm=norm)
    m2.load_state_dict(new)
    back = m2.state_dict()
    assert list(back) == want and all(np.array_equal(back[k], new[k]) for k in want)
    assert np.array_equal(m2.p["we1"].numpy(), new["conv1.lin.weight"].T)                 # stored [edge_dim, in]
    with pytest.raises(KeyError):
        GINE(ctx=_HostContext(), hidden_channels=32, edge_dim=3).load_state_dict({k: v for k, v in new.items() if k != "conv2.lin.bias"})
    if not train_eps:
        with pytest.raises(KeyError):
            GINE(ctx=_HostContext(), hidden_channels=32, edge_dim=3, readout=readout, norm=norm).load_state_dict(
                {k: v for k, v in new.items() if k != "conv2.eps"})
    with pytest.raises(ValueError):
        GINE(ctx=_HostContext(), hidden_channels=32, edge_dim=2, readout=readout, norm=norm).load_state_dict(new)   # another edge_dim

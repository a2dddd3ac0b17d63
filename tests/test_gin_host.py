"""CPU tests of the GINConv feature (gcnx.GINConv, gcnx.GIN): the float64 oracle (tests/gin_ref.py) pinned against a
plain-torch autograd restatement, the C ABI of the new entry points, and what the model class promises without a device.
torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gin_ref as GR
from test_sage_host import _graphs


def _torch_model(x, a, gp, y, p):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, a, gp, y, p)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, a, gp, y, p):
    """The model from torch.nn modules + a hand-written PyG GINConv(Sequential(Linear, ReLU, Linear), train_eps=True):
    nn((1 + eps) x + the sum of the sources' rows by index_add_); scatter_reduce("amax") for global_max_pool;
    BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.nn.0.bias"].shape[0]
    coo = a.tocoo()
    src, dst = torch.tensor(coo.col, dtype=torch.long), torch.tensor(coo.row, dtype=torch.long)   # row = target

    class Conv(torch.nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.eps = torch.nn.Parameter(torch.zeros(1))
            self.nn = torch.nn.Sequential(torch.nn.Linear(fi, fo), torch.nn.ReLU(), torch.nn.Linear(fo, fo))

        def forward(self, xx):
            agg = torch.zeros(n, xx.shape[1]).index_add_(0, dst, xx[src])
            return self.nn((1 + self.eps) * xx + agg)

    mods = {"conv1": Conv(f, h), "conv2": Conv(h, h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    assert list(named)[:10] == list(GR.CONV_KEYS) and set(named) == set(GR.KEYS)     # eps first, as a Parameter of the conv
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
    p = GR.init_params(16, 64, seed=3, eps=(-0.3, 0.2))
    out_t, loss_t, g_t = _torch_model(x, a, gp, y, p)
    r = GR.model(x, a, gp, p, y)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(GR.KEYS) == set(r["grads"])
    for k in GR.KEYS:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert all(abs(r["grads"][k][0]) > 1e-6 for k in GR.EPS_KEYS)            # the eps gradients are exercised
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


def test_oracle_conv_pair_is_consistent():
    """gin_conv_bwd is the adjoint of gin_conv_fwd's linearisation at a fixed ReLU mask: <dz, J v> = <J^T dz, v>; a row
    without entries has T = (1 + eps) x; d eps is the directional derivative along x."""
    x, a, gp, _ = _graphs("directed", n_graphs=4, seed=5)
    rng = np.random.default_rng(0)
    A = GR.sum_operator(a, x.shape[0])
    wa, ba, wb, bb, eps = rng.normal(size=(24, 16)), rng.normal(size=24), rng.normal(size=(8, 24)), rng.normal(size=8), np.array([-0.3])
    out, t, u, mask = GR.gin_conv_fwd(A, x, eps, wa, ba, wb, bb)
    empty = np.diff(A.indptr) == 0
    assert empty.any() and np.array_equal(t[empty], 0.7 * x[empty]) and mask.any() and not mask.all()
    dz, v = rng.normal(size=out.shape), rng.normal(size=x.shape)
    dx, deps, dwa, dba, dwb, dbb = GR.gin_conv_bwd(A, x, eps, t, u, mask, wa, wb, dz)
    lin = lambda xx, e: ((((1 + e) * xx + A @ xx) @ wa.T) * mask) @ wb.T       # the map at the forward's mask, biases dropped
    jv = lin(v, eps[0])
    assert abs(np.sum(dz * jv) - np.sum(dx * v)) <= 1e-10 * abs(np.sum(dz * jv))
    assert abs(np.sum(dz * (lin(x, 1.0) - lin(x, 0.0))) - deps[0]) <= 1e-10 * abs(deps[0])
    assert np.allclose(dwb, dz.T @ u) and np.allclose(dbb, dz.sum(0)) and np.allclose(dwa, ((dz @ wb) * mask).T @ t)
    # the mask argument takes the caller's side of the kink
    out2 = GR.gin_conv_fwd(A, x, eps, wa, ba, wb, bb, relu_mask=np.ones_like(mask))[0]
    assert np.allclose(out2, (t @ wa.T + ba) @ wb.T + bb)


def test_abi_declares_and_exports_the_gin_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    names = ("gcnx_gin_conv_ok", "gcnx_gin_conv", "gcnx_gin_aggregate", "gcnx_gin_eps_grad")
    for nm in names:
        assert re.search(r"GCNX_API\s+int\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 408
    ok = lib.gcnx_gin_conv_ok                                # answers without a context: (n, k0, k1, k2, ldx)
    assert ok(1000, 16, 64, 64, 16) == 1 and ok(1000, 128, 128, 128, 256) == 1 and ok(1000, 32, 48, 16, 32) == 1
    assert ok(1000, 64, 16, 0, 64) == 1 and ok(1000, 128, 16, 112, 128) == 1                 # single stage; unequal widths
    assert ok(1000, 96, 64, 64, 96) == 0 and ok(1000, 16, 256, 64, 16) == 0 and ok(1000, 16, 64, 24, 16) == 0
    assert ok(1000, 16, 0, 0, 16) == 0 and ok(1000, 16, 64, 144, 16) == 0 and ok(1000, 16, 24, 0, 16) == 0
    assert ok(1000, 16, 64, 64, 18) == 0 and ok(1000, 64, 64, 64, 32) == 0 and ok(-1, 16, 64, 64, 16) == 0
    assert ok(2 ** 26, 16, 64, 64, 16) == 0 and ok(2 ** 26 - 8, 16, 64, 64, 16) == 1     # n * ldx * 4 reaches 2^32 / stays below


def test_package_exports_the_new_names():
    import gcnx
    assert "GINConv" in gcnx.__all__ and "GIN" in gcnx.__all__
    from gcnx.layers import GINConv
    from gcnx.models import GCN, GIN
    assert gcnx.GINConv is GINConv and gcnx.GIN is GIN and issubclass(GIN, GCN) and GIN.uses_edge_features is False
    with pytest.raises(NotImplementedError):
        GINConv(64, activation="relu")
    lay = GINConv(64, seed=1)
    assert lay.mlp_hidden == 64 and not lay.train_eps and lay.eps == 0.0
    spec = lay._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("nn.0.weight", (16, 64)), ("nn.0.bias", (64,)), ("nn.2.weight", (64, 64)), ("nn.2.bias", (64,))]
    assert np.max(np.abs(spec[0][2])) <= 0.25 and np.max(np.abs(spec[1][2])) <= 0.25 and np.max(np.abs(spec[2][2])) <= 0.125   # U(+-1/sqrt(fan_in))
    spec = GINConv(32, mlp_hidden=48, eps=-0.3, train_eps=True, use_bias=False, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("eps", (1,)), ("nn.0.weight", (16, 48)), ("nn.2.weight", (48, 32))]
    assert spec[0][2] == np.float32(-0.3)


# ---- the model without a device -------------------------------------------------------------------------------------------
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
    """Stands in for gcnx.Context in build(): records zeros(n) and every flat(off, n, shape) of what it hands back."""

    def __init__(self):
        self.buffers = []

    def zeros(self, n):
        self.buffers.append(_Buffer(n))
        return self.buffers[-1]


def test_gin_constructor_refusals_and_keys():
    from gcnx.models import GCN, GIN
    with pytest.raises(NotImplementedError):
        GIN(num_classes=2)
    with pytest.raises(NotImplementedError):
        GIN(hidden_channels=64, comm=object())
    with pytest.raises(NotImplementedError):
        GIN(ctx=_RecordingContext(), hidden_channels=512).build(16)
    for te in (False, True):
        m = GIN(ctx=_RecordingContext(), hidden_channels=64, train_eps=te)
        keys = [k for k, _, _ in m.TORCH_KEYS]
        assert keys == [k for k in GR.KEYS if te or k not in GR.EPS_KEYS]
        assert keys[-16:] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
        assert {k: tr for k, _, tr in m.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in keys if k.startswith("conv")}
        assert sorted(k for _, k, _ in m.TORCH_KEYS) == sorted(m.PARAM_ORDER) and m.PROBE_KEY == "conv1.nn.0.weight"
        assert ("e1" in m.PARAM_ORDER) == ("e2" in m.PARAM_ORDER) == te


@pytest.mark.parametrize("train_eps", [False, True])
def test_gin_flat_buffer_starts_every_tensor_on_four_floats(train_eps):
    from gcnx.models import GIN
    ctx = _RecordingContext()
    m = GIN(ctx=ctx, hidden_channels=3, train_eps=train_eps)
    m.build(5)
    shapes = {"wa1": (5, 3), "wb1": (3, 3), "wa2": (3, 3), "wb2": (3, 3), "w3": (3, 3), "w4": (1, 3)}
    shapes.update({k: (3,) for k in ("ba1", "bb1", "g1", "be1", "ba2", "bb2", "g2", "be2", "b3", "g3", "be3")})
    shapes.update({k: (1,) for k in ("a1", "a2", "a3", "b4", "g4", "be4", "a4")})
    order = ["wa1", "ba1", "wb1", "bb1", "g1", "be1", "a1", "wa2", "ba2", "wb2", "bb2", "g2", "be2", "a2",
             "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4"]
    if train_eps:                              # one float, padded to four like every other tensor, in front of its conv
        shapes.update(e1=(1,), e2=(1,))
        order.insert(order.index("wa2"), "e2")
        order.insert(0, "e1")
    assert list(m.PARAM_ORDER) == order
    offsets, off = {}, 0
    for k in order:
        offsets[k] = off
        off += -(-int(np.prod(shapes[k])) // 4) * 4
    assert all(o % 4 == 0 for o in offsets.values()) and off == (148 if train_eps else 140)
    want = [(offsets[k], int(np.prod(shapes[k])), shapes[k]) for k in order]
    assert m.flat_p is ctx.buffers[0] and m.flat_g is ctx.buffers[1] and m.n_params == off
    assert [b.size for b in ctx.buffers[:2]] == [off, off + 2]
    assert sorted(m.flat_p.views) == sorted(want)                              # every parameter, nothing else
    assert sorted(m.flat_g.views) == sorted(want + [(off, 2, (2,))])           # the same places, then (loss sum, correct count)
    assert set(m.p) == set(m.g) == set(order) and all(m.p[k].shape == shapes[k] for k in order)
    # without train_eps the two constants live outside the flat buffers (no gradient, no update): one more small buffer
    assert len(ctx.buffers) == (2 if train_eps else 3)

"""Host tests of gcnx.APPNP / gcnx.APPNPConv: the float64 restatement tests/appnp_ref.py pinned to a hand-written
torch model with autograd, the adjoint identity of the propagation, the launch sequences of gcnx/convs.py, the ABI, the exports,
the refusals and the state dict.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

import appnp_ref as AP
import attn_pool_ref as AR
import gcn_bn_ref as R
import pdn_ref as PR
from host_fakes import HostContext as _HostContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gcnx_appnp_resident_ok", "gcnx_appnp_scratch_floats", "gcnx_appnp_propagate")


def _batch(f, seed=3, directed=False):
    """Four small graphs (node 11 isolated, every other node with or without a stored loop): x, scipy a, graph_ptr, y [B]."""
    x, a, _, gp, y = PR.make_batch((12, 19, 10, 25), f, 1, seed=seed, directed=directed, loops="some")
    return x, a, gp, y


# ---- 1. the restatement against a hand-written torch model ---------------------------------------------------------------------
def _torch_model(f, h, K, alpha, norm, readout):
    """The reference's GCN with each GCNConv replaced by Linear + K hops on the dense A^; modules in registration order lin1, lin2,
    then the reference's."""
    import torch
    from torch import nn

    class GraphNorm(nn.Module):
        def __init__(self):
            super().__init__()
            self.weight, self.bias, self.mean_scale = (nn.Parameter(torch.ones(h)), nn.Parameter(torch.zeros(h)),
                                                       nn.Parameter(torch.ones(h)))

        def forward(self, z, gp):
            parts = []
            for g in range(len(gp) - 1):
                zg = z[gp[g]:gp[g + 1]]
                o = zg - self.mean_scale * zg.mean(0)
                parts.append(o / torch.sqrt((o * o).mean(0) + 1e-5))
            return self.weight * torch.cat(parts) + self.bias

    class Pool(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_nn = nn.Linear(h, 1, bias=False)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin1, self.lin2 = nn.Linear(f, h), nn.Linear(h, h)
            self.linear_1, self.linear_2 = nn.Linear(h, h), nn.Linear(h, 1)
            self.prelu_1, self.prelu_2, self.prelu_3, self.prelu_4 = nn.PReLU(), nn.PReLU(), nn.PReLU(), nn.PReLU()
            bn = lambda w: nn.BatchNorm1d(w, track_running_stats=False)
            self.batch_norm_1 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_2 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_3, self.batch_norm_4 = bn(h), bn(1)
            if readout == "attention":
                self.pool = Pool()

        @staticmethod
        def hops(A, hk):
            z = hk
            for _ in range(K):
                z = (1 - alpha) * (A @ z) + alpha * hk
            return z

        def forward(self, x, A, gp):
            nrm = (lambda m, z: m(z, gp)) if norm == "graph" else (lambda m, z: m(z))
            y1 = self.prelu_1(nrm(self.batch_norm_1, self.hops(A, self.lin1(x))))
            y2 = self.prelu_2(nrm(self.batch_norm_2, self.hops(A, self.lin2(y1))))
            if readout == "attention":
                sc = self.pool.gate_nn(y2).reshape(-1)
                P = torch.stack([torch.softmax(sc[gp[g]:gp[g + 1]], 0) @ y2[gp[g]:gp[g + 1]] for g in range(len(gp) - 1)])
            else:
                P = torch.stack([y2[gp[g]:gp[g + 1]].max(0).values for g in range(len(gp) - 1)])
            y3 = self.prelu_3(self.batch_norm_3(self.linear_1(P)))
            return self.prelu_4(self.batch_norm_4(self.linear_2(y3)))

    return Net().double()


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.max(np.abs(got - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), (what, np.max(np.abs(got - ref)))


TORCH_CASES = [(K, alpha, False, "batch", "max") for K in (0, 1, 10) for alpha in (0.0, 0.1, 1.0)] + \
              [(10, 0.1, True, "batch", "max"), (10, 0.1, False, "graph", "max"), (3, 0.1, True, "batch", "attention")]


@pytest.mark.parametrize("K,alpha,directed,norm,readout", TORCH_CASES)
def test_ref_matches_torch_autograd(K, alpha, directed, norm, readout):
    import torch
    f, h = 7, 12
    x, a, gp, y = _batch(f, directed=directed)
    n = x.shape[0]
    assert directed == ((a != a.T).nnz != 0) and a[11].nnz == 0
    p = AP.init_params(f, h, seed=11, readout=readout, norm=norm)
    net = _torch_model(f, h, K, alpha, norm, readout)
    assert [k for k, _ in net.named_parameters()] == list(AP.keys(readout, norm))      # named_parameters() order = the key order
    net.load_state_dict({k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}, strict=True)
    T = lambda v: torch.tensor(np.asarray(v, np.float64))
    out = net(T(x), T(R.pyg_norm(a, n).toarray()), [int(v) for v in gp])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out.reshape(-1), T(y), reduction="sum") / (len(gp) - 1)
    loss.backward()
    r = AP.model(x, a, gp, p, K, alpha, y, readout=readout, norm=norm)
    _close(r["out"], out.detach().numpy(), "out")
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * max(1.0, abs(float(loss.detach())))
    assert set(r["grads"]) == set(AP.keys(readout, norm))
    for k, v in net.named_parameters():
        _close(r["grads"][k], v.grad.numpy(), k)
    if K > 0 and alpha < 1:               # P (1 b^T) is not constant over rows: BatchNorm does not cancel the Linear's bias
        assert np.abs(r["grads"]["lin1.bias"]).max() > 1e-6 and np.abs(r["grads"]["lin2.bias"]).max() > 1e-6


@pytest.mark.parametrize("K,alpha", [(0, 0.3), (1, 0.0), (10, 0.1), (64, 0.05), (5, 1.0)])
def test_propagation_adjoint_identity(K, alpha):
    """<P x, y> = <x, P^T y> with P^T the same recursion on A^T (a directed pattern: A^ is not symmetric)."""
    x, a, gp, _ = _batch(5, seed=8, directed=True)
    A = R.pyg_norm(a, x.shape[0])
    assert (abs(A - A.T) > 1e-12).nnz > 0
    rng = np.random.default_rng(K)
    u, v = rng.normal(size=(x.shape[0], 5)), rng.normal(size=(x.shape[0], 5))
    lhs, rhs = np.sum(AP.propagate(A, u, K, alpha) * v), np.sum(u * AP.propagate(A.T, v, K, alpha))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    if alpha == 1.0 or K == 0:
        assert np.array_equal(AP.propagate(A, u, K, alpha), u)
    # the closed form: P = M^K + alpha sum_{k<K} M^k, M = (1 - alpha) A
    M, d = (1 - alpha) * A.toarray(), np.eye(x.shape[0])
    Pm = np.linalg.matrix_power(M, K) + alpha * sum((np.linalg.matrix_power(M, k) for k in range(K)), np.zeros_like(d))
    assert np.max(np.abs(Pm @ u - AP.propagate(A, u, K, alpha))) <= 1e-12 * max(1.0, np.abs(u).max())


def test_conv_pair_is_consistent():
    x, a, gp, _ = _batch(6, seed=2, directed=True)
    A = R.pyg_norm(a, x.shape[0])
    rng = np.random.default_rng(0)
    w, b = rng.normal(size=(8, 6)), rng.normal(size=8)
    out, h = AP.conv_fwd(A, x, w, b, 10, 0.1)
    dz, v = rng.normal(size=out.shape), rng.normal(size=x.shape)
    dx, dw, db = AP.conv_bwd(A, x, w, dz, 10, 0.1)
    jv = AP.conv_fwd(A, v, w, None, 10, 0.1)[0]
    assert abs(np.sum(dz * jv) - np.sum(dx * v)) <= 1e-10 * abs(np.sum(dz * jv))
    dh = AP.propagate(A.T, dz, 10, 0.1)
    assert np.allclose(dw, dh.T @ x) and np.allclose(db, dh.sum(0)) and np.abs(db - dz.sum(0)).max() > 1e-3


# ---- 2. the launch sequences -----------------------------------------------------------------------------------------------------
class _Op:
    def __init__(self, name):
        self.name = name


@pytest.fixture
def rec(monkeypatch):
    """gcnx.device's launch wrappers replaced by recorders: [(name, [operand names or values], {keyword: ...})]."""
    import gcnx.device as D
    calls = []

    def recorder(name):
        def f(ctx, *args, **kw):
            assert ctx == "ctx"
            show = lambda v: v.name if isinstance(v, _Op) else v
            calls.append((name, [show(v) for v in args], {k: show(v) for k, v in kw.items()}))
        return f
    for name in ("gemm", "gemm_dw", "gemm_dx", "act_bias_grad", "appnp_propagate", "spmm", "add", "gemm_dw2"):
        monkeypatch.setattr(D, name, recorder(name))
    return calls


def test_appnp_sequences(rec):
    from gcnx import convs
    o = {k: _Op(k) for k in "a x w bias h out scratch".split()}
    convs.appnp_forward("ctx", **o, k=10, alpha=0.1)
    assert rec == [("gemm", ["x", "w", "bias", "h"], {}),
                   ("appnp_propagate", ["a", "h", "out", 10, 0.1], {"scratch": "scratch", "col_block": 0})]
    del rec[:]
    convs.appnp_forward("ctx", **dict(o, bias=None), k=3, alpha=0.5, col_block=-1)
    assert rec == [("gemm", ["x", "w", None, "h"], {}),
                   ("appnp_propagate", ["a", "h", "out", 3, 0.5], {"scratch": "scratch", "col_block": -1})]
    del rec[:]
    b = {k: _Op(k) for k in "a_t x dz w g_w g_bias dh scratch dx".split()}
    convs.appnp_backward("ctx", **b, k=10, alpha=0.1)
    assert rec == [("appnp_propagate", ["a_t", "dz", "dh", 10, 0.1], {"scratch": "scratch", "col_block": 0}),
                   ("act_bias_grad", ["dh", None, "dh", None], {"db": "g_bias"}),
                   ("gemm_dw", ["x", "dh", "g_w"], {}),
                   ("gemm_dx", ["dh", "w", "dx"], {})]
    del rec[:]
    convs.appnp_backward("ctx", **dict(b, g_bias=None, dx=None), k=10, alpha=0.1, col_block=-1)
    assert rec == [("appnp_propagate", ["a_t", "dz", "dh", 10, 0.1], {"scratch": "scratch", "col_block": -1}),
                   ("gemm_dw", ["x", "dh", "g_w"], {})]


def test_model_hooks_issue_the_conv_sequences(rec, monkeypatch):
    """gcnx.APPNP's two hooks call convs.appnp_forward / appnp_backward with h = bufs["h1"], dh = bufs["t"], scratch = bufs["s2"];
    GCNX_APPNP_RESIDENT=0 (read at construction) forces col_block = -1."""
    from gcnx.models import APPNP
    for env, cb in ((None, 0), ("0", -1), ("1", 0)):
        if env is None:
            monkeypatch.delenv("GCNX_APPNP_RESIDENT", raising=False)
        else:
            monkeypatch.setenv("GCNX_APPNP_RESIDENT", env)
        m = APPNP(ctx="ctx", hidden_channels=16, K=7, alpha=0.25)
        m.p = {k: _Op(k) for k in ("w1", "b1", "w2", "b2")}
        m.g = {k: _Op("g_" + k) for k in ("w1", "b1", "w2", "b2")}
        bufs = {k: _Op(k) for k in ("h1", "t", "s2", "z1", "z2")}
        del rec[:]
        m._conv_fwd(_Op("a"), _Op("x"), 2, bufs, True)
        assert rec == [("gemm", ["x", "w2", "b2", "h1"], {}),
                       ("appnp_propagate", ["a", "h1", "z2", 7, 0.25], {"scratch": "s2", "col_block": cb})]
        del rec[:]
        m._conv_bwd(_Op("a_t"), _Op("x"), 1, _Op("dz1"), bufs, None)
        assert [c[0] for c in rec] == ["appnp_propagate", "act_bias_grad", "gemm_dw"]
        assert rec[0] == ("appnp_propagate", ["a_t", "dz1", "t", 7, 0.25], {"scratch": "s2", "col_block": cb})
        assert rec[1][2] == {"db": "g_b1"} and rec[2][1] == ["x", "t", "g_w1"]


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_appnp_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert len(_lib.SIGNATURES["gcnx_appnp_propagate"]) == 17
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 426
    ok, sf = lib.gcnx_appnp_resident_ok, lib.gcnx_appnp_scratch_floats                  # both answer without a context
    assert ok(640, 64, 64) == 1 and ok(63, 4, 4) == 1 and ok(1500, 64, 128) == 1 and ok(3640, 16, 16) == 1 and ok(3641, 16, 16) == 0
    assert ok(0, 64, 64) == 0 and ok(5000, 4, 4) == 0 and ok(640, 50, 50) == 0 and ok(640, 64, 66) == 0 and ok(640, 64, 32) == 0
    assert ok(-1, 64, 64) == 0 and ok(640, 0, 0) == 0
    # two buffers of rows x 4 floats and the rows + 1 row pointers (padded to 4) within 128 KiB
    fits = lambda rows: 2 * rows * 16 + 4 * ((rows + 1 + 3) // 4 * 4) <= 128 * 1024
    top = max(r for r in range(3000, 4200) if fits(r))
    assert ok(top, 4, 4) == 1 and ok(top + 1, 4, 4) == 0
    assert sf(100, 64) == 6400 and sf(0, 64) == 0 and sf(100, 3) == 300


# ---- 4. exports, refusals, the state dict ----------------------------------------------------------------------------------------
def test_exports_and_constructor_refusals():
    import gcnx
    from gcnx import layers, models
    assert gcnx.APPNP is models.APPNP and gcnx.APPNPConv is layers.APPNPConv and {"APPNP", "APPNPConv"} <= set(gcnx.__all__)
    APPNP = models.APPNP
    assert issubclass(APPNP, models.GCN) and APPNP.uses_edge_features is False
    assert (APPNP.OPERATOR, APPNP.SELF_LOOPS, APPNP.PROBE_KEY) == ("gcn", True, "lin1.weight")
    for bad in (-1, 65, 2.5, "3", True, None):
        with pytest.raises(NotImplementedError, match="K="):
            APPNP(ctx=_HostContext(), K=bad)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            APPNP(ctx=_HostContext(), alpha=bad)
    with pytest.raises(NotImplementedError):
        APPNP(ctx=_HostContext(), num_classes=2)
    with pytest.raises(NotImplementedError, match="comm"):
        APPNP(ctx=_HostContext(), comm=object())
    with pytest.raises(NotImplementedError):
        APPNP(ctx=_HostContext(), readout="mean")
    with pytest.raises(NotImplementedError):
        APPNP(ctx=_HostContext(), norm="layer")
    m = APPNP(ctx=_HostContext())
    assert (m.hidden, m.K, m.alpha) == (64, 10, 0.1)
    assert (APPNP(ctx=_HostContext(), K=0).K, APPNP(ctx=_HostContext(), K=np.int64(64), alpha=1).K) == (0, 64)
    with pytest.raises(NotImplementedError):
        gcnx.Explainer(m)                                                                 # the explainer serves gcnx.GCN alone
    # the layer: Spektral's signature and what of it is served
    Conv = layers.APPNPConv
    lay = Conv(8)
    assert (lay.channels, lay.alpha, lay.propagations, lay.use_bias) == (8, 0.2, 1, True)
    for kw in (dict(mlp_hidden=[16]), dict(mlp_hidden=()), dict(dropout_rate=0.5), dict(activation="relu"), dict(propagations=-1),
               dict(propagations=65), dict(propagations=1.5)):
        with pytest.raises(NotImplementedError):
            Conv(8, **kw)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            Conv(8, alpha=bad)
    spec = Conv(8, seed=1)._param_spec(5)
    assert [(n, s) for n, s, _ in spec] == [("kernel", (5, 8)), ("bias", (8,))] and not spec[1][2].any()
    assert [n for n, _, _ in Conv(8, use_bias=False)._param_spec(5)] == ["kernel"]
    assert Conv.preprocess is layers.GCNConv.preprocess


@pytest.mark.parametrize("readout,norm", [("max", "batch"), ("attention", "graph")])
def test_state_dict_keys_shapes_initialisation_and_round_trip(readout, norm):
    from gcnx.models import APPNP, GCN
    m = APPNP(ctx=_HostContext(), hidden_channels=64, K=10, alpha=0.1, seed=4, readout=readout, norm=norm)
    m.build(16)
    want = list(AP.keys(readout, norm))
    assert [k for k, _, _ in m.TORCH_KEYS] == want and want[4:8] == [k for k, _, _ in GCN.TORCH_KEYS[4:8]]
    sd = m.state_dict()
    assert list(sd) == want and len(m.get_weights()) == len(want)
    assert sd["lin1.weight"].shape == (64, 16) and sd["lin2.weight"].shape == (64, 64)
    assert sd["lin1.bias"].shape == sd["lin2.bias"].shape == (64,)
    # the draw order and torch's Linear initialisation: lin1.weight, lin1.bias, lin2.weight, lin2.bias, then the head's w3, b3, w4, b4
    rng = np.random.default_rng(4)
    u = lambda fan_in, *s: rng.uniform(-1 / np.sqrt(fan_in), 1 / np.sqrt(fan_in), s).astype(np.float32)
    assert np.array_equal(sd["lin1.weight"], u(16, 16, 64).T) and np.array_equal(sd["lin1.bias"], u(16, 64))
    assert np.array_equal(sd["lin2.weight"], u(64, 64, 64).T) and np.array_equal(sd["lin2.bias"], u(64, 64))
    assert np.array_equal(sd["linear_1.weight"], u(64, 64, 64)) and np.array_equal(sd["linear_1.bias"], u(64, 64))
    # as many parameters as gcnx.GCN of the same sizes, every tensor on a 16-byte boundary
    ref = GCN(ctx=_HostContext(), hidden_channels=64, seed=4, readout=readout, norm=norm)
    ref.build(16)
    count = lambda mod: sum(int(np.prod(v.shape)) for v in mod.state_dict().values())
    assert count(m) == count(ref) and m.flat_p.size == ref.flat_p.size
    assert all(off % 4 == 0 for off, _, _ in m.flat_p.views)
    # the same seed gives the same bits twice
    m_again = APPNP(ctx=_HostContext(), hidden_channels=64, K=3, alpha=0.5, seed=4, readout=readout, norm=norm)
    m_again.build(16)
    assert all(np.array_equal(sd[k], v) for k, v in m_again.state_dict().items())
    # the head tensors of readout / norm sit where the family puts them
    if norm == "graph":
        assert want[want.index("batch_norm_1.bias") + 1] == "batch_norm_1.mean_scale" and not (sd["batch_norm_2.mean_scale"] - 1).any()
    if readout == "attention":
        assert want[-1] == AR.GATE_KEY and sd[AR.GATE_KEY].shape == (1, 64)
        plain = APPNP(ctx=_HostContext(), hidden_channels=64, seed=4)
        plain.build(16)
        assert all(np.array_equal(sd[k], v) for k, v in plain.state_dict().items())
    new = {k: np.random.default_rng(1).normal(size=v.shape).astype(np.float32) for k, v in sd.items()}
    m2 = APPNP(ctx=_HostContext(), hidden_channels=64, seed=9, readout=readout, norm=norm)
    m2.load_state_dict(new)
    back = m2.state_dict()
    assert list(back) == want and all(np.array_equal(back[k], new[k]) for k in want)
    assert m2.f_in == 16 and np.array_equal(m2.p["w1"].numpy(), new["lin1.weight"].T)
    with pytest.raises(KeyError):
        APPNP(ctx=_HostContext(), readout=readout, norm=norm).load_state_dict({k: v for k, v in new.items() if k != "lin2.bias"})
    with pytest.raises(ValueError):
        APPNP(ctx=_HostContext(), hidden_channels=32, readout=readout, norm=norm).load_state_dict(new)

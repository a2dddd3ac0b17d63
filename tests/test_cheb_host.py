"""Host tests of gcnx.Cheb / gcnx.ChebConv: the float64 restatement tests/cheb_ref.py pinned to torch autograd of
PyG's ChebConv written out in plain torch (get_laplacian's and ChebConv.__norm__'s steps on a dense matrix), Clenshaw summation
against the explicit sum, the adjoint identity behind the backward, the launch sequences of gcnx/convs.py, the ABI, the exports,
the refusals and the state dict.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

import attn_pool_ref as AR
import cheb_ref as CH
import pdn_ref as PR
from host_fakes import HostContext as _HostContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gcnx_cheb_norm", "gcnx_cheb_resident_ok", "gcnx_cheb_scratch_floats", "gcnx_cheb_basis", "gcnx_cheb_sum")
KS, LAMBDAS = (1, 2, 3, 5), (2.0, 3.0)


def _hand():
    """The hand-made batch as (scipy adjacency with its stored zeros kept, graph_ptr, n)."""
    import scipy.sparse as sp
    rowptr, colidx, vals, gp = CH.hand_batch()
    n = int(gp[-1])
    a = sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n))
    assert (a != a.T).nnz > 0 and a[4].nnz == 0 and a[:, 4].nnz == 0 and a[5].nnz == 0 and a[11].nnz == 1 and a[11, 11] != 0
    assert all(a[i, i] != 0 for i in (0, 2, 7, 10, 11)) and list(gp) == [0, 5, 6, 6, 12]
    return a, gp, n


# ---- 1. the restatement against PyG's steps in plain torch --------------------------------------------------------------------
def _pyg_lhat(a, n, lambda_max):
    """The dense [target, source] matrix ChebConv propagates with, by PyG's steps: get_laplacian(edge_index, edge_weight, "sym")
    -- remove_self_loops, deg = scatter_add(w, source), w <- deg^-1/2[source] w deg^-1/2[target] (inf -> 0), L = I - A with unit
    loops on every node --, then ChebConv.__norm__: w <- 2 w / lambda_max (inf -> 0), -1 on the loops."""
    import torch
    coo = a.tocoo()
    src, dst, w = torch.tensor(coo.col, dtype=torch.long), torch.tensor(coo.row, dtype=torch.long), torch.tensor(coo.data, dtype=torch.float64)
    keep = src != dst                                                                 # remove_self_loops
    src, dst, w = src[keep], dst[keep], w[keep]
    deg = torch.zeros(n, dtype=torch.float64).scatter_add_(0, src, w)                 # scatter(edge_weight, row = source)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    w = dis[src] * w * dis[dst]
    loops = torch.arange(n)                                                           # L = I - A: add_self_loops(-w, fill_value=1)
    src, dst, w = torch.cat([src, loops]), torch.cat([dst, loops]), torch.cat([-w, torch.ones(n, dtype=torch.float64)])
    w = (2.0 * w) / lambda_max                                                        # ChebConv.__norm__
    w.masked_fill_(w == float("inf"), 0)
    w = torch.where(src == dst, w - 1.0, w)
    return torch.zeros(n, n, dtype=torch.float64).index_put_((dst, src), w, accumulate=True)


def _torch_cheb(f_in, c, K):
    import torch
    from torch import nn

    class ChebConv(nn.Module):
        """PyG's ChebConv.forward on a dense L^: Tx_0 = x, Tx_1 = L^ x, Tx_k = 2 L^ Tx_{k-1} - Tx_{k-2}; out = sum lins[k](Tx_k) + bias."""

        def __init__(self):
            super().__init__()
            self.lins = nn.ModuleList([nn.Linear(f_in, c, bias=False) for _ in range(K)])
            self.bias = nn.Parameter(torch.zeros(c))

        def forward(self, x, L):
            tx0 = x
            out = self.lins[0](tx0)
            if K > 1:
                tx1 = L @ x
                out = out + self.lins[1](tx1)
            for lin in list(self.lins)[2:]:
                tx2 = 2.0 * (L @ tx1) - tx0
                out = out + lin(tx2)
                tx0, tx1 = tx1, tx2
            return out + self.bias

    return ChebConv().double()


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.max(np.abs(got - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), (what, np.max(np.abs(got - ref)))


def test_operator_is_pyg_laplacian_for_any_lambda_max():
    a, gp, n = _hand()
    S = CH.operator(a, n)
    assert S.nnz == a.nnz and np.array_equal(S.indices, a.indices)                    # the stored pattern, diagonal included
    d = S.toarray()
    assert not d.diagonal().any() and not d[4].any() and not d[:, 4].any() and not d[11].any() and d[9, 11] != 0
    for lam in (1.5, 2.0, 3.0):
        cs, cd = CH.coefs(lam)
        _close(cs * d + cd * np.eye(n), _pyg_lhat(a, n, lam).numpy(), f"L^ lambda_max={lam}")
    # values NULL means ones
    ones = a.copy()
    ones.data[:] = 1.0
    assert np.array_equal(CH.operator_values(a.indptr, a.indices, None, n), CH.operator(ones, n).data)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("lambda_max", LAMBDAS)
def test_conv_matches_torch_autograd(K, lambda_max):
    import torch
    a, gp, n = _hand()
    f_in, c = 7, 6
    rng = np.random.default_rng(10 * K + int(lambda_max))
    x, dz = rng.normal(size=(n, f_in)), rng.normal(size=(n, c))
    ws, b = [rng.normal(size=(c, f_in)) for _ in range(K)], rng.normal(size=c)
    net = _torch_cheb(f_in, c, K)
    net.load_state_dict({**{f"lins.{k}.weight": torch.tensor(w) for k, w in enumerate(ws)}, "bias": torch.tensor(b)}, strict=True)
    xt = torch.tensor(x, requires_grad=True)
    out = net(xt, _pyg_lhat(a, n, lambda_max))
    (out * torch.tensor(dz)).sum().backward()
    S = CH.operator(a, n)
    _close(CH.conv_fwd(S, x, ws, b, K, lambda_max), out.detach().numpy(), "out")
    dx, dws, db = CH.conv_bwd(S, x, ws, dz, K, lambda_max)
    _close(dx, xt.grad.numpy(), "dx")
    _close(db, net.bias.grad.numpy(), "db")
    for k in range(K):
        _close(dws[k], net.lins[k].weight.grad.numpy(), f"dW_{k}")
    # isolated nodes: L^ z = c_d z, so T_k z = T_k(c_d) z
    tk = [1.0, CH.coefs(lambda_max)[1]]
    for _ in range(2, K):
        tk.append(2 * tk[1] * tk[-1] - tk[-2])
    B = CH.basis(S, x, K, lambda_max)
    for k in range(K):
        _close(B[4, k * f_in:(k + 1) * f_in], tk[k] * x[4], f"T_{k} on the isolated node")


def _torch_model(f, h, K, norm, readout):
    """The reference's GCN with each GCNConv replaced by the ChebConv above (modules conv1, conv2, then the reference's)."""
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
            self.conv1, self.conv2 = _torch_cheb(f, h, K), _torch_cheb(h, h, K)
            self.linear_1, self.linear_2 = nn.Linear(h, h), nn.Linear(h, 1)
            self.prelu_1, self.prelu_2, self.prelu_3, self.prelu_4 = nn.PReLU(), nn.PReLU(), nn.PReLU(), nn.PReLU()
            bn = lambda w: nn.BatchNorm1d(w, track_running_stats=False)
            self.batch_norm_1 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_2 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_3, self.batch_norm_4 = bn(h), bn(1)
            if readout == "attention":
                self.pool = Pool()

        def forward(self, x, L, gp):
            nrm = (lambda m, z: m(z, gp)) if norm == "graph" else (lambda m, z: m(z))
            y1 = self.prelu_1(nrm(self.batch_norm_1, self.conv1(x, L)))
            y2 = self.prelu_2(nrm(self.batch_norm_2, self.conv2(y1, L)))
            if readout == "attention":
                sc = self.pool.gate_nn(y2).reshape(-1)
                P = torch.stack([torch.softmax(sc[gp[g]:gp[g + 1]], 0) @ y2[gp[g]:gp[g + 1]] for g in range(len(gp) - 1)])
            else:
                P = torch.stack([y2[gp[g]:gp[g + 1]].max(0).values for g in range(len(gp) - 1)])
            y3 = self.prelu_3(self.batch_norm_3(self.linear_1(P)))
            return self.prelu_4(self.batch_norm_4(self.linear_2(y3)))

    return Net().double()


MODEL_CASES = [(K, lam, True, "batch", "max") for K in KS for lam in LAMBDAS] + \
              [(3, 2.0, False, "graph", "max"), (3, 3.0, True, "batch", "attention")]


@pytest.mark.parametrize("K,lambda_max,directed,norm,readout", MODEL_CASES)
def test_model_matches_torch_autograd(K, lambda_max, directed, norm, readout):
    """The whole gcnx.Cheb step on four small graphs (node 11 isolated, every other node with or without a stored loop)."""
    import torch
    f, h = 7, 12
    x, a, _, gp, y = PR.make_batch((12, 19, 10, 25), f, 1, seed=3, directed=directed, loops="some")
    n = x.shape[0]
    assert directed == ((a != a.T).nnz != 0) and a[11].nnz == 0 and a.diagonal().any()
    p = CH.init_params(f, h, K, seed=11, readout=readout, norm=norm)
    net = _torch_model(f, h, K, norm, readout)
    assert {k for k, _ in net.named_parameters()} == set(CH.keys(K, readout, norm))
    net.load_state_dict({k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}, strict=True)
    T = lambda v: torch.tensor(np.asarray(v, np.float64))
    ones = a.copy()
    ones.data[:] = 1.0                                                                # the model reads the pattern, unweighted
    out = net(T(x), _pyg_lhat(ones, n, lambda_max), [int(v) for v in gp])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out.reshape(-1), T(y), reduction="sum") / (len(gp) - 1)
    loss.backward()
    r = CH.model(x, a, gp, p, K, lambda_max, y, readout=readout, norm=norm)
    _close(r["out"], out.detach().numpy(), "out")
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * max(1.0, abs(float(loss.detach())))
    assert set(r["grads"]) == set(CH.keys(K, readout, norm))
    for k, v in net.named_parameters():
        _close(r["grads"][k], v.grad.numpy(), k)


# ---- 2. Clenshaw, the adjoint ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 2, 3, 5, 16))
@pytest.mark.parametrize("lambda_max", (1.5, 2.0, 3.0))
def test_clenshaw_equals_the_explicit_sum_and_the_adjoint_identity(K, lambda_max):
    a, gp, n = _hand()
    S = CH.operator(a, n)
    rng = np.random.default_rng(K)
    f = 5
    H, dz, bias = rng.normal(size=(n, K * f)), rng.normal(size=(n, f)), rng.normal(size=f)
    for fp32 in (False, True):
        got, ref = CH.cheb_sum(S, H, bias, K, lambda_max, fp32), CH.cheb_sum_explicit(S, H, bias, K, lambda_max, fp32)
        # (below the spectrum's edge the terms grow: the scale is the largest term of the sum, not the sum)
        scale = max(1.0, max(np.abs(CH.basis(S, H[:, j * f:(j + 1) * f], K, lambda_max, fp32)).max() for j in range(K)))
        assert np.max(np.abs(got - ref)) <= 1e-10 * scale, (K, lambda_max)
        # <cheb_sum(A, H), dZ> = sum_k <H_k, basis(A^T, dZ)_k>
        lhs = np.sum(CH.cheb_sum(S, H, None, K, lambda_max, fp32) * dz)
        rhs = np.sum(H * CH.basis(S.T.tocsr(), dz, K, lambda_max, fp32))
        assert abs(lhs - rhs) <= 1e-11 * max(1.0, np.sum(np.abs(H * CH.basis(S.T.tocsr(), dz, K, lambda_max, fp32)))), (K, lambda_max)
    if K == 1:
        assert np.array_equal(CH.basis(S, dz, 1), dz) and np.array_equal(CH.cheb_sum(S, H, None, 1), H)
    if K >= 2 and lambda_max == 2.0:                                                  # T_1 = L^ = -S
        assert np.allclose(CH.basis(S, dz, K)[:, f:2 * f], -(S @ dz), rtol=0, atol=1e-14)
    assert CH.coefs(3.0, fp32=True) == (np.float64(np.float32(-2.0 / 3.0)), np.float64(np.float32(2.0 / 3.0 - 1.0)))


# ---- 3. the launch sequences -----------------------------------------------------------------------------------------------------
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
    for name in ("gemm", "gemm_dw", "gemm_dx", "act_bias_grad", "cheb_sum", "cheb_basis", "spmm", "add", "gemm_dw2"):
        monkeypatch.setattr(D, name, recorder(name))
    return calls


def test_cheb_sequences(rec):
    from gcnx import convs
    o = {k: _Op(k) for k in "a x w bias h out scratch".split()}
    convs.cheb_forward("ctx", **o, k=3, lambda_max=2.0)
    assert rec == [("gemm", ["x", "w", None, "h"], {}),
                   ("cheb_sum", ["a", "h", "bias", "out", 3, 2.0], {"scratch": "scratch", "col_block": 0})]
    del rec[:]
    b = {k: _Op(k) for k in "a_t x dz w g_w g_bias g scratch dx".split()}
    convs.cheb_backward("ctx", **b, k=5, lambda_max=3.0, col_block=-1)
    assert rec == [("act_bias_grad", ["dz", None, "dz", None], {"db": "g_bias"}),
                   ("cheb_basis", ["a_t", "dz", "g", 5, 3.0], {"scratch": "scratch", "col_block": -1}),
                   ("gemm_dw", ["x", "g", "g_w"], {}),
                   ("gemm_dx", ["g", "w", "dx"], {})]
    del rec[:]
    convs.cheb_backward("ctx", **dict(b, g_bias=None, dx=None), k=1, lambda_max=2.0)
    assert rec == [("cheb_basis", ["a_t", "dz", "g", 1, 2.0], {"scratch": "scratch", "col_block": 0}),
                   ("gemm_dw", ["x", "g", "g_w"], {})]


def test_model_hooks_issue_the_conv_sequences(rec, monkeypatch):
    """gcnx.Cheb's two hooks call convs.cheb_forward / cheb_backward with the panel bufs["ch"] and scratch = bufs["s2"];
    GCNX_CHEB_RESIDENT=0 (read at construction) forces col_block = -1."""
    from gcnx.models import Cheb
    for env, cb in ((None, 0), ("0", -1), ("1", 0)):
        if env is None:
            monkeypatch.delenv("GCNX_CHEB_RESIDENT", raising=False)
        else:
            monkeypatch.setenv("GCNX_CHEB_RESIDENT", env)
        m = Cheb(ctx="ctx", hidden_channels=16, K=4, lambda_max=3.0)
        m.p = {k: _Op(k) for k in ("w1", "b1", "w2", "b2")}
        m.g = {k: _Op("g_" + k) for k in ("w1", "b1", "w2", "b2")}
        bufs = {k: _Op(k) for k in ("ch", "s2", "z1", "z2")}
        del rec[:]
        m._conv_fwd(_Op("s"), _Op("x"), 2, bufs, True)
        assert rec == [("gemm", ["x", "w2", None, "ch"], {}),
                       ("cheb_sum", ["s", "ch", "b2", "z2", 4, 3.0], {"scratch": "s2", "col_block": cb})]
        del rec[:]
        m._conv_bwd(_Op("s_t"), _Op("x"), 1, _Op("dz1"), bufs, None)
        assert rec == [("act_bias_grad", ["dz1", None, "dz1", None], {"db": "g_b1"}),
                       ("cheb_basis", ["s_t", "dz1", "ch", 4, 3.0], {"scratch": "s2", "col_block": cb}),
                       ("gemm_dw", ["x", "ch", "g_w1"], {})]


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_cheb_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert len(_lib.SIGNATURES["gcnx_cheb_basis"]) == 17 and len(_lib.SIGNATURES["gcnx_cheb_sum"]) == 18
    assert len(_lib.SIGNATURES["gcnx_cheb_norm"]) == 9
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 426
    ok, sf = lib.gcnx_cheb_resident_ok, lib.gcnx_cheb_scratch_floats                    # both answer without a context
    assert ok(640, 64, 64) == 1 and ok(63, 4, 4) == 1 and ok(808, 64, 5 * 64) == 1 and ok(3640, 16, 16) == 1 and ok(3641, 16, 16) == 0
    assert ok(0, 64, 64) == 0 and ok(5000, 4, 4) == 0 and ok(640, 50, 50) == 0 and ok(640, 64, 66) == 0 and ok(640, 64, 32) == 0
    assert ok(-1, 64, 64) == 0 and ok(640, 0, 0) == 0
    assert all(ok(r, f, f) == lib.gcnx_appnp_resident_ok(r, f, f) for r in (1, 64, 808, 3640, 3641) for f in (4, 16, 50, 64))
    assert sf(100, 64) == 6400 and sf(0, 64) == 0 and sf(100, 3) == 300


# ---- 5. exports, refusals, the state dict ----------------------------------------------------------------------------------------
def test_exports_and_constructor_refusals():
    import gcnx
    from gcnx import layers, models
    assert gcnx.Cheb is models.Cheb and gcnx.ChebConv is layers.ChebConv and {"Cheb", "ChebConv"} <= set(gcnx.__all__)
    Cheb = models.Cheb
    assert issubclass(Cheb, models.GCN) and Cheb.uses_edge_features is False
    assert (Cheb.OPERATOR, Cheb.SELF_LOOPS, Cheb.PROBE_KEY) == ("cheb", False, "conv1.lins.0.weight")
    for bad in (0, -1, 17, 2.5, "3", True, None):
        with pytest.raises(NotImplementedError, match="K="):
            Cheb(ctx=_HostContext(), K=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_max"):
            Cheb(ctx=_HostContext(), lambda_max=bad)
    with pytest.raises(NotImplementedError):
        Cheb(ctx=_HostContext(), num_classes=2)
    with pytest.raises(NotImplementedError, match="comm"):
        Cheb(ctx=_HostContext(), comm=object())
    with pytest.raises(NotImplementedError):
        Cheb(ctx=_HostContext(), readout="mean")
    with pytest.raises(NotImplementedError):
        Cheb(ctx=_HostContext(), norm="layer")
    m = Cheb(ctx=_HostContext())
    assert (m.hidden, m.K, m.lambda_max) == (64, 3, 2.0)
    assert (Cheb(ctx=_HostContext(), K=1).K, Cheb(ctx=_HostContext(), K=np.int64(16), lambda_max=3).K) == (1, 16)
    with pytest.raises(NotImplementedError):
        gcnx.Explainer(m)                                                                 # the explainer serves gcnx.GCN alone
    # the layer: PyG's signature and what of it is served
    Conv = layers.ChebConv
    lay = Conv(8)
    assert (lay.channels, lay.K, lay.lambda_max, lay.use_bias, lay.col_block) == (8, 3, 2.0, True, 0)
    for kw in (dict(activation="relu"), dict(normalization=None), dict(normalization="rw"), dict(K=0), dict(K=17), dict(K=1.5), dict(K=True)):
        with pytest.raises(NotImplementedError):
            Conv(8, **kw)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            Conv(8, lambda_max=bad)
    spec = Conv(8, K=3, seed=1)._param_spec(5)
    assert [(n, s) for n, s, _ in spec] == [("lins.0.weight", (5, 8)), ("lins.1.weight", (5, 8)), ("lins.2.weight", (5, 8)), ("bias", (8,))]
    assert not spec[3][2].any() and all(np.abs(v).max() <= np.sqrt(6 / 13) for _, _, v in spec[:3])
    assert [n for n, _, _ in Conv(8, K=2, use_bias=False)._param_spec(5)] == ["lins.0.weight", "lins.1.weight"]
    # the layer's storage: the K weights are the column blocks of one stacked tensor
    lay = Conv(8, K=3, seed=1)
    lay.build(_HostContext(), 5)
    assert list(lay.params) == ["lins.0.weight", "lins.1.weight", "lins.2.weight", "bias"] and lay.weight.shape == (5, 24)
    assert lay.weight_grad.shape == (5, 24)
    for k in range(3):
        assert np.array_equal(lay.params[f"lins.{k}.weight"].numpy(), lay.weight.numpy()[:, 8 * k:8 * k + 8])
        assert np.array_equal(lay.params[f"lins.{k}.weight"].numpy(), spec[k][2])


@pytest.mark.parametrize("readout,norm", [("max", "batch"), ("attention", "graph")])
def test_state_dict_keys_shapes_initialisation_and_round_trip(readout, norm):
    from gcnx.layers import glorot_uniform
    from gcnx.models import Cheb, GCN
    K = 3
    m = Cheb(ctx=_HostContext(), hidden_channels=64, K=K, seed=4, readout=readout, norm=norm)
    m.build(16)
    want = list(CH.keys(K, readout, norm))
    assert want[:8] == ["conv1.lins.0.weight", "conv1.lins.1.weight", "conv1.lins.2.weight", "conv1.bias",
                        "conv2.lins.0.weight", "conv2.lins.1.weight", "conv2.lins.2.weight", "conv2.bias"]
    assert [k for k, _, _ in m.TORCH_KEYS] == want and want[8:12] == [k for k, _, _ in GCN.TORCH_KEYS[4:8]]
    sd = m.state_dict()
    assert list(sd) == want and len(m.get_weights()) == len(want)
    assert all(sd[f"conv1.lins.{k}.weight"].shape == (64, 16) and sd[f"conv2.lins.{k}.weight"].shape == (64, 64) for k in range(K))
    assert sd["conv1.bias"].shape == sd["conv2.bias"].shape == (64,) and not sd["conv1.bias"].any() and not sd["conv2.bias"].any()
    # one stacked tensor per convolution, [in, K hidden]; PyG's tensors are its column blocks
    assert m.p["w1"].shape == (16, K * 64) and m.p["w2"].shape == (64, K * 64)
    assert all(np.array_equal(m.p["w2"].numpy()[:, 64 * k:64 * k + 64], sd[f"conv2.lins.{k}.weight"].T) for k in range(K))
    # the draw order: glorot weights conv1.lins.0 .. conv2.lins.{K-1}, then the head's w3, b3, w4, b4
    rng = np.random.default_rng(4)
    for c, f in ((1, 16), (2, 64)):
        for k in range(K):
            assert np.array_equal(sd[f"conv{c}.lins.{k}.weight"], glorot_uniform(rng, f, 64).T), (c, k)
    u = lambda fan_in, *s: rng.uniform(-1 / np.sqrt(fan_in), 1 / np.sqrt(fan_in), s).astype(np.float32)
    assert np.array_equal(sd["linear_1.weight"], u(64, 64, 64)) and np.array_equal(sd["linear_1.bias"], u(64, 64))
    assert all(off % 4 == 0 for off, _, _ in m.flat_p.views)
    if norm == "graph":
        assert want[want.index("batch_norm_1.bias") + 1] == "batch_norm_1.mean_scale" and not (sd["batch_norm_2.mean_scale"] - 1).any()
    if readout == "attention":
        assert want[-1] == AR.GATE_KEY and sd[AR.GATE_KEY].shape == (1, 64)
        plain = Cheb(ctx=_HostContext(), hidden_channels=64, K=K, seed=4)
        plain.build(16)
        assert all(np.array_equal(sd[k], v) for k, v in plain.state_dict().items())
    new = {k: np.random.default_rng(1).normal(size=v.shape).astype(np.float32) for k, v in sd.items()}
    m2 = Cheb(ctx=_HostContext(), hidden_channels=64, K=K, seed=9, readout=readout, norm=norm)
    m2.load_state_dict(new)
    back = m2.state_dict()
    assert list(back) == want and all(np.array_equal(back[k], new[k]) for k in want)
    assert m2.f_in == 16 and np.array_equal(m2.p["w1"].numpy(), np.concatenate([new[f"conv1.lins.{k}.weight"].T for k in range(K)], axis=1))
    with pytest.raises(KeyError):
        Cheb(ctx=_HostContext(), K=K, readout=readout, norm=norm).load_state_dict({k: v for k, v in new.items() if k != "conv2.lins.1.weight"})
    with pytest.raises(ValueError):
        Cheb(ctx=_HostContext(), hidden_channels=32, K=K, readout=readout, norm=norm).load_state_dict(new)
    with pytest.raises(KeyError):                                                     # a model of more terms misses lins.3
        Cheb(ctx=_HostContext(), K=K + 1, readout=readout, norm=norm).load_state_dict(new)

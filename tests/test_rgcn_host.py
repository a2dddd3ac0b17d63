"""Host tests of gcnx.RGCN / gcnx.RGCNConv: the float64 restatement tests/rgcn_ref.py pinned to torch autograd of
PyG's RGCNConv written out in plain torch (a scatter-mean per relation, x @ root, bias), both relation rules, R = 1 against the
SAGE restatement, the adjoint identity behind the backward, the launch sequences of gcnx/convs.py, the ABI, the exports, the
refusals and the state dict.  torch is imported inside the tests only.

Sections 1 and 2 exercise tests/rgcn_ref.py alone (against torch and scipy; gcnx is not imported): they pin the restatement the GPU
tests compare the library with.  Sections 3 to 5 are the checks of the library's host code."""
import os
import re
import subprocess

import numpy as np
import pytest

import attn_pool_ref as AR
import rgcn_ref as RR
import sage_ref as SR
from host_fakes import HostContext as _HostContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gcnx_rgcn_operator", "gcnx_rgcn_conv_ok", "gcnx_rgcn_conv", "gcnx_rgcn_aggregate")


def _hand(R=3):
    """The hand batch with the relations of R: 3 -> "nonzero" on its (dca, proximity) features; 2 and 1 -> "index" on a column
    derived from them (2: bridges 0, everything else 1; 1: all 0)."""
    rowptr, colidx, e, gp = RR.hand_batch()
    rel3 = RR.relations(e, "nonzero")
    if R == 3:
        return rowptr, colidx, e, gp, "nonzero", rel3
    idx = (np.minimum(rel3, R - 1)).astype(np.float32)[:, None]
    return rowptr, colidx, idx, gp, "index", RR.relations(idx, "index", R)


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.max(np.abs(got - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), (what, np.max(np.abs(got - ref)))


# ---- 1. the restatement against PyG's steps in plain torch --------------------------------------------------------------------
def _torch_rgcn(f_in, c, R, root_weight):
    import torch
    from torch import nn

    class RGCNConv(nn.Module):
        """PyG's RGCNConv.forward without a decomposition: per relation, propagate(aggr="mean") over the edges of that type --
        a scatter-sum of x[source] onto the targets divided by the count, 0 where the count is 0 --, @ weight[r]; + x @ root + bias."""

        def __init__(self):
            super().__init__()
            self.weight = nn.Parameter(torch.zeros(R, f_in, c))
            if root_weight:
                self.root = nn.Parameter(torch.zeros(f_in, c))
            self.bias = nn.Parameter(torch.zeros(c))

        def forward(self, x, src, dst, edge_type):
            n = x.shape[0]
            out = torch.zeros(n, c, dtype=x.dtype)
            for r in range(R):
                sel = edge_type == r
                s, d = src[sel], dst[sel]
                summed = torch.zeros(n, f_in, dtype=x.dtype).index_add_(0, d, x[s])
                count = torch.zeros(n, dtype=x.dtype).index_add_(0, d, torch.ones(len(d), dtype=x.dtype))
                out = out + (summed / count.clamp(min=1).unsqueeze(1)) @ self.weight[r]
            if root_weight:
                out = out + x @ self.root
            return out + self.bias

    return RGCNConv().double()


def _edges(rowptr, colidx, rel):
    import torch
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return torch.tensor(colidx.astype(np.int64)), torch.tensor(rows.astype(np.int64)), torch.tensor(rel.astype(np.int64))


@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("R", [1, 2, 3])
def test_conv_matches_torch_autograd(R, root_weight):
    import torch
    rowptr, colidx, e, gp, rule, rel = _hand(R)
    n, f_in, c = int(gp[-1]), 7, 6
    rng = np.random.default_rng(10 * R + root_weight)
    x, dz = rng.normal(size=(n, f_in)), rng.normal(size=(n, c))
    w, root, b = rng.normal(size=(R, f_in, c)), (rng.normal(size=(f_in, c)) if root_weight else None), rng.normal(size=c)
    net = _torch_rgcn(f_in, c, R, root_weight)
    net.load_state_dict({"weight": torch.tensor(w), "bias": torch.tensor(b), **({"root": torch.tensor(root)} if root_weight else {})},
                        strict=True)
    xt = torch.tensor(x, requires_grad=True)
    out = net(xt, *_edges(rowptr, colidx, rel))
    (out * torch.tensor(dz)).sum().backward()
    ops = RR.operators(rowptr, colidx, rel, R)
    got, m = RR.conv_fwd(ops, x, w, root, b)
    _close(got, out.detach().numpy(), "out")
    assert m.shape == (n, R * f_in) and not m[4].any() and not m[5].any()             # rows without entries: means of nothing
    dx, dw, droot, db = RR.conv_bwd(ops, x, w, root, dz)
    _close(dx, xt.grad.numpy(), "dx")
    _close(dw, net.weight.grad.numpy(), "dweight")
    _close(db, net.bias.grad.numpy(), "dbias")
    if root_weight:
        _close(droot, net.root.grad.numpy(), "droot")
    else:
        assert droot is None


def _torch_model(f, h, R, root_weight, norm, readout):
    """The reference's GCN with each GCNConv replaced by the RGCNConv above (modules conv1, conv2, then the reference's)."""
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
            self.conv1, self.conv2 = _torch_rgcn(f, h, R, root_weight), _torch_rgcn(h, h, R, root_weight)
            self.linear_1, self.linear_2 = nn.Linear(h, h), nn.Linear(h, 1)
            self.prelu_1, self.prelu_2, self.prelu_3, self.prelu_4 = nn.PReLU(), nn.PReLU(), nn.PReLU(), nn.PReLU()
            bn = lambda w: nn.BatchNorm1d(w, track_running_stats=False)
            self.batch_norm_1 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_2 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_3, self.batch_norm_4 = bn(h), bn(1)
            if readout == "attention":
                self.pool = Pool()

        def forward(self, x, edges, gp):
            nrm = (lambda m, z: m(z, gp)) if norm == "graph" else (lambda m, z: m(z))
            y1 = self.prelu_1(nrm(self.batch_norm_1, self.conv1(x, *edges)))
            y2 = self.prelu_2(nrm(self.batch_norm_2, self.conv2(y1, *edges)))
            if readout == "attention":
                sc = self.pool.gate_nn(y2).reshape(-1)
                P = torch.stack([torch.softmax(sc[gp[g]:gp[g + 1]], 0) @ y2[gp[g]:gp[g + 1]] for g in range(len(gp) - 1)])
            else:
                P = torch.stack([y2[gp[g]:gp[g + 1]].max(0).values for g in range(len(gp) - 1)])
            y3 = self.prelu_3(self.batch_norm_3(self.linear_1(P)))
            return self.prelu_4(self.batch_norm_4(self.linear_2(y3)))

    return Net().double()


def _model_batch(R, seed=3):
    """Four small graphs (pdn_ref.make_batch: directed, some stored loops, node 11 isolated) with edge features for R relations:
    R = 3: (dca, proximity) with neither on the loops; otherwise an index column."""
    import pdn_ref as PR
    x, a, _, gp, y = PR.make_batch((12, 19, 10, 25), 7, 1, seed=seed, directed=True, loops="some")
    a = a.tocsr()
    a.sort_indices()
    rows = np.repeat(np.arange(a.shape[0]), np.diff(a.indptr))
    rng = np.random.default_rng(seed + 1)
    kind = np.where(rows == a.indices, 2, np.where(rng.random(a.nnz) < 0.25, 0, 1))    # loops: neither; a quarter bridges
    if R == 3:
        e = np.zeros((a.nnz, 2))
        e[kind == 0, 0], e[kind == 1, 1] = rng.uniform(0.2, 1.5, (kind == 0).sum()), rng.uniform(0.2, 1.5, (kind == 1).sum())
        rule = "nonzero"
    else:
        e, rule = np.minimum(kind, R - 1).astype(np.float64)[:, None], "index"
    rel = RR.relations(e, rule, R)
    assert all((rel == r).any() for r in range(R)) and a[11].nnz == 0
    return x, a, e, gp, y, rule, rel


MODEL_CASES = [(R, rw, "batch", "max") for R in (1, 2, 3) for rw in (True, False)] + \
              [(3, True, "graph", "max"), (2, True, "batch", "attention"), (3, False, "graph", "attention")]


@pytest.mark.parametrize("R,root_weight,norm,readout", MODEL_CASES)
def test_model_matches_torch_autograd(R, root_weight, norm, readout):
    import torch
    f, h = 7, 12
    x, a, e, gp, y, rule, rel = _model_batch(R)
    p = RR.init_params(f, h, R, seed=11, root_weight=root_weight, readout=readout, norm=norm)
    net = _torch_model(f, h, R, root_weight, norm, readout)
    assert {k for k, _ in net.named_parameters()} == set(RR.keys(root_weight, readout, norm))
    net.load_state_dict({k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}, strict=True)
    T = lambda v: torch.tensor(np.asarray(v, np.float64))
    out = net(T(x), _edges(a.indptr, a.indices, rel), [int(v) for v in gp])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out.reshape(-1), T(y), reduction="sum") / (len(gp) - 1)
    loss.backward()
    r = RR.model(x, a.indptr, a.indices, e, gp, p, y, rule=rule, num_relations=R, readout=readout, norm=norm)
    _close(r["out"], out.detach().numpy(), "out")
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * max(1.0, abs(float(loss.detach())))
    assert set(r["grads"]) == set(RR.keys(root_weight, readout, norm))
    for k, v in net.named_parameters():
        _close(r["grads"][k], v.grad.numpy(), k)


# ---- 2. the relation rules, R = 1, the adjoint ---------------------------------------------------------------------------------
def test_relation_rules_on_the_hand_batch():
    rowptr, colidx, e, gp = RR.hand_batch()
    rows = np.repeat(np.arange(12), np.diff(rowptr))
    rel = RR.relations(e, "nonzero")
    # reference-style features: dca on the bridges only, proximity on the contacts only -> bridges 0, contacts 1, neither 2
    assert np.array_equal(rel[e[:, 0] != 0], np.zeros((e[:, 0] != 0).sum(), np.int64)) and (e[:, 0] != 0).sum() == 5
    assert np.array_equal(rel == 1, (e[:, 0] == 0) & (e[:, 1] != 0))
    assert np.array_equal(rel == 2, ~e.any(1)) and set(zip(rows[rel == 2], colidx[rel == 2])) == {(0, 0), (2, 2), (7, 7), (10, 10), (11, 11), (8, 10)}
    assert not (rel[rows < 5] == 0).any()                                              # a relation no row of the first graph holds
    assert set(rel[rows == 1]) == {1} and set(rel[rows == 11]) == {2} and rowptr[5] == rowptr[4] and rowptr[6] == rowptr[5]
    # a first non-zero column wins over a later one
    assert list(RR.relations(np.array([[0.5, 0.7], [0, 0.7], [0, 0], [-1, 0]]), "nonzero")) == [0, 1, 2, 0]
    val = RR.values(rowptr, rel, 3)
    cnt = {(i, r): int(((rows == i) & (rel == r)).sum()) for i in range(12) for r in range(3)}
    assert all(val[k] == 1.0 / cnt[(rows[k], rel[k])] for k in range(len(rel)))
    ops = RR.operators(rowptr, colidx, rel, 3)
    for r, A in enumerate(ops):                                                        # every row of A_r sums to 1 or is empty
        s = np.asarray(A.sum(1)).ravel()
        assert np.allclose(s[[cnt[(i, r)] > 0 for i in range(12)]], 1.0) and not s[[cnt[(i, r)] == 0 for i in range(12)]].any()
    # "index": integers pass, the clamp is the kernel's; the host check is the model's
    idx = rel.astype(np.float32)[:, None]
    assert np.array_equal(RR.relations(idx, "index", 3), rel) and RR.check_index(idx, 3) and not RR.check_index(idx, 2)
    assert list(RR.relations(np.array([[-1.0], [0.0], [1.0], [2.0], [7.0], [np.nan], [1.5]]), "index", 3)) == [0, 0, 1, 2, 2, 0, 1]
    assert not RR.check_index(np.array([[1.5]]), 3) and not RR.check_index(np.array([[-1.0]]), 3) and not RR.check_index(np.array([[np.nan]]), 3)
    assert not RR.check_index(np.zeros((4, 2)), 3) and RR.check_index(np.zeros((0, 1)), 3)


def test_one_relation_is_sageconv():
    import scipy.sparse as sp
    rowptr, colidx, e, gp, rule, rel = _hand(1)
    n, f, c = 12, 5, 4
    rng = np.random.default_rng(2)
    x, dz, w, root, b = rng.normal(size=(n, f)), rng.normal(size=(n, c)), rng.normal(size=(1, f, c)), rng.normal(size=(f, c)), rng.normal(size=c)
    ops = RR.operators(rowptr, colidx, rel, 1)
    A = SR.mean_operator(sp.csr_matrix((np.ones(len(colidx)), colidx, rowptr), shape=(n, n)), n)
    assert np.array_equal(ops[0].toarray(), A.toarray())
    out, m = RR.conv_fwd(ops, x, w, root, b)
    s_out, s = SR.sage_conv_fwd(A, x, w[0].T, root.T, b)
    _close(out, s_out, "out")
    _close(m, s, "M = S")
    dx, dw, droot, db = RR.conv_bwd(ops, x, w, root, dz)
    s_dx, s_dwl, s_dwr, s_db = SR.sage_conv_bwd(A, x, s, w[0].T, root.T, dz)
    _close(dx, s_dx, "dx")
    _close(dw[0], s_dwl.T, "dW")
    _close(droot, s_dwr.T, "dW_root")
    _close(db, s_db, "db")


@pytest.mark.parametrize("R", [1, 2, 3])
def test_adjoint_identity_through_the_entry_permutation(R):
    """<A_r x, y> = <x, A_r^T y> with A_r^T walked as the library does: the transposed pattern, rel_t = rel[perm_t],
    val_t = val[perm_t]."""
    import graph_prep_ref as GP
    rowptr, colidx, e, gp, rule, rel = _hand(R)
    n = 12
    val = RR.values(rowptr, rel, R)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    perm = np.lexsort((rows, colidx))                                                  # transposed order: by column, then row
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n))])
    ci_t, rel_t, val_t = rows[perm], rel[perm], val[perm]
    if hasattr(GP, "transpose_perm"):
        g_rp, g_ci, g_pm = GP.transpose_perm(rowptr, colidx, n)
        assert np.array_equal(g_rp, rp_t) and np.array_equal(g_ci, ci_t) and np.array_equal(g_pm, perm)
    rng = np.random.default_rng(R)
    x, y = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    rows_t = np.repeat(np.arange(n), np.diff(rp_t))
    ops = RR.operators(rowptr, colidx, rel, R)
    for r in range(R):
        at_y = np.zeros((n, 3))
        sel = rel_t == r
        np.add.at(at_y, rows_t[sel], val_t[sel, None] * y[ci_t[sel]])
        _close(at_y, ops[r].T @ y, f"A_{r}^T y through perm_t")
        assert abs(np.sum((ops[r] @ x) * y) - np.sum(x * at_y)) <= 1e-12 * max(1.0, np.sum(np.abs(x * at_y)))


# ---- 3. the launch sequences -----------------------------------------------------------------------------------------------------
class _Op:
    """A named operand: flat / cols views are named after what they cut out; transpose_perm hands out the pattern's parts."""

    def __init__(self, name, shape=None):
        self.name, self.shape = name, shape
        self.rowptr, self.colidx = name + ".rowptr", name + ".colidx"

    def flat(self, off, n, shape=None):
        return _Op(f"{self.name}[{off}:{off + n}]", shape)

    def cols(self, c0, c1):
        return _Op(f"{self.name}[:, {c0}:{c1}]")

    def transpose_perm(self):
        return self.name + ".rowptr_t", self.name + ".colidx_t", self.name + ".perm_t"


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
    for name in ("gemm", "gemm_dw", "gemm_dw2", "gemm_dx", "act_bias_grad", "rgcn_conv", "rgcn_aggregate", "add", "spmm"):
        monkeypatch.setattr(D, name, recorder(name))
    return calls


OPS = ("rel", "val", "rel_t", "val_t")


def test_rgcn_sequences_one_launch(rec):
    from gcnx import convs
    o = dict(a=_Op("a"), ops=OPS, x=_Op("x", (40, 16)), w=_Op("w"), bias=_Op("bias"), m=_Op("m"), out=_Op("out", (40, 64)), h_tmp=_Op("h"))
    convs.rgcn_forward("ctx", **o, r=3, root_weight=True, one_launch=True)
    assert rec == [("rgcn_conv", ["a.rowptr", "a.colidx", "rel", "val", "x", "w", "bias", "out", 3, True], {"m": "m"})]
    del rec[:]
    convs.rgcn_forward("ctx", **o, r=3, root_weight=True, one_launch=True, keep=False)
    assert rec == [("rgcn_conv", ["a.rowptr", "a.colidx", "rel", "val", "x", "w", "bias", "out", 3, True], {"m": None})]
    del rec[:]
    b = dict(a=_Op("a"), ops=OPS, x=_Op("x", (40, 16)), m=_Op("m"), dz=_Op("dz", (40, 64)), w=_Op("w"), g_w=_Op("g_w"), g_bias=_Op("g_b"),
             mt=_Op("mt"))
    convs.rgcn_backward("ctx", **b, r=3, root_weight=True, one_launch=True, dx=_Op("dx"))
    assert rec == [("act_bias_grad", ["dz", None, "dz", None], {"db": "g_b"}),
                   ("gemm_dw2", ["m", "dz", "g_w[0:3072]", "x", "dz", "g_w[3072:4096]"], {}),
                   ("rgcn_conv", ["a.rowptr_t", "a.colidx_t", "rel_t", "val_t", "dz", "w", None, "dx", 3, True], {"w_transposed": True})]
    del rec[:]
    convs.rgcn_backward("ctx", **dict(b, g_bias=None), r=2, root_weight=False, one_launch=False, dx=None)      # conv1: no dx
    assert rec == [("gemm_dw", ["m", "dz", "g_w[0:2048]"], {})]


def test_rgcn_sequences_composed(rec):
    from gcnx import convs
    o = dict(a=_Op("a"), ops=OPS, x=_Op("x", (40, 7)), w=_Op("w"), bias=_Op("bias"), m=_Op("m"), out=_Op("out", (40, 5)), h_tmp=_Op("h"))
    convs.rgcn_forward("ctx", **o, r=2, root_weight=True, one_launch=False)
    assert rec == [("rgcn_aggregate", ["a.rowptr", "a.colidx", "rel", "val", "x", "m", 2], {}),
                   ("gemm", ["m", "w[0:70]", "bias", "out"], {}),
                   ("gemm", ["x", "w[70:105]", None, "h"], {}),
                   ("add", ["out", "h", "out"], {})]
    del rec[:]
    convs.rgcn_forward("ctx", **o, r=2, root_weight=False, one_launch=False)
    assert rec == [("rgcn_aggregate", ["a.rowptr", "a.colidx", "rel", "val", "x", "m", 2], {}),
                   ("gemm", ["m", "w[0:70]", "bias", "out"], {})]
    del rec[:]
    b = dict(a=_Op("a"), ops=OPS, x=_Op("x", (40, 7)), m=_Op("m"), dz=_Op("dz", (40, 5)), w=_Op("w"), g_w=_Op("g_w"), g_bias=_Op("g_b"),
             mt=_Op("mt"))
    convs.rgcn_backward("ctx", **b, r=2, root_weight=True, one_launch=False, dx=_Op("dx"))
    assert rec == [("act_bias_grad", ["dz", None, "dz", None], {"db": "g_b"}),
                   ("gemm_dw", ["m", "dz", "g_w[0:70]"], {}),                          # 70 floats: the root block is off a 16-byte boundary
                   ("gemm_dw", ["x", "dz", "g_w[70:105]"], {}),
                   ("rgcn_aggregate", ["a.rowptr_t", "a.colidx_t", "rel_t", "val_t", "dz", "mt", 2], {}),
                   ("gemm_dx", ["dz", "w[70:105]", "dx"], {}),
                   ("gemm_dx", ["mt[:, 0:5]", "w[0:35]", "dx"], {"accumulate": True}),
                   ("gemm_dx", ["mt[:, 5:10]", "w[35:70]", "dx"], {"accumulate": True})]
    del rec[:]
    convs.rgcn_backward("ctx", **b, r=2, root_weight=False, one_launch=False, dx=_Op("dx"))
    assert [c[0] for c in rec] == ["act_bias_grad", "gemm_dw", "rgcn_aggregate", "gemm_dx", "gemm_dx"]
    assert rec[3] == ("gemm_dx", ["mt[:, 0:5]", "w[0:35]", "dx"], {"accumulate": False}) and rec[4][2] == {"accumulate": True}


def test_model_hooks_issue_the_conv_sequences(rec, monkeypatch):
    """gcnx.RGCN's two hooks call convs.rgcn_forward / rgcn_backward with the panels bufs["pm{k}"]; GCNX_RGCN_FUSED=0 (read at
    construction) takes the composed route."""
    import gcnx.device as D
    from gcnx.models import RGCN
    monkeypatch.setattr(D, "rgcn_conv_ok", lambda ctx, n, fi, fo, r, ldx=None: fi in (16, 32, 64, 128) and fo in (16, 32, 64, 128))
    for env, fused in ((None, True), ("0", False), ("1", True)):
        if env is None:
            monkeypatch.delenv("GCNX_RGCN_FUSED", raising=False)
        else:
            monkeypatch.setenv("GCNX_RGCN_FUSED", env)
        m = RGCN(ctx="ctx", hidden_channels=16)
        assert m._fused == fused and (m.R, m.relations, m.edge_dim, m.root_weight) == (3, "nonzero", 2, True)
        m.p = {k: _Op(k) for k in ("w1", "b1", "w2", "b2")}
        m.g = {k: _Op("g_" + k) for k in ("w1", "b1", "w2", "b2")}
        m._rel_ops = OPS

        def buf(name, shape):
            o = _Op(name, shape)
            o.ptr, o.ld = 0, shape[1]
            return o
        bufs = {k: buf(k, (40, 16)) for k in ("z1", "z2", "h1", "dy1")}
        bufs.update(pm1=buf("pm1", (40, 48)), pm2=buf("pm2", (40, 48)), pmt=buf("pmt", (40, 48)))
        x, dz = buf("x", (40, 16)), buf("dz2", (40, 16))
        del rec[:]
        m._conv_fwd(_Op("a"), x, 2, bufs, True)
        if fused:
            assert rec == [("rgcn_conv", ["a.rowptr", "a.colidx", "rel", "val", "x", "w2", "b2", "z2", 3, True], {"m": "pm2"})]
        else:
            assert [c[0] for c in rec] == ["rgcn_aggregate", "gemm", "gemm", "add"] and rec[0][1][5] == "pm2" and rec[2][1][3] == "h1"
        del rec[:]
        m._conv_bwd(_Op("a"), x, 2, dz, bufs, bufs["dy1"])
        assert rec[:2] == [("act_bias_grad", ["dz2", None, "dz2", None], {"db": "g_b2"}),
                           ("gemm_dw2", ["pm2", "dz2", "g_w2[0:768]", "x", "dz2", "g_w2[768:1024]"], {})]
        if fused:
            assert rec[2:] == [("rgcn_conv", ["a.rowptr_t", "a.colidx_t", "rel_t", "val_t", "dz2", "w2", None, "dy1", 3, True],
                                {"w_transposed": True})]
        else:
            assert [c[0] for c in rec[2:]] == ["rgcn_aggregate", "gemm_dx", "gemm_dx", "gemm_dx", "gemm_dx"] and rec[2][1][5] == "pmt"
        del rec[:]
        m._conv_bwd(_Op("a"), x, 1, buf("dz1", (40, 16)), bufs, None)
        assert [c[0] for c in rec] == ["act_bias_grad", "gemm_dw2"] and rec[1][1][0] == "pm1"


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_rgcn_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert [len(_lib.SIGNATURES[nm]) for nm in NAMES] == [14, 5, 19, 12]
    assert "GCNX_RGCN_NONZERO = 0" in hdr and "GCNX_RGCN_INDEX = 1" in hdr and _lib.RGCN_RULES == {"nonzero": 0, "index": 1}
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 428
    ok = lib.gcnx_rgcn_conv_ok                                                          # answers without a context
    assert all(ok(600, fi, fo, r, fi) == 1 for fi in (16, 32, 64, 128) for fo in (16, 32, 64, 128) for r in (1, 2, 3, 4))
    assert ok(600, 64, 64, 0, 64) == 0 and ok(600, 64, 64, 5, 64) == 0 and ok(600, 48, 64, 3, 48) == 0 and ok(600, 64, 48, 3, 64) == 0
    assert ok(600, 256, 64, 3, 256) == 0 and ok(600, 64, 256, 3, 64) == 0 and ok(600, 64, 64, 3, 66) == 0 and ok(600, 64, 64, 3, 32) == 0
    assert ok(-1, 64, 64, 3, 64) == 0 and ok(0, 64, 64, 3, 64) == 1 and ok(1 << 24, 64, 64, 3, 64) == 0 and ok(600, 64, 64, 3, 128) == 1


# ---- 5. exports, refusals, the state dict ----------------------------------------------------------------------------------------
def test_exports_and_constructor_refusals():
    import gcnx
    from gcnx import layers, models
    assert gcnx.RGCN is models.RGCN and gcnx.RGCNConv is layers.RGCNConv and {"RGCN", "RGCNConv"} <= set(gcnx.__all__)
    RGCN = models.RGCN
    assert issubclass(RGCN, models.GCN) and RGCN.uses_edge_features is True
    assert (RGCN.OPERATOR, RGCN.SELF_LOOPS) == ("perm", False)
    m = RGCN(ctx=_HostContext())
    assert (m.hidden, m.R, m.relations, m.edge_dim, m.root_weight) == (64, 3, "nonzero", 2, True)
    assert RGCN(ctx=_HostContext(), edge_dim=1).R == 2 and RGCN(ctx=_HostContext(), edge_dim=3, num_relations=4).R == 4
    m = RGCN(ctx=_HostContext(), relations="index", num_relations=np.int64(2), root_weight=False)
    assert (m.R, m.edge_dim, m.root_weight) == (2, 1, False)
    for bad in (0, 5, -1, 2.0, "3", True):                                            # R outside 1 .. 4, or not an int
        with pytest.raises(NotImplementedError, match="num_relations"):
            RGCN(ctx=_HostContext(), relations="index", num_relations=bad)
    with pytest.raises(NotImplementedError, match="num_relations"):
        RGCN(ctx=_HostContext(), edge_dim=4)                                          # "nonzero": R = edge_dim + 1 = 5
    with pytest.raises(ValueError, match="num_relations"):
        RGCN(ctx=_HostContext(), relations="index")
    for nr in (2, 4):
        with pytest.raises(ValueError, match="edge_dim \\+ 1"):
            RGCN(ctx=_HostContext(), num_relations=nr)                                # "nonzero" with edge_dim = 2
    with pytest.raises(ValueError):
        RGCN(ctx=_HostContext(), relations="type")
    with pytest.raises(ValueError):
        RGCN(ctx=_HostContext(), edge_dim=None)
    with pytest.raises(NotImplementedError, match="comm"):
        RGCN(ctx=_HostContext(), comm=object())
    with pytest.raises(NotImplementedError):
        RGCN(ctx=_HostContext(), num_classes=2)
    with pytest.raises(NotImplementedError):
        RGCN(ctx=_HostContext(), readout="mean")
    with pytest.raises(NotImplementedError):
        RGCN(ctx=_HostContext(), norm="layer")
    with pytest.raises(NotImplementedError):
        gcnx.Explainer(RGCN(ctx=_HostContext()))                                      # the explainer serves gcnx.GCN alone
    # a batch without e, and e of the wrong shape
    m = RGCN(ctx=_HostContext())
    x, a, i = np.zeros((3, 4), np.float32), None, np.zeros(3, np.int64)
    with pytest.raises(ValueError, match="takes \\(x, a, e, i\\)"):
        m._as_batch((x, a, i))

    class _E:
        def __init__(self, shape):
            self.shape = shape

    class _B:
        def __init__(self, e):
            self.e, self.a = e, type("A", (), {"nnz": 10})()
    with pytest.raises(ValueError, match="\\[10, 2\\]"):
        m._check_e(_B(None))
    with pytest.raises(ValueError, match="\\[10, 2\\]"):
        m._check_e(_B(_E((10, 3))))
    with pytest.raises(ValueError, match="\\[10, 2\\]"):
        m._check_e(_B(_E((9, 2))))
    m._check_e(_B(_E((10, 2))))
    mi = RGCN(ctx=_HostContext(), relations="index", num_relations=3)
    with pytest.raises(ValueError, match="\\[10, 1\\]"):
        mi._check_e(_B(_E((10, 2))))
    # relations="index": a host batch is checked in NumPy before the upload
    for bad in ([[0.0], [1.5]], [[0.0], [3.0]], [[-1.0], [0.0]], [[np.nan], [0.0]]):
        with pytest.raises(ValueError, match="integers in 0 .. 2"):
            mi._host_inputs((x, a, np.asarray(bad, np.float32), i))
    assert mi._host_inputs((x, a, np.array([[0.0], [2.0]], np.float32), i))[1] is None
    # the layer: PyG's signature and what of it is served
    Conv = layers.RGCNConv
    lay = Conv(8)
    assert (lay.channels, lay.R, lay.relations, lay.root_weight, lay.use_bias) == (8, None, "nonzero", True, True)
    for kw in (dict(activation="relu"), dict(num_bases=2), dict(num_blocks=2), dict(aggr="add"), dict(num_relations=0), dict(num_relations=5),
               dict(num_relations=1.5)):
        with pytest.raises(NotImplementedError):
            Conv(8, **kw)
    with pytest.raises(ValueError):
        Conv(8, relations="index")
    with pytest.raises(ValueError):
        Conv(8, relations="type")
    lay = Conv(8, num_relations=3, seed=1)
    spec = lay._param_spec(5)
    assert [(n, s) for n, s, _ in spec] == [("weight", (15, 8)), ("root", (5, 8)), ("bias", (8,))]
    assert not spec[2][2].any() and all(np.abs(v).max() <= np.sqrt(6 / 13) for _, _, v in spec[:2])
    assert [n for n, _, _ in Conv(8, num_relations=2, root_weight=False, use_bias=False)._param_spec(5)] == ["weight"]
    # the layer's storage: weight and root are the row blocks of one stored tensor
    lay = Conv(8, num_relations=3, seed=1)
    lay.build(_HostContext(), 5)
    assert list(lay.params) == ["weight", "root", "bias"] and lay.stack.shape == (20, 8) and lay.stack_grad.shape == (20, 8)
    assert np.array_equal(lay.stack.numpy()[:15], spec[0][2]) and np.array_equal(lay.stack.numpy()[15:], spec[1][2])
    assert np.array_equal(lay.params["weight"].numpy(), spec[0][2]) and np.array_equal(lay.params["root"].numpy(), spec[1][2])
    assert lay._pyg(lay.params)["weight"].shape == (3, 5, 8) and lay.n_params(5) == 160 + 8


@pytest.mark.parametrize("root_weight,readout,norm", [(True, "max", "batch"), (False, "attention", "graph")])
def test_state_dict_keys_shapes_initialisation_and_round_trip(root_weight, readout, norm):
    from gcnx.layers import glorot_uniform
    from gcnx.models import RGCN, GCN
    R = 3
    m = RGCN(ctx=_HostContext(), hidden_channels=64, seed=4, root_weight=root_weight, readout=readout, norm=norm)
    m.build(16)
    want = list(RR.keys(root_weight, readout, norm))
    nc = 3 if root_weight else 2
    assert want[:2 * nc] == (["conv1.weight", "conv1.root", "conv1.bias", "conv2.weight", "conv2.root", "conv2.bias"] if root_weight
                             else ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"])
    assert [k for k, _, _ in m.TORCH_KEYS] == want and want[2 * nc:2 * nc + 4] == [k for k, _, _ in GCN.TORCH_KEYS[4:8]]
    sd = m.state_dict()
    assert list(sd) == want and len(m.get_weights()) == len(want)
    assert sd["conv1.weight"].shape == (R, 16, 64) and sd["conv2.weight"].shape == (R, 64, 64)
    assert sd["conv1.bias"].shape == sd["conv2.bias"].shape == (64,) and not sd["conv1.bias"].any() and not sd["conv2.bias"].any()
    # one row-stacked tensor per convolution, [(R + 1) in, hidden]: weight, then root, adjacent
    nb = R + (1 if root_weight else 0)
    assert m.p["w1"].shape == (nb * 16, 64) and m.p["w2"].shape == (nb * 64, 64) and m.g["w2"].shape == (nb * 64, 64)
    assert np.array_equal(m.p["w2"].numpy()[:R * 64].reshape(R, 64, 64), sd["conv2.weight"])
    if root_weight:
        assert sd["conv1.root"].shape == (16, 64) and np.array_equal(m.p["w1"].numpy()[R * 16:], sd["conv1.root"])
        assert m.p["wo2"].offset == m.p["wr2"].offset + R * 64 * 64 == m.p["w2"].offset + R * 64 * 64
    # the draw order: glorot conv1.weight[0 .. R-1], conv1.root, conv2.weight[..], conv2.root, then the head's w3, b3, w4, b4
    rng = np.random.default_rng(4)
    for c, f in ((1, 16), (2, 64)):
        for r in range(R):
            assert np.array_equal(sd[f"conv{c}.weight"][r], glorot_uniform(rng, f, 64)), (c, r)
        if root_weight:
            assert np.array_equal(sd[f"conv{c}.root"], glorot_uniform(rng, f, 64)), c
    u = lambda fan_in, *s: rng.uniform(-1 / np.sqrt(fan_in), 1 / np.sqrt(fan_in), s).astype(np.float32)
    assert np.array_equal(sd["linear_1.weight"], u(64, 64, 64)) and np.array_equal(sd["linear_1.bias"], u(64, 64))
    assert all(off % 4 == 0 for off, _, _ in m.flat_p.views)
    if norm == "graph":
        assert want[want.index("batch_norm_1.bias") + 1] == "batch_norm_1.mean_scale" and not (sd["batch_norm_2.mean_scale"] - 1).any()
    if readout == "attention":
        assert want[-1] == AR.GATE_KEY and sd[AR.GATE_KEY].shape == (1, 64)
    new = {k: np.random.default_rng(1).normal(size=v.shape).astype(np.float32) for k, v in sd.items()}
    kw = dict(root_weight=root_weight, readout=readout, norm=norm)
    m2 = RGCN(ctx=_HostContext(), hidden_channels=64, seed=9, **kw)
    m2.load_state_dict(new)
    back = m2.state_dict()
    assert list(back) == want and all(np.array_equal(back[k], new[k]) for k in want)
    assert m2.f_in == 16 and np.array_equal(m2.p["w1"].numpy()[:R * 16], new["conv1.weight"].reshape(R * 16, 64))
    g = m2.gradients()
    assert list(g) == want and g["conv1.weight"].shape == (R, 16, 64)
    with pytest.raises(KeyError):
        RGCN(ctx=_HostContext(), **kw).load_state_dict({k: v for k, v in new.items() if k != "conv2.weight"})
    with pytest.raises(ValueError):
        RGCN(ctx=_HostContext(), hidden_channels=32, **kw).load_state_dict(new)
    with pytest.raises(ValueError):                                                   # a model of another R
        RGCN(ctx=_HostContext(), edge_dim=1, **kw).load_state_dict(new)

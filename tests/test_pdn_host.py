"""Host tests of gcnx.PDN / gcnx.PDNConv: the float64 restatement tests/pdn_ref.py pinned to a hand-written
torch model and to finite differences, the unit-loop host helper, the margins of the GPU tests' cases, the ABI, the exports,
the refusals and the state dict.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

import attn_pool_ref as AR
import pdn_ref as PR
from host_fakes import HostContext as _HostContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gcnx_pdn_ok", "gcnx_pdn_operator", "gcnx_pdn_bwd_scratch_floats", "gcnx_pdn_operator_bwd")


# ---- 1. the restatement against a hand-written torch model ---------------------------------------------------------------------
def _torch_model(f, h, d, he, norm, readout):
    """The reference's GCN with both GCNConv layers replaced by a PDNConv written out from index_add_ and gcn_norm; modules in
    the reference's registration order, inside PDNConv PyG's (bias, lin, mlp)."""
    import torch
    from torch import nn

    class PDNConv(nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.bias = nn.Parameter(torch.zeros(fo))
            self.lin = nn.Linear(fi, fo, bias=False)
            self.mlp = nn.Sequential(nn.Linear(d, he), nn.ReLU(), nn.Linear(he, 1), nn.Sigmoid())

        def forward(self, x, src, dst, e):
            n = x.shape[0]
            w = self.mlp(e).squeeze(-1)
            # add_remaining_self_loops(fill_value=1): the nodes that store no loop get one of weight exactly 1, outside the MLP
            has = torch.zeros(n, dtype=torch.bool)
            has[dst[src == dst]] = True
            miss = torch.nonzero(~has).reshape(-1)
            src, dst, w = torch.cat([src, miss]), torch.cat([dst, miss]), torch.cat([w, torch.ones(len(miss), dtype=w.dtype)])
            deg = torch.zeros(n, dtype=w.dtype).index_add_(0, dst, w)
            dinv = deg.pow(-0.5)
            dinv = torch.where(torch.isinf(dinv), torch.zeros_like(dinv), dinv)
            v = dinv[dst] * w * dinv[src]
            xw = self.lin(x)
            return torch.zeros(n, xw.shape[1], dtype=xw.dtype).index_add_(0, dst, v[:, None] * xw[src]) + self.bias

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
            self.conv1, self.conv2 = PDNConv(f, h), PDNConv(h, h)
            self.linear_1, self.linear_2 = nn.Linear(h, h), nn.Linear(h, 1)
            self.prelu_1, self.prelu_2, self.prelu_3, self.prelu_4 = nn.PReLU(), nn.PReLU(), nn.PReLU(), nn.PReLU()
            bn = lambda w: nn.BatchNorm1d(w, track_running_stats=False)
            self.batch_norm_1 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_2 = GraphNorm() if norm == "graph" else bn(h)
            self.batch_norm_3, self.batch_norm_4 = bn(h), bn(1)
            if readout == "attention":
                self.pool = Pool()

        def forward(self, x, src, dst, e, gp):
            nrm = (lambda m, z: m(z, gp)) if norm == "graph" else (lambda m, z: m(z))
            y1 = self.prelu_1(nrm(self.batch_norm_1, self.conv1(x, src, dst, e)))
            y2 = self.prelu_2(nrm(self.batch_norm_2, self.conv2(y1, src, dst, e)))
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


# (directed, loops, norm, readout): a symmetric pattern (its e is asymmetric by construction), a directed one, stored loops mixed
# with unit loops, no stored loop at all, norm="graph" once, readout="attention" once; node 11 is isolated in every case
TORCH_CASES = [(False, "all", "batch", "max"), (True, "all", "batch", "max"), (False, "some", "batch", "max"),
               (True, "none", "batch", "max"), (False, "some", "graph", "max"), (True, "all", "batch", "attention")]


@pytest.mark.parametrize("directed,loops,norm,readout", TORCH_CASES)
def test_ref_matches_torch_autograd(directed, loops, norm, readout):
    import torch
    f, h, d, he = 7, 12, 3, 5
    x, a, e, gp, y = PR.make_batch((12, 19, 10, 25), f, d, seed=3, directed=directed, loops=loops)
    n = x.shape[0]
    assert directed == ((a != a.T).nnz != 0) and a[11].nnz == (1 if loops == "all" else 0)
    rows = PR.rows_of(a.indptr)
    twin = {(i, j): k for k, (i, j) in enumerate(zip(rows, a.indices))}
    assert any((j, i) in twin and not np.array_equal(e[k], e[twin[(j, i)]]) for (i, j), k in twin.items() if i != j)
    p = PR.init_params(f, h, d, he, seed=11, readout=readout, norm=norm)
    net = _torch_model(f, h, d, he, norm, readout)
    assert [k for k, _ in net.named_parameters()] == list(PR.keys(readout, norm))      # named_parameters() order = the key order
    net.load_state_dict({k: torch.tensor(np.asarray(v, np.float64)) for k, v in p.items()}, strict=True)
    T = lambda v: torch.tensor(np.asarray(v, np.float64))
    out = net(T(x), torch.tensor(a.indices.astype(np.int64)), torch.tensor(rows), T(e), [int(v) for v in gp])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(out.reshape(-1), T(y), reduction="sum") / (len(gp) - 1)
    loss.backward()
    rp, ci, e2, unit = PR.with_unit_self_loops(a.indptr, a.indices, e)
    assert int(unit.sum()) == n - int((rows == a.indices).sum())
    r = PR.model(x, rp, ci, e2, gp, p, y, readout=readout, norm=norm, unit=unit)
    _close(r["out"], out.detach().numpy(), "out")
    assert abs(r["loss"] - float(loss.detach())) <= 1e-10 * max(1.0, abs(float(loss.detach())))
    assert set(r["grads"]) == set(PR.keys(readout, norm))
    for k, v in net.named_parameters():
        _close(r["grads"][k], v.grad.numpy(), k)
    for k in PR.GATE_KEYS:
        assert np.abs(r["grads"][k]).max() > 0, k


# ---- 2. finite differences ---------------------------------------------------------------------------------------------------------
def test_ref_finite_difference_spots():
    f, h, d, he = 5, 8, 2, 4
    x, a, e, gp, y = PR.make_batch((12, 19, 10), f, d, seed=8, loops="some")
    rp, ci, e2, unit = PR.with_unit_self_loops(a.indptr, a.indices, e)
    p = PR.init_params(f, h, d, he, seed=2)
    r = PR.model(x, rp, ci, e2, gp, p, y, unit=unit)
    kink = {"masks": {k: r[k] for k in ("m1", "m2", "m3", "m4", "gate1", "gate2")}, "argmax": r["argmax"]}
    eps = 1e-6
    for key, idx in (("conv1.mlp.0.weight", (1, 0)), ("conv2.mlp.2.bias", (0,))):
        hi, lo = ({**p, key: p[key].copy()} for _ in range(2))
        hi[key][idx] += eps
        lo[key][idx] -= eps
        fd = (PR.model(x, rp, ci, e2, gp, hi, y, unit=unit, **kink)["loss"] - PR.model(x, rp, ci, e2, gp, lo, y, unit=unit, **kink)["loss"]) / (2 * eps)
        want = r["grads"][key][idx]
        # a central difference of step 1e-6 on an O(1) loss in float64: truncation ~1e-12, cancellation ~1e-10 / 1e-6
        assert abs(fd - want) <= 1e-6 * max(1e-3, abs(want)) + 1e-9, (key, fd, want)


# ---- 3. the unit-loop host helper ------------------------------------------------------------------------------------------------
def test_unit_self_loops_on_a_hand_made_batch():
    import scipy.sparse as sp
    from gcnx.models import _with_unit_self_loops
    # graph 0: nodes 0, 1, 2 (path 0 - 1 - 2; 1 stores its loop); graph 1: nodes 3, 4 (3 -> 4 only; 4 stores its loop)
    rows = np.array([0, 1, 1, 1, 2, 4, 4])
    cols = np.array([1, 0, 1, 2, 1, 3, 4])
    e = np.arange(1, 15, dtype=np.float32).reshape(7, 2)
    a = sp.csr_matrix((np.full(7, 3.0), (rows, cols)), shape=(5, 5))
    t, e2, unit = _with_unit_self_loops(a, e, 5)
    idx = np.asarray(t.indices)
    assert idx.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [1, 2], [2, 1], [2, 2], [3, 3], [4, 3], [4, 4]]
    assert unit.dtype == np.uint8 and unit.tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert np.array_equal(e2[unit == 0], e) and not e2[unit == 1].any() and e2.dtype == np.float32   # existing entries untouched
    assert np.all(np.asarray(t.values) == 1.0)
    rp, ci, e3, un = PR.with_unit_self_loops(a.indptr, a.indices, e)                     # the restatement's helper agrees
    assert np.array_equal(ci, idx[:, 1]) and np.array_equal(un, unit.astype(bool)) and np.array_equal(e3, e2)
    # nothing missing: no flags, the entries as they were
    full = sp.csr_matrix(a + sp.identity(5))
    full.sort_indices()
    t, e4, unit = _with_unit_self_loops(full, np.ones((full.nnz, 2), np.float32), 5)
    assert unit is None and len(t.indices) == full.nnz and e4.shape == (full.nnz, 2)
    with pytest.raises(ValueError):
        _with_unit_self_loops(a, e[:5], 5)


# ---- 4. the GPU tests' cases keep their margins ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,d,he", PR.operator_cases())
def test_gpu_operator_cases_keep_the_relu_margin(shape, d, he):
    c = PR.operator_case(shape, d, he)
    deg = np.diff(c["rowptr"])
    assert (deg == 0).any() and (deg == 1).any() and c["e"].shape == (c["nnz"], d) and c["w1"].shape == (he, d)
    if shape == 1200:
        assert deg.max() > 1024 and deg[-1] == 0
    else:
        assert deg.max() <= 12 and shape % 32 != 0 and shape > 64
    assert 0 < c["unit"].sum() < c["nnz"]                                                 # some stored diagonal entries, not all
    z = c["e"].astype(np.float64) @ c["w1"].astype(np.float64).T + c["b1"]
    assert np.min(np.abs(z)) >= PR.GATE_MARGIN                                            # every entry, unit or not
    assert np.array_equal(PR.gate_z32(c["e"], c["w1"], c["b1"]) > 0, z > 0)
    rows, cols = PR.rows_of(c["rowptr"]), c["colidx"]
    pairs = set(zip(rows.tolist(), cols.tolist()))
    assert any((j, i) not in pairs for i, j in pairs)                                     # asymmetric
    rp_t, ci_t, perm = PR.transpose_perm(c["rowptr"], cols)
    assert np.array_equal(cols[perm], PR.rows_of(rp_t)) and np.array_equal(rows[perm], ci_t)


def test_gpu_step_cases_are_what_they_say():
    routes = set()
    for name, (f, h, d, he, norm, readout, directed, loops, route) in PR.STEP_CASES.items():
        x, a, e, gp, y, p = PR.step_case(name)
        assert list(p) == list(PR.keys(readout, norm)) and len(gp) == 5 and np.all((np.diff(gp) >= 14) & (np.diff(gp) <= 40))
        assert directed == ((a != a.T).nnz != 0), name
        stored = int((PR.rows_of(a.indptr) == a.indices).sum())
        assert (stored == x.shape[0]) == (loops == "all") and (route == "host" or loops == "all"), name
        assert a[13].nnz == (1 if loops == "all" else 0)                                  # the isolated node
        routes.add(route)
        # no gate gradient is a cancellation that fp32 cannot resolve to 1e-4 of the result (pdn_ref.STEP_COND, reasoned there)
        rp, ci, e2, unit = PR.with_unit_self_loops(a.indptr, a.indices, e)
        r = PR.model(x, rp, ci, e2, gp, p, y, readout=readout, norm=norm, unit=unit)
        for k in PR.GATE_KEYS:
            assert np.max(r["gate_cond"][k]) <= PR.STEP_COND * np.max(np.abs(r["grads"][k])), (name, k)
    assert routes == {"device", "host"}
    he_set = {c[3] for c in PR.STEP_CASES.values()}
    assert {1, 64} <= he_set and any(c[4] == "graph" for c in PR.STEP_CASES.values()) and any(c[5] == "attention" for c in PR.STEP_CASES.values())


# ---- 5. the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_pdn_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"gcn\.py:71(?:(?!\*/).)*\*/\s*GCNX_API\s+(?:int|int64_t)\s+" + nm + r"\s*\(", hdr, re.S), nm   # its comment cites gcn.py:71
        assert nm in _lib.SIGNATURES, nm
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 425
    assert len(_lib.SIGNATURES["gcnx_pdn_operator"]) == 19 and len(_lib.SIGNATURES["gcnx_pdn_operator_bwd"]) == 25
    ok = lib.gcnx_pdn_ok
    assert ok(1, 1) and ok(8, 64) and ok(2, 16) and not ok(0, 16) and not ok(9, 16) and not ok(2, 0) and not ok(2, 65)
    sf = lib.gcnx_pdn_bwd_scratch_floats
    cols = lambda d, he: d * he + 2 * he + 1
    assert sf(10, 1, 2, 16) == 4 + cols(2, 16) and sf(10, 64, 2, 16) == 64 + cols(2, 16) and sf(10, 65, 2, 16) == 68 + 2 * cols(2, 16)
    assert sf(70, 64 * 256, 8, 64) == 64 * 256 + 256 * cols(8, 64)
    assert sf(70, 64 * 256 + 1, 8, 64) == 64 * 256 + 4 + 256 * cols(8, 64) and sf(10, 10 ** 7, 1, 1) == 10 ** 7 + 256 * 4   # never over 256 parts
    assert sf(10, 100, 9, 16) == 0 and sf(10, -1, 2, 16) == 0 and sf(0, 0, 2, 16) == cols(2, 16)


# ---- 6. exports, refusals, the state dict ----------------------------------------------------------------------------------------
def test_exports_and_constructor_refusals():
    import gcnx
    from gcnx import layers, models
    assert gcnx.PDN is models.PDN and gcnx.PDNConv is layers.PDNConv and {"PDN", "PDNConv"} <= set(gcnx.__all__)
    PDN = models.PDN
    with pytest.raises(NotImplementedError, match="edge_dim"):
        PDN(ctx=_HostContext(), edge_dim=None)
    for bad in (0, 9):
        with pytest.raises(NotImplementedError):
            PDN(ctx=_HostContext(), edge_dim=bad)
    for bad in (0, 65):
        with pytest.raises(NotImplementedError, match="edge_hidden"):
            PDN(ctx=_HostContext(), edge_hidden=bad)
    with pytest.raises(NotImplementedError):
        PDN(ctx=_HostContext(), num_classes=2)
    with pytest.raises(NotImplementedError, match="comm"):
        PDN(ctx=_HostContext(), comm=object())
    with pytest.raises(NotImplementedError):
        PDN(ctx=_HostContext(), readout="mean")
    m = PDN(ctx=_HostContext())
    assert (m.hidden, m.edge_dim, m.edge_hidden) == (64, 2, 16) and m.uses_edge_features and m.OPERATOR == "perm"
    with pytest.raises(ValueError):
        m.forward(np.zeros((4, 16), np.float32), np.zeros((2, 0), np.int64), np.zeros(4, np.int64))   # (x, a, i) for a model that reads e
    with pytest.raises(NotImplementedError):
        gcnx.Explainer(m)                                                                 # the explainer serves gcnx.GCN alone
    for kw in (dict(normalize=False), dict(edge_dim=None), dict(edge_dim=9), dict(hidden_channels=0), dict(hidden_channels=65)):
        with pytest.raises(NotImplementedError):
            layers.PDNConv(**{"channels": 8, "edge_dim": 2, "hidden_channels": 4, **kw})
    with pytest.raises(NotImplementedError):
        import scipy.sparse as sp
        layers.PDNConv(8, 2, 4, add_self_loops=False).preprocess(sp.identity(3, format="csr"), np.zeros((3, 2)))


@pytest.mark.parametrize("readout,norm", [("max", "batch"), ("attention", "graph")])
def test_state_dict_keys_shapes_initialisation_and_round_trip(readout, norm):
    from gcnx.layers import glorot_uniform
    from gcnx.models import GCN, PDN
    m = PDN(ctx=_HostContext(), hidden_channels=64, edge_dim=2, edge_hidden=16, seed=4, readout=readout, norm=norm)
    m.build(16)
    want = list(PR.keys(readout, norm))
    assert [k for k, _, _ in m.TORCH_KEYS] == want and want[12:12 + 4] == [k for k, _, _ in GCN.TORCH_KEYS[4:8]]
    sd = m.state_dict()
    assert list(sd) == want and len(m.get_weights()) == len(want)
    shapes = {"bias": (64,), "lin.weight": (64, None), "mlp.0.weight": (16, 2), "mlp.0.bias": (16,), "mlp.2.weight": (1, 16),
              "mlp.2.bias": (1,)}
    for k, f in ((1, 16), (2, 64)):
        for s, shp in shapes.items():
            assert sd[f"conv{k}.{s}"].shape == tuple(f if v is None else v for v in shp), (k, s)
            if s.endswith("bias"):
                assert not sd[f"conv{k}.{s}"].any()                                      # every bias starts at zero
    # the draw order: lin.weight, mlp.0.weight, mlp.2.weight per convolution, glorot-uniform
    rng = np.random.default_rng(4)
    for k, f in ((1, 16), (2, 64)):
        for s, (fi, fo) in (("lin.weight", (f, 64)), ("mlp.0.weight", (2, 16)), ("mlp.2.weight", (16, 1))):
            assert np.array_equal(sd[f"conv{k}.{s}"], glorot_uniform(rng, fi, fo).T), (k, s)
    assert all(off % 4 == 0 for off, _, _ in m.flat_p.views)                             # every tensor on a 16-byte boundary
    new = {k: np.random.default_rng(1).normal(size=v.shape).astype(np.float32) for k, v in sd.items()}
    m2 = PDN(ctx=_HostContext(), hidden_channels=64, edge_dim=2, edge_hidden=16, seed=9, readout=readout, norm=norm)
    m2.load_state_dict(new)
    back = m2.state_dict()
    assert list(back) == want and all(np.array_equal(back[k], new[k]) for k in want)
    assert np.array_equal(m2.p["pa1"].numpy(), new["conv1.mlp.0.weight"].T) and m2.p["pc2"].numpy().shape == (16, 1)
    with pytest.raises(KeyError):
        PDN(ctx=_HostContext(), readout=readout, norm=norm).load_state_dict({k: v for k, v in new.items() if k != "conv2.mlp.2.bias"})
    with pytest.raises(ValueError):
        PDN(ctx=_HostContext(), edge_hidden=8, readout=readout, norm=norm).load_state_dict(new)
    assert AR.GATE_KEY not in want or want[-1] == AR.GATE_KEY

"""CPU tests of the PNAConv feature (gcnx.PNAConv, gcnx.PNA): the float64 oracle (tests/pna_ref.py) pinned against a
plain-torch autograd restatement, the adjoint identity of the aggregate pair, the C ABI of the new entry points, and what the
model class promises without a device.  torch is imported inside the tests only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import pna_ref as PR


def _torch_model(x, a, gp, y, p, delta):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, a, gp, y, p, delta)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, a, gp, y, p, delta):
    """The model from torch.nn modules + a hand-written PyG PNAConv: messages pre_nn([x_i | x_j]) per edge, their mean and
    variance by index_add_, minimum and maximum by scatter_reduce("amin" / "amax", include_self=False) into zeros, the three
    degree scalers, post_nn and lin; scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.lin.bias"].shape[0]
    coo = a.tocoo()
    src, dst = torch.tensor(coo.col, dtype=torch.long), torch.tensor(coo.row, dtype=torch.long)   # row = target
    deg = torch.zeros(n).index_add_(0, dst, torch.ones(len(dst))).clamp(min=1)
    amp = (torch.log(deg + 1) / delta)[:, None]

    class Conv(torch.nn.Module):
        def __init__(self, fi, fo):
            super().__init__()
            self.pre_nns = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(2 * fi, fi))])
            self.post_nns = torch.nn.ModuleList([torch.nn.Sequential(torch.nn.Linear(13 * fi, fo))])
            self.lin = torch.nn.Linear(fo, fo)

        def forward(self, xx):
            w = xx.shape[1]
            msg = self.pre_nns[0](torch.cat([xx[dst], xx[src]], dim=-1))
            idx = dst[:, None].expand(-1, w)
            mean = torch.zeros(n, w).index_add_(0, dst, msg) / deg[:, None]
            var = torch.zeros(n, w).index_add_(0, dst, (msg - mean[dst]) ** 2) / deg[:, None]
            mn = torch.zeros(n, w).scatter_reduce(0, idx, msg, "amin", include_self=False)
            mx = torch.zeros(n, w).scatter_reduce(0, idx, msg, "amax", include_self=False)
            agg = torch.cat([mean, mn, mx, torch.sqrt(torch.relu(var) + 1e-5)], dim=-1)
            return self.lin(self.post_nns[0](torch.cat([xx, agg, amp * agg, agg / amp], dim=-1)))

    mods = {"conv1": Conv(f, h), "conv2": Conv(h, h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    assert list(named)[:12] == list(PR.CONV_KEYS) and set(named) == set(PR.KEYS)     # named_parameters() order inside the convs
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
    x, a, gp, y = PR.graphs(kind, n_graphs=8, f=16, seed=2 if kind == "directed" else 0)
    pat = a != 0
    d = np.diff(a.indptr)
    assert (d == 0).any() and (d == 1).any() and 1 in np.diff(gp)              # empty rows, d = 1 rows, a single-node graph
    assert len(np.unique(x, axis=0)) < x.shape[0]                             # duplicated feature rows
    assert ((pat != pat.T).nnz == 0) == (kind == "symmetric")
    delta = PR.avg_deg_log(np.bincount(d))
    p = PR.init_params(16, 24, seed=3)
    out_t, loss_t, g_t = _torch_model(x, a, gp, y, p, delta)
    r = PR.model(x, a, gp, p, delta, y)
    st, w = r["stats1"], 16                   # at least one tie of a minimum and of a maximum (layer 1: duplicated x rows)
    assert st[:, 4 * w:5 * w].max() >= 2 and st[:, 5 * w:6 * w].max() >= 2
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(PR.KEYS) == set(r["grads"])
    for k in PR.KEYS:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))


def _jv(rp, ci, pq, stats, v, delta):
    """The linearisation of pna_ref.aggregate with respect to pq along v, blocks 1 .. 12 (block 0 does not depend on pq); at a
    tie the tied entries' average, the subgradient the backward takes."""
    n, f = pq.shape[0], pq.shape[1] // 2
    Q, vP, vQ = pq[:, f:], v[:, :f], v[:, f:]
    mean, mn, mx, std, cmin, cmax = (stats[:, k * f:(k + 1) * f] for k in range(6))
    d = np.diff(rp)
    t = np.repeat(np.arange(n), d)
    qe, ve = Q[ci], vQ[ci]
    seg = lambda vals: PR._segsum(vals, t, n)
    dd, ne = np.maximum(d, 1)[:, None], (d > 0)[:, None]
    jm = ne * (vP + seg(ve) / dd)
    jmin = ne * (vP + seg(ve * (qe == mn[t])) / np.maximum(cmin, 1))
    jmax = ne * (vP + seg(ve * (qe == mx[t])) / np.maximum(cmax, 1))
    jstd = (mx > mn) * seg((qe - mean[t]) * ve) / (dd * std)
    A = np.concatenate([jm, jmin, jmax, jstd], axis=1)
    amp, att = PR.scalers(d, delta)
    return np.concatenate([A, amp[:, None] * A, att[:, None] * A], axis=1)


def test_bwd_is_the_adjoint_of_the_forward_linearisation():
    """<dc, J v> = <J^T dc, v> on a batch with ties, empty rows and d = 1 rows; without ties J v is also the finite difference
    of the forward."""
    x, a, gp, _ = PR.graphs("directed", n_graphs=6, f=8, seed=5)
    rp, ci = PR.pattern(a, x.shape[0])
    rng = np.random.default_rng(0)
    n, f, delta = x.shape[0], 8, 1.3
    pq = np.concatenate([rng.normal(size=(n, f)), x @ rng.normal(size=(f, f))], axis=1)      # Q from x: duplicated rows tie
    c, stats = PR.aggregate(rp, ci, x, pq, delta)
    d = np.diff(rp)
    assert stats[:, 4 * f:].max() >= 2 and (d == 0).any() and (d == 1).any()
    assert np.array_equal(c[d == 0, f:5 * f], np.tile(np.repeat([0.0, 0.0, 0.0, np.sqrt(1e-5)], f), ((d == 0).sum(), 1)))
    assert np.array_equal(stats[d == 1, 3 * f:4 * f], np.full(((d == 1).sum(), f), np.sqrt(1e-5)))
    dc, v = rng.normal(size=c.shape), rng.normal(size=pq.shape)
    dpq, big = PR.aggregate_bwd(rp, ci, pq, stats, dc, delta)
    lhs, rhs = np.sum(dc[:, f:] * _jv(rp, ci, pq, stats, v, delta)), np.sum(dpq * v)
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)
    assert np.all(big[:, :] >= 0) and np.all(dpq[d == 0, :f] == 0)
    # block 0 of dc is not read
    dc2 = dc.copy()
    dc2[:, :f] = 7.0
    assert np.array_equal(PR.aggregate_bwd(rp, ci, pq, stats, dc2, delta)[0], dpq)
    # no ties: the linearisation is the derivative
    pq = rng.normal(size=(n, 2 * f))
    c, stats = PR.aggregate(rp, ci, x, pq, delta)
    assert stats[:, 4 * f:].max() == 1
    e = 1e-6
    fd = (PR.aggregate(rp, ci, x, pq + e * v, delta)[0] - PR.aggregate(rp, ci, x, pq - e * v, delta)[0]) / (2 * e)
    jv = _jv(rp, ci, pq, stats, v, delta)
    assert np.max(np.abs(fd[:, f:] - jv)) <= 1e-6 * np.max(np.abs(jv))


def test_abi_declares_and_exports_the_pna_entry_points():
    import ctypes as C
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    names = ("gcnx_pna_aggregate", "gcnx_pna_bwd", "gcnx_pna_bwd_scratch_floats")
    for nm in names:
        assert re.search(r"GCNX_API\s+int\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 409
    nf = C.c_int64(-1)                                        # answers without a context
    assert lib.gcnx_pna_bwd_scratch_floats(1000, 64, C.byref(nf)) == 0 and nf.value == 4 * 1000 * 64
    assert lib.gcnx_pna_bwd_scratch_floats(2 ** 31, 128, C.byref(nf)) == 0 and nf.value == 4 * 2 ** 31 * 128
    assert lib.gcnx_pna_bwd_scratch_floats(10, 0, C.byref(nf)) != 0 and lib.gcnx_pna_bwd_scratch_floats(-1, 4, C.byref(nf)) != 0
    assert lib.gcnx_pna_bwd_scratch_floats(10, 4, None) != 0


def test_package_exports_the_new_names():
    import gcnx
    assert "PNAConv" in gcnx.__all__ and "PNA" in gcnx.__all__
    from gcnx.layers import PNAConv
    from gcnx.models import GCN, PNA
    assert gcnx.PNAConv is PNAConv and gcnx.PNA is PNA and issubclass(PNA, GCN) and PNA.uses_edge_features is False
    with pytest.raises(ValueError):
        PNAConv(64)                                           # neither deg nor avg_deg_log
    with pytest.raises(ValueError):
        PNAConv(64, deg=[0, 3, 2], avg_deg_log=1.0)           # both
    for kw in (dict(aggregators=["mean", "max"]), dict(scalers=["identity"]), dict(towers=2), dict(edge_dim=3), dict(train_norm=True),
               dict(aggregators=["min", "mean", "max", "std"]), dict(pre_layers=2), dict(post_layers=2), dict(divide_input=True)):
        with pytest.raises(NotImplementedError):
            PNAConv(64, avg_deg_log=1.0, **kw)
    lay = PNAConv(32, deg=[0, 3, 2], seed=1, aggregators=["mean", "min", "max", "std"], scalers=["identity", "amplification", "attenuation"])
    assert abs(lay.avg_deg_log - (3 * np.log(2) + 2 * np.log(3)) / 5) < 1e-15 and lay.channels == 32
    spec = lay._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("pre_nns.0.0.weight", (32, 16)), ("pre_nns.0.0.bias", (16,)), ("post_nns.0.0.weight", (208, 32)),
                                            ("post_nns.0.0.bias", (32,)), ("lin.weight", (32, 32)), ("lin.bias", (32,))]
    for (_, _, v), fan_in in zip(spec, (32, 32, 208, 208, 32, 32)):                   # U(+-1/sqrt(fan_in))
        assert v.dtype == np.float32 and np.max(np.abs(v)) <= 1 / np.sqrt(fan_in) and np.max(np.abs(v)) > 0.5 / np.sqrt(fan_in)
    spec = PNAConv(8, avg_deg_log=0.9, use_bias=False)._param_spec(4)
    assert [(n, s) for n, s, _ in spec] == [("pre_nns.0.0.weight", (8, 4)), ("post_nns.0.0.weight", (52, 8)), ("lin.weight", (8, 8))]


# ---- the model without a device -------------------------------------------------------------------------------------------
class _View:
    def __init__(self, shape):
        self.shape, self.host = shape, None

    def copy_from_host(self, host, wait=True):
        assert host.shape == tuple(self.shape)
        self.host = np.array(host)

    def numpy(self):
        return np.zeros(self.shape, np.float32) if self.host is None else self.host.copy()     # (ctx.zeros: never written)


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


def test_pna_constructor_refusals_and_keys():
    from gcnx.models import GCN, PNA
    with pytest.raises(NotImplementedError):
        PNA(num_classes=2, avg_deg_log=1.0)
    with pytest.raises(NotImplementedError):
        PNA(hidden_channels=64, avg_deg_log=1.0, comm=object())
    with pytest.raises(NotImplementedError):
        PNA(ctx=_RecordingContext(), hidden_channels=512, avg_deg_log=1.0).build(16)
    with pytest.raises(ValueError):
        PNA(ctx=_RecordingContext())
    with pytest.raises(ValueError):
        PNA(ctx=_RecordingContext(), deg=[1, 2], avg_deg_log=1.0)
    for kw in (dict(towers=4), dict(edge_dim=2), dict(train_norm=True), dict(aggregators=["sum"]), dict(scalers=["identity", "linear"])):
        with pytest.raises(NotImplementedError):
            PNA(ctx=_RecordingContext(), avg_deg_log=1.0, **kw)
    m = PNA(64, [0, 3, 2], ctx=_RecordingContext())                          # positional, as GCN(hidden_channels, ...)
    assert m.hidden == 64 and m.avg_deg_log == [PR.avg_deg_log([0, 3, 2])] * 2
    keys = [k for k, _, _ in m.TORCH_KEYS]
    assert keys == list(PR.KEYS) and keys[-16:] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
    assert {k: tr for k, _, tr in m.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in keys if k.startswith("conv")}
    assert sorted(k for _, k, _ in m.TORCH_KEYS) == sorted(m.PARAM_ORDER) and m.DELTA_KEYS == PR.DELTA_KEYS


def test_pna_state_dict_keys_order_and_the_constant():
    from gcnx.models import PNA
    m = PNA(ctx=_RecordingContext(), hidden_channels=8, avg_deg_log=1.25, seed=1)
    m.build(5)
    sd = m.state_dict()
    assert list(sd) == list(PR.STATE_KEYS)
    assert sd["conv1.pre_nns.0.0.weight"].shape == (5, 10) and sd["conv1.post_nns.0.0.weight"].shape == (8, 65)
    assert sd["conv2.pre_nns.0.0.weight"].shape == (8, 16) and sd["conv2.post_nns.0.0.weight"].shape == (8, 104)
    assert sd["conv1.lin.weight"].shape == (8, 8) and sd["conv1.pre_nns.0.0.bias"].shape == (5,)
    for dk in PR.DELTA_KEYS:                                  # a constant: in the state dict, not in the flat buffers
        assert sd[dk].shape == (1,) and sd[dk].dtype == np.float32 and sd[dk][0] == np.float32(1.25)
    assert not any("avg_deg_log" in tk for tk, _, _ in m.TORCH_KEYS) and len(m.get_weights()) == len(PR.KEYS)
    sd["conv2.aggr_module.avg_deg_log"] = np.array([0.75])
    m2 = PNA(ctx=_RecordingContext(), hidden_channels=8, avg_deg_log=2.0)
    m2.load_state_dict(sd)                                    # builds from pre_nns.0.0.weight [F, 2F]
    assert m2.f_in == 5 and m2.avg_deg_log == [1.25, 0.75]
    back = m2.state_dict()
    assert list(back) == list(sd) and all(np.array_equal(back[k], np.asarray(sd[k], np.float32)) for k in sd)
    del sd["conv1.lin.bias"]
    with pytest.raises(KeyError):
        m2.load_state_dict(sd)


def test_pna_flat_buffer_starts_every_tensor_on_four_floats():
    from gcnx.models import PNA
    ctx = _RecordingContext()
    m = PNA(ctx=ctx, hidden_channels=3, avg_deg_log=1.0)
    m.build(5)
    shapes = {"wpre1": (10, 5), "bpre1": (5,), "wpost1": (65, 3), "wlin1": (3, 3), "wpre2": (6, 3), "wpost2": (39, 3), "wlin2": (3, 3),
              "w3": (3, 3), "w4": (1, 3)}
    shapes.update({k: (3,) for k in ("bpost1", "blin1", "g1", "be1", "bpre2", "bpost2", "blin2", "g2", "be2", "b3", "g3", "be3")})
    shapes.update({k: (1,) for k in ("a1", "a2", "a3", "b4", "g4", "be4", "a4")})
    order = ["wpre1", "bpre1", "wpost1", "bpost1", "wlin1", "blin1", "g1", "be1", "a1",
             "wpre2", "bpre2", "wpost2", "bpost2", "wlin2", "blin2", "g2", "be2", "a2",
             "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4"]
    assert list(m.PARAM_ORDER) == order
    offsets, off = {}, 0
    for k in order:
        offsets[k] = off
        off += -(-int(np.prod(shapes[k])) // 4) * 4
    assert all(o % 4 == 0 for o in offsets.values())
    want = [(offsets[k], int(np.prod(shapes[k])), shapes[k]) for k in order]
    assert m.flat_p is ctx.buffers[0] and m.flat_g is ctx.buffers[1] and m.n_params == off
    assert [b.size for b in ctx.buffers] == [off, off + 2]                    # avg_deg_log lives in no device buffer
    assert sorted(m.flat_p.views) == sorted(want)                              # every parameter, nothing else
    assert sorted(m.flat_g.views) == sorted(want + [(off, 2, (2,))])           # the same places, then (loss sum, correct count)
    assert set(m.p) == set(m.g) == set(order) and all(m.p[k].shape == shapes[k] for k in order)


def test_degree_histogram_and_delta_on_a_hand_made_case():
    import scipy.sparse as sp
    from gcnx.models import PNA

    class G:
        def __init__(self, a):
            self.a = a
    a1 = sp.csr_matrix(np.array([[0, 1, 1], [0, 0, 0], [1, 0, 0]], float))    # rows with 2, 0 and 1 stored entries
    a2 = np.array([[1, 1, 1, 1], [0, 0, 0, 2], [0, 0, 0, 0], [0, 3, 0, 0]], float)   # 4, 1, 0, 1
    hist = PNA.degree_histogram([G(a1), a2])
    assert hist.dtype == np.int64 and hist.tolist() == [2, 3, 1, 0, 1]
    delta = (3 * np.log(2) + np.log(3) + np.log(5)) / 7
    assert abs(PR.avg_deg_log(hist) - delta) < 1e-15
    assert abs(PNA(ctx=_RecordingContext(), deg=hist).avg_deg_log[0] - delta) < 1e-15
    assert PNA.degree_histogram([]).tolist() == [0]
    with pytest.raises(ValueError):
        PNA(ctx=_RecordingContext(), deg=[5])                                 # only nodes without entries: delta = 0

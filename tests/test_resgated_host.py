"""CPU tests of the ResGatedGraphConv feature (gcnx.ResGatedGraphConv, gcnx.ResGated): the float64 oracle (tests/resgated_ref.py)
pinned against a plain-torch autograd restatement of PyG's message(), the adjoint identity between the two backward passes, the C
ABI of the new entry points, and what the model and layer classes promise without a device.  torch is imported inside the tests
only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import resgated_ref as RG
from test_gat_host import _graphs


def _edge_features(nnz, d, seed):
    return np.random.default_rng(seed).uniform(0, 1, (nnz, d)) if d else None


def _torch_model(x, rp, ci, e, gp, y, p, root_weight):
    import torch
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return _torch_model64(torch, x, rp, ci, e, gp, y, p, root_weight)
    finally:
        torch.set_default_dtype(prev)


def _torch_model64(torch, x, rp, ci, e, gp, y, p, root_weight):
    """The model from torch.nn modules + a literal restatement of PyG's ResGatedGraphConv.message(): k_i, q_j and v_j are
    cat([x, e]) through three torch.nn.Linear(in + D, out), the gated messages are summed over the targets by index_add_,
    lin_skip(x) and bias are added; scatter_reduce("amax") for global_max_pool; BCEWithLogitsLoss."""
    F = torch.nn.functional
    n, f = x.shape
    h = p["conv1.bias"].shape[0]
    src = torch.tensor(ci, dtype=torch.long)                                                   # row = target
    dst = torch.tensor(np.repeat(np.arange(n), np.diff(rp)), dtype=torch.long)
    et = None if e is None else torch.tensor(e)
    d = 0 if e is None else e.shape[1]

    class Conv(torch.nn.Module):
        def __init__(self, fi):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(h))
            self.lin_key = torch.nn.Linear(fi + d, h)
            self.lin_query = torch.nn.Linear(fi + d, h)
            self.lin_value = torch.nn.Linear(fi + d, h)
            if root_weight:
                self.lin_skip = torch.nn.Linear(fi, h, bias=False)

        def forward(self, xx):
            k_i, q_j, v_j = xx[dst], xx[src], xx[src]
            if et is not None:
                k_i, q_j, v_j = (torch.cat([t, et], dim=-1) for t in (k_i, q_j, v_j))
            msg = torch.sigmoid(self.lin_key(k_i) + self.lin_query(q_j)) * self.lin_value(v_j)
            out = torch.zeros(n, h).index_add_(0, dst, msg)
            if root_weight:
                out = out + self.lin_skip(xx)
            return out + self.bias

    mods = {"conv1": Conv(f), "conv2": Conv(h), "linear_1": torch.nn.Linear(h, h), "linear_2": torch.nn.Linear(h, 1)}
    for k in range(1, 5):
        mods[f"prelu_{k}"] = torch.nn.PReLU()
        mods[f"batch_norm_{k}"] = torch.nn.BatchNorm1d(h if k < 4 else 1, track_running_stats=False, momentum=None)
    net = torch.nn.ModuleDict(mods)
    named = dict(net.named_parameters())
    want = RG.keys(root_weight)
    assert set(named) == set(want)
    assert [k for k in named if k.startswith("conv")] == [k for k in want if k.startswith("conv")]    # bias, lin_key, lin_query, lin_value, lin_skip
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


@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("edge_dim", [0, 2])
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
def test_oracle_matches_torch_autograd(kind, edge_dim, root_weight):
    """Pins the split W[:, :in] / W[:, in:] of the three Linears and dW_ke == dW_qe: torch's gradients of lin_key.weight and
    lin_query.weight differ in their node blocks and agree in their edge blocks."""
    x, a, gp, y = _graphs(kind, seed=2 if kind == "directed" else 0)
    pat = a != 0
    if kind == "directed":
        assert (pat != pat.T).nnz > 0 and (np.diff(a.indptr) == 0).any()                      # rows without entries: lin_skip(x) + bias
    rp, ci, _ = RG.stored_pattern(a)
    e = _edge_features(len(ci), edge_dim, 11)
    p = RG.init_params(16, 64, edge_dim or None, root_weight, seed=3)
    assert p["conv1.lin_key.weight"].shape == (64, 16 + edge_dim) and p["conv2.lin_value.weight"].shape == (64, 64 + edge_dim)
    assert ("conv1.lin_skip.weight" in p) == root_weight
    out_t, loss_t, g_t = _torch_model(x, rp, ci, e, gp, y, p, root_weight)
    r = RG.model(x, rp, ci, e, gp, p, y, edge_dim=edge_dim or None)
    assert np.max(np.abs(r["out"] - out_t)) <= 1e-10 * max(1.0, np.max(np.abs(out_t)))
    assert abs(r["loss"] - loss_t) <= 1e-10
    assert set(g_t) == set(RG.keys(root_weight)) == set(r["grads"])
    for k in g_t:
        ref = g_t[k].reshape(r["grads"][k].shape)
        assert np.max(np.abs(r["grads"][k] - ref)) <= 1e-10 * max(1e-3, np.max(np.abs(ref))), k
    assert r["hits"] == np.sum((out_t[:, 0] > 0) == (y[:, 1] > 0.5))
    for k in (1, 2):
        gk, gq = g_t[f"conv{k}.lin_key.weight"], g_t[f"conv{k}.lin_query.weight"]
        f = gk.shape[1] - edge_dim
        assert not np.allclose(gk[:, :f], gq[:, :f])
        if edge_dim:
            assert np.max(np.abs(gk[:, f:] - gq[:, f:])) <= 1e-12 * np.max(np.abs(gk[:, f:]))
            assert np.array_equal(r["grads"][f"conv{k}.lin_key.weight"][:, f:], r["grads"][f"conv{k}.lin_query.weight"][:, f:])


@pytest.mark.parametrize("edge_dim", [0, 2])
def test_targets_and_sources_passes_are_adjoint_on_a_directed_pattern(edge_dim):
    """conv_bwd is the adjoint of the Jacobian of conv_fwd, operand by operand: <dout, J v> = <J^T dout, v>, J v by a central
    difference in float64 (step 1e-6), agreement 1e-6 relative.  dK comes from the pass over the targets, dQ | dV from the pass
    over the sources: on a non-symmetric pattern a pass that walked the wrong pattern fails here.  A row without entries gives
    skip + bias exactly and dK = 0."""
    x, a, _, _ = _graphs("directed", n_graphs=4, seed=5)
    rp, ci, _ = RG.stored_pattern(a)
    n, H, step = x.shape[0], 8, 1e-6
    empty = np.diff(rp) == 0
    assert empty.any() and ((a != 0) != (a != 0).T).nnz > 0
    rng = np.random.default_rng(10 * edge_dim + 1)
    e = _edge_features(len(ci), edge_dim, 13)
    names = ["P", "skip", "bias"] + (["We"] if edge_dim else [])
    base = [rng.normal(size=(n, 3 * H)), rng.normal(size=(n, H)), rng.normal(size=H)] + ([rng.normal(size=(edge_dim, 3 * H)) / 2] if edge_dim else [])

    def fwd(ops):
        return RG.conv_fwd(rp, ci, ops[0], H, e, ops[3] if edge_dim else None, ops[1], ops[2])

    out, cache = fwd(base)
    assert np.array_equal(out[empty], base[1][empty] + base[2])
    dout = rng.normal(size=out.shape)
    r = RG.conv_bwd(cache, dout)
    assert not r["dK"][empty].any() and np.array_equal(r["dS"], dout)
    grads = [np.hstack([r["dK"], r["dQ"], r["dV"]]), r["dS"], r["dbias"]] + ([r["dWe"]] if edge_dim else [])
    if edge_dim:
        assert np.array_equal(r["dWe"][:, :H], r["dWe"][:, H:2 * H])
    v = [rng.normal(size=t.shape) for t in base]
    for i, k in enumerate(names):
        vs = [d if j == i else np.zeros_like(d) for j, d in enumerate(v)]
        plus, minus = fwd([t + step * d for t, d in zip(base, vs)])[0], fwd([t - step * d for t, d in zip(base, vs)])[0]
        lhs, rhs = np.sum(dout * (plus - minus) / (2 * step)), np.sum(grads[i] * v[i])
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)
    # dQ and dV, one column block at a time (a sources pass that wrote dV into dQ's place would pass the sum over P)
    for blk in range(3):
        d = np.zeros_like(base[0])
        d[:, blk * H:(blk + 1) * H] = v[0][:, blk * H:(blk + 1) * H]
        vs = [d] + [np.zeros_like(t) for t in base[1:]]
        plus, minus = fwd([t + step * w for t, w in zip(base, vs)])[0], fwd([t - step * w for t, w in zip(base, vs)])[0]
        lhs, rhs = np.sum(dout * (plus - minus) / (2 * step)), np.sum(grads[0] * d)
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (blk, lhs, rhs)


def test_sigmoid_of_the_oracle_saturates_without_nan():
    g = RG.sigmoid(np.array([-800.0, -200.0, 0.0, 200.0, 800.0]))
    assert np.isfinite(g).all() and g[0] == 0.0 and g[2] == 0.5 and g[4] == 1.0 and np.isfinite(g * (1 - g)).all()


ERR_INVALID = 1                       # GCNX_ERR_INVALID (include/gcnx.h)
NAMES = ("gcnx_resgated_conv_ok", "gcnx_resgated_aggregate", "gcnx_resgated_bwd_targets", "gcnx_resgated_bwd_sources",
         "gcnx_resgated_bwd_scratch_floats")


def test_abi_declares_and_exports_the_resgated_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 410


def test_bwd_scratch_floats_answers_and_refuses_without_a_context():
    from gcnx import _lib
    fn = _lib.load().gcnx_resgated_bwd_scratch_floats
    out = ctypes.c_int64(-7)
    assert fn(1659, 64, 2, ctypes.byref(out)) == _lib.OK and out.value >= 2 * 2 * 64 * -(-1659 // 32)
    assert fn(1659, 128, 8, ctypes.byref(out)) == _lib.OK and out.value >= 2 * 8 * 128 * -(-1659 // 32)
    assert fn(1659, 64, 0, ctypes.byref(out)) == _lib.OK and out.value == 0            # no edge features: no parts
    assert fn(0, 64, 2, ctypes.byref(out)) == _lib.OK and out.value == 0
    out.value = -7
    for args in ((10, 0, 2), (10, -16, 2), (-1, 64, 2), (10, 64, -1)):
        assert fn(*args, ctypes.byref(out)) == ERR_INVALID and out.value == -7, args
    assert fn(10, 64, 2, None) == ERR_INVALID


def test_resgated_conv_ok_truth_table():
    from gcnx import _lib
    ok = _lib.load().gcnx_resgated_conv_ok                   # answers without a context
    for n, h, ld, d in ((1000, 16, 48, 0), (1000, 32, 128, 2), (1000, 64, 256, 8), (1000, 128, 384, 1), (1000, 64, 192, 0),
                        (1000, 16, 52, 2), (0, 16, 48, 0)):
        assert ok(n, h, ld, d) == 1, (n, h, ld, d)
    for n, h, ld, d in ((1000, 64, 256, 9), (1000, 64, 256, -1),     # edge_dim 9, negative
                        (1000, 8, 32, 0), (1000, 48, 192, 0), (1000, 96, 384, 0), (1000, 256, 1024, 0), (1000, 0, 64, 0),   # h
                        (1000, 64, 128, 0), (1000, 64, 188, 0),      # ldp < 3 h
                        (1000, 16, 50, 0),                           # ldp % 4
                        (-1, 64, 256, 0)):
        assert ok(n, h, ld, d) == 0, (n, h, ld, d)
    assert ok(2 ** 24, 16, 64, 0) == 0 and ok(2 ** 24 - 1, 16, 64, 0) == 1             # n * ldp * 4 reaches 2^32 / stays below


# ---- the model and the layer without a device ----------------------------------------------------------------------------------
class _View:
    """A view of a recording buffer: its place (off, n, shape), column and flat sub-views, what was copied into it."""

    def __init__(self, shape):
        self.shape, self.host = tuple(shape), None

    def copy_from_host(self, host, wait=True):
        assert np.shape(host) == self.shape, (np.shape(host), self.shape)
        self.host = np.array(host, np.float32)

    def numpy(self):
        return np.zeros(self.shape, np.float32) if self.host is None else self.host.copy()     # (ctx.zeros: never written)

    def cols(self, c0, c1):
        return _Sub(self, lambda t: t[:, c0:c1], (self.shape[0], c1 - c0))

    def flat(self, off, n, shape=None):
        return _Sub(self, lambda t: t.reshape(-1)[off:off + n].reshape(shape or (n,)), shape or (n,))


class _Sub:
    def __init__(self, base, cut, shape):
        self.base, self.cut, self.shape = base, cut, tuple(shape)

    def numpy(self):
        return self.cut(self.base.numpy()).copy()


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


def test_package_exports_the_new_names():
    import gcnx
    assert "ResGatedGraphConv" in gcnx.__all__ and "ResGated" in gcnx.__all__
    assert gcnx.ResGatedGraphConv is gcnx.layers.ResGatedGraphConv and gcnx.ResGated is gcnx.models.ResGated


def test_resgated_constructor_refusals_and_keys():
    from gcnx.models import GATv2, GCN, ResGated
    with pytest.raises(NotImplementedError):
        ResGated(num_classes=2)
    with pytest.raises(NotImplementedError):
        ResGated(hidden_channels=64, comm=object())
    for kw in (dict(hidden_channels=8), dict(hidden_channels=96), dict(hidden_channels=256), dict(edge_dim=9), dict(edge_dim=0)):
        with pytest.raises(NotImplementedError):
            ResGated(**kw)
    assert issubclass(ResGated, GCN) and not issubclass(ResGated, GATv2)
    nodev = object()                                            # stands in for the context: nothing here touches a device
    assert ResGated(ctx=nodev, edge_dim=2).uses_edge_features is True and ResGated(ctx=nodev).uses_edge_features is False
    for d in (None, 2):
        for root in (True, False):
            m = ResGated(ctx=nodev, hidden_channels=64, edge_dim=d, root_weight=root)
            keys = [k for k, _, _ in m.TORCH_KEYS]
            assert keys == list(RG.keys(root))
            parts = RG.CONV_PARTS if root else RG.CONV_PARTS[:-1]
            assert keys[:2 * len(parts)] == [f"conv{k}.{t}" for k in (1, 2) for t in parts]
            assert keys[2 * len(parts):] == [k for k, _, _ in GCN.TORCH_KEYS[4:]]
            assert {k: tr for k, _, tr in m.TORCH_KEYS if k.startswith("conv")} == {k: k.endswith("weight") for k in keys if k.startswith("conv")}
            # one stacked weight, one stacked bias (the zero bias of the S block behind it) and one edge weight per convolution
            want = ["b1", "w1", "lb1"] + (["lz1"] if root else []) + (["we1"] if d else [])
            assert [k for k in m.PARAM_ORDER if k.endswith("1") and k not in ("g1", "be1", "a1")] == want
            s = m._shapes(16)
            w = 256 if root else 192
            assert s["w1"] == (16, w) and s["w2"] == (64, w) and s["lb1"] == (192,) and s["lz2"] == (64,) and s["we2"] == (d or 0, 192)
    for phrase in ("named dicts", "not a live module", "as stored", "dW_ke"):
        assert phrase in ResGated.__doc__


def test_layer_refusals_param_spec_and_init_bounds():
    from gcnx.layers import ResGatedGraphConv
    for kw, word in ((dict(act="relu"), "act"), (dict(act=None), "act"), (dict(activation="relu"), "activation"), (dict(edge_dim=9), "edge_dim"),
                     (dict(edge_dim=0), "edge_dim")):
        with pytest.raises(NotImplementedError) as err:
            ResGatedGraphConv(64, **kw)
        assert word in str(err.value)
    for ch in (8, 24, 96, 256):
        with pytest.raises(NotImplementedError) as err:
            ResGatedGraphConv(ch)
        assert "channels" in str(err.value)
    with pytest.raises(NotImplementedError) as err:
        ResGatedGraphConv(16)([(object(), object()), object()])                 # bipartite (x_source, x_target)
    assert "bipartite" in str(err.value)
    spec = ResGatedGraphConv(64, edge_dim=2, seed=1)._param_spec(16)
    assert [(n, s) for n, s, _ in spec] == [("bias", (64,)), ("lin_key.weight", (64, 18)), ("lin_key.bias", (64,)),
                                            ("lin_query.weight", (64, 18)), ("lin_query.bias", (64,)), ("lin_value.weight", (64, 18)),
                                            ("lin_value.bias", (64,)), ("lin_skip.weight", (64, 16))]
    init = {n: v for n, _, v in spec}
    assert all(v.shape == s and v.dtype == np.float32 for _, s, v in spec)
    assert not init["bias"].any()                                               # the conv bias starts at zero
    for k in ("lin_key", "lin_query", "lin_value"):                             # torch's Linear: U(+-1 / sqrt(fan_in)), fan_in = in + D
        for t in (".weight", ".bias"):
            top = np.max(np.abs(init[k + t]))
            assert 0.8 / np.sqrt(18) < top <= 1 / np.sqrt(18), (k + t, top)
    top = np.max(np.abs(init["lin_skip.weight"]))
    assert 1 / np.sqrt(18) < top <= 1 / np.sqrt(16)                             # fan_in = in
    assert not np.array_equal(init["lin_key.weight"], init["lin_query.weight"])
    assert [n for n, _, _ in ResGatedGraphConv(64, root_weight=False, use_bias=False)._param_spec(16)] == [
        "lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias"]
    # the named tensors, and with root_weight the zero bias of the S block
    assert ResGatedGraphConv(32, edge_dim=3).n_params(8) == 32 + 3 * (32 * 11 + 32) + 32 * 8 + 32
    assert ResGatedGraphConv(32, root_weight=False).n_params(8) == 32 + 3 * (32 * 8 + 32)


@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("edge_dim", [None, 2])
def test_state_dict_keys_order_shapes_and_round_trip(edge_dim, root_weight):
    from gcnx.models import ResGated
    d = edge_dim or 0
    m = ResGated(ctx=_RecordingContext(), hidden_channels=16, edge_dim=edge_dim, root_weight=root_weight, seed=1)
    m.build(5)
    sd = m.state_dict()
    assert list(sd) == list(RG.keys(root_weight))
    for k, f in ((1, 5), (2, 16)):
        for s in RG.LINS:
            assert sd[f"conv{k}.{s}.weight"].shape == (16, f + d) and sd[f"conv{k}.{s}.bias"].shape == (16,)
            top = np.max(np.abs(sd[f"conv{k}.{s}.weight"]))
            assert 0 < top <= 1 / np.sqrt(f + d)                               # U(+-1 / sqrt(fan_in)), node and edge block alike
        assert sd[f"conv{k}.bias"].shape == (16,) and not sd[f"conv{k}.bias"].any()
        assert (f"conv{k}.lin_skip.weight" in sd) == root_weight
        if root_weight:
            assert sd[f"conv{k}.lin_skip.weight"].shape == (16, f)
    assert len(m.get_weights()) == len(RG.keys(root_weight))
    # a checkpoint in PyG's layout: the joined [H, in + D] tensors are split on load and joined again on save
    p = {k: v.astype(np.float32) for k, v in RG.init_params(5, 16, edge_dim, root_weight, seed=9).items()}
    m2 = ResGated(ctx=_RecordingContext(), hidden_channels=16, edge_dim=edge_dim, root_weight=root_weight)
    m2.load_state_dict(p)                                                       # builds from conv1.lin_key.weight [H, F + D]
    assert m2.f_in == 5
    back = m2.state_dict()
    assert list(back) == list(p) and all(np.array_equal(back[k], p[k]) for k in p)
    # the stored form: node blocks side by side, edge blocks side by side
    W1, b1, We1, bias1, root = RG.split(p, 1, edge_dim)
    assert root == root_weight and np.array_equal(m2.p["w1"].numpy(), W1.astype(np.float32)) and np.array_equal(m2.p["lb1"].numpy(), b1.astype(np.float32))
    assert m2.p["w2"].shape == (16, 64 if root_weight else 48)
    if edge_dim:
        assert np.array_equal(m2.p["we1"].numpy(), We1.astype(np.float32)) and m2.p["we2"].shape == (2, 48)
    g = m2.gradients()
    assert list(g) == list(p) and all(g[k].shape == p[k].shape for k in p)
    del p["conv1.lin_query.bias"]
    with pytest.raises(KeyError):
        m2.load_state_dict(p)
    p = {k: v.astype(np.float32) for k, v in RG.init_params(5, 16, edge_dim, root_weight, seed=9).items()}
    p["conv2.lin_value.weight"] = p["conv2.lin_value.weight"][:, :-1]
    with pytest.raises(ValueError):
        m2.load_state_dict(p)


@pytest.mark.parametrize("root_weight", [True, False])
def test_flat_buffer_starts_every_tensor_on_four_floats(root_weight):
    from gcnx.models import ResGated
    ctx = _RecordingContext()
    m = ResGated(ctx=ctx, hidden_channels=16, edge_dim=3, root_weight=root_weight)
    m.build(5)
    w = 64 if root_weight else 48
    shapes = {"b1": (16,), "w1": (5, w), "lb1": (48,), "lz1": (16,), "we1": (3, 48), "b2": (16,), "w2": (16, w), "lb2": (48,), "lz2": (16,),
              "we2": (3, 48), "w3": (16, 16), "w4": (1, 16)}
    shapes.update({k: (16,) for k in ("g1", "be1", "g2", "be2", "b3", "g3", "be3")})
    shapes.update({k: (1,) for k in ("a1", "a2", "a3", "b4", "g4", "be4", "a4")})
    conv = lambda k: [f"b{k}", f"w{k}", f"lb{k}"] + ([f"lz{k}"] if root_weight else []) + [f"we{k}"]
    order = conv(1) + conv(2) + ["g1", "be1", "a1", "g2", "be2", "a2", "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4"]
    assert list(m.PARAM_ORDER) == order
    offsets, off = {}, 0
    for k in order:
        offsets[k] = off
        off += -(-int(np.prod(shapes[k])) // 4) * 4
    assert all(o % 4 == 0 for o in offsets.values())
    want = [(offsets[k], int(np.prod(shapes[k])), shapes[k]) for k in order]
    # the bias of the one product: the stacked bias and the zero bias of the S block behind it, ONE run of floats
    prod_bias = [(offsets[f"lb{k}"], w, (w,)) for k in (1, 2)]
    if root_weight:
        assert all(offsets[f"lz{k}"] == offsets[f"lb{k}"] + 48 for k in (1, 2))
    assert m.flat_p is ctx.buffers[0] and m.flat_g is ctx.buffers[1] and m.n_params == off
    assert [b.size for b in ctx.buffers] == [off, off + 2]
    assert sorted(m.flat_p.views) == sorted(want + prod_bias)                  # every parameter, the product's bias, nothing else
    assert sorted(m.flat_g.views) == sorted(want + [(off, 2, (2,))])           # the same places, then (loss sum, correct count)
    assert all(not m.p[f"lz{k}"].numpy().any() for k in (1, 2) if root_weight)  # never initialised away from zero

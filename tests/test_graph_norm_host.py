"""CPU tests of GraphNorm (gcnx.GraphNorm, norm="graph"): the float64 oracle tests/graph_norm_ref.py against torch-CPU autograd of
a plain-torch restatement of PyG's forward, the C ABI of the new entry points, and what the layer and the models of the GCN
family promise without a device.  torch is imported inside the test only."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import graph_norm_ref as GN
from test_conv_family_host import CONFIGS, GOLDEN, _HostContext, _built, _init_record, _new, _sha

NEW = ("gcnx_graph_norm_scratch_floats", "gcnx_graph_norm_act", "gcnx_graph_norm_act_bwd")
SIZES = [1, 0, 3, 65, 64, 130]
MS = ("batch_norm_1.mean_scale", "batch_norm_2.mean_scale")


@pytest.mark.parametrize("slope", [None, 0.25])
def test_oracle_equals_torch_autograd(slope):
    import torch
    rng = np.random.default_rng(0)
    f = 16
    gp = np.concatenate([[0], np.cumsum(SIZES)])
    n, b = int(gp[-1]), len(SIZES)
    z, dy = rng.normal(size=(n, f)), rng.normal(size=(n, f))
    a, gamma, beta = rng.uniform(0.5, 1.5, f), rng.uniform(0.5, 1.5, f), rng.normal(size=f)
    assert np.min(np.abs(a - 1)) > 0
    t64 = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
    tz, ta, tg, tb, ts = t64(z), t64(a), t64(gamma), t64(beta), t64(np.array([slope or 0.0]))
    batch = torch.tensor(np.repeat(np.arange(b), np.diff(gp)))
    # torch_geometric.nn.GraphNorm.forward: mean = scatter(x, batch, reduce="mean"); out = x - mean[batch] * mean_scale;
    # var = scatter(out^2, batch, reduce="mean"); return weight * out / (var + eps).sqrt()[batch] + bias
    cnt = torch.zeros(b, dtype=torch.float64).index_add_(0, batch, torch.ones(n, dtype=torch.float64)).clamp(min=1)[:, None]
    mean = torch.zeros(b, f, dtype=torch.float64).index_add(0, batch, tz) / cnt
    out = tz - mean[batch] * ta
    var = torch.zeros(b, f, dtype=torch.float64).index_add(0, batch, out * out) / cnt
    t = tg * out / (var + 1e-5).sqrt()[batch] + tb
    ty = t if slope is None else torch.where(t > 0, t, ts * t)
    (ty * torch.tensor(dy)).sum().backward()
    y, c = GN.forward(z, gp, a, gamma, beta, slope)
    dz, dg, db, da, ds = GN.backward(dy, z, gp, a, gamma, beta, slope)
    err = lambda u, v: float(np.max(np.abs(u - v.detach().numpy())))
    assert err(y, ty) < 1e-12 and err(c["mean"], mean) < 1e-12
    full = np.diff(gp) > 0
    assert err(c["inv"][full], 1.0 / (var + 1e-5).sqrt()[torch.tensor(full)]) < 1e-9
    assert err(dz, tz.grad) < 1e-11 and err(dg, tg.grad) < 1e-11 and err(db, tb.grad) < 1e-11 and err(da, ta.grad) < 1e-11
    if slope is not None:
        assert err(ds, ts.grad) < 1e-11
    else:
        assert not ds.any()
    assert not c["mean"][1].any() and not c["inv"][1].any()                  # the empty graph
    # the one-row graph: o = (1 - a) z, and y = beta exactly at a = 1
    y1, _ = GN.forward(z, gp, np.ones(f), gamma, beta)
    assert np.array_equal(y1[0], beta)


def test_fp32_two_pass_variance_holds_where_the_moment_form_fails():
    """The case of tests/test_gpu_graph_norm.py::test_the_variance_is_centred, restated in fp32 on the host: the centred second
    pass stays within 2e-5 of float64, E[z^2] - mu^2 does not."""
    rng = np.random.default_rng(3)
    gp = np.concatenate([[0], np.cumsum(SIZES)])
    n, f = int(gp[-1]), 16
    z = (256 + rng.integers(-32, 33, size=(n, f)) / 8).astype(np.float32)
    one, zero = np.ones(f), np.zeros(f)
    want, _ = GN.forward(z, gp, one, one, zero)
    two, mom = np.zeros_like(z), np.zeros_like(z)
    eps = np.float32(1e-5)
    for g in range(len(gp) - 1):
        lo, hi = gp[g], gp[g + 1]
        if hi == lo:
            continue
        m = np.float32(hi - lo)
        mu = z[lo:hi].sum(0, dtype=np.float32) / m
        o = z[lo:hi] - mu
        two[lo:hi] = o / np.sqrt((o * o).sum(0, dtype=np.float32) / m + eps)
        v = np.maximum((z[lo:hi] * z[lo:hi]).sum(0, dtype=np.float32) / m - mu * mu, np.float32(0))
        mom[lo:hi] = o / np.sqrt(v + eps)
    scale = np.max(np.abs(want))
    assert np.max(np.abs(two - want)) / scale < 2e-5 < np.max(np.abs(mom - want)) / scale


def test_new_entry_points_are_declared_listed_and_exported():
    from gcnx import _lib
    header = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for name in NEW:
        assert re.search(r"GCNX_API\s+[\w\s\*]+\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    assert "gcn_utills.py:816-826" in header[header.index("gcnx_graph_norm_scratch_floats") - 400:]
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name
    lib = _lib.load()
    assert lib.gcnx_version() >= 422
    # the scratch answer needs no context: three partial rows per slot (the backward's; the forward uses two)
    sf = lib.gcnx_graph_norm_scratch_floats
    assert sf(0, 3, 16, 0) == 0 and sf(100, 0, 16, 0) == 0 and sf(100, 3, 16, -1) == 0
    assert sf(1659, 3, 16, 7) == 3 * 240 * 16                                # 1659 // 7 + 3 slots
    assert sf(1659, 3, 10, 7) == 3 * 240 * 12                                # partial rows on a 4-float stride
    assert sf(1659, 3, 16, 0) == 3 * (1659 // 64 + 3) * 16                   # the library's slices are at least 64 rows


def test_layer_is_exported_and_has_pygs_parameters():
    import gcnx
    from gcnx import layers
    assert "GraphNorm" in gcnx.__all__ and gcnx.GraphNorm is layers.GraphNorm
    layer = layers.GraphNorm()
    assert layer.eps == 1e-5 and layers.GraphNorm(eps=1e-3).eps == 1e-3
    spec = layer._param_spec(24)
    assert [(n, s) for n, s, _ in spec] == [("weight", (24,)), ("bias", (24,)), ("mean_scale", (24,))]
    assert all(v.dtype == np.float32 for _, _, v in spec)
    assert (spec[0][2] == 1).all() and (spec[1][2] == 0).all() and (spec[2][2] == 1).all()
    layer.build(_HostContext(), 24)
    assert list(layer.params) == list(layer.grads) == ["weight", "bias", "mean_scale"]
    assert [w.shape for w in layer.get_weights()] == [(24,)] * 3


def _golden(name):
    with open(GOLDEN) as fh:
        return json.load(fh)[name]


def _record(name, **extra):
    cls, kw = CONFIGS[name]
    m = _new(cls, 16, seed=0, **extra, **kw)
    m.build(5)
    rec = {"n_params": int(m.n_params), "flat_p": _sha(m.flat_p.numpy()), "p": {}}
    for k, v in m.p.items():
        rec["p"][k] = {"offset": int(v.offset), "shape": list(v.shape), "uploaded": None if v.uploaded is None else _sha(v.uploaded)}
    return m, rec


@pytest.mark.parametrize("name", list(CONFIGS))
def test_norm_batch_is_the_model_as_it_was(name):
    want = _golden(name)
    m, got = _record(name, norm="batch")
    assert got == want == _init_record(name)
    assert m.norm == "batch" and _built(name).norm == "batch"
    assert "ms1" not in m.p and not set(MS) & set(m.state_dict())
    assert m.PARAM_ORDER == _built(name).PARAM_ORDER and m.TORCH_KEYS == _built(name).TORCH_KEYS


@pytest.mark.parametrize("readout", ["max", "attention"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_norm_graph_adds_two_tensors_behind_the_class_list(name, readout):
    want = _golden(name)
    plain = _record(name, readout=readout)[0]
    m, got = _record(name, norm="graph", readout=readout)
    gate = ("ar",) if readout == "attention" else ()
    assert tuple(m.PARAM_ORDER) == tuple(_built(name).PARAM_ORDER) + ("ms1", "ms2") + gate
    assert set(got["p"]) == set(want["p"]) | {"ms1", "ms2"} | set(gate)
    for k in want["p"]:                                                      # every existing view keeps its offset and its bits
        assert got["p"][k] == want["p"][k], (name, k)
    for k in ("ms1", "ms2"):
        assert got["p"][k]["shape"] == [16] and got["p"][k]["offset"] >= want["n_params"] and got["p"][k]["offset"] % 4 == 0
        assert (m.p[k].numpy() == 1).all()
    assert got["p"]["ms1"]["offset"] < got["p"]["ms2"]["offset"]
    assert np.array_equal(m.flat_p.numpy()[:want["n_params"]], _built(name).flat_p.numpy())
    if gate:                                                                 # no draw for mean_scale: the gate keeps its bits, and stays last
        assert got["p"]["ar"]["offset"] > got["p"]["ms2"]["offset"]
        assert np.array_equal(m.p["ar"].numpy(), plain.p["ar"].numpy())
    # torch's names: mean_scale directly behind its bias, everything else where it was
    keys, base = [tk for tk, _, _ in m.TORCH_KEYS], [tk for tk, _, _ in plain.TORCH_KEYS]
    assert [k for k in keys if k not in MS] == base
    for i in (1, 2):
        assert keys[keys.index(f"batch_norm_{i}.bias") + 1] == f"batch_norm_{i}.mean_scale"
    assert ("batch_norm_1.mean_scale", "ms1", False) in m.TORCH_KEYS and ("batch_norm_2.mean_scale", "ms2", False) in m.TORCH_KEYS
    if gate:
        assert keys[-1] == "pool.gate_nn.weight"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_mean_scale_is_in_the_state_dict_and_round_trips(name):
    m, _ = _record(name, norm="graph")
    sd, gr, plain = m.state_dict(), m.gradients(), _built(name).state_dict()
    assert [k for k in sd if k not in MS] == list(plain)
    assert all(sd[k].shape == (16,) and (sd[k] == 1).all() and gr[k].shape == (16,) for k in MS)
    assert len(m.get_weights()) == len(_built(name).get_weights()) + 2
    assert all(np.array_equal(sd[k], plain[k]) for k in plain)
    rng = np.random.default_rng(2)
    new = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in sd.items()}
    if name == "PNA":
        new.update({k: np.ones(1, np.float32) for k in m.DELTA_KEYS})
    cls, kw = CONFIGS[name]
    fresh = _new(cls, 16, seed=0, norm="graph", **kw)                        # (built lazily from the dict)
    fresh.load_state_dict(new)
    back = fresh.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and np.array_equal(back[k], new[k]), (name, k)
    assert np.array_equal(fresh.p["ms2"].numpy(), new["batch_norm_2.mean_scale"])
    if name in ("GCN", "SAGE", "GAT-heads4"):                                # (models whose get_weights() lists every state_dict key)
        fresh.set_weights(m.get_weights())
        assert all(np.array_equal(u, v) for u, v in zip(fresh.get_weights(), m.get_weights()))
    for k in MS:
        with pytest.raises(KeyError, match=r"load_state_dict: missing \['" + re.escape(k) + r"'\]"):
            m.load_state_dict({q: v for q, v in new.items() if q != k})
    tv = m.trainable_variables
    assert any(v is m.p["ms1"] for v in tv) and any(v is m.p["ms2"] for v in tv)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_norms_are_refused(name):
    cls, kw = CONFIGS[name]
    with pytest.raises(NotImplementedError, match=r'norm=\'layer\' must be "batch" or "graph"'):
        _new(cls, 16, norm="layer", **kw)


def test_model_oracle_gradients_are_those_of_its_loss():
    """graph_norm_ref.model: finite differences of the loss in mean_scale, weight and bias of both norms, for GCN and GAT and both
    readouts, on fixed kink sides."""
    from test_gcn_bn_host import _graphs
    x, a, gp, y = _graphs(6, 8, seed=2)
    for heads, readout in ((None, "max"), (None, "attention"), (2, "max")):
        p = GN.init_params(8, 16, seed=1, heads=heads, readout=readout)
        r = GN.model(x, a, gp, p, y, heads=heads, readout=readout)
        fixed = {"masks": {k: r[k] for k in ("m1", "m2", "m3", "m4", "e1", "e2") if k in r}, "heads": heads, "readout": readout}
        if readout == "max":
            fixed["argmax"] = r["argmax"]
        for key in ("batch_norm_1.mean_scale", "batch_norm_2.mean_scale", "batch_norm_1.weight", "batch_norm_2.bias", "prelu_1.weight"):
            for j in (0, p[key].size - 1):
                lo, hi = dict(p), dict(p)
                lo[key], hi[key] = p[key].copy(), p[key].copy()
                lo[key][j] -= 1e-6
                hi[key][j] += 1e-6
                fd = (GN.model(x, a, gp, hi, y, **fixed)["loss"] - GN.model(x, a, gp, lo, y, **fixed)["loss"]) / 2e-6
                got = np.asarray(r["grads"][key]).reshape(-1)[j]
                assert abs(fd - got) <= 2e-6 * max(1.0, abs(got)), (heads, readout, key, j, fd, got)

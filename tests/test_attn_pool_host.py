"""CPU tests of the learned readout (GlobalAttnSumPool, readout="attention"): the float64 oracle tests/attn_pool_ref.py against
torch-CPU autograd of the same readout in plain torch, the C ABI of the new entry points, and what the layer and the eight
models of the GCN family promise without a device.  torch is imported inside the test only."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import attn_pool_ref as AR
from test_conv_family_host import CONFIGS, GOLDEN, _HostContext, _built, _init_record, _new, _sha

NEW = ("gcnx_attn_pool_scratch_floats", "gcnx_attn_pool", "gcnx_attn_pool_bwd")
SIZES = [1, 0, 3, 65, 64, 130]


def test_oracle_equals_torch_autograd():
    import torch
    rng = np.random.default_rng(0)
    f = 16
    gp = np.concatenate([[0], np.cumsum(SIZES)])
    n, b = int(gp[-1]), len(SIZES)
    x, a, dp = rng.normal(size=(n, f)), rng.normal(size=f) / np.sqrt(f), rng.normal(size=(b, f))
    tx, ta = torch.tensor(x, dtype=torch.float64, requires_grad=True), torch.tensor(a, dtype=torch.float64, requires_grad=True)
    rows, alphas = [], []
    for g in range(b):                   # AttentionalAggregation: softmax(gate_nn(x), index) * x, summed per graph
        xs = tx[gp[g]:gp[g + 1]]
        al = torch.softmax(xs @ ta, 0)
        alphas.append(al)
        rows.append((al[:, None] * xs).sum(0))
    pooled = torch.stack(rows)
    (pooled * torch.tensor(dp)).sum().backward()
    P, alpha = AR.forward(x, a, gp)
    dx, da = AR.backward(x, a, gp, dp)
    assert np.max(np.abs(P - pooled.detach().numpy())) < 1e-10
    assert np.max(np.abs(alpha - torch.cat(alphas).detach().numpy())) < 1e-10
    assert np.max(np.abs(dx - tx.grad.numpy())) < 1e-10 and np.max(np.abs(da - ta.grad.numpy())) < 1e-10
    assert not P[1].any() and alpha[0] == 1.0 and np.array_equal(P[0], x[0])       # the empty graph, the one-row graph
    # the saved alpha / pooled give the same backward as the recomputed ones
    dx2, da2 = AR.backward(x, a, gp, dp, alpha, P)
    assert np.array_equal(dx, dx2) and np.array_equal(da, da2)


def test_new_entry_points_are_declared_listed_and_exported():
    from gcnx import _lib
    header = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for name in NEW:
        assert re.search(r"GCNX_API\s+[\w\s\*]+\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW:
        assert name in exported, name
    lib = _lib.load()
    assert lib.gcnx_version() >= 421
    # the scratch answer needs no context: slots of (m, l) pairs and partial rows forward, at most 1024 partial rows backward
    sf = lib.gcnx_attn_pool_scratch_floats
    assert sf(0, 3, 16, 0) == 0 and sf(100, 0, 16, 0) == 0 and sf(100, 3, 16, -1) == 0
    assert sf(1659, 3, 16, 7) == 2 * 240 + 240 * 16                          # 1659 // 7 + 3 slots
    assert sf(1659, 3, 10, 7) == 2 * 240 + 240 * 12                          # partial rows on a 4-float stride
    assert sf(1659, 3, 16, 0) >= max((1659 // 64 + 3) * 18, -(-1659 // 64) * 16)
    assert sf(10 ** 6, 2, 256, 0) >= 1024 * 256


def test_layer_is_exported_and_has_spektrals_weight():
    import gcnx
    from gcnx import layers
    assert "GlobalAttnSumPool" in gcnx.__all__ and gcnx.GlobalAttnSumPool is layers.GlobalAttnSumPool
    layer = layers.GlobalAttnSumPool(seed=3)
    (name, shape, init), = layer._param_spec(24)
    assert name == "attn_kernel" and shape == (24, 1) and init.shape == (24, 1) and init.dtype == np.float32
    assert np.max(np.abs(init)) <= np.sqrt(6 / 25) and np.ptp(init) > 0      # glorot-uniform over (F, 1)
    layer.build(_HostContext(), 24)
    assert [w.shape for w in layer.get_weights()] == [(24, 1)] and list(layer.params) == ["attn_kernel"]
    with pytest.raises(NotImplementedError):
        layers.GlobalAttnSumPool(attn_kernel_initializer="zeros")


def _golden(name):
    with open(GOLDEN) as fh:
        return json.load(fh)[name]


def _record(name, readout):
    cls, kw = CONFIGS[name]
    m = _new(cls, 16, seed=0, readout=readout, **kw)
    m.build(5)
    rec = {"n_params": int(m.n_params), "flat_p": _sha(m.flat_p.numpy()), "p": {}}
    for k, v in m.p.items():
        rec["p"][k] = {"offset": int(v.offset), "shape": list(v.shape), "uploaded": None if v.uploaded is None else _sha(v.uploaded)}
    return m, rec


@pytest.mark.parametrize("name", list(CONFIGS))
def test_readout_max_is_the_model_as_it_was(name):
    want = _golden(name)
    m, got = _record(name, "max")
    assert got == want == _init_record(name)
    assert "ar" not in m.p and "pool.gate_nn.weight" not in m.state_dict()
    assert m.PARAM_ORDER == _built(name).PARAM_ORDER and m.TORCH_KEYS == _built(name).TORCH_KEYS


@pytest.mark.parametrize("name", list(CONFIGS))
def test_readout_attention_adds_one_tensor_behind_the_others(name):
    want = _golden(name)
    m, got = _record(name, "attention")
    assert set(got["p"]) == set(want["p"]) | {"ar"}
    for k in want["p"]:
        assert got["p"][k] == want["p"][k], (name, k)
    ar = got["p"]["ar"]
    assert ar["shape"] == [16] and ar["offset"] >= want["n_params"] and ar["offset"] % 4 == 0
    assert got["n_params"] == ar["offset"] + 16
    values = m.p["ar"].numpy()
    assert np.max(np.abs(values)) <= 0.25 and np.ptp(values) > 0             # U(+-1 / sqrt(16))
    # everything in front of it keeps its bits
    base = _built(name).flat_p.numpy()
    assert np.array_equal(m.flat_p.numpy()[:want["n_params"]], base)
    assert m.PARAM_ORDER[-1] == "ar" and m.PARAM_ORDER[:-1] == tuple(_built(name).PARAM_ORDER)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_gate_weight_is_last_in_the_state_dict_and_round_trips(name):
    m, _ = _record(name, "attention")
    sd, gr, plain = m.state_dict(), m.gradients(), _built(name).state_dict()
    assert list(sd)[-1] == "pool.gate_nn.weight" and list(sd)[:-1] == list(plain)
    assert sd["pool.gate_nn.weight"].shape == (1, 16) and gr["pool.gate_nn.weight"].shape == (1, 16)
    assert list(gr)[-1] == "pool.gate_nn.weight"
    assert m.get_weights()[-1].shape == (1, 16) and len(m.get_weights()) == len(_built(name).get_weights()) + 1
    assert all(np.array_equal(sd[k], plain[k]) for k in plain)
    rng = np.random.default_rng(2)
    new = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in sd.items()}
    if name == "PNA":
        new.update({k: np.ones(1, np.float32) for k in m.DELTA_KEYS})
    for squeeze in (False, True):
        cls, kw = CONFIGS[name]
        fresh = _new(cls, 16, seed=0, readout="attention", **kw)             # (built lazily from the dict)
        fresh.load_state_dict({k: (v[0] if squeeze and k == "pool.gate_nn.weight" else v) for k, v in new.items()})
        back = fresh.state_dict()
        assert list(back) == list(sd)
        for k in sd:
            assert back[k].shape == sd[k].shape and np.array_equal(back[k], new[k]), (name, k)
        assert np.array_equal(fresh.p["ar"].numpy(), new["pool.gate_nn.weight"][0])
    with pytest.raises(KeyError, match=r"load_state_dict: missing \['pool\.gate_nn\.weight'\]"):
        m.load_state_dict({k: v for k, v in new.items() if k != "pool.gate_nn.weight"})
    assert m.trainable_variables[-1] is m.p["ar"]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_other_readouts_are_refused(name):
    cls, kw = CONFIGS[name]
    with pytest.raises(NotImplementedError, match=r'readout=\'sum\' must be "max" or "attention"'):
        _new(cls, 16, readout="sum", **kw)


def test_model_oracle_reduces_to_its_parts():
    """attn_pool_ref.model is gcn_bn_ref's / gat_ref's restatement up to y2, and its readout gradient is that of the stand-alone
    oracle (checked by finite differences of the loss in the gate's weight)."""
    import gat_ref as GR
    import gcn_bn_ref as R
    from test_gcn_bn_host import _graphs
    x, a, gp, y = _graphs(6, 8, seed=2)
    for heads in (None, 2):
        p = AR.init_params(8, 16, seed=1, heads=heads)
        r = AR.model(x, a, gp, p, y, heads=heads)
        base = {k: v for k, v in p.items() if k != AR.GATE_KEY}
        ref = R.model(x, a, gp, base, y) if heads is None else GR.model(x, a, gp, base, y, heads=heads)
        assert np.max(np.abs(r["y2"] - ref["y2"])) < 1e-12
        masks = {k: r[k] for k in ("m1", "m2", "m3", "m4", "e1", "e2") if k in r}
        g = r["grads"][AR.GATE_KEY]
        for j in (0, 7, 15):
            lo, hi = dict(p), dict(p)
            lo[AR.GATE_KEY], hi[AR.GATE_KEY] = p[AR.GATE_KEY].copy(), p[AR.GATE_KEY].copy()
            lo[AR.GATE_KEY][0, j] -= 1e-6
            hi[AR.GATE_KEY][0, j] += 1e-6
            fd = (AR.model(x, a, gp, hi, y, masks=masks, heads=heads)["loss"] - AR.model(x, a, gp, lo, y, masks=masks, heads=heads)["loss"]) / 2e-6
            assert abs(fd - g[0, j]) <= 1e-6 * max(1.0, abs(g[0, j])), (heads, j, fd, g[0, j])

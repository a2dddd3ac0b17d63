"""GPU tests of the reference's torch GCN (gcnx.GCN) and its kernels: shared-slope PReLU in gcnx_bn_act(_bwd), the fused
BatchNorm·PReLU·max-pool pair, the one-launch BN·PReLU·BCE head, the model, its torch-style surface and the layer
classes -- each against the float64 oracle tests/gcn_bn_ref.py evaluated on the device's side of every kink."""
import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R

pytestmark = pytest.mark.gpu

# The bias of a layer that feeds a BatchNorm has an analytically ZERO gradient (the normalisation removes the mean): both
# sides are rounding noise, so it is compared relative to the same layer's weight gradient.
# batch_norm_2.bias too: its gradient is sum_g dPooled[g] * PReLU'(argmax row), and sum_g dPooled[g] = 0 exactly (dPooled =
# dZ3 W3 and BatchNorm3's backward output has zero column sums) -- with every pooled maximum on the positive side (large
# graphs) it vanishes; it is compared relative to the same BatchNorm's weight gradient.
UNDER_BN = {"conv1.bias": "conv1.lin.weight", "conv2.bias": "conv2.lin.weight", "linear_1.bias": "linear_1.weight",
            "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _cmp_grads(got, ref, tol, what, keys=None):
    for k in keys or ref:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        if k in UNDER_BN:
            scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN[k]], np.float64))))
            assert float(np.max(np.abs(g - r))) <= tol * scale, (what, k, float(np.max(np.abs(g - r))), scale)
        else:
            assert_close(g, r, tol, f"{what} {k}")


def _tiny_host(n_graphs=16, f=16, seed=0):
    """synth.tiny_graphs collated: HostBatch (CSR with self-loops, unit values)."""
    import scipy.sparse as sp
    from gcnx import synth
    raw = synth.tiny_graphs(n_graphs, f, seed=seed)
    a = sp.block_diag([g[1] for g in raw], format="csr")
    a.sort_indices()
    gp = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in raw])]).astype(np.int32)
    x = np.concatenate([g[0] for g in raw]).astype(np.float32)
    y = np.stack([g[2] for g in raw]).astype(np.float32)
    return synth.HostBatch(x, a.indptr.astype(np.int32), a.indices.astype(np.int32), None, gp, y)


def _ecoli_host(f=16):
    from gcnx import synth
    return synth.ecoli_batch(f=f)


def _device_batch(ctx, hb):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))


def _scipy_adj(hb):
    import scipy.sparse as sp
    return sp.csr_matrix((np.ones(len(hb.colidx)), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))


def _bn_inputs(ctx, n, f, seed, per_feature=False):
    from gcnx import device as D
    rng = np.random.default_rng(seed)
    z = (rng.normal(size=(n, f)) * rng.uniform(0.5, 3, f) + rng.normal(size=f)).astype(np.float32)
    gamma = (1 + 0.3 * rng.normal(size=f)).astype(np.float32)
    beta = (0.3 * rng.normal(size=f)).astype(np.float32)
    alpha = rng.uniform(0.05, 0.4, f if per_feature else 1).astype(np.float32)
    dz = ctx.to_device(z)
    mean, inv = ctx.empty(f), ctx.empty(f)
    D.bn_moments(ctx, dz, None, mean, inv, eps=D.TORCH_BN_EPS)
    return z, gamma, beta, alpha, dz, mean, inv


# ---- 1. shared-slope PReLU in gcnx_bn_act / gcnx_bn_act_bwd ----------------------------------------------------------
@pytest.mark.parametrize("n,f", [(200, 64), (1500, 16), (3000, 256)])
def test_bn_act_shared_prelu_against_oracle(ctx, n, f):
    from gcnx import device as D
    z, gamma, beta, alpha, dz, mean, inv = _bn_inputs(ctx, n, f, seed=n + f)
    g, b, a = ctx.to_device(gamma), ctx.to_device(beta), ctx.to_device(alpha)
    y = ctx.empty((n, f))
    D.bn_act(ctx, dz, mean, inv, g, b, y, act="prelu_shared", alpha=a)
    zb, cache = R.bn_fwd(z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    pos = R.device_prelu_sides(z, mean.numpy(), inv.numpy(), gamma, beta)
    ref, _ = R.prelu_fwd(zb, float(alpha[0]), pos)
    assert_close(y.numpy(), ref, 1e-5, f"bn_act prelu_shared n={n} f={f}")
    dy = np.random.default_rng(n).normal(size=(n, f)).astype(np.float32)
    ddz, dg, dbe, da = ctx.empty((n, f)), ctx.empty(f), ctx.empty(f), ctx.zeros(4)
    D.bn_act_bwd(ctx, ctx.to_device(dy), dz, mean, inv, g, b, ddz, ctx.empty(3 * f), act="prelu_shared", alpha=a,
                 dgamma=dg, dbeta=dbe, dalpha=da)
    dzb, da_ref = R.prelu_bwd(dy.astype(np.float64), zb, float(alpha[0]), pos)
    dz_ref, dg_ref, db_ref = R.bn_bwd(dzb, cache, gamma.astype(np.float64))
    assert_close(ddz.numpy(), dz_ref, 1e-5, "dz")
    assert_close(dg.numpy(), dg_ref, 1e-5, "dgamma")
    assert_close(dbe.numpy(), db_ref, 1e-5, "dbeta")
    got = da.numpy()
    assert abs(got[0] - da_ref[0]) <= 1e-5 * max(1.0, abs(da_ref[0])) and np.all(got[1:] == 0)   # one float written


def test_other_entry_points_refuse_the_shared_slope(ctx):
    from gcnx import _lib, device as D
    x, w, out = ctx.zeros((8, 16)), ctx.zeros((16, 16)), ctx.zeros((8, 16))
    with pytest.raises(_lib.GcnxError):
        D.gemm(ctx, x, w, None, out, act="prelu_shared", alpha=ctx.zeros(16))
    with pytest.raises(_lib.GcnxError):
        D.act_bias_grad(ctx, x, x, out, "prelu_shared", alpha=ctx.zeros(16))


# ---- 2. gcnx_bn_act_pool(_bwd) ---------------------------------------------------------------------------------------
def _pool_case(sizes, f, seed):
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return gp


@pytest.mark.parametrize("f", [16, 64, 256])
@pytest.mark.parametrize("per_feature", [False, True])
def test_bn_act_pool_is_bn_act_plus_max_pool(ctx, f, per_feature):
    from gcnx import device as D
    from gcnx.device import Segments
    sizes = [1, 2, 7, 600, 33, 1, 250, 64, 5, 129]
    gp = _pool_case(sizes, f, 0)
    n = int(gp[-1])
    z, gamma, beta, alpha, dz, mean, inv = _bn_inputs(ctx, n, f, seed=f, per_feature=per_feature)
    z[gp[3] + 10:gp[3] + 20] = z[gp[3] + 5]                 # exact ties inside one graph: the first row must win
    dz.copy_from_host(z)
    D.bn_moments(ctx, dz, None, mean, inv, eps=D.TORCH_BN_EPS)
    seg = Segments(ctx, gp)
    act = "prelu" if per_feature else "prelu_shared"
    g, b, a = ctx.to_device(gamma), ctx.to_device(beta), ctx.to_device(alpha)
    pooled, arg = ctx.empty((len(sizes), f)), ctx.empty((len(sizes), f), np.int32)
    D.bn_act_pool(ctx, seg, dz, mean, inv, g, b, pooled, arg, act=act, alpha=a)
    y, pooled2, arg2 = ctx.empty((n, f)), ctx.empty((len(sizes), f)), ctx.empty((len(sizes), f), np.int32)
    D.bn_act(ctx, dz, mean, inv, g, b, y, act=act, alpha=a)
    D.segment_pool(ctx, seg, y, pooled2, "max", arg2)
    assert np.array_equal(pooled.numpy().view(np.uint32), pooled2.numpy().view(np.uint32))
    assert np.array_equal(arg.numpy(), arg2.numpy())
    # backward: fused vs the unfused pair, and vs the kink-separated oracle
    dp = np.random.default_rng(f).normal(size=(len(sizes), f)).astype(np.float32)
    ddp = ctx.to_device(dp)
    out = {k: ctx.zeros(s) for k, s in (("dz", (n, f)), ("dg", f), ("db", f), ("da", alpha.size))}
    D.bn_act_pool_bwd(ctx, seg, ddp, arg, dz, mean, inv, g, b, out["dz"], act=act, alpha=a, dgamma=out["dg"], dbeta=out["db"],
                      dalpha=out["da"])
    dy = ctx.empty((n, f))
    D.segment_pool_bwd(ctx, seg, ddp, dy, "max", arg2)
    ref = {k: ctx.zeros(s) for k, s in (("dz", (n, f)), ("dg", f), ("db", f), ("da", alpha.size))}
    D.bn_act_bwd(ctx, dy, dz, mean, inv, g, b, ref["dz"], ctx.empty(3 * f), act=act, alpha=a, dgamma=ref["dg"], dbeta=ref["db"],
                 dalpha=ref["da"])
    pos = R.device_prelu_sides(z, mean.numpy(), inv.numpy(), gamma, beta)
    orc = R.bn_act_pool_bwd(dp.astype(np.float64), arg.numpy(), z, gamma.astype(np.float64), beta.astype(np.float64), alpha, gp, pos)
    for k, o in zip(("dz", "dg", "db", "da"), orc):
        assert_close(out[k].numpy(), ref[k].numpy(), 1e-5, f"bn_act_pool_bwd {k} vs unfused f={f}")
        assert_close(out[k].numpy(), o, 1e-4, f"bn_act_pool_bwd {k} vs oracle f={f}")


def test_bn_act_pool_at_config2_size(ctx):
    from gcnx import device as D
    from gcnx.device import Segments
    hb = _ecoli_host(f=16)
    gp, n, f = hb.graph_ptr, hb.n, 64
    z, gamma, beta, alpha, dz, mean, inv = _bn_inputs(ctx, n, f, seed=11)
    seg = Segments(ctx, gp)
    g, b, a = ctx.to_device(gamma), ctx.to_device(beta), ctx.to_device(alpha)
    B = len(gp) - 1
    pooled, arg = ctx.empty((B, f)), ctx.empty((B, f), np.int32)
    D.bn_act_pool(ctx, seg, dz, mean, inv, g, b, pooled, arg, alpha=a)
    y, pooled2, arg2 = ctx.empty((n, f)), ctx.empty((B, f)), ctx.empty((B, f), np.int32)
    D.bn_act(ctx, dz, mean, inv, g, b, y, act="prelu_shared", alpha=a)
    D.segment_pool(ctx, seg, y, pooled2, "max", arg2)
    assert np.array_equal(pooled.numpy().view(np.uint32), pooled2.numpy().view(np.uint32))
    assert np.array_equal(arg.numpy(), arg2.numpy())


def test_bn_act_pool_refuses_other_pools(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import Segments
    z = ctx.zeros((4, 16))
    seg = Segments(ctx, np.array([0, 2, 4], np.int32))
    one = ctx.to_device(np.ones(16, np.float32))
    with pytest.raises(_lib.GcnxError) as e:
        D.bn_act_pool(ctx, seg, z, one, one, one, one, ctx.empty((2, 16)), ctx.empty((2, 16), np.int32), alpha=one, mode="sum")
    assert e.value.code == _lib.ERR_UNSUPPORTED


# ---- 3. gcnx_bn_prelu_bce_head ------------------------------------------------------------------------------------------
HEAD_KEYS = {"w3": "linear_1.weight", "b3": "linear_1.bias", "g3": "batch_norm_3.weight", "be3": "batch_norm_3.bias",
             "a3": "prelu_3.weight", "w4": "linear_2.weight", "b4": "linear_2.bias", "g4": "batch_norm_4.weight",
             "be4": "batch_norm_4.bias", "a4": "prelu_4.weight"}


def _head_run(ctx, P, p, y, grads=True):
    from gcnx import device as D
    B, H = P.shape
    dp = {k: ctx.to_device(np.asarray(p[t], np.float32)) for k, t in HEAD_KEYS.items()}
    dg = {k: ctx.zeros(v.shape) for k, v in dp.items()}
    dP, dPd = ctx.to_device(P), ctx.zeros((B, H))
    out, probs, la = ctx.empty((B, 1)), ctx.empty((B, 1)), ctx.zeros(2)
    scratch = ctx.empty(D.bce_head_scratch_floats(ctx, B, H))
    dy = ctx.to_device(np.asarray(y, np.float32)) if y is not None else None
    args = D.bce_head_args(dP, dp, scratch, out, probs, y=dy, loss_acc=la if y is not None else None, denom=B,
                           g=dg if grads else None, dpooled=dPd if grads else None)
    D.bn_prelu_bce_head(ctx, args)
    return out.numpy(), probs.numpy(), la.numpy(), dPd.numpy(), {HEAD_KEYS[k]: v.numpy() for k, v in dg.items()}


@pytest.mark.parametrize("B", [2, 3, 32, 50, 1000])
@pytest.mark.parametrize("H", [16, 64, 256])
def test_bce_head_against_oracle(ctx, B, H):
    rng = np.random.default_rng(B * 1000 + H)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=B + H).items()}
    P = rng.normal(size=(B, H)).astype(np.float32)
    lab = rng.integers(0, 2, B)
    layouts = {"onehot": np.eye(2)[lab], "col": lab[:, None].astype(np.float64), "flat": lab.astype(np.float64)}
    name = ("onehot", "col", "flat")[(B + H) % 3]
    y = layouts[name]
    out, probs, la, dP, g = _head_run(ctx, P, p, y)
    r = R.head(P.astype(np.float64), p, y)
    assert_close(out, r["out"], 1e-4, f"head out B={B} H={H}")
    assert_close(probs, r["probs"], 1e-4, "probs")
    assert rel_err(la[0], r["loss"]) < 1e-4, (la[0], r["loss"])
    assert la[1] == r["hits"]
    if B == 2:
        # BatchNorm over two rows outputs +-1 whatever its input: everything below BN4 has a zero gradient (noise on
        # both sides); the output layer's own parameters still have one
        _cmp_grads(g, r["grads"], 1e-4, f"head B=2 H={H}", ("batch_norm_4.weight", "batch_norm_4.bias", "prelu_4.weight"))
        assert np.all(np.isfinite(dP)) and all(np.all(np.isfinite(v)) for v in g.values())
    else:
        assert_close(dP, r["dP"], 1e-4, f"dP B={B} H={H} {name}")
        _cmp_grads(g, r["grads"], 1e-4, f"head B={B} H={H}")
    # forward only (model(inputs)): the same logits, nothing else written
    out2, probs2, la2, dP2, g2 = _head_run(ctx, P, p, None, grads=False)
    assert np.array_equal(out2, out) and np.array_equal(probs2, probs) and not la2.any() and not dP2.any()


def test_bce_head_limits(ctx):
    from gcnx import _lib
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 257).items()}
    with pytest.raises(_lib.GcnxError) as e:
        _head_run(ctx, np.zeros((4, 257), np.float32), p, np.zeros(4))
    assert e.value.code == _lib.ERR_UNSUPPORTED and "256" in str(e.value)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 16).items()}
    with pytest.raises(_lib.GcnxError):
        _head_run(ctx, np.zeros((1, 16), np.float32), p, np.zeros(1))


# ---- 4. gcnx.GCN: full step against the kink-separated oracle ------------------------------------------------------------
def _model(ctx, f, seed=0, knob=None, monkeypatch=None):
    import gcnx
    if monkeypatch is not None:
        monkeypatch.setenv("GCNX_BN_POOL", knob)
    m = gcnx.GCN(ctx, hidden_channels=64, seed=seed)
    m.build(f)
    return m


def _device_sides(m):
    b, p = m._bufs, m.p
    return {"m1": R.device_prelu_sides(b["z1"].numpy(), b["m1"].numpy(), b["i1"].numpy(), p["g1"].numpy(), p["be1"].numpy()),
            "m2": R.device_prelu_sides(b["z2"].numpy(), b["m2"].numpy(), b["i2"].numpy(), p["g2"].numpy(), p["be2"].numpy())}


def _check_step(m, batch, hb, p, tol, what):
    m.loss_and_grads(batch)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = R.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, hb.y, masks=_device_sides(m), argmax=arg)
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol and la[1] == r["hits"], (la, r["loss"], r["hits"])
    _cmp_grads(m.gradients(), r["grads"], tol, what)
    return r


@pytest.mark.parametrize("shape", ["config1", "config2"])
def test_gcn_step_against_oracle(ctx, shape):
    hb = _tiny_host(16, 16, seed=4) if shape == "config1" else _ecoli_host(f=16)
    batch = _device_batch(ctx, hb)
    m = _model(ctx, 16)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 64, seed=7).items()}
    m.load_state_dict(p)
    _check_step(m, batch, hb, p, 1e-4, shape)
    # five SGD steps at the reference's first learning rate (gcn.py:321-324), each oracle step on the device's kink sides of
    # that step
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    for _ in range(5):
        m.train_step(batch, lr=0.02)
        arg = m._bufs["arg"].numpy().astype(np.int64)
        r = R.model(hb.x, _scipy_adj(hb), hb.graph_ptr, ph, hb.y, masks=_device_sides(m), argmax=arg)
        ph = R.sgd(ph, r["grads"], 0.02)
    sd = m.state_dict()
    for k in R.KEYS:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{shape} after 5 steps {k}")


@pytest.mark.parametrize("shape", ["config1", "config2"])
def test_gcn_bn_pool_knob_agrees(ctx, shape, monkeypatch):
    hb = _tiny_host(16, 16, seed=5) if shape == "config1" else _ecoli_host(f=16)
    batch = _device_batch(ctx, hb)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 64, seed=8).items()}
    res = []
    for knob in ("1", "0"):
        m = _model(ctx, 16, knob=knob, monkeypatch=monkeypatch)
        assert m._bn_pool == (knob == "1")
        m.load_state_dict(p)
        m.loss_and_grads(batch)
        res.append((m._bufs["out"].numpy(), m.loss_acc.numpy(), m.gradients()))
    assert np.array_equal(res[0][0], res[1][0])          # the forward is bit-identical (same pooled rows)
    assert np.array_equal(res[0][1], res[1][1])
    _cmp_grads(res[0][2], res[1][2], 1e-5, "knob")


# ---- 5. torch-style surface ------------------------------------------------------------------------------------------
def test_gcn_forward_state_dict_and_single_graph(ctx):
    import gcnx
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.GCN(ctx, seed=1)
    ids = hb.ids()
    a = _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1)
    coo = a.tocoo()
    edge_index = np.stack([coo.col, coo.row])               # PyG: source -> target, target = CSR row
    assert np.array_equal(m.forward(hb.x, edge_index, ids), logits)
    sd = m.state_dict()
    assert sd["conv1.lin.weight"].shape == (64, 16) and sd["linear_2.weight"].shape == (1, 64) and sd["prelu_1.weight"].shape == (1,)
    assert sd["batch_norm_4.bias"].shape == (1,)
    assert [k for k, _, _ in m.TORCH_KEYS] == list(R.KEYS)
    m2 = gcnx.GCN(ctx, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(v, sd[k]), k
    assert np.array_equal(m2((hb.x, a, ids)), logits)
    w = m.get_weights()
    assert [x.shape for x in w] == [sd[k].shape for k in R.KEYS]
    # a graph without stored self-loops gets them (add_remaining_self_loops) on the raw path
    import scipy.sparse as sp
    a_noloop = sp.csr_matrix(a - sp.diags(a.diagonal()))
    a_noloop.eliminate_zeros()
    assert np.array_equal(m((hb.x, a_noloop, ids)), logits)
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


# ---- 6. gcnx.fit ------------------------------------------------------------------------------------------------------
def test_fit_runs_the_gcn(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:10]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[10:]])
    m = gcnx.GCN(ctx, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])
    (loss, acc), preds = gcnx.train.evaluate(m, DisjointLoader(te, batch_size=3, shuffle=False))
    probs = np.concatenate(preds).ravel()
    assert probs.size == 6 and np.all((probs >= 0) & (probs <= 1))
    labels = np.array([y[1] for _, _, y in raw[10:]])
    fpr, tpr, _ = gcnx.roc_curve(labels, probs)
    assert 0.0 <= gcnx.auc(fpr, tpr) <= 1.0


# ---- 7. the layer classes compose to the model -------------------------------------------------------------------------
def test_layers_compose_to_the_model(ctx):
    import gcnx
    from gcnx import device as D
    from gcnx.layers import BatchNorm1d, Dense, GCNConv, GlobalMaxPool, PReLU
    hb = _tiny_host(16, 16, seed=2)
    batch = _device_batch(ctx, hb)
    m = gcnx.GCN(ctx, seed=3)
    m.build(16)
    m.loss_and_grads(batch)
    sd, g_model = m.state_dict(), m.gradients()
    a_hat = batch.a.unweighted().gcn_norm("pyg")
    L = {"conv1": GCNConv(64), "conv2": GCNConv(64), "lin1": Dense(64), "lin2": Dense(1), "pool": GlobalMaxPool()}
    for k in range(1, 5):
        L[f"bn{k}"], L[f"pr{k}"] = BatchNorm1d(), PReLU()
    t = L["conv1"]([batch.x, a_hat])
    t = L["pr1"](L["bn1"](t, training=True))
    t = L["pr2"](L["bn2"](L["conv2"]([t, a_hat]), training=True))
    t = L["pool"]([t, batch.seg])
    t = L["pr3"](L["bn3"](L["lin1"](t), training=True))
    out = L["pr4"](L["bn4"](L["lin2"](t), training=True))
    for name, key in (("conv1", "conv1"), ("conv2", "conv2"), ("lin1", "linear_1"), ("lin2", "linear_2")):
        w = sd[f"{key}.lin.weight" if name.startswith("conv") else f"{key}.weight"]
        L[name].params["kernel"].copy_from_host(np.ascontiguousarray(w.T))        # Keras [in, out] = torch weight^T
        L[name].params["bias"].copy_from_host(sd[f"{key}.bias"])
    for k in range(1, 5):
        L[f"bn{k}"].params["weight"].copy_from_host(sd[f"batch_norm_{k}.weight"])
        L[f"bn{k}"].params["bias"].copy_from_host(sd[f"batch_norm_{k}.bias"])
        L[f"pr{k}"].params["weight"].copy_from_host(sd[f"prelu_{k}.weight"])
    # forward again with the model's weights
    t = L["conv1"]([batch.x, a_hat])
    t = L["pr1"](L["bn1"](t, training=True))
    t = L["pr2"](L["bn2"](L["conv2"]([t, a_hat]), training=True))
    t = L["pool"]([t, batch.seg])
    t = L["pr3"](L["bn3"](L["lin1"](t), training=True))
    out = L["pr4"](L["bn4"](L["lin2"](t), training=True))
    logits = out.numpy()
    assert_close(logits, m._bufs["out"].numpy(), 1e-6, "layers logits")
    t_lab = hb.y[:, 1:2].astype(np.float64)
    dout = ((1 / (1 + np.exp(-logits.astype(np.float64))) - t_lab) / hb.n_graphs).astype(np.float32)
    d = L["pr4"].backward(ctx.to_device(dout))
    d = L["lin2"].backward(L["bn4"].backward(d))
    d = L["lin1"].backward(L["bn3"].backward(L["pr3"].backward(d)))
    d = L["pool"].backward(d)
    d = L["conv2"].backward(L["bn2"].backward(L["pr2"].backward(d)))
    L["conv1"].backward(L["bn1"].backward(L["pr1"].backward(d)), need_dx=False)
    got = {}
    for name, key in (("conv1", "conv1"), ("conv2", "conv2"), ("lin1", "linear_1"), ("lin2", "linear_2")):
        got[f"{key}.lin.weight" if name.startswith("conv") else f"{key}.weight"] = L[name].grads["kernel"].numpy().T
        got[f"{key}.bias"] = L[name].grads["bias"].numpy()
    for k in range(1, 5):
        got[f"batch_norm_{k}.weight"] = L[f"bn{k}"].grads["weight"].numpy()
        got[f"batch_norm_{k}.bias"] = L[f"bn{k}"].grads["bias"].numpy()
        got[f"prelu_{k}.weight"] = L[f"pr{k}"].grads["weight"].numpy()
    _cmp_grads(got, g_model, 1e-6, "layers")

"""GPU tests of gcnx.GCN's sync-BN training over graph shards: the phased BN·PReLU·BCE head (gcnx_bce_head_phase), the split
backward of the fused BN·PReLU·max-pool (gcnx_bn_act_pool_bwd_stats / _apply), and the sharded model step on thread ranks
that share one GPU (tests/thread_comm.py) -- against the one-launch kernels, the single-rank step on the whole batch and
the float64 oracle on the device's side of every kink.

Kernel tests shard inside one process and add the partial sums on the host between the launches, in rank order and in
fp32, as ThreadCommunicator does."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import gcn_sync_bn_ref as S
from test_gpu_gcn_bn import HEAD_KEYS, _bn_inputs, _cmp_grads, _device_batch, _head_run, _scipy_adj, _tiny_host
from test_gpu_gcn_routes import _assert_hits, _check_head, _with_empty_graphs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu


def _host_allreduce(parts):
    out = np.asarray(parts[0], np.float32).copy()
    for p in parts[1:]:
        out = out + np.asarray(p, np.float32)
    return out


# ---- 1. gcnx_bce_head_phase ----------------------------------------------------------------------------------------------
def _phased_head(ctx, P, p, y, bounds, count=None):
    """The head over row shards P[bounds[s]:bounds[s + 1]], each phase's red slice added over the shards before the next.
    Returns (out, probs, loss_acc, dP, grads) of the whole batch -- loss_acc and grads summed over the shards -- and the
    device's PReLU sides {"m3", "m4"} (y3 > 0 after phase 2, out > 0)."""
    from gcnx import device as D
    B, H = P.shape
    dp = {k: ctx.to_device(np.asarray(p[t], np.float32)) for k, t in HEAD_KEYS.items()}
    sh = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        b = hi - lo
        s = {"g": {k: ctx.zeros(v.shape) for k, v in dp.items()}, "P": ctx.to_device(P[lo:hi]), "dP": ctx.zeros((b, H)),
             "out": ctx.empty((b, 1)), "probs": ctx.empty((b, 1)), "la": ctx.zeros(2), "b": b,
             "scratch": ctx.empty(D.bce_head_phase_scratch_floats(ctx, b, H)), "red": ctx.zeros(D.bce_head_phase_red_floats(ctx, H)),
             "y": ctx.to_device(np.asarray(y[lo:hi], np.float32))}
        s["args"] = D.bce_head_args(s["P"], dp, s["scratch"], s["out"], s["probs"], y=s["y"], loss_acc=s["la"], denom=B, g=s["g"],
                                    dpooled=s["dP"])
        sh.append(s)
    m3 = []
    for k in range(7):
        for s in sh:
            D.bce_head_phase(ctx, s["args"], k, count or B, s["red"])
        if k == 2:
            m3 = [s["scratch"].numpy()[s["b"] * H:2 * s["b"] * H].reshape(s["b"], H) > 0 for s in sh]
        sl = D.bce_head_phase_slice(k, H)
        if sl is not None and len(sh) > 1:
            tot = _host_allreduce([s["red"].numpy()[sl[0]:sl[0] + sl[1]] for s in sh])
            for s in sh:
                s["red"].flat(*sl).copy_from_host(tot)
    cat = lambda key: np.concatenate([s[key].numpy() for s in sh])
    out = cat("out")
    la = np.sum([s["la"].numpy().astype(np.float64) for s in sh], 0)
    g = {HEAD_KEYS[k]: np.sum([s["g"][k].numpy().astype(np.float64) for s in sh], 0) for k in dp}
    return (out, cat("probs"), la, cat("dP"), g), {"m3": np.concatenate(m3), "m4": out > 0}


@pytest.mark.parametrize("H", [1, 16, 64, 256])
def test_phased_head_one_shard_equals_the_one_launch_head(ctx, H):
    B = 50
    rng = np.random.default_rng(H)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=H).items()}
    P = rng.normal(size=(B, H)).astype(np.float32)
    y = np.eye(2)[rng.integers(0, 2, B)]
    (out, probs, la, dP, g), _ = _phased_head(ctx, P, p, y, [0, B])
    out1, probs1, la1, dP1, g1 = _head_run(ctx, P, p, y)
    for a, b, what in ((out, out1, "out"), (probs, probs1, "probs"), (la, la1, "loss_acc"), (dP, dP1, "dP")):
        assert rel_err(a, b) <= 1e-6, (H, what, rel_err(a, b))
    assert la[1] == la1[1]
    for k in g1:
        # the Linear biases (and at H = 1 the Linear weights too) feed a BatchNorm: analytically zero, both sides rounding
        # noise -- compared in absolute terms, against the same BatchNorm's weight gradient
        bn = {"linear_1": "batch_norm_3.weight", "linear_2": "batch_norm_4.weight"}.get(k.split(".")[0])
        ok = rel_err(g[k], g1[k]) <= 1e-6 or (bn and np.max(np.abs(g[k] - g1[k])) <= 1e-5 * np.max(np.abs(g1[bn])))
        assert ok, (H, k, rel_err(g[k], g1[k]))


@pytest.mark.parametrize("H", [1, 64, 100, 256])
@pytest.mark.parametrize("bounds", [[0, 19, 40], [0, 1, 23, 40], [0, 13, 39, 40]], ids=["2", "3_one_row_first", "3_one_row_last"])
def test_phased_head_on_shards_against_oracle(ctx, H, bounds):
    B = bounds[-1]
    rng = np.random.default_rng(H * 10 + len(bounds))
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=H + 1).items()}
    P = rng.normal(size=(B, H)).astype(np.float32)
    y = np.eye(2)[rng.integers(0, 2, B)]
    got, sides = _phased_head(ctx, P, p, y, bounds)
    r = R.head(P.astype(np.float64), p, y, masks=sides)
    if H > 1:
        _check_head(got, r, y, f"phased head H={H} bounds={bounds}")
        return
    # H = 1: every Linear gradient is analytically zero (its BatchNorm's backward output is orthogonal to the Linear's input
    # span{1, xhat}), and BN3's gradients are small sums of large terms.  On shards each is a sum of LOCAL parts that cancel
    # in the all-reduce, so its rounding scale is the sum of the absolute terms, sum_r |dz_r x_r| (from the sharded oracle)
    out, probs, la, dP, g = got
    assert_close(out, r["out"], 1e-4, "H=1 out")
    assert_close(probs, r["probs"], 1e-4, "H=1 probs")
    assert rel_err(la[0], r["loss"]) < 1e-4, (la[0], r["loss"])
    _assert_hits(la[1], r, y)
    assert_close(dP, r["dP"], 1e-4, "H=1 dP")
    parts = S.head([P[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:])], p, [y[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:])],
                   denom=B, masks=sides)
    cat = lambda key: np.concatenate([q[key] for q in parts])
    dz3, dz4, y3, dzb3, xh3 = cat("dz3"), cat("dz4"), cat("y3"), cat("dzb3"), cat("xh3")
    terms = {"linear_1.weight": np.abs(dz3 * P), "linear_1.bias": np.abs(dz3), "linear_2.weight": np.abs(dz4 * y3),
             "linear_2.bias": np.abs(dz4), "batch_norm_3.weight": np.abs(dzb3 * xh3), "batch_norm_3.bias": np.abs(dzb3)}
    for k, t in terms.items():
        err = float(np.max(np.abs(g[k] - np.asarray(r["grads"][k]).reshape(g[k].shape))))
        assert err <= 1e-4 * float(t.sum()), (k, err, float(t.sum()))
    _cmp_grads(g, r["grads"], 1e-4, "H=1", [k for k in r["grads"] if k not in terms])


def test_phased_head_saturated_logits(ctx):
    B, H = 48, 32
    rng = np.random.default_rng(3)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=4).items()}
    p["batch_norm_4.weight"] = np.array([70.0], np.float32)
    p["batch_norm_4.bias"] = np.array([30.0], np.float32)
    p["prelu_4.weight"] = np.array([0.9], np.float32)
    P = rng.normal(size=(B, H)).astype(np.float32)
    y = np.eye(2)[rng.integers(0, 2, B)]
    got, sides = _phased_head(ctx, P, p, y, [0, 1, 30, B])
    r = R.head(P.astype(np.float64), p, y, masks=sides)
    assert np.max(np.abs(r["out"])) > 90
    assert all(np.all(np.isfinite(v)) for v in got[:4]) and all(np.all(np.isfinite(v)) for v in got[4].values())
    _check_head(got, r, y, "phased head saturated")


def test_phased_head_limits(ctx):
    from gcnx import _lib, device as D
    H = 16
    p = {k: ctx.to_device(np.asarray(v, np.float32)) for k, v in zip(HEAD_KEYS, [np.zeros((H, H)), np.zeros(H), np.ones(H),
                                                                                  np.zeros(H), np.full(1, .25), np.zeros((1, H)),
                                                                                  np.zeros(1), np.ones(1), np.zeros(1),
                                                                                  np.full(1, .25)])}
    P, out, probs = ctx.zeros((1, H)), ctx.empty((1, 1)), ctx.empty((1, 1))
    red = ctx.zeros(D.bce_head_phase_red_floats(ctx, H))
    args = D.bce_head_args(P, p, ctx.empty(D.bce_head_phase_scratch_floats(ctx, 1, H)), out, probs)
    D.bce_head_phase(ctx, args, 0, 2, red)                           # one local row of a two-row batch: served
    for bad in (dict(phase=0, count=1), dict(phase=7, count=2), dict(phase=5, count=2)):   # count < 2, no phase 7, 5 needs grads
        with pytest.raises(_lib.GcnxError) as e:
            D.bce_head_phase(ctx, args, bad["phase"], bad["count"], red)
        assert e.value.code == 1                                      # GCNX_ERR_INVALID
    small = D.bce_head_args(P, p, ctx.empty(D.bce_head_scratch_floats(ctx, 1, H)), out, probs)   # the one-launch size is too small
    with pytest.raises(_lib.GcnxError):
        D.bce_head_phase(ctx, small, 0, 2, red)


# ---- 2. gcnx_bn_act_pool_bwd_stats / _apply --------------------------------------------------------------------------------
def _pool_case(ctx, sizes, f, seed):
    from gcnx import device as D
    from gcnx.device import Segments
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, B = int(gp[-1]), len(sizes)
    z, gamma, beta, alpha, dz, mean, inv = _bn_inputs(ctx, n, f, seed=seed)
    g, b, a = ctx.to_device(gamma), ctx.to_device(beta), ctx.to_device(alpha)
    pooled, arg = ctx.empty((B, f)), ctx.empty((B, f), np.int32)
    D.bn_act_pool(ctx, Segments(ctx, gp), dz, mean, inv, g, b, pooled, arg, alpha=a)
    dp = np.random.default_rng(seed).normal(size=(B, f)).astype(np.float32)
    return dict(gp=gp, n=n, B=B, z=z, gamma=gamma, beta=beta, alpha=alpha, dz=dz, mean=mean, inv=inv, g=g, b=b, a=a, arg=arg,
                dp=dp)


@pytest.mark.parametrize("f", [16, 64, 100])
def test_pool_bwd_split_one_shard_is_bit_identical(ctx, f):
    from gcnx import device as D
    from gcnx.device import Segments
    c = _pool_case(ctx, [1, 7, 0, 120, 33, 5, 0, 64], f, seed=f)
    seg, ddp = Segments(ctx, c["gp"]), ctx.to_device(c["dp"])
    ref = {k: ctx.zeros(s) for k, s in (("dz", (c["n"], f)), ("dg", f), ("db", f), ("da", 1))}
    D.bn_act_pool_bwd(ctx, seg, ddp, c["arg"], c["dz"], c["mean"], c["inv"], c["g"], c["b"], ref["dz"], alpha=c["a"],
                      dgamma=ref["dg"], dbeta=ref["db"], dalpha=ref["da"])
    got = {k: ctx.zeros(s) for k, s in (("dz", (c["n"], f)), ("dg", f), ("db", f), ("da", 1))}
    sums = ctx.zeros(3 * f)
    D.bn_act_pool_bwd_stats(ctx, seg, ddp, c["arg"], c["dz"], c["mean"], c["inv"], c["g"], c["b"], sums, alpha=c["a"],
                            dgamma=got["dg"], dbeta=got["db"], dalpha=got["da"])
    D.bn_act_pool_bwd_apply(ctx, seg, ddp, c["arg"], c["dz"], c["mean"], c["inv"], c["g"], c["b"], sums, c["n"], got["dz"],
                            alpha=c["a"])
    for k in ref:
        assert np.array_equal(got[k].numpy().view(np.uint32), ref[k].numpy().view(np.uint32)), (f, k)


@pytest.mark.parametrize("f", [16, 100])
@pytest.mark.parametrize("gbounds", [[0, 3, 9], [0, 1, 4, 9], [0, 2, 5, 6, 9]])
def test_pool_bwd_split_on_graph_shards_against_oracle(ctx, f, gbounds):
    """Graph shards (one of one graph, empty graphs inside shards): local sums added on the host, dZ with the global row
    count, the parameter gradients summed over the shards -- against R.bn_act_pool_bwd on the whole batch."""
    from gcnx import device as D
    from gcnx.device import Segments
    sizes = [3, 0, 50, 1, 0, 40, 7, 0, 12]
    c = _pool_case(ctx, sizes, f, seed=f + len(gbounds))
    gp, arg = c["gp"], c["arg"].numpy()
    shards = []
    for g0, g1 in zip(gbounds[:-1], gbounds[1:]):
        lo, hi = int(gp[g0]), int(gp[g1])
        s = {"seg": Segments(ctx, (gp[g0:g1 + 1] - lo).astype(np.int32)), "dp": ctx.to_device(c["dp"][g0:g1]),
             "arg": ctx.to_device((arg[g0:g1] - lo).astype(np.int32)), "z": ctx.to_device(c["z"][lo:hi]),
             "sums": ctx.zeros(3 * f), "dz": ctx.zeros((hi - lo, f)), "dg": ctx.zeros(f), "db": ctx.zeros(f), "da": ctx.zeros(1)}
        assert hi > lo
        D.bn_act_pool_bwd_stats(ctx, s["seg"], s["dp"], s["arg"], s["z"], c["mean"], c["inv"], c["g"], c["b"], s["sums"],
                                alpha=c["a"], dgamma=s["dg"], dbeta=s["db"], dalpha=s["da"])
        shards.append(s)
    tot = _host_allreduce([s["sums"].numpy() for s in shards])
    for s in shards:
        s["sums"].copy_from_host(tot)
        D.bn_act_pool_bwd_apply(ctx, s["seg"], s["dp"], s["arg"], s["z"], c["mean"], c["inv"], c["g"], c["b"], s["sums"], c["n"],
                                s["dz"], alpha=c["a"])
    got = {"dz": np.concatenate([s["dz"].numpy() for s in shards])}
    for k in ("dg", "db", "da"):
        got[k] = np.sum([s[k].numpy().astype(np.float64) for s in shards], 0)
    pos = R.device_prelu_sides(c["z"], c["mean"].numpy(), c["inv"].numpy(), c["gamma"], c["beta"])
    orc = R.bn_act_pool_bwd(c["dp"].astype(np.float64), arg, c["z"], c["gamma"].astype(np.float64), c["beta"].astype(np.float64),
                            c["alpha"], gp, pos)
    for k, o in zip(("dz", "dg", "db", "da"), orc):
        assert_close(got[k], o, 1e-4, f"pool bwd shards {gbounds} f={f} {k}")


# ---- 3. the sharded model step ---------------------------------------------------------------------------------------------
def _whole_steps(hb, h, p, steps, lr):
    import gcnx
    ctx = gcnx.Context(0)
    try:
        m = gcnx.GCN(ctx, hidden_channels=h, seed=0)
        m.build(hb.f)
        m.load_state_dict(p)
        batch = _device_batch(ctx, hb)
        out = []
        for _ in range(steps):
            loss, acc = m.train_step(batch, lr=lr)
            out.append({"loss": loss, "acc": acc, "g": m.flat_g.numpy()[:m.n_params], "w": m.flat_p.numpy()})
        return out
    finally:
        ctx.close()


def _sharded_steps(hb, h, p, world, steps, lr, gbounds=None):
    """world thread ranks, each with its own Context and GCN(comm=...), train `steps` steps on their shards of hb."""
    import gcnx
    from gcnx import shard

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            if gbounds is None:
                part, gb = shard.shard_batch(hb, rank, world)
            else:
                part, gb = hb.slice_graphs(gbounds[rank], gbounds[rank + 1]), hb.n_graphs
            m = gcnx.GCN(ctx, hidden_channels=h, seed=0, comm=make_comm(ctx))
            m.build(hb.f)
            m.load_state_dict(p)
            batch = _device_batch(ctx, part)
            out = []
            for _ in range(steps):
                pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}      # the kink sides are those of the step's weights
                loss, acc = m.train_step(batch, lr=lr, global_batch=gb)
                b = m._bufs
                sides = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"],
                                                       pre[f"be{i}"]) for i in (1, 2)}
                out.append({"loss": loss, "acc": acc, "g": m.flat_g.numpy()[:m.n_params], "w": m.flat_p.numpy(),
                            "grads": m.gradients(), "sides": sides, "arg": m._bufs["arg"].numpy().astype(np.int64),
                            "n": part.n, "b": part.n_graphs, "s2_ok": m._bufs["s2_ok"], "bn_pool": m._bn_pool,
                            "calls": m.comm.calls})
            return out
        finally:
            ctx.close()

    return ThreadWorld(world).run(rank_fn)


def _check_sharded(hb, h, world, route, steps=1, gbounds=None, lr=0.05, seed=7):
    p = {k: v.astype(np.float32) for k, v in R.init_params(hb.f, h, seed=seed).items()}
    whole = _whole_steps(hb, h, p, steps, lr)
    ranks = _sharded_steps(hb, h, p, world, steps, lr, gbounds)
    assert sum(r[0]["b"] for r in ranks) == hb.n_graphs
    for s in range(steps):
        for r in ranks:
            st = r[s]
            assert st["s2_ok"] == route["s2"] and st["bn_pool"] == route["bn_pool"]
            assert abs(st["loss"] - whole[s]["loss"]) < 1e-5 * max(1.0, abs(whole[s]["loss"])), (s, st["loss"], whole[s]["loss"])
            assert st["acc"] == whole[s]["acc"], (s, st["acc"], whole[s]["acc"])
            assert rel_err(st["g"], whole[s]["g"]) < 1e-4, (s, rel_err(st["g"], whole[s]["g"]))
            assert rel_err(st["w"], whole[s]["w"]) < 1e-4, (s, rel_err(st["w"], whole[s]["w"]))
        for r in ranks[1:]:
            assert np.array_equal(r[s]["w"].view(np.uint32), ranks[0][s]["w"].view(np.uint32)), s   # identical on every rank
    # 13 all-reduces per step: BN1 / BN2 forward 4, head forward 4, head backward 2, pool backward 1, BN1 backward 1, gradients 1
    assert ranks[0][0]["calls"] == 13 and ranks[0][-1]["calls"] == 13 * steps
    # the first step against the fp64 oracle on the ranks' kink sides and argmax rows (global row numbers)
    first = [r[0] for r in ranks]
    offs = np.concatenate([[0], np.cumsum([st["n"] for st in first])])
    masks = {k: np.concatenate([st["sides"][k] for st in first]) for k in ("m1", "m2")}
    arg = np.concatenate([st["arg"] + offs[i] for i, st in enumerate(first)])
    r = R.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, hb.y, masks=masks, argmax=arg)
    _cmp_grads(first[0]["grads"], r["grads"], 1e-4, f"sharded world={world} h={h}")


MODEL_CASES = {
    # name: (host batch, hidden, world, route, kwargs)
    "ref_h64_w2": (lambda: _tiny_host(50, 16, seed=11), 64, 2, dict(s2=True, bn_pool=True), {}),
    "ref_h64_w4": (lambda: _tiny_host(50, 16, seed=11), 64, 4, dict(s2=True, bn_pool=True), {}),
    "h100_w2": (lambda: _tiny_host(20, 16, seed=14), 100, 2, dict(s2=False, bn_pool=True), {}),
    "one_graph_shard_w4": (lambda: _tiny_host(12, 16, seed=3), 64, 4, dict(s2=True, bn_pool=True), dict(gbounds=[0, 1, 5, 11, 12])),
    "empty_graphs_w2": (lambda: _with_empty_graphs(_tiny_host(12, 16, seed=21), 1), 64, 2, dict(s2=True, bn_pool=True), {}),
    "three_steps_w2": (lambda: _tiny_host(24, 16, seed=5), 48, 2, dict(s2=False, bn_pool=True), dict(steps=3)),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_gcn_sync_bn_step_equals_the_whole_batch(case):
    build, h, world, route, kw = MODEL_CASES[case]
    _check_sharded(build(), h, world, route, **kw)


@pytest.mark.parametrize("h,s2", [(64, True), (100, False)])
def test_gcn_sync_bn_step_unfused_pool(monkeypatch, h, s2):
    monkeypatch.setenv("GCNX_BN_POOL", "0")
    _check_sharded(_tiny_host(20, 16, seed=8), h, 2, dict(s2=s2, bn_pool=False), steps=2)


# ---- 4. semantics --------------------------------------------------------------------------------------------------------
def test_forward_and_evaluate_with_a_communicator_keep_per_rank_statistics():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16, seed=9)

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            part, _ = shard.shard_batch(hb, rank, 2)
            a = gcnx.GCN(ctx, seed=2, comm=make_comm(ctx))
            b = gcnx.GCN(ctx, seed=2)
            batch = _device_batch(ctx, part)
            la, lb = a(batch), b(batch)
            ea, eb = a.evaluate_batch(batch, part.y), b.evaluate_batch(batch, part.y)
            assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
            assert ea[0] == eb[0] and ea[1] == eb[1] and np.array_equal(ea[2], eb[2])
            assert a.comm.calls == 0
            return True
        finally:
            ctx.close()

    assert ThreadWorld(2).run(rank_fn) == [True, True]


def test_global_batch_of_one_graph_raises_on_every_rank():
    import gcnx
    hb = _tiny_host(2, 16, seed=10)
    one = hb.slice_graphs(0, 1)
    errors = []

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            part = one if rank == 0 else one.slice_graphs(1, 1)       # rank 1 holds nothing: the batch has one graph
            m = gcnx.GCN(ctx, seed=0, comm=make_comm(ctx))
            m.build(16)
            try:
                m.train_step(_device_batch(ctx, part), lr=0.01)
            except ValueError as e:
                errors.append((rank, str(e)))
            return True
        finally:
            ctx.close()

    ThreadWorld(2).run(rank_fn)
    assert sorted(r for r, _ in errors) == [0, 1]
    assert all("Expected more than 1 value per channel when training" in msg for _, msg in errors)

    errors.clear()

    def rank_fn2(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            m = gcnx.GCN(ctx, seed=0, comm=make_comm(ctx))
            m.build(16)
            try:
                m.train_step(_device_batch(ctx, one), lr=0.01)     # one graph on each rank, but the batch lists it once
            except ValueError as e:
                errors.append((rank, str(e)))
            return True
        finally:
            ctx.close()

    # one graph per rank makes a global batch of two: that trains
    ThreadWorld(2).run(rank_fn2)
    assert errors == []


def test_world_size_one_communicator_is_bit_identical_to_none():
    import gcnx
    hb = _tiny_host(16, 16, seed=12)
    res = []

    def run(comm_factory):
        ctx = gcnx.Context(0)
        try:
            m = gcnx.GCN(ctx, seed=4, comm=comm_factory(ctx))
            batch = _device_batch(ctx, hb)
            for _ in range(2):
                m.train_step(batch, lr=0.05)
            return m.flat_g.numpy().view(np.uint32).copy(), m.flat_p.numpy().view(np.uint32).copy()
        finally:
            ctx.close()

    res.append(ThreadWorld(1).run(lambda rank, make_comm: run(make_comm))[0])
    res.append(run(lambda ctx: None))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])

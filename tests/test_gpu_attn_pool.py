"""GPU tests of the learned readout: the kernels of csrc/attn_pool.hip (gcnx_attn_pool on its whole and sliced routes,
gcnx_attn_pool_bwd), the layer gcnx.GlobalAttnSumPool and the models with readout="attention" -- each against the float64 oracle
tests/attn_pool_ref.py, the models on the device's side of every kink.  Tolerances: TIGHT = 2e-5 for a single fp32 kernel,
1e-4 for a whole step.

Routes: ``None`` = the whole route (one workgroup per graph: slice_rows = 0 without scratch), 0 = the library's choice with
scratch, 32 and 7 = slices of that many rows (7: more slices than row groups, slices that end inside a wave's rows)."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import attn_pool_ref as AR
import gat_ref as GR
import gcn_bn_ref as R
from gpu_frames import SENTINEL, Frame, same
from test_gpu_gcn_bn import _cmp_grads, _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SIZES = [1, 0, 3, 65, 64, 130]
WIDTHS = [16, 48, 64, 128, 256, 10]          # 10: the scalar route
ROUTES = (None, 0, 32, 7)


@functools.lru_cache(maxsize=None)
def _case(kind, f):
    """(graph_ptr, x, a, dp) and the oracle's (pooled, alpha, dx, da), computed once and never modified.  x unit-scale,
    a ~ N(0, 1) / sqrt(f): the softmax neither flat nor saturated."""
    rng = np.random.default_rng(100 + f)
    if kind == "sizes":
        gp = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        x = rng.standard_normal((int(gp[-1]), f)).astype(np.float32)
    else:
        from gcnx import synth
        hb = synth.ecoli_batch(3, f)
        assert hb.n % 32 != 0 and hb.n > 1024
        gp, x = hb.graph_ptr.astype(np.int32), hb.x.astype(np.float32)
    a = (rng.standard_normal(f) / np.sqrt(f)).astype(np.float32)
    dp = rng.standard_normal((len(gp) - 1, f)).astype(np.float32)
    P, alpha = AR.forward(x, a, gp)
    dx, da = AR.backward(x, a, gp, dp, alpha, P)
    for v in (gp, x, a, dp, P, alpha, dx, da):
        v.setflags(write=False)
    return gp, x, a, dp, P, alpha, dx, da


class _Dev:
    """The operands of one case on the device, and the two calls."""

    def __init__(self, ctx, gp, x, a, dp=None):
        from gcnx.device import Segments
        self.ctx, self.seg, self.n, self.b, self.f = ctx, Segments(ctx, gp), x.shape[0], len(gp) - 1, x.shape[1]
        self.x, self.a = ctx.to_device(x), ctx.to_device(a)
        self.dp = ctx.to_device(dp) if dp is not None else None

    def scratch(self, route):
        from gcnx import device as D
        return None if route is None else self.ctx.empty(max(D.attn_pool_scratch_floats(self.ctx, self.n, self.b, self.f, route), 4))

    def fwd(self, route, with_alpha=True):
        from gcnx import device as D
        pooled = self.ctx.to_device(np.full((self.b, self.f), SENTINEL, np.float32))
        alpha = self.ctx.to_device(np.full(self.n, SENTINEL, np.float32)) if with_alpha else None
        D.attn_pool(self.ctx, self.seg, self.x, self.a, pooled, alpha, self.scratch(route), route or 0)
        return pooled, alpha

    def bwd(self, pooled, alpha, dx=True, da=True):
        from gcnx import device as D
        ddx = self.ctx.to_device(np.full((self.n, self.f), SENTINEL, np.float32)) if dx else None
        dda = self.ctx.to_device(np.full(self.f, SENTINEL, np.float32)) if da else None
        D.attn_pool_bwd(self.ctx, self.seg, self.x, self.a, alpha, pooled, self.dp, ddx, dda, self.scratch(0) if da else None)
        return ddx, dda


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("kind", ["sizes", "ecoli3"])
def test_forward_against_float64_on_every_route(ctx, kind, f):
    gp, x, a, _, P, alpha, _, _ = _case(kind, f)
    d = _Dev(ctx, gp, x, a)
    got = {}
    for route in ROUTES:
        pooled, al = d.fwd(route)
        got[route] = pooled.numpy(), al.numpy()
        what = f"{kind} f={f} route={route}"
        print(f"{what}: pooled {rel_err(got[route][0], P):.2e} alpha {rel_err(got[route][1], alpha):.2e}")
        assert_close(got[route][0], P, TIGHT, what + " pooled")
        assert_close(got[route][1], alpha, TIGHT, what + " alpha")
        if kind == "sizes":
            assert not got[route][0][1].any(), what + ": the empty graph's row is exactly 0"
            assert got[route][1][0] == 1.0 and np.array_equal(got[route][0][0], x[0]), what + ": the one-row graph"
        # without alpha: the same pooled rows, bit for bit
        assert same(d.fwd(route, with_alpha=False)[0].numpy(), got[route][0]), what + " alpha=None"
    for route in ROUTES[1:]:
        assert_close(got[route][0], got[None][0], TIGHT, f"{kind} f={f} pooled route {route} vs whole")
        assert_close(got[route][1], got[None][1], TIGHT, f"{kind} f={f} alpha route {route} vs whole")


def test_tall_graphs_take_the_sliced_route_by_themselves(ctx):
    """Two graphs of 8 192 rows (the config-5 shape): slice_rows = 0 cuts them into 64-row slices on any device of 128 CUs or more
    (the same launches, so the same bits, as slice_rows = 64), and every route matches float64."""
    rng = np.random.default_rng(5)
    gp = np.array([0, 8192, 16384], np.int32)
    x = rng.standard_normal((16384, 64)).astype(np.float32)
    a = (rng.standard_normal(64) / 8).astype(np.float32)
    dp = rng.standard_normal((2, 64)).astype(np.float32)
    P, alpha = AR.forward(x, a, gp)
    dx, da = AR.backward(x, a, gp, dp, alpha, P)
    d = _Dev(ctx, gp, x, a, dp)
    got = {route: d.fwd(route) for route in (None, 0, 64)}
    for route, (pooled, al) in got.items():
        assert_close(pooled.numpy(), P, TIGHT, f"tall route={route} pooled")
        assert_close(al.numpy(), alpha, TIGHT, f"tall route={route} alpha")
    assert ctx.info()["cus"] < 128 or (same(got[0][0].numpy(), got[64][0].numpy()) and same(got[0][1].numpy(), got[64][1].numpy()))
    gx, ga = d.bwd(*got[0])
    assert_close(gx.numpy(), dx, TIGHT, "tall dx")
    assert_close(ga.numpy(), da, TIGHT, "tall da")


# ---- 2. extremes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_zero_gate_is_the_mean_pool(ctx, route):
    from gcnx import device as D
    gp, x, _, _, _, _, _, _ = _case("sizes", 64)
    d = _Dev(ctx, gp, x, np.zeros(64, np.float32))
    pooled, alpha = d.fwd(route)
    avg = ctx.empty((d.b, 64))
    D.segment_pool(ctx, d.seg, d.x, avg, "avg")
    assert_close(pooled.numpy(), avg.numpy(), TIGHT, f"a = 0 route={route}")
    sizes = np.repeat(np.diff(gp), np.diff(gp))
    assert_close(alpha.numpy(), 1.0 / sizes, TIGHT, "uniform alpha")


@pytest.mark.parametrize("route", ROUTES)
def test_large_scores_stay_finite_and_match(ctx, route):
    gp, x, a, dp, _, _, _, _ = _case("ecoli3", 64)
    s = x.astype(np.float64) @ a.astype(np.float64)
    big = (a * np.float32(100.0 / np.max(np.abs(s)))).astype(np.float32)
    assert 99.0 < np.max(np.abs(x.astype(np.float64) @ big.astype(np.float64))) < 101.0
    P, alpha = AR.forward(x, big, gp)
    d = _Dev(ctx, gp, x, big, dp)
    pooled, al = d.fwd(route)
    got_p, got_a = pooled.numpy(), al.numpy()
    print(f"|s| ~ 100 route={route}: pooled {rel_err(got_p, P):.2e} alpha {rel_err(got_a, alpha):.2e}")
    assert np.isfinite(got_p).all() and np.isfinite(got_a).all()
    assert_close(got_p, P, TIGHT, "pooled at |s| ~ 100")
    assert_close(got_a, alpha, TIGHT, "alpha at |s| ~ 100")
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(100.0)) == np.inf            # what a kernel without the subtraction would sum
    # the backward at this scale: da is a cancellation (the float32 restatement alone is off by 3e-3), so finiteness only
    dx, da = d.bwd(pooled, al)
    assert np.isfinite(dx.numpy()).all() and np.isfinite(da.numpy()).all()


# ---- 3. backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("kind", ["sizes", "ecoli3"])
def test_backward_against_float64(ctx, kind, f):
    gp, x, a, dp, _, _, dx, da = _case(kind, f)
    d = _Dev(ctx, gp, x, a, dp)
    for route in ROUTES:                  # alpha and pooled as each forward route wrote them
        pooled, alpha = d.fwd(route)
        gx, ga = d.bwd(pooled, alpha)
        what = f"{kind} f={f} route={route}"
        print(f"{what}: dx {rel_err(gx.numpy(), dx):.2e} da {rel_err(ga.numpy(), da):.2e}")
        assert_close(gx.numpy(), dx, TIGHT, what + " dx")
        assert_close(ga.numpy(), da, TIGHT, what + " da")
        if route in (None, 7):
            only_a = d.bwd(pooled, alpha, dx=False)
            only_x = d.bwd(pooled, alpha, da=False)
            assert only_a[0] is None and same(only_a[1].numpy(), ga.numpy()), what + " dx=None"
            assert only_x[1] is None and same(only_x[0].numpy(), gx.numpy()), what + " da=None"


# ---- 4. strides and frames ------------------------------------------------------------------------------------------------------
def _frame_check(fr, want, tol, what):
    got = fr.buf.numpy()
    body = fr._body(got)
    assert rel_err(body[:, :fr.f], want) < tol, (what, rel_err(body[:, :fr.f], want))
    assert (body[:, fr.f:] == SENTINEL).all() and (got[:fr.lead] == SENTINEL).all() \
        and (got[fr.lead + fr.n * fr.ld:] == SENTINEL).all(), (what, "written outside the view")


@pytest.mark.parametrize("route", [None, 32, 7])
@pytest.mark.parametrize("f,pad,lead", [(64, 8, 4), (10, 3, 3)])
def test_strided_operands_inside_sentinel_frames(ctx, f, pad, lead, route):
    """f = 64: float4 lanes on aligned views; f = 10: scalar lanes on views off every 16-byte boundary."""
    from gcnx import device as D
    from gcnx.device import Segments
    gp, x, a, dp, P, alpha, dx, da = _case("ecoli3", f)
    n, b = x.shape[0], len(gp) - 1
    seg = Segments(ctx, gp)
    fx = Frame(ctx, n, f, 2 * f + pad, lead, data=x)              # x: a column view of a buffer more than twice as wide
    f_p, f_dp, f_dx = Frame(ctx, b, f, f + pad, lead), Frame(ctx, b, f, f + 2 * pad, lead, data=dp), Frame(ctx, n, f, f + pad, lead)
    f_al, f_da = Frame(ctx, n, 1, 1, 4), Frame(ctx, 1, f, f, 4)
    ns = max(D.attn_pool_scratch_floats(ctx, n, b, f, route or 0), 4)
    f_s = Frame(ctx, 1, ns, ns, 4)                                # the scratch too: nothing is written past what was asked for
    assert all(fr.aligned() for fr in (fx, f_p, f_dp, f_dx)) == (f == 64) and f_s.aligned()
    da_dev = ctx.to_device(a)
    al_view, da_view = f_al.view.flat(0, n), f_da.view.flat(0, f)
    D.attn_pool(ctx, seg, fx.view, da_dev, f_p.view, al_view, f_s.view.flat(0, ns) if route is not None else None, route or 0)
    _frame_check(f_p, P, TIGHT, "pooled")
    _frame_check(f_al, alpha[:, None], TIGHT, "alpha")
    D.attn_pool_bwd(ctx, seg, fx.view, da_dev, al_view, f_p.view, f_dp.view, f_dx.view, da_view, f_s.view.flat(0, ns))
    _frame_check(f_dx, dx, TIGHT, "dx")
    _frame_check(f_da, da[None, :], TIGHT, "da")
    _frame_check(f_p, P, TIGHT, "pooled is not written by the backward")
    f_s.numpy()                                                   # asserts the sentinels around the scratch
    fx.untouched("x")
    f_dp.untouched("dpooled")


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [None, 32])
def test_two_calls_give_the_same_bits(ctx, route):
    gp, x, a, dp, _, _, _, _ = _case("ecoli3", 64)
    d = _Dev(ctx, gp, x, a, dp)
    p1, a1 = d.fwd(route)
    p2, a2 = d.fwd(route)
    assert same(p1.numpy(), p2.numpy()) and same(a1.numpy(), a2.numpy())
    x1, g1 = d.bwd(p1, a1)
    x2, g2 = d.bwd(p2, a2)
    assert same(x1.numpy(), x2.numpy()) and same(g1.numpy(), g2.numpy())


def test_captured_replay_is_bit_identical(ctx):
    """Nothing is allocated and nothing synchronises: the sliced forward and the backward (four launches, a linear graph) are
    captured and replayed, and leave the bits of the eager calls."""
    from gcnx import device as D
    gp, x, a, dp, _, _, _, _ = _case("ecoli3", 64)
    d = _Dev(ctx, gp, x, a, dp)
    p_e, a_e = d.fwd(32)
    x_e, g_e = d.bwd(p_e, a_e)
    pooled, alpha, dx, da = ctx.zeros((d.b, 64)), ctx.zeros(d.n), ctx.zeros((d.n, 64)), ctx.zeros(64)
    scratch = d.scratch(32)

    def seq():
        D.attn_pool(ctx, d.seg, d.x, d.a, pooled, alpha, scratch, 32)
        D.attn_pool_bwd(ctx, d.seg, d.x, d.a, alpha, pooled, d.dp, dx, da, scratch)

    g = ctx.capture(seq)
    try:
        assert not pooled.numpy().any()                                   # captured, not yet executed
        for _ in range(2):
            for t in (pooled, alpha, dx, da):
                t.fill_zero()
            g.launch()
            assert same(pooled.numpy(), p_e.numpy()) and same(alpha.numpy(), a_e.numpy())
            assert same(dx.numpy(), x_e.numpy()) and same(da.numpy(), g_e.numpy())
    finally:
        g.destroy()


def test_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import Segments
    gp, x, a, dp, _, _, _, _ = _case("sizes", 16)
    d = _Dev(ctx, gp, x, a, dp)
    pooled, alpha = d.fwd(None)
    lib, h = ctx.lib, ctx.h
    bad = [lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 16, d.a.ptr, d.n, d.b, 16, 8, pooled.ptr, 16, alpha.ptr, None),   # slices, no scratch
           lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 16, d.a.ptr, -1, d.b, 16, 0, pooled.ptr, 16, alpha.ptr, None),
           lib.gcnx_attn_pool(h, d.seg.dev.ptr, None, 16, d.a.ptr, d.n, d.b, 16, 0, pooled.ptr, 16, alpha.ptr, None),
           lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 8, d.a.ptr, d.n, d.b, 16, 0, pooled.ptr, 16, alpha.ptr, None),          # ldx < f
           lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 300, d.a.ptr, d.n, d.b, 300, 0, pooled.ptr, 300, alpha.ptr, None),      # f > 256
           lib.gcnx_attn_pool_bwd(h, d.seg.dev.ptr, d.x.ptr, 16, d.a.ptr, None, pooled.ptr, 16, d.dp.ptr, 16, d.n, d.b, 16, None, 0,
                                  None, None)]
    assert bad == [_lib.OK + 1] * len(bad)                        # GCNX_ERR_INVALID, nothing launched
    before = pooled.numpy()
    assert lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 16, d.a.ptr, 0, d.b, 16, 0, pooled.ptr, 16, alpha.ptr, None) == _lib.OK
    assert lib.gcnx_attn_pool(h, d.seg.dev.ptr, d.x.ptr, 16, d.a.ptr, d.n, 0, 16, 0, pooled.ptr, 16, alpha.ptr, None) == _lib.OK
    assert same(pooled.numpy(), before)                           # n == 0 or b == 0 writes nothing


# ---- 6. the layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True])
def test_layer_forward_and_backward(ctx, ids):
    import gcnx
    gp, x, a, dp, P, _, dx, da = _case("sizes", 48)
    layer = gcnx.GlobalAttnSumPool(seed=5)
    seg = np.repeat(np.arange(len(gp) - 1), np.diff(gp)) if ids else gcnx.Segments(ctx, gp)
    if ids:                               # graph ids cannot name a trailing empty graph; SIZES ends with a full one
        assert np.diff(gp)[-1] > 0
    dev_x = ctx.to_device(x)
    first = layer((dev_x, seg))
    assert first.shape == (len(gp) - 1, 48) and layer.get_weights()[0].shape == (48, 1)
    k0 = layer.get_weights()[0]
    P0, _ = AR.forward(x, k0, gp)
    assert_close(first.numpy(), P0, TIGHT, "layer forward, its own initial kernel")
    layer.set_weights([a[:, None]])
    pooled = layer((dev_x, seg))
    assert_close(pooled.numpy(), P, TIGHT, "layer forward")
    got_dx = layer.backward(ctx.to_device(dp))
    assert_close(got_dx.numpy(), dx, TIGHT, "layer dx")
    assert layer.grads["attn_kernel"].shape == (48, 1)
    assert_close(layer.grads["attn_kernel"].numpy()[:, 0], da, TIGHT, "layer d attn_kernel")
    assert layer.backward(ctx.to_device(dp), need_dx=False) is None


# ---- 7. the models --------------------------------------------------------------------------------------------------------------
def _sides(m, hb, gat, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    s = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
         for i in (1, 2)}
    if gat:
        s.update({f"e{i}": GR.device_score_sides(b[f"asrc{i}"].numpy(), b[f"adst{i}"].numpy(), hb.rowptr, hb.colidx) for i in (1, 2)})
    return s


def _make(ctx, heads, comm=None):
    import gcnx
    if heads is None:
        return gcnx.GCN(ctx, hidden_channels=64, seed=0, readout="attention", comm=comm)
    return gcnx.GAT(ctx, hidden_channels=64, heads=heads, seed=0, readout="attention", comm=comm)


@pytest.mark.parametrize("heads", [None, 4], ids=["GCN", "GAT-heads4"])
def test_model_step_against_oracle(ctx, heads):
    hb = _tiny_host(16, 16, seed=4)
    batch, a = _device_batch(ctx, hb), _scipy_adj(hb)
    m = _make(ctx, heads)
    p = {k: v.astype(np.float32) for k, v in AR.init_params(16, 64, seed=7, heads=heads).items()}
    m.load_state_dict(p)
    what = "GCN" if heads is None else f"GAT heads={heads}"
    m.loss_and_grads(batch)
    for k in ("y2", "dy2", "alpha", "attn"):
        assert k in m._bufs, k
    r = AR.model(hb.x, a, hb.graph_ptr, p, hb.y, masks=_sides(m, hb, heads is not None), heads=heads)
    assert_close(m._bufs["alpha"].numpy(), r["alpha"], 1e-4, f"{what} alpha")
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < 1e-4 and la[1] == r["hits"], (la, r["loss"], r["hits"])
    grads = m.gradients()
    assert list(grads)[-1] == AR.GATE_KEY and set(grads) == set(r["grads"])
    _cmp_grads(grads, r["grads"], 1e-4, what)
    # the update: p - lr g of the step's own gradients, and the oracle's SGD step on the device's kink sides of that step
    w0 = m.flat_p.numpy()
    loss, _ = m.train_step(batch, lr=0.05)
    assert rel_err(loss, r["loss"]) < 1e-4
    g = m.flat_g.numpy()[:m.n_params]
    assert_close(m.flat_p.numpy(), w0 - np.float32(0.05) * g, 1e-6, f"{what} p - lr g")
    ph = R.sgd({k: v.astype(np.float64) for k, v in p.items()}, r["grads"], 0.05)
    sd = m.state_dict()
    for k in ph:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after the step {k}")
    # evaluation: the probabilities are the sigmoid of the logits of __call__
    logits = m(batch)
    loss_e, acc_e, probs = m.evaluate_batch(batch, None)
    assert_close(probs, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), 1e-6, f"{what} probabilities")
    assert np.isfinite(loss_e) and 0.0 <= acc_e <= 1.0


def test_readout_max_runs_the_launches_it_ran(ctx):
    """readout="max" passed explicitly: the same bits as the default, and none of the readout's buffers."""
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    batch = _device_batch(ctx, hb)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 64, seed=7).items()}
    res = []
    for kw in ({}, {"readout": "max"}):
        m = gcnx.GCN(ctx, hidden_channels=64, seed=0, **kw)
        m.load_state_dict(p)
        m.loss_and_grads(batch)
        assert "ar" not in m.p and not {"dy2", "alpha", "attn"} & set(m._bufs)
        res.append((m._bufs["out"].numpy(), m.flat_g.numpy()))
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])


# ---- 8. sync-BN over graph shards -------------------------------------------------------------------------------------------------
def test_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in AR.init_params(16, 64, seed=7).items()}

    def step(ctx, part, comm, gb):
        m = _make(ctx, None, comm)
        m.build(hb.f)
        m.load_state_dict(p)
        loss, acc = m.train_step(_device_batch(ctx, part), lr=0.05, global_batch=gb)
        return {"loss": loss, "acc": acc, "g": m.gradients(), "w": m.flat_p.numpy(), "b": part.n_graphs}

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            part, gb = shard.shard_batch(hb, rank, 2)
            return step(ctx, part, make_comm(ctx), gb)
        finally:
            ctx.close()

    ctx = gcnx.Context(0)
    try:
        whole = step(ctx, hb, None, None)
    finally:
        ctx.close()
    ranks = ThreadWorld(2).run(rank_fn)
    assert sum(r["b"] for r in ranks) == hb.n_graphs and all(r["b"] > 0 for r in ranks)
    for r in ranks:
        assert abs(r["loss"] - whole["loss"]) < 1e-5 * max(1.0, abs(whole["loss"])), (r["loss"], whole["loss"])
        assert r["acc"] == whole["acc"]
        _cmp_grads(r["g"], whole["g"], 1e-4, "sync-BN")
        assert rel_err(r["w"], whole["w"]) < 1e-4
    assert same(ranks[0]["w"], ranks[1]["w"])

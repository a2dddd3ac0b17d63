"""GPU tests of the device optimizers (csrc/optim.hip, gcnx/optim.py): gcnx_grad_sqnorm, gcnx_adam and gcnx_sgd_momentum
against the fp64 restatement tests/optim_ref.py, and gcnx.Adam behind every model.

Bounds, with U = 2^-24 (the unit roundoff of fp32) and every reference value in fp64 from the fp32 inputs:
  norm   |norm - ref| <= k U ref, k = optim_ref.norm_chain(n, n_partials): the longest addition chain of the documented order
         (the sum's relative error is at most k U over non-negative terms; the square root halves it and adds one rounding);
  m      |m - ref| <= 4 U (|b1 m0| + |(1 - b1) g'|);        v   the same with 6 U and the summands of v;
  p      |p - ref| <= U |ref| + 32 U |u|, u = what the step subtracts from p: the Adam term, and with weight_decay also
         lr wd p0 -- the two in absolute value, |u| = |lr wd p0| + |Adam term| (the kernel forms their sum with one fma and
         subtracts it from p with one rounding).  About 14 roundings lie on the path to the Adam term, doubled.
  SGD    |p - ref|, |vel - ref| <= 3 U (|p0| + |vel0| + |lr g'|).
In the clipped cases the oracle takes the clip factor from the norm the DEVICE reported (which has its own check above).
The bound on p presumes that the Adam term carries a RELATIVE error, also where b1 m0 and (1 - b1) g' cancel in m (the kernel
cases draw the sign of m0 independently of g's, and a model's noise-only gradients do it by themselves): gcnx_adam keeps the
rounded product of m as a hi + lo pair for that, so that m ends within 2 U of itself."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import golden_batch, load_golden
import optim_ref as OR
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

U = OR.U
SIZES = [1, 3, 255, 257, 2048 * 256 + 37]          # the last one passes the grid caps: threads loop


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _host_state(n, seed=0):
    """(p, g, m, v, vel) fp32, never modified: |g| and |m| log-uniform in [1e-6, 1e2] with independent signs, v >= 0."""
    rng = np.random.default_rng(1000 * seed + n % 997)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    m = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 2, n)).astype(np.float32)
    v = (10.0 ** rng.uniform(-12, 4, n)).astype(np.float32)
    vel = (0.1 * rng.standard_normal(n)).astype(np.float32)
    for a in (p, g, m, v, vel):
        a.setflags(write=False)
    return p, g, m, v, vel


class _Dev:
    """Device copies of a host state as views at element ``off`` of larger buffers (off = 1: no 16-byte alignment)."""

    def __init__(self, ctx, arrays, off):
        self.bufs = []
        for a in arrays:
            b = ctx.zeros(a.size + 8)
            v = b.flat(off, a.size)
            v.copy_from_host(a)
            self.bufs.append(v)
            assert (v.ptr % 16 == 0) == (off % 4 == 0)


def _assert_adam(got_p, got_m, got_v, p0, g, m0, v0, t, lr, norm, what, **hyper):
    p_ref, m_ref, v_ref, info = OR.adam(p0, g, m0, v0, t, lr, norm=norm, **hyper)
    em, ev, ep = np.abs(got_m - m_ref), np.abs(got_v - v_ref), np.abs(got_p - p_ref)
    bm, bv = 4 * U * info["m_terms"], 6 * U * info["v_terms"]
    bp = U * np.abs(p_ref) + 32 * U * (np.abs(info["update"]) + np.abs(info["decay"]))
    worst = lambda e, b: float(np.max(e / np.maximum(b, 1e-300))) if e.size else 0.0
    print(f"{what}: worst error / bound  m {worst(em, bm):.3f}  v {worst(ev, bv):.3f}  p {worst(ep, bp):.3f}")
    assert np.all(em <= bm), (what, "m", worst(em, bm))
    assert np.all(ev <= bv), (what, "v", worst(ev, bv))
    assert np.all(ep <= bp), (what, "p", worst(ep, bp))
    return p_ref, m_ref, v_ref, info


def _assert_norm(norm_dev, g, n_partials, what):
    ref = OR.grad_norm(g)
    k = OR.norm_chain(g.size, n_partials)
    print(f"{what}: norm {norm_dev!r} ref {ref!r} rel {abs(norm_dev - ref) / ref:.3e} bound {k * U:.3e}")
    assert abs(norm_dev - ref) <= k * U * ref, (what, norm_dev, ref, k)


# ---- 1. the kernels, one step from a random state ---------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_against_float64(ctx, n, off):
    from gcnx import device as D
    p0, g, m0, v0, _ = _host_state(n)
    lr = 1e-2
    t_dev, partials, norm_out = ctx.zeros(1, np.int32), ctx.zeros(256), ctx.zeros(1)
    for t in (1, 2, 1000):
        for wd in (0.0, 0.01):
            for clip in (None, "on"):
                d = _Dev(ctx, (p0, g, m0, v0), off)
                p, gd, m, v = d.bufs
                t_dev.copy_from_host(np.asarray([t - 1], np.int32))
                D.counter_add(ctx, t_dev, 1)
                k, norm, c = 0, None, None
                if clip:
                    c = 0.25 * OR.grad_norm(g)                       # below the norm: the clip is active
                    k = D.grad_sqnorm(ctx, gd, partials)
                    assert k == D.grad_sqnorm_partials(n) == min(256, -(-n // 256))
                D.adam(ctx, p, gd, m, v, t_dev, lr, weight_decay=wd, partials=partials if clip else None, n_partials=k, clipnorm=c,
                       norm_out=norm_out if clip else None)
                what = f"adam n={n} off={off} t={t} wd={wd} clip={clip}"
                if clip:
                    norm = float(norm_out.numpy()[0])
                    _assert_norm(norm, g, k, what)
                _, _, _, info = _assert_adam(p.numpy(), m.numpy(), v.numpy(), p0, g, m0, v0, t, lr, norm, what, weight_decay=wd,
                                             clipnorm=c)
                assert (info["s"] < 1.0) == bool(clip)
                assert np.array_equal(_bits(gd.numpy()), _bits(g)), "the update wrote the gradients"
                assert int(t_dev.numpy().view(np.uint32)[0]) == t


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_momentum_step_against_float64(ctx, n, off):
    from gcnx import device as D
    p0, g, _, _, vel0 = _host_state(n)
    lr = 0.02
    partials, norm_out = ctx.zeros(256), ctx.zeros(1)
    for nesterov in (False, True):
        for clip in (None, "on"):
            p, gd, vel = _Dev(ctx, (p0, g, vel0), off).bufs
            k, norm, c = 0, None, None
            if clip:
                c = 0.25 * OR.grad_norm(g)
                k = D.grad_sqnorm(ctx, gd, partials)
            D.sgd_momentum(ctx, p, gd, vel, lr, momentum=0.9, nesterov=nesterov, partials=partials if clip else None, n_partials=k,
                           clipnorm=c, norm_out=norm_out if clip else None)
            what = f"sgd_momentum n={n} off={off} nesterov={nesterov} clip={clip}"
            if clip:
                norm = float(norm_out.numpy()[0])
                _assert_norm(norm, g, k, what)
            p_ref, vel_ref, info = OR.sgd_momentum(p0, g, vel0, lr, momentum=0.9, nesterov=nesterov, clipnorm=c, norm=norm)
            bound = 3 * U * (np.abs(p0.astype(np.float64)) + np.abs(vel0.astype(np.float64)) + np.abs(info["lr_g"]))
            ep, ev = np.abs(p.numpy() - p_ref), np.abs(vel.numpy() - vel_ref)
            print(f"{what}: worst error / bound  p {float(np.max(ep / bound)):.3f}  vel {float(np.max(ev / bound)):.3f}")
            assert np.all(ep <= bound) and np.all(ev <= bound), what
            assert np.array_equal(_bits(gd.numpy()), _bits(g))


def test_sgd_without_momentum_is_the_plain_sgd_launch(ctx):
    """gcnx.SGD() (no momentum, no clipnorm) behind a model's flat buffers calls gcnx_sgd: the bits of D.sgd, and no velocity."""
    from gcnx import device as D
    n = 257
    p0, g, _, _, _ = _host_state(n)
    pa, gd = ctx.to_device(p0), ctx.to_device(g)
    D.sgd(ctx, pa, gd, 0.02)

    class _Flat:                                             # the part of a model an optimizer steps on
        pass
    m = _Flat()
    m.ctx, m.n_params, m.flat_p, m.flat_g = ctx, n, ctx.to_device(p0), ctx.to_device(np.concatenate([g, [0, 0]]).astype(np.float32))
    import gcnx
    opt = gcnx.SGD()
    opt.step(m, 0.02)
    assert np.array_equal(_bits(m.flat_p.numpy()), _bits(pa.numpy())) and opt.state_dict() == {"t": 1}


def test_padding_stays_zero_under_weight_decay(ctx):
    from gcnx import device as D
    n = 64
    p0, g0, m0, v0, _ = (a.copy() for a in _host_state(n))
    pad = np.arange(n) % 4 == 3
    for a in (p0, g0, m0, v0):
        a[pad] = 0.0
    p, g, m, v = (ctx.to_device(a) for a in (p0, g0, m0, v0))
    t = ctx.to_device(np.asarray([0], np.int32))
    for _ in range(3):
        D.counter_add(ctx, t, 1)
        D.adam(ctx, p, g, m, v, t, 1e-2, weight_decay=0.1)
    for a in (p, m, v):
        h = a.numpy()
        assert np.all(_bits(h[pad]) == 0) and np.all(h[~pad] != 0)


def test_captured_replays_equal_eager_calls_bitwise(ctx):
    from gcnx import device as D
    n = 2048 + 37
    host = _host_state(n)[:4]
    g = host[1]

    def make():
        p, gd, m, v = (ctx.to_device(a) for a in host)
        return dict(p=p, g=gd, m=m, v=v, t=ctx.zeros(1, np.int32), part=ctx.zeros(256), norm=ctx.zeros(1))

    def step(s):
        D.counter_add(ctx, s["t"], 1)
        k = D.grad_sqnorm(ctx, s["g"], s["part"])
        D.adam(ctx, s["p"], s["g"], s["m"], s["v"], s["t"], 1e-2, weight_decay=0.01, partials=s["part"], n_partials=k,
               clipnorm=0.25 * OR.grad_norm(g), norm_out=s["norm"])

    eager, replay = make(), make()
    for _ in range(5):
        step(eager)
    graph = ctx.capture(lambda: step(replay))
    try:
        for _ in range(5):
            graph.launch()
        for k in ("p", "m", "v", "norm", "part"):
            assert np.array_equal(_bits(eager[k].numpy()), _bits(replay[k].numpy())), k
        assert int(eager["t"].numpy()[0]) == int(replay["t"].numpy()[0]) == 5
    finally:
        graph.destroy()


def test_lr_source_changes_a_captured_step(ctx):
    from gcnx import device as D
    n = 300
    host = _host_state(n)[:4]
    lrs = (1e-2, 3e-3, 1e-2, 5e-4)

    def make():
        p, gd, m, v = (ctx.to_device(a) for a in host)
        return dict(p=p, g=gd, m=m, v=v, t=ctx.zeros(1, np.int32))

    def step(s, lr):
        D.counter_add(ctx, s["t"], 1)
        D.adam(ctx, s["p"], s["g"], s["m"], s["v"], s["t"], lr)

    eager, replay = make(), make()
    for lr in lrs:
        step(eager, lr)
    lr_buf = ctx.zeros(1)
    ctx.set_lr_source(lr_buf)
    try:
        graph = ctx.capture(lambda: step(replay, 123.0))        # (the argument is ignored while a source is set)
    finally:
        ctx.set_lr_source(None)
    try:
        for lr in lrs:
            lr_buf.copy_from_host(np.asarray([lr], np.float32))
            graph.launch()
        ctx.sync()
    finally:
        graph.destroy()
    for k in ("p", "m", "v"):
        assert np.array_equal(_bits(eager[k].numpy()), _bits(replay[k].numpy())), k
    # NULL restores the argument: an eager call after set_lr_source(None) takes its own lr (a zero rate moves nothing)
    before = replay["p"].numpy()
    step(replay, 0.0)
    assert np.array_equal(_bits(before), _bits(replay["p"].numpy()))


def test_argument_checks(ctx):
    from gcnx import _lib
    lib, h = ctx.lib, ctx.h
    b = [ctx.zeros(8) for _ in range(4)]
    t, part = ctx.zeros(1, np.int32), ctx.zeros(256)
    P = [a.ptr for a in b]
    ok = dict(p=P[0], g=P[1], m=P[2], v=P[3], n=8, t=t.ptr, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, part=None, k=0, clip=0.0, norm=None)

    def adam(**kw):
        a = dict(ok, **kw)
        return lib.gcnx_adam(h, a["p"], a["g"], a["m"], a["v"], a["n"], a["t"], a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], a["part"],
                             a["k"], a["clip"], a["norm"])

    def mom(p=P[0], g=P[1], vel=P[2], n=8, momentum=0.9, part=None, k=0, clip=0.0):
        return lib.gcnx_sgd_momentum(h, p, g, vel, n, 0.01, momentum, 0, part, k, clip, None)

    inv = 1                                                       # GCNX_ERR_INVALID
    assert adam() == _lib.OK and mom() == _lib.OK
    # n = 0 is a no-op, whatever the pointers
    assert adam(n=0, p=None, g=None, m=None, v=None, t=None) == _lib.OK
    assert mom(n=0, p=None, g=None, vel=None) == _lib.OK and lib.gcnx_grad_sqnorm(h, None, 0, None, 1) == _lib.OK
    for key in ("p", "g", "m", "v", "t"):
        assert adam(**{key: None}) == inv, key
    assert adam(n=-1) == inv and mom(n=-1) == inv and lib.gcnx_grad_sqnorm(h, P[0], -1, part.ptr, 1) == inv
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert adam(b1=bad) == inv and adam(b2=bad) == inv and mom(momentum=bad) == inv, bad
    assert adam(part=part.ptr, k=257, clip=1.0) == inv and mom(part=part.ptr, k=257, clip=1.0) == inv
    assert lib.gcnx_grad_sqnorm(h, P[0], 8, part.ptr, 257) == inv and lib.gcnx_grad_sqnorm(h, P[0], 8, part.ptr, 0) == inv
    assert adam(clip=1.0) == inv and mom(clip=1.0) == inv         # clipnorm without partials
    for key in ("p", "g", "vel"):
        assert mom(**{key: None}) == inv, key
    assert lib.gcnx_grad_sqnorm(h, None, 8, part.ptr, 1) == inv and lib.gcnx_grad_sqnorm(h, P[0], 8, None, 1) == inv
    assert "gcnx_grad_sqnorm" in _lib.last_error(h)
    assert all(not a.numpy().any() for a in b) and int(t.numpy()[0]) == 0      # nothing above ran an update on non-zero state


# ---- 2. the models -------------------------------------------------------------------------------------------------------
LR = 1e-2


def _gcn2(ctx, graph):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch, GCN2
    g = load_golden("gcn2_cfg1_tiny_weighted")
    hb = golden_batch(g)
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, hb.vals, hb.graph_ptr)
    batch = DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))
    m = GCN2(ctx, 2, hidden=32, use_graph=graph)
    m.build(hb.f)
    m.set_weights([g["p_" + k] for k in GCN2.PARAM_ORDER])
    return m, batch


def _tiny_model(name):
    def make(ctx, graph):
        import gcnx
        hb = _tiny_host(16, 16)
        inputs, y = (hb.x, _scipy_adj(hb), hb.ids()), hb.y
        if name == "GeneralGNN":
            m = gcnx.GeneralGNN(ctx, 2, activation="softmax", hidden=32, message_passing=2, use_graph=graph)
        elif name == "ECCNet":
            m = gcnx.ECCNet(ctx, 2, channels=32, seed=1)
            e = np.random.default_rng(4).standard_normal((hb.nnz, 2)).astype(np.float32)
            inputs = (hb.x, _scipy_adj(hb), e, hb.ids())
        elif name == "TopKNet":
            m = gcnx.TopKNet(ctx, hidden=32, ratio=0.5, seed=0)
        elif name == "GAT":
            m = gcnx.GAT(ctx, hidden_channels=64, heads=4, seed=0)
        else:
            m = getattr(gcnx, name)(ctx, hidden_channels=64, seed=0)
        batch = m._as_batch(inputs, y)
        m._ensure(batch)                                            # builds the model for the batch's widths
        return m, batch
    return make


MODELS = {"GCN2": _gcn2, **{k: _tiny_model(k) for k in ("GeneralGNN", "GCN", "SAGE", "GAT", "ECCNet", "TopKNet")}}
CASES = [("GCN2", False), ("GCN2", True), ("GeneralGNN", False), ("GeneralGNN", True), ("GCN", False), ("SAGE", False),
         ("GAT", False), ("ECCNet", False), ("TopKNet", False)]


def _fill_zeros(m, seed=11):
    """Parameters that start at zero (biases) get small non-zero values: with weight_decay every tensor then moves at step
    1 even where its gradient is exactly zero (a bias in front of a BatchNorm), so the check that none is left out of the
    flat range holds for every tensor.  Padding between tensors is not touched."""
    rng = np.random.default_rng(seed)
    for t in m.trainable_variables:
        h = t.numpy()
        z = h == 0
        if z.any():
            h[z] = (rng.choice([-1.0, 1.0], int(z.sum())) * rng.uniform(0.02, 0.1, int(z.sum()))).astype(np.float32)
            t.copy_from_host(h)


def _first_norm(m, batch):
    """The gradient norm at the initial weights (no update)."""
    m.loss_and_grads(batch, None)
    return OR.grad_norm(m.flat_g.numpy()[:m.n_params])


def _checked_steps(m, batch, opt, steps, what, t0=0, **step_kw):
    """``steps`` train_steps; after each one the device's parameters and state against the restatement applied to THAT step's
    device gradients and the previous device state.  Returns the reported norms."""
    n = m.n_params
    norms = []
    p0, m0, v0 = m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy()
    for step in range(1, steps + 1):
        before = [t.numpy() for t in m.trainable_variables] if t0 + step == 1 else None
        m.train_step(batch, None, lr=LR, **step_kw)
        g = m.flat_g.numpy()[:n]
        assert len(m.gradients()) > 0                                # (views of the same flat buffer, still readable after the update)
        p1, m1, v1 = m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy()
        norm = opt.last_grad_norm()
        _assert_norm(norm, g, min(256, -(-n // 256)), f"{what} step {step}")
        _, _, _, info = _assert_adam(p1, m1, v1, p0, g, m0, v0, t0 + step, LR, norm, f"{what} step {step}", beta1=opt.beta1,
                                     beta2=opt.beta2, eps=opt.eps, weight_decay=opt.weight_decay, clipnorm=opt.clipnorm)
        if before is not None:
            assert info["s"] < 1.0, "the clip is meant to be active at step 1"
            moved = [not np.array_equal(_bits(b), _bits(t.numpy())) for b, t in zip(before, m.trainable_variables)]
            assert all(moved), (what, "tensors that did not move", [i for i, ok in enumerate(moved) if not ok])
        norms.append(norm)
        p0, m0, v0 = p1, m1, v1
    return norms


@functools.lru_cache(maxsize=None)
def _gcn2_final(ctx, graph):
    """(final flat_p, norms) of the GCN2 case -- shared by the per-case test and the eager / replay comparison."""
    return _run_case(ctx, "GCN2", graph)


def _run_case(ctx, name, graph):
    import gcnx
    m, batch = MODELS[name](ctx, graph)
    _fill_zeros(m)
    c = 0.5 * _first_norm(m, batch)
    opt = gcnx.Adam(weight_decay=0.01, clipnorm=c)
    m.set_optimizer(opt)
    assert set(opt.m) == set(opt.v) and len(opt.m) > 0 and opt.flat("m").size == m.n_params
    norms = _checked_steps(m, batch, opt, 4, f"{name} graph={graph}")
    assert opt.state_dict()["t"] == 4
    return m.flat_p.numpy(), norms


@pytest.mark.parametrize("name,graph", CASES)
def test_model_steps_follow_the_restatement(ctx, name, graph):
    if name == "GCN2":
        _gcn2_final(ctx, graph)
    else:
        _run_case(ctx, name, graph)


def test_gcn2_eager_and_replay_end_bitwise_equal(ctx):
    (pe, ne), (pr, nr) = _gcn2_final(ctx, False), _gcn2_final(ctx, True)
    assert np.array_equal(_bits(pe), _bits(pr)) and ne == nr


def test_resume_from_state_dicts_is_bitwise(ctx):
    import gcnx
    hb = _tiny_host(16, 16)

    def fresh():
        m = gcnx.GCN(ctx, hidden_channels=64, seed=0)
        return m, _device_batch(ctx, hb)

    m, batch = fresh()
    m.build(hb.f)
    c = 0.5 * _first_norm(m, batch)
    opt = gcnx.Adam(weight_decay=0.01, clipnorm=c)
    m.set_optimizer(opt)
    for _ in range(2):
        m.train_step(batch, lr=LR)
    sd_m, sd_o = m.state_dict(), opt.state_dict()
    assert sd_o["t"] == 2 and sd_o["m"].shape == sd_o["v"].shape == (m.n_params,)
    for _ in range(2):
        m.train_step(batch, lr=LR)
    m2, batch2 = fresh()
    opt2 = gcnx.Adam(weight_decay=0.01, clipnorm=c)
    opt2.load_state_dict(sd_o)                                   # before the state exists: applied when it does
    m2.load_state_dict(sd_m)
    m2.set_optimizer(opt2)
    assert opt2.state_dict()["t"] == 2 and np.array_equal(_bits(opt2.state_dict()["v"]), _bits(sd_o["v"]))
    for _ in range(2):
        m2.train_step(batch2, lr=LR)
    assert np.array_equal(_bits(m.flat_p.numpy()), _bits(m2.flat_p.numpy()))
    for k in ("m", "v"):
        assert np.array_equal(_bits(opt.state_dict()[k]), _bits(opt2.state_dict()[k]))
    assert opt2.state_dict()["t"] == 4
    assert np.array_equal(_bits(opt.m["w1"].numpy()), _bits(opt.state_dict()["m"][:hb.f * 64].reshape(hb.f, 64)))


def test_two_ranks_stay_bitwise_equal():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    ctx0 = gcnx.Context(0)
    try:
        m0 = gcnx.GCN(ctx0, hidden_channels=64, seed=0)
        m0.build(hb.f)
        c = 0.5 * _first_norm(m0, _device_batch(ctx0, hb))
    finally:
        ctx0.close()

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            part, gb = shard.shard_batch(hb, rank, 2)
            m = gcnx.GCN(ctx, hidden_channels=64, seed=0, comm=make_comm(ctx))
            m.build(hb.f)
            _fill_zeros(m)
            opt = gcnx.Adam(clipnorm=c)
            m.set_optimizer(opt)
            norms = _checked_steps(m, _device_batch(ctx, part), opt, 4, f"rank {rank}", global_batch=gb)
            return {"w": m.flat_p.numpy(), "norms": norms, "t": opt.state_dict()["t"]}
        finally:
            ctx.close()

    r0, r1 = ThreadWorld(2).run(rank_fn)
    assert np.array_equal(_bits(r0["w"]), _bits(r1["w"])) and r0["norms"] == r1["norms"] and r0["t"] == r1["t"] == 4


def test_adam_makes_progress_on_gcn2(ctx):
    """On the CPU the restatement, fed with oracle.gcn_oracle's gradients of the golden batch, takes the loss from 1.342 to
    0.0008 in 30 steps at lr 1e-2 (a fall of far more than a tenth), so lr 1e-2 it is: 30 device steps end below the first loss."""
    import gcnx
    m, batch = _gcn2(ctx, False)
    m.set_optimizer(gcnx.Adam())
    losses = [m.train_step(batch, None, lr=1e-2)[0] for _ in range(30)]
    print(f"Adam on GCN2: loss {losses[0]:.4f} -> {losses[-1]:.6f}")
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_fit_takes_an_optimizer(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:10]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[10:]])
    m = gcnx.GAT(ctx, heads=4, seed=0)
    opt = gcnx.Adam()
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False, optimizer=opt)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])
    assert opt.state_dict()["t"] == 4 and opt.last_grad_norm() is None


@pytest.mark.parametrize("graph", [False, True])
def test_set_optimizer_none_restores_plain_sgd(ctx, graph):
    import gcnx
    plain, batch = _gcn2(ctx, graph)
    for _ in range(3):
        plain.train_step(batch, None, lr=0.02)
    m, batch2 = _gcn2(ctx, graph)
    w0 = m.get_weights()
    m.set_optimizer(gcnx.Adam(clipnorm=1.0))
    m.train_step(batch2, None, lr=0.02)
    assert not np.array_equal(_bits(m.flat_p.numpy()), _bits(np.concatenate([w.ravel() for w in w0])))
    m.set_optimizer(None)
    m.set_weights(w0)
    for _ in range(3):
        m.train_step(batch2, None, lr=0.02)
    assert np.array_equal(_bits(plain.flat_p.numpy()), _bits(m.flat_p.numpy()))

"""GPU tests of GraphNorm: the kernels of csrc/graph_norm.hip (gcnx_graph_norm_act and gcnx_graph_norm_act_bwd on their whole and
sliced routes), the layer gcnx.GraphNorm and the models with norm="graph" -- each against the float64 oracle
tests/graph_norm_ref.py on the device's side of every kink.  Tolerances: TIGHT = 2e-5 for a single fp32 kernel, 1e-4 for a
whole step.

Routes: ``None`` = the whole route (one workgroup per graph: slice_rows = 0 without scratch), 0 = the library's choice with
scratch, 32 and 7 = slices of that many rows (7: more slices than row groups, slices that end inside a wave's rows).

PReLU sides: the oracle takes them from the device's own y (the slope is positive, so y > 0 <=> t > 0).  The backward recomputes t
from z, mean and inv with the forward's arithmetic, so it stands on the sides of the forward whose mean and inv it reads."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gat_ref as GR
import gcn_bn_ref as R
import graph_norm_ref as GN
from gpu_frames import SENTINEL, Frame, same
from test_gpu_gcn_bn import _cmp_grads, _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SIZES = [1, 0, 3, 65, 64, 130]
WIDTHS = [16, 48, 64, 128, 256, 10]          # 10: the scalar route
ROUTES = (None, 0, 32, 7)
SLOPE = 0.25
OUT = ("dz", "dgamma", "dbeta", "da", "dslope")


@functools.lru_cache(maxsize=None)
def _case(kind, f):
    """(graph_ptr, z, dy, a, gamma, beta), computed once and never modified.  a, gamma ~ U(0.5, 1.5), beta ~ N(0, 1)."""
    rng = np.random.default_rng(200 + f)
    if kind == "sizes":
        gp = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        z = rng.standard_normal((int(gp[-1]), f)).astype(np.float32)
    else:
        from gcnx import synth
        hb = synth.ecoli_batch(3, f)
        assert hb.n % 32 != 0 and hb.n > 1024
        gp, z = hb.graph_ptr.astype(np.int32), hb.x.astype(np.float32)
    dy = rng.standard_normal(z.shape).astype(np.float32)
    a, gamma = rng.uniform(0.5, 1.5, f).astype(np.float32), rng.uniform(0.5, 1.5, f).astype(np.float32)
    beta = rng.standard_normal(f).astype(np.float32)
    for v in (gp, z, dy, a, gamma, beta):
        v.setflags(write=False)
    return gp, z, dy, a, gamma, beta


class _Dev:
    """The operands of one case on the device, and the two calls."""

    def __init__(self, ctx, gp, z, dy, a, gamma, beta, slope=SLOPE):
        from gcnx.device import Segments
        self.ctx, self.seg, self.n, self.b, self.f = ctx, Segments(ctx, gp), z.shape[0], len(gp) - 1, z.shape[1]
        self.z, self.dy = ctx.to_device(z), ctx.to_device(dy)
        self.a, self.gamma, self.beta = ctx.to_device(a), ctx.to_device(gamma), ctx.to_device(beta)
        self.act = None if slope is None else "prelu_shared"
        self.alpha = None if slope is None else ctx.to_device(np.array([slope], np.float32))

    def scratch(self, route):
        from gcnx import device as D
        return None if route is None else self.ctx.empty(max(D.graph_norm_scratch_floats(self.ctx, self.n, self.b, self.f, route), 4))

    def fwd(self, route):
        from gcnx import device as D
        full = lambda *s: self.ctx.to_device(np.full(s, SENTINEL, np.float32))
        y, mean, inv = full(self.n, self.f), full(self.b, self.f), full(self.b, self.f)
        D.graph_norm_act(self.ctx, self.seg, self.z, self.a, self.gamma, self.beta, y, mean, inv, act=self.act, alpha=self.alpha,
                         scratch=self.scratch(route), slice_rows=route or 0)
        return y, mean, inv

    def bwd(self, route, mean, inv, skip=()):
        """{name: host array} of OUT; a name in ``skip`` goes in as NULL."""
        from gcnx import device as D
        full = lambda *s: self.ctx.to_device(np.full(s, SENTINEL, np.float32))
        o = {"dz": full(self.n, self.f), "dgamma": full(self.f), "dbeta": full(self.f), "da": full(self.f), "dslope": full(1)}
        for k in skip:
            o[k] = None
        D.graph_norm_act_bwd(self.ctx, self.seg, self.dy, self.z, mean, inv, self.a, self.gamma, self.beta, o["dz"], act=self.act,
                             alpha=self.alpha, dgamma=o["dgamma"], dbeta=o["dbeta"], dmean_scale=o["da"], dalpha=o["dslope"],
                             scratch=self.scratch(route), slice_rows=route or 0)
        return {k: v.numpy() for k, v in o.items() if v is not None}


def _ref_bwd(case, pos, slope=SLOPE):
    gp, z, dy, a, gamma, beta = case
    return dict(zip(OUT, GN.backward(dy, z, gp, a, gamma, beta, slope, pos)))


# ---- 1. both directions against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("kind", ["sizes", "ecoli3"])
def test_forward_and_backward_against_float64_on_every_route(ctx, kind, f):
    case = _case(kind, f)
    gp, z, dy, a, gamma, beta = case
    d = _Dev(ctx, *case)
    fw, bw = {}, {}
    for route in ROUTES:
        what = f"{kind} f={f} route={route}"
        y, mean, inv = d.fwd(route)
        fw[route] = y.numpy(), mean.numpy(), inv.numpy()
        want, c = GN.forward(z, gp, a, gamma, beta, SLOPE, pos=fw[route][0] > 0)
        print(f"{what}: y {rel_err(fw[route][0], want):.2e} mean {rel_err(fw[route][1], c['mean']):.2e} inv {rel_err(fw[route][2], c['inv']):.2e}")
        assert_close(fw[route][0], want, TIGHT, what + " y")
        assert_close(fw[route][1], c["mean"], TIGHT, what + " mean")
        assert_close(fw[route][2], c["inv"], TIGHT, what + " inv")
        if kind == "sizes":
            assert not fw[route][1][1].any() and not fw[route][2][1].any(), what + ": the empty graph's mean and inv rows are 0"
        again = d.fwd(route)
        assert all(same(u.numpy(), v) for u, v in zip(again, fw[route])), what + ": two runs, the same bits"
        # the backward of this route on the sides of this route's forward
        bw[route] = d.bwd(route, mean, inv)
        ref = _ref_bwd(case, fw[route][0] > 0)
        print(f"{what}: " + " ".join(f"{k} {rel_err(bw[route][k], ref[k]):.2e}" for k in OUT))
        for k in OUT:
            assert_close(bw[route][k], ref[k].reshape(bw[route][k].shape), TIGHT, f"{what} {k}")
        twice = d.bwd(route, mean, inv)
        assert all(same(twice[k], bw[route][k]) for k in OUT), what + ": two backward runs, the same bits"
    for r0, r1 in itertools.combinations(ROUTES, 2):
        for i, k in enumerate(("y", "mean", "inv")):
            assert_close(fw[r1][i], fw[r0][i], TIGHT, f"{kind} f={f} {k} route {r1} vs {r0}")
    # the backward routes against each other: all on the whole route's mean and inv, hence on the same sides
    y, mean, inv = d.fwd(None)
    on_whole = {route: d.bwd(route, mean, inv) for route in ROUTES}
    assert all(same(on_whole[None][k], bw[None][k]) for k in OUT)
    for r0, r1 in itertools.combinations(ROUTES, 2):
        for k in OUT:
            assert_close(on_whole[r1][k], on_whole[r0][k], TIGHT, f"{kind} f={f} {k} route {r1} vs {r0}")


@pytest.mark.parametrize("slope", [None, SLOPE])
@pytest.mark.parametrize("f", [16, 10])
def test_one_row_graph_is_beta_at_mean_scale_one(ctx, f, slope):
    gp, z, dy, _, gamma, beta = _case("sizes", f)
    d = _Dev(ctx, gp, z, dy, np.ones(f, np.float32), gamma, beta, slope)
    want = beta if slope is None else np.where(beta > 0, beta, np.float32(slope) * beta).astype(np.float32)
    for route in ROUTES:
        y, _, _ = d.fwd(route)
        assert same(y.numpy()[0], want), f"f={f} route={route}: o = (1 - a) z = 0 exactly, so t = beta"


def test_no_activation_against_float64(ctx):
    case = _case("sizes", 48)
    gp, z, dy, a, gamma, beta = case
    d = _Dev(ctx, *case, slope=None)
    want, c = GN.forward(z, gp, a, gamma, beta)
    ref = _ref_bwd(case, None, slope=None)
    for route in ROUTES:
        y, mean, inv = d.fwd(route)
        assert_close(y.numpy(), want, TIGHT, f"act=None route={route} y")
        got = d.bwd(route, mean, inv)
        for k in OUT[:4]:
            assert_close(got[k], ref[k], TIGHT, f"act=None route={route} {k}")
        assert got["dslope"][0] == 0.0


# ---- 2. the variance is centred ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_the_variance_is_centred(ctx, route):
    """z = 256 + k / 8 with integer k in [-32, 32], mean_scale = 1: every column sum is exact in fp32, the mean of the centred
    squares stays within 4e-6 of float64 in fp32, and E[z^2] - mu^2 is 1.6e-3 away (tests/test_graph_norm_host.py restates both
    on the host)."""
    rng = np.random.default_rng(3)
    gp = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    n, f = int(gp[-1]), 16
    z = (256 + rng.integers(-32, 33, size=(n, f)) / 8).astype(np.float32)
    one, zero = np.ones(f, np.float32), np.zeros(f, np.float32)
    d = _Dev(ctx, gp, z, z, one, one, zero)
    y = d.fwd(route)[0].numpy()
    want, _ = GN.forward(z, gp, one, one, zero, SLOPE, pos=y > 0)
    print(f"centred variance route={route}: y {rel_err(y, want):.2e}")
    assert_close(y, want, TIGHT, f"z = 256 + k / 8 route={route}")


# ---- 3. strides, aliasing, NULL gradients -------------------------------------------------------------------------------------------
def _frame_check(fr, want, tol, what, rows=None):
    got = fr.buf.numpy()
    body = fr._body(got)
    rows = fr.n if rows is None else rows
    assert rel_err(body[:rows, :fr.f], want) < tol, (what, rel_err(body[:rows, :fr.f], want))
    assert (body[rows:, :fr.f] == SENTINEL).all(), (what, "rows outside the graphs were written")
    assert (body[:, fr.f:] == SENTINEL).all() and (got[:fr.lead] == SENTINEL).all() \
        and (got[fr.lead + fr.n * fr.ld:] == SENTINEL).all(), (what, "written outside the view")


def _rows(fr, n):
    """The first n rows of a frame's view."""
    from gcnx.device import DeviceArray
    return DeviceArray(fr.ctx, fr.view.ptr, (n, fr.f), np.float32, ld=fr.ld, base=fr.buf)


@pytest.mark.parametrize("route", [None, 32, 7])
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("f,pad,lead", [(64, 8, 4), (10, 3, 3)])
def test_strided_operands_inside_sentinel_frames(ctx, f, pad, lead, alias, route):
    """f = 64: float4 lanes on aligned views; f = 10: scalar lanes on views off every 16-byte boundary.  alias: y written over z
    and dz over dy.  Two rows behind the last graph belong to no graph and stay as they were."""
    from gcnx import device as D
    from gcnx.device import Segments
    case = _case("ecoli3", f)
    gp, z, dy, a, gamma, beta = case
    n, b, extra = z.shape[0], len(gp) - 1, 2
    seg = Segments(ctx, gp)
    pad_rows = lambda v: np.concatenate([v, np.full((extra, f), SENTINEL, np.float32)])
    fz = Frame(ctx, n + extra, f, 2 * f + pad, lead, data=pad_rows(z))     # z: a column view of a buffer more than twice as wide
    fdy = Frame(ctx, n + extra, f, f + 2 * pad, lead, data=pad_rows(dy))
    fy = Frame(ctx, n + extra, f, f + pad, lead)
    fdz = Frame(ctx, n + extra, f, f + pad, lead)
    ns = max(D.graph_norm_scratch_floats(ctx, n, b, f, route or 0), 4)
    f_s = Frame(ctx, 1, ns, ns, 4)                                          # the scratch too: nothing is written past what was asked for
    assert all(fr.aligned() for fr in (fz, fdy, fy, fdz)) == (f == 64) and f_s.aligned()
    scratch = f_s.view.flat(0, ns) if route is not None else None
    dev = [ctx.to_device(v) for v in (a, gamma, beta)]
    alpha = ctx.to_device(np.array([SLOPE], np.float32))
    mean, inv = ctx.empty((b, f)), ctx.empty((b, f))
    # the forward into its own frame first: the sides, and the z that the backward needs after an in-place forward
    D.graph_norm_act(ctx, seg, _rows(fz, n), *dev, _rows(fy, n), mean, inv, act="prelu_shared", alpha=alpha, scratch=scratch,
                     slice_rows=route or 0)
    pos = fy.buf.numpy()[lead:lead + (n + extra) * fy.ld].reshape(n + extra, fy.ld)[:n, :f] > 0
    want, _ = GN.forward(z, gp, a, gamma, beta, SLOPE, pos=pos)
    _frame_check(fy, want, TIGHT, "y", rows=n)
    fz.untouched("z")
    ref = _ref_bwd(case, pos)
    grads = {k: Frame(ctx, 1, w, w, 4) for k, w in (("dgamma", f), ("dbeta", f), ("da", f), ("dslope", 1))}
    gview = {k: fr.view.flat(0, fr.f) for k, fr in grads.items()}
    dz_to = fdy if alias else fdz
    D.graph_norm_act_bwd(ctx, seg, _rows(fdy, n), _rows(fz, n), mean, inv, *dev, _rows(dz_to, n), act="prelu_shared", alpha=alpha,
                         dgamma=gview["dgamma"], dbeta=gview["dbeta"], dmean_scale=gview["da"], dalpha=gview["dslope"],
                         scratch=scratch, slice_rows=route or 0)
    _frame_check(dz_to, ref["dz"], TIGHT, "dz over dy" if alias else "dz", rows=n)
    for k, fr in grads.items():
        _frame_check(fr, ref[k][None, :], TIGHT, k)
    fz.untouched("z")
    if alias:
        fdz.untouched("the other dz frame")
        zz = Frame(ctx, n + extra, f, 2 * f + pad, lead, data=pad_rows(z))  # y over z, on a second copy
        D.graph_norm_act(ctx, seg, _rows(zz, n), *dev, _rows(zz, n), mean, inv, act="prelu_shared", alpha=alpha, scratch=scratch,
                         slice_rows=route or 0)
        assert same(zz.numpy()[:n], fy.numpy()[:n]), "in place: the bits of the forward into another buffer"
        _frame_check(zz, want, TIGHT, "y over z", rows=n)
    else:
        fdy.untouched("dy")
    f_s.numpy()                                                             # asserts the sentinels around the scratch


@pytest.mark.parametrize("route", [None, 7])
def test_each_parameter_gradient_may_be_null(ctx, route):
    case = _case("sizes", 48)
    d = _Dev(ctx, *case)
    _, mean, inv = d.fwd(route)
    full = d.bwd(route, mean, inv)
    for k in OUT[1:]:
        got = d.bwd(route, mean, inv, skip=(k,))
        assert k not in got and all(same(got[q], full[q]) for q in got), f"route={route} without {k}"
    got = d.bwd(route, mean, inv, skip=OUT[1:])
    assert list(got) == ["dz"] and same(got["dz"], full["dz"])


# ---- 4. one tall case ---------------------------------------------------------------------------------------------------------------
def test_tall_graphs_on_every_route(ctx):
    """Two graphs of 8 192 rows (the config-5 shape): whole, the library's choice (slices on any device of 128 CUs or more) and
    64-row slices all match float64."""
    rng = np.random.default_rng(5)
    gp = np.array([0, 8192, 16384], np.int32)
    z, dy = rng.standard_normal((16384, 64)).astype(np.float32), rng.standard_normal((16384, 64)).astype(np.float32)
    a, gamma = rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.uniform(0.5, 1.5, 64).astype(np.float32)
    beta = rng.standard_normal(64).astype(np.float32)
    case = (gp, z, dy, a, gamma, beta)
    d = _Dev(ctx, *case)
    got = {}
    for route in (None, 0, 64):
        y, mean, inv = d.fwd(route)
        got[route] = y.numpy()
        pos = got[route] > 0
        want, c = GN.forward(z, gp, a, gamma, beta, SLOPE, pos=pos)
        assert_close(got[route], want, TIGHT, f"tall route={route} y")
        assert_close(mean.numpy(), c["mean"], TIGHT, f"tall route={route} mean")
        assert_close(inv.numpy(), c["inv"], TIGHT, f"tall route={route} inv")
        back, ref = d.bwd(route, mean, inv), _ref_bwd(case, pos)
        print(f"tall route={route}: " + " ".join(f"{k} {rel_err(back[k], ref[k]):.2e}" for k in OUT))
        for k in OUT:
            assert_close(back[k], ref[k], TIGHT, f"tall route={route} {k}")
    assert ctx.info()["cus"] < 128 or same(got[0], got[64])


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from gcnx import _lib
    case = _case("sizes", 16)
    d = _Dev(ctx, *case)
    y, mean, inv = d.fwd(None)
    dz = ctx.to_device(np.full((d.n, 16), SENTINEL, np.float32))
    lib, h, gp = ctx.lib, ctx.h, d.seg.dev.ptr
    par = (d.a.ptr, d.gamma.ptr, d.beta.ptr)

    def fwd(gp=gp, z=d.z.ptr, ldz=16, par=par, act=_lib.ACTS["prelu_shared"], alpha=d.alpha.ptr, n=d.n, b=d.b, f=16, s=0, y=y.ptr,
            ldy=16, mean=mean.ptr, inv=inv.ptr, scratch=None):
        return lib.gcnx_graph_norm_act(h, gp, z, ldz, *par, 1e-5, act, alpha, n, b, f, s, y, ldy, mean, inv, scratch)

    def bwd(gp=gp, dy=d.dy.ptr, z=d.z.ptr, mean=mean.ptr, inv=inv.ptr, par=par, act=_lib.ACTS["prelu_shared"], alpha=d.alpha.ptr,
            n=d.n, b=d.b, f=16, s=0, dz=dz.ptr, lddz=16, scratch=None):
        return lib.gcnx_graph_norm_act_bwd(h, gp, dy, 16, z, 16, mean, inv, *par, act, alpha, n, b, f, s, dz, lddz, None, None, None,
                                           None, scratch)

    before = y.numpy()
    invalid = [fwd(s=8), fwd(n=-1), fwd(b=-1), fwd(f=-1), fwd(s=-1), fwd(z=None), fwd(gp=None), fwd(par=(None,) + par[1:]),
               fwd(par=par[:2] + (None,)), fwd(y=None), fwd(mean=None), fwd(inv=None), fwd(alpha=None), fwd(ldz=8), fwd(ldy=8),
               fwd(f=300, ldz=300, ldy=300),
               bwd(s=8), bwd(n=-1), bwd(dy=None), bwd(z=None), bwd(mean=None), bwd(inv=None), bwd(dz=None), bwd(alpha=None),
               bwd(par=(par[0], None, par[2])), bwd(lddz=8)]
    assert invalid == [_lib.OK + 1] * len(invalid)                # GCNX_ERR_INVALID, nothing launched
    unsupported = [fwd(act=_lib.ACTS["relu"]), fwd(act=_lib.ACTS["prelu"]), fwd(act=7), bwd(act=_lib.ACTS["relu"]),
                   bwd(act=_lib.ACTS["prelu"])]
    assert unsupported == [_lib.ERR_UNSUPPORTED] * len(unsupported)
    assert "GCNX_ACT_PRELU_SHARED" in ctx.lib.gcnx_last_error(h).decode()
    assert [fwd(n=0), fwd(b=0), fwd(f=0), bwd(n=0), bwd(b=0), bwd(f=0)] == [_lib.OK] * 6
    assert same(y.numpy(), before) and (dz.numpy() == SENTINEL).all()       # nothing was written by any of them
    assert fwd(act=_lib.ACTS[None], alpha=None) == _lib.OK                  # no activation needs no slope


# ---- 6. the layer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [False, True])
def test_layer_forward_and_backward(ctx, ids):
    import gcnx
    case = _case("sizes", 48)
    gp, z, dy, a, gamma, beta = case
    layer = gcnx.GraphNorm()
    seg = np.repeat(np.arange(len(gp) - 1), np.diff(gp)) if ids else gcnx.Segments(ctx, gp)
    dev_z = ctx.to_device(z)
    first = layer((dev_z, seg))
    assert first.shape == z.shape and [w.shape for w in layer.get_weights()] == [(48,)] * 3
    one, zero = np.ones(48), np.zeros(48)
    assert_close(first.numpy(), GN.forward(z, gp, one, one, zero)[0], TIGHT, "layer forward, its initial parameters")
    layer.set_weights([gamma, beta, a])                                     # weight, bias, mean_scale
    y = layer((dev_z, seg))
    assert_close(y.numpy(), GN.forward(z, gp, a, gamma, beta)[0], TIGHT, "layer forward")
    dx = layer.backward(ctx.to_device(dy))
    ref = _ref_bwd(case, None, slope=None)
    assert_close(dx.numpy(), ref["dz"], TIGHT, "layer dx")
    for k, r in (("weight", "dgamma"), ("bias", "dbeta"), ("mean_scale", "da")):
        assert_close(layer.grads[k].numpy(), ref[r], TIGHT, f"layer d {k}")
    # one row is legal
    single = gcnx.GraphNorm()
    out = single((ctx.to_device(z[:1]), np.zeros(1, np.int64)))
    assert same(out.numpy(), np.zeros((1, 48), np.float32))                 # y = bias = 0 at mean_scale = 1


# ---- 7. the models ------------------------------------------------------------------------------------------------------------------
def _make(ctx, heads, readout, comm=None, norm="graph", h=64):
    import gcnx
    if heads is None:
        return gcnx.GCN(ctx, hidden_channels=h, seed=0, readout=readout, norm=norm, comm=comm)
    return gcnx.GAT(ctx, hidden_channels=h, heads=heads, seed=0, readout=readout, norm=norm, comm=comm)


def _sides(m, batch, hb, gat):
    """The kink sides of a step on the model's current weights, from a forward of their own (the max readout's backward
    overwrites y2): {"masks": ..., "argmax": ...} as graph_norm_ref.model takes them."""
    m(batch)
    b = m._bufs
    s = {"masks": {"m1": b["y1"].numpy() > 0, "m2": b["y2"].numpy() > 0}}
    if gat:
        s["masks"].update({f"e{i}": GR.device_score_sides(b[f"asrc{i}"].numpy(), b[f"adst{i}"].numpy(), hb.rowptr, hb.colidx) for i in (1, 2)})
    if m.readout == "max":
        s["argmax"] = b["arg"].numpy().astype(np.int64)
    return s


@pytest.mark.parametrize("readout", ["max", "attention"])
@pytest.mark.parametrize("heads", [None, 4], ids=["GCN", "GAT-heads4"])
def test_model_step_against_oracle(ctx, heads, readout):
    hb = _tiny_host(16, 16, seed=4)
    batch, a = _device_batch(ctx, hb), _scipy_adj(hb)
    m = _make(ctx, heads, readout)
    p = {k: v.astype(np.float32) for k, v in GN.init_params(16, 64, seed=7, heads=heads, readout=readout).items()}
    m.load_state_dict(p)
    what = ("GCN" if heads is None else f"GAT heads={heads}") + f" readout={readout}"
    back = m.state_dict()
    assert set(back) == set(p) and all(same(back[k], p[k].reshape(back[k].shape)) for k in p), what + ": state_dict round trip"
    sides = _sides(m, batch, hb, heads is not None)
    m.loss_and_grads(batch)
    for k in ("gm1", "gi1", "gm2", "gi2", "gn"):
        assert k in m._bufs, k
    r = GN.model(hb.x, a, hb.graph_ptr, p, hb.y, heads=heads, readout=readout, **sides)
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < 1e-4 and la[1] == r["hits"], (la, r["loss"], r["hits"])
    grads = m.gradients()
    assert set(grads) == set(r["grads"]) and set(GN.SCALE_KEYS) <= set(grads)
    for k in sorted(grads):
        print(f"{what} {k}: {rel_err(grads[k], np.reshape(r['grads'][k], grads[k].shape)):.2e}")
    _cmp_grads(grads, r["grads"], 1e-4, what)
    # three SGD steps, each oracle step on the device's kink sides of that step
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    for _ in range(3):
        sides = _sides(m, batch, hb, heads is not None)
        m.train_step(batch, lr=0.02)
        r = GN.model(hb.x, a, hb.graph_ptr, ph, hb.y, heads=heads, readout=readout, **sides)
        ph = R.sgd(ph, r["grads"], 0.02)
    sd = m.state_dict()
    for k in ph:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after 3 steps {k}")


OTHERS = {"SAGE": {}, "GIN": {}, "PNA": {"avg_deg_log": 1.0}, "GATv2": {}, "ResGated": {}, "Transformer": {}}


@pytest.mark.parametrize("name", list(OTHERS))
def test_the_other_models_take_a_step(ctx, name):
    import gcnx
    hb = _tiny_host(8, 16, seed=2)
    batch = _device_batch(ctx, hb)
    m = getattr(gcnx, name)(ctx, hidden_channels=16, seed=0, norm="graph", **OTHERS[name])
    loss, acc = m.train_step(batch, lr=0.01)
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    g = m.gradients()
    for k in GN.SCALE_KEYS:
        assert g[k].shape == (16,) and np.isfinite(g[k]).all() and g[k].any(), (name, k, g[k])
    assert all(np.isfinite(v).all() for v in g.values())


def test_norm_batch_runs_the_launches_it_ran(ctx):
    """norm="batch" passed explicitly: the same bits as the default, and none of GraphNorm's buffers."""
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    batch = _device_batch(ctx, hb)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 64, seed=7).items()}
    res = []
    for kw in ({}, {"norm": "batch"}):
        m = gcnx.GCN(ctx, hidden_channels=64, seed=0, **kw)
        m.load_state_dict(p)
        m.loss_and_grads(batch)
        assert "ms1" not in m.p and not {"gm1", "gi1", "gm2", "gi2", "gn"} & set(m._bufs)
        res.append((m._bufs["out"].numpy(), m.flat_g.numpy()))
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])


# ---- 8. graph shards ----------------------------------------------------------------------------------------------------------------
class _Counting:
    """A communicator that counts the all-reduces it passes on."""

    def __init__(self, comm):
        self._comm, self.sums = comm, 0
        self.rank, self.world_size = comm.rank, comm.world_size

    def allreduce_sum(self, arr, n=None):
        self.sums += 1
        return self._comm.allreduce_sum(arr, n)

    def __getattr__(self, name):
        return getattr(self._comm, name)


def test_sharded_step_equals_the_whole_batch_without_node_norm_allreduces():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in GN.init_params(16, 64, seed=7).items()}
    base = {k: v for k, v in p.items() if k not in GN.SCALE_KEYS}

    def step(ctx, part, comm, gb, norm="graph"):
        m = _make(ctx, None, "max", comm, norm)
        m.build(hb.f)
        m.load_state_dict(p if norm == "graph" else base)
        loss, acc = m.train_step(_device_batch(ctx, part), lr=0.05, global_batch=gb)
        return {"loss": loss, "acc": acc, "g": m.gradients(), "w": m.flat_p.numpy(), "b": part.n_graphs,
                "sums": comm.sums if comm is not None else 0}

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        try:
            part, gb = shard.shard_batch(hb, rank, 2)
            graph = step(ctx, part, _Counting(make_comm(ctx)), gb)
            batch = step(ctx, part, _Counting(make_comm(ctx)), gb, norm="batch")
            return graph, batch["sums"]
        finally:
            ctx.close()

    ctx = gcnx.Context(0)
    try:
        whole = step(ctx, hb, None, None)
    finally:
        ctx.close()
    ranks = ThreadWorld(2).run(rank_fn)
    assert sum(r["b"] for r, _ in ranks) == hb.n_graphs and all(r["b"] > 0 for r, _ in ranks)
    for r, batch_sums in ranks:
        assert abs(r["loss"] - whole["loss"]) < 1e-5 * max(1.0, abs(whole["loss"])), (r["loss"], whole["loss"])
        assert r["acc"] == whole["acc"]
        _cmp_grads(r["g"], whole["g"], 1e-4, "graph shards")
        assert rel_err(r["w"], whole["w"]) < 1e-4
        assert r["sums"] == batch_sums - 6, (r["sums"], batch_sums)         # BN1 / BN2: four forward moment sums, two backward sums
    assert same(ranks[0][0]["w"], ranks[1][0]["w"])

"""GPU tests of APPNP propagation: gcnx_appnp_propagate (csrc/appnp.hip) on its one-launch (resident) and K-launch (streamed)
routes, the layer gcnx.APPNPConv and the model gcnx.APPNP on both routes (GCNX_APPNP_RESIDENT) -- each against the float64
restatement tests/appnp_ref.py, the model on the device's side of every kink.  Tolerances: TIGHT = 2e-5 for the single fp32
kernel whatever K (an fp32 emulation of the recursion on ecoli_batch(3) stays below 2.1e-7 up to K = 64), 1e-4 for a whole step.
Both routes and every column block evaluate one expression per element, so they are compared bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import appnp_ref as AP
import gcn_bn_ref as R
import sage_ref as SR
from gpu_frames import SENTINEL, Frame, bits, same
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
STEP = 1e-4
CBS = (128, 64, 48, 32, 16, 8, 4)
KS, ALPHAS = (0, 1, 2, 3, 10), (0.0, 0.1, 1.0)
WORST = {}                                       # what -> the worst error / tolerance ratio seen


def _worst(what, value):
    WORST[what] = max(WORST.get(what, 0.0), float(value))


def _fits(rows, cb):
    """include/gcnx.h: two buffers of rows x cb floats and the row pointers (rows + 1, padded to 4) within 128 KiB; cb <= 256."""
    return 0 < cb <= 256 and cb % 4 == 0 and 2 * rows * cb * 4 + 4 * ((rows + 1 + 3) // 4 * 4) <= 128 * 1024


@functools.lru_cache(maxsize=None)
def _host(kind):
    """The batch's pattern (f does not matter to it), its float64 operators and a feature matrix without zeros, computed once."""
    from gcnx import synth
    hb = _tiny_host(16, 4) if kind == "tiny" else synth.ecoli_batch(3, 4)
    sizes = np.diff(hb.graph_ptr)
    if kind == "tiny":
        assert sizes.min() >= 8 and sizes.max() <= 64 and hb.n_graphs == 16
    else:
        assert list(sizes) == [808, 525, 326] and int(np.diff(hb.rowptr).max()) == 22
    ones = _scipy_adj(hb)
    mean = SR.mean_operator(ones, hb.n)
    ops = {"gcn": R.pyg_norm(ones, hb.n), "ones": ones, "mean_t": mean.T.tocsr()}
    ops["gcn_t"] = ops["gcn"].T.tocsr()
    return hb, ops


@functools.lru_cache(maxsize=None)
def _x(n, f, seed=0):
    x = np.random.default_rng(1000 * f + seed).standard_normal((n, f)).astype(np.float32)
    x[x == 0] = 1.0
    return x


def _dev_ops(ctx, hb):
    from gcnx.device import DeviceCSR
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    g = a.gcn_norm("pyg")
    ops = {"gcn": g, "gcn_t": g.transpose(), "ones": a.unweighted(), "mean_t": a.row_mean().transpose()}
    assert ops["ones"].vals is None and ops["mean_t"] is not a.row_mean() and a.max_block_rows == int(np.diff(hb.graph_ptr).max())
    return ops


def _prop(ctx, a, xd, k, alpha, col_block=0, scratch=True):
    from gcnx import device as D
    n, f = xd.shape
    out = ctx.empty((n, f))
    D.appnp_propagate(ctx, a, xd, out, k, alpha, scratch=ctx.empty((max(n * f, 4),)) if scratch else None, col_block=col_block)
    return out.numpy()


def _forced(ctx, a, xd, k, alpha, cb):
    """The forced resident call, or None where the library answers GCNX_ERR_UNSUPPORTED."""
    from gcnx import _lib
    try:
        return _prop(ctx, a, xd, k, alpha, col_block=cb, scratch=False)
    except _lib.GcnxError as e:
        assert e.code == _lib.ERR_UNSUPPORTED, e
        return None


# ---- 1. against float64, and the same bits on every route --------------------------------------------------------------------
@pytest.mark.parametrize("kind,f", [("tiny", 4), ("tiny", 16), ("tiny", 48), ("tiny", 64), ("tiny", 128), ("ecoli", 16), ("ecoli", 64)])
def test_propagate_against_float64_and_same_bits_on_every_route(ctx, kind, f):
    from gcnx import device as D
    hb, refs = _host(kind)
    ops = _dev_ops(ctx, hb)
    rows = int(np.diff(hb.graph_ptr).max())
    x = _x(hb.n, f)
    xd = ctx.to_device(x)
    assert D.appnp_resident_ok(ctx, rows, f)
    worst, n_forced = 0.0, 0
    for name, a in ops.items():
        for k in KS:
            for alpha in ALPHAS:
                ref = AP.propagate(refs[name], x, k, np.float64(np.float32(alpha)))
                got = _prop(ctx, a, xd, k, alpha)
                err = rel_err(got, ref)
                worst = max(worst, err)
                assert err < TIGHT, (name, k, alpha, err)
                streamed = _prop(ctx, a, xd, k, alpha, col_block=-1)
                assert same(streamed, got), (name, k, alpha, "streamed")
                for cb in CBS:
                    res = _forced(ctx, a, xd, k, alpha, cb)
                    assert (res is not None) == (cb <= f and _fits(rows, cb)), (name, k, alpha, cb)
                    if res is not None:
                        n_forced += 1
                        assert same(res, got), (name, k, alpha, cb)
                if k >= 1 and alpha == 1.0:
                    assert same(got, x), (name, k, "alpha = 1 returns x")
                if k == 0:
                    assert same(got, x)
        assert same(_prop(ctx, a, xd, 10, 0.1), _prop(ctx, a, xd, 10, 0.1)), (name, "a second call")
    assert n_forced >= len(ops) * len(KS) * len(ALPHAS) * (1 if f == 4 else 2)
    # K = 1, alpha = 0 is one aggregation: gcnx_spmm_csr on the same operator
    out = ctx.empty((hb.n, f))
    D.spmm(ctx, ops["gcn"], xd, None, out)
    assert rel_err(_prop(ctx, ops["gcn"], xd, 1, 0.0), out.numpy()) < TIGHT
    print(f"appnp_propagate {kind} f={f}: worst rel_err {worst:.2e} = {worst / TIGHT:.3f} of TIGHT")
    _worst("kernel err / TIGHT", worst / TIGHT)


def test_propagate_64_hops(ctx):
    hb, refs = _host("ecoli")
    a = _dev_ops(ctx, hb)["gcn"]
    x = _x(hb.n, 16)
    xd = ctx.to_device(x)
    got = _prop(ctx, a, xd, 64, 0.05)
    err = rel_err(got, AP.propagate(refs["gcn"], x, 64, np.float64(np.float32(0.05))))
    print(f"appnp_propagate K=64 alpha=0.05: rel_err {err:.2e}")
    assert err < TIGHT
    assert same(_prop(ctx, a, xd, 64, 0.05, col_block=-1), got) and same(_forced(ctx, a, xd, 64, 0.05, 4), got)
    _worst("kernel err / TIGHT", err / TIGHT)


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------
def _hand_batch(sizes, empty_row, seed=3):
    """Ring graphs (self-loop, both neighbours) of the given sizes with random values; ``empty_row`` stores no entry."""
    rng = np.random.default_rng(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows, cols = [], []
    for g, m in enumerate(sizes):
        for i in range(m):
            r = gp[g] + i
            if r == empty_row:
                continue
            for c in sorted({(i - 1) % m, i, (i + 1) % m}):
                rows.append(r); cols.append(gp[g] + c)
    n = int(gp[-1])
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    vals = rng.uniform(0.1, 0.6, len(cols)).astype(np.float32)
    return rowptr, np.asarray(cols, np.int32), vals, gp


def test_propagate_hand_made_batch(ctx):
    import scipy.sparse as sp
    from gcnx import _lib
    from gcnx.device import DeviceCSR
    sizes = [1, 0, 2, 33, 64, 65]
    rowptr, colidx, vals, gp = _hand_batch(sizes, empty_row=40)
    n, f = int(gp[-1]), 8
    assert n == 165 and rowptr[41] == rowptr[40]
    A = sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n))
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    assert a.max_block_rows == 65 and a.n_blocks == 6
    x = _x(n, f, seed=1)
    xd = ctx.to_device(x)
    for op, ref_op in ((a, A), (a.transpose(), A.T.tocsr())):
        for k in (1, 2, 5):
            ref = AP.propagate(ref_op, x, k, np.float64(np.float32(0.1)))
            got = _prop(ctx, op, xd, k, 0.1)
            assert rel_err(got, ref) < TIGHT
            assert same(_prop(ctx, op, xd, k, 0.1, col_block=-1), got)
            for cb in (8, 4):
                assert same(_forced(ctx, op, xd, k, 0.1, cb), got), (k, cb)
            if op is a:                      # the row without stored entries: z = alpha * x after any K >= 1
                assert same(got[40], np.float32(0.1) * x[40])
    # n = 0 and b = 0: nothing is launched, whatever the pointers
    out = Frame(ctx, n, f, f, 0)
    args = lambda nn, bb: (ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, a.block_ptr.ptr, bb, 65, xd.ptr, f, nn, f, 3, 0.1, 0,
                           out.view.ptr, f, None)
    assert ctx.lib.gcnx_appnp_propagate(*args(0, 6)) == _lib.OK and ctx.lib.gcnx_appnp_propagate(*args(n, 0)) == _lib.OK
    ctx.sync()
    out.untouched("n = 0 / b = 0")


@functools.lru_cache(maxsize=None)
def _ring_pair():
    rowptr, colidx, vals, gp = _hand_batch([5000, 10], empty_row=-1, seed=5)
    return rowptr, colidx, vals, gp


def test_a_graph_too_tall_for_lds_is_streamed(ctx):
    import scipy.sparse as sp
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    rowptr, colidx, vals, gp = _ring_pair()
    n, f = 5010, 4
    A = sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n))
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    assert a.max_block_rows == 5000 and not D.appnp_resident_ok(ctx, 5000, f) and not _fits(5000, 4)
    x = _x(n, f, seed=2)
    xd = ctx.to_device(x)
    got = _prop(ctx, a, xd, 10, 0.1)
    assert rel_err(got, AP.propagate(A, x, 10, np.float64(np.float32(0.1)))) < TIGHT
    assert same(_prop(ctx, a, xd, 10, 0.1, col_block=-1), got)
    assert _forced(ctx, a, xd, 10, 0.1, 4) is None
    # max_graph_rows understated and the resident route forced: the tall graph's rows are left untouched, the others are correct
    low = DeviceCSR(ctx, n, a.nnz, a.rowptr, a.colidx, a.vals, a.block_ptr, 2, False, max_block_rows=10)
    out = Frame(ctx, n, f, f, 0)
    D.appnp_propagate(ctx, low, xd, out.view, 10, 0.1, col_block=4)
    res = out.numpy()
    assert (res[:5000] == SENTINEL).all() and same(res[5000:], got[5000:])


# ---- 3. strides and alignment --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_block", [0, 16, -1])
def test_propagate_strided_operands(ctx, col_block):
    from gcnx import device as D
    hb, refs = _host("tiny")
    a = _dev_ops(ctx, hb)["mean_t"]
    f = 32
    x = _x(hb.n, f, seed=3)
    want = _prop(ctx, a, ctx.to_device(x), 3, 0.1, col_block=col_block)
    assert rel_err(want, AP.propagate(refs["mean_t"], x, 3, np.float64(np.float32(0.1)))) < TIGHT
    fx, fo = Frame(ctx, hb.n, f, 2 * f, 4, data=x), Frame(ctx, hb.n, f, f + 8, 8)
    assert fx.aligned() and fo.aligned()
    D.appnp_propagate(ctx, a, fx.view, fo.view, 3, 0.1, scratch=ctx.empty((hb.n * f,)), col_block=col_block)
    fo.check(want, "out")
    fx.untouched("x")


@pytest.mark.parametrize("f", [1, 3, 50])
def test_streamed_route_serves_any_width_and_alignment(ctx, f):
    from gcnx import device as D
    hb, refs = _host("tiny")
    a = _dev_ops(ctx, hb)["gcn"]
    x = _x(hb.n, f, seed=4)
    assert not D.appnp_resident_ok(ctx, a.max_block_rows, f) or f % 4 == 0
    for k in (1, 2, 3):
        fx, fo = Frame(ctx, hb.n, f, f + 3, 1, data=x), Frame(ctx, hb.n, f, f + 1, 3)
        fs = Frame(ctx, 1, hb.n * f, hb.n * f, 1)
        assert fx.view.ptr % 16 == 4 and fo.view.ptr % 16 == 12 and fs.view.ptr % 16 == 4
        for cb in (0, -1):
            D.appnp_propagate(ctx, a, fx.view, fo.view, k, 0.1, scratch=fs.row(0), col_block=cb)
            got = fo.numpy()
            assert rel_err(got, AP.propagate(refs["gcn"], x, k, np.float64(np.float32(0.1)))) < TIGHT, (f, k, cb)
        fs.numpy()                           # (nothing behind the scratch was written)
        fx.untouched("x")
    if f == 50:                              # an aligned f % 4 != 0 batch is streamed too, with the same bits as off the boundary
        assert same(_prop(ctx, a, ctx.to_device(x), 3, 0.1), got)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------
def test_propagate_refusals(ctx):
    from gcnx import _lib, device as D
    hb, _ = _host("ecoli")
    a = _dev_ops(ctx, hb)["gcn"]
    n, f, rows = hb.n, 64, 808
    xd = ctx.to_device(_x(n, f))
    out = Frame(ctx, n, f, f, 0)
    scratch = ctx.empty((n * f,))

    def rc(k=3, alpha=0.1, cb=0, x=xd.ptr, o=out.view.ptr, s=scratch.ptr, gptr=a.block_ptr.ptr, mgr=rows, ldx=f, ldo=f, width=f):
        return ctx.lib.gcnx_appnp_propagate(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, gptr, 3, mgr, x, ldx, n, width, k, alpha, cb,
                                            o, ldo, s)

    INVALID = 1
    for bad in (dict(k=-1), dict(k=65), dict(alpha=-0.01), dict(alpha=1.5), dict(alpha=float("nan")), dict(cb=-2),
                dict(o=xd.ptr), dict(o=xd.ptr + 4 * f * (n - 1)), dict(s=out.view.ptr), dict(s=xd.ptr, cb=-1),
                dict(cb=-1, s=None), dict(cb=-1, s=None, k=2), dict(gptr=None, s=None), dict(mgr=0, s=None), dict(ldx=f - 4),
                dict(ldo=f - 4)):
        assert rc(**bad) == INVALID, bad
    assert rc(cb=-1, s=None, k=1) == _lib.OK                                             # K = 1 needs no scratch
    assert same(out.numpy(), _prop(ctx, a, xd, 1, 0.1))
    out = Frame(ctx, n, f, f, 0)
    for cb in (6, 128, 32, 2):               # not float4 groups; wider than f; 2 * 808 * 32 * 4 B over the LDS budget
        assert not (_fits(rows, cb) and cb <= f)
        assert rc(cb=cb) == _lib.ERR_UNSUPPORTED, cb
    for bad in (dict(gptr=None), dict(mgr=0), dict(mgr=5000), dict(x=xd.ptr + 4, ldx=f), dict(width=62)):
        assert rc(cb=4, **bad) == _lib.ERR_UNSUPPORTED, bad
    ctx.sync()
    out.untouched("refused calls write nothing")
    # gcnx_appnp_resident_ok says what a forced call of the narrowest block accepts
    for mgr, width in ((808, 64), (3640, 64), (3641, 64), (808, 62), (0, 64)):
        ok = D.appnp_resident_ok(ctx, mgr, width)
        assert ok == (mgr > 0 and width % 4 == 0 and _fits(mgr, 4))
        assert (rc(cb=4, mgr=mgr, width=width, k=1) == _lib.OK) == ok, (mgr, width)
    assert not D.appnp_resident_ok(ctx, 808, 64, 66) and D.appnp_resident_ok(ctx, 808, 64, 128)


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_block", [0, -1])
def test_appnp_captured_replay_is_bit_identical(ctx, col_block):
    from gcnx import device as D
    hb, _ = _host("ecoli")
    a = _dev_ops(ctx, hb)["gcn"]
    f = 64
    xd = ctx.to_device(_x(hb.n, f))
    eager = _prop(ctx, a, xd, 10, 0.1, col_block=col_block)
    out, scratch = ctx.zeros((hb.n, f)), ctx.zeros((hb.n * f,))
    g = ctx.capture(lambda: D.appnp_propagate(ctx, a, xd, out, 10, 0.1, scratch=scratch, col_block=col_block))
    try:
        assert not out.numpy().any()                                     # captured, not yet executed
        for _ in range(2):
            out.fill_zero()
            g.launch()
            assert same(out.numpy(), eager)
    finally:
        g.destroy()


# ---- 6. the adjoint -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col_block", [0, -1])
def test_adjoint_identity_on_the_device(ctx, col_block):
    hb, refs = _host("tiny")
    ops = _dev_ops(ctx, hb)
    from gcnx.device import DeviceCSR
    mean = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).row_mean()
    f = 16
    x, y = _x(hb.n, f, seed=5), _x(hb.n, f, seed=6)
    px = _prop(ctx, mean, ctx.to_device(x), 10, 0.1, col_block=col_block).astype(np.float64)
    pty = _prop(ctx, ops["mean_t"], ctx.to_device(y), 10, 0.1, col_block=col_block).astype(np.float64)
    al = np.float64(np.float32(0.1))
    ref_px = AP.propagate(refs["mean_t"].T.tocsr(), x, 10, al)
    ref = float(np.sum(ref_px * y))
    terms = float(np.sum(np.abs(ref_px * y)))
    lhs, rhs = float(np.sum(px * y)), float(np.sum(x.astype(np.float64) * pty))
    print(f"adjoint: <Px, y> {lhs:.9g}  <x, P^T y> {rhs:.9g}  float64 {ref:.9g}  sum |terms| {terms:.3g}")
    assert abs(lhs - ref) <= TIGHT * terms and abs(rhs - ref) <= TIGHT * terms
    _worst("adjoint err / (TIGHT sum |terms|)", max(abs(lhs - ref), abs(rhs - ref)) / (TIGHT * terms))


# ---- 7. the layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [16, 50])
@pytest.mark.parametrize("propagations", [1, 10])
def test_appnpconv_layer_forward_and_backward(ctx, channels, propagations):
    from gcnx import device as D
    from gcnx.layers import APPNPConv
    hb, refs = _host("tiny")
    a = _dev_ops(ctx, hb)["mean_t"]          # an operator whose transpose is another matrix
    A = refs["mean_t"]
    assert D.appnp_resident_ok(ctx, a.max_block_rows, channels) == (channels == 16)      # 50 takes the streamed route
    x = _x(hb.n, 16, seed=7)
    lay = APPNPConv(channels, alpha=0.2, propagations=propagations, seed=3)
    xd = ctx.to_device(x)
    lay([xd, a])
    assert list(lay.params) == ["kernel", "bias"] and not lay.params["bias"].numpy().any()
    bias = np.random.default_rng(1).uniform(-0.5, 0.5, channels).astype(np.float32)
    lay.params["bias"].copy_from_host(bias)
    y = lay([xd, a]).numpy()
    w = lay.params["kernel"].numpy().astype(np.float64).T
    al = np.float64(np.float32(0.2))
    r_y, _ = AP.conv_fwd(A, x, w, bias, propagations, al)
    assert rel_err(y, r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((hb.n, channels)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r_dx, r_dw, r_db = AP.conv_bwd(A, x, w, dy, propagations, al)
    errs = (rel_err(dx.numpy(), r_dx), rel_err(lay.grads["kernel"].numpy(), r_dw.T), rel_err(lay.grads["bias"].numpy(), r_db))
    print(f"APPNPConv channels={channels} K={propagations}: rel_err y {rel_err(y, r_y):.2e} dx {errs[0]:.2e} dW {errs[1]:.2e} db {errs[2]:.2e}")
    assert max(errs) < TIGHT
    _worst("layer err / TIGHT", max(errs + (rel_err(y, r_y),)) / TIGHT)
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    if channels == 16:                       # the layer on the streamed route: the same bits
        lay2 = APPNPConv(channels, alpha=0.2, propagations=propagations, seed=3, col_block=-1)
        lay2([xd, a])
        lay2.params["bias"].copy_from_host(bias)
        assert same(lay2([xd, a]).numpy(), y)


# ---- 8. gcnx.APPNP: a whole step against the kink-separated restatement -----------------------------------------------------------
HEAD_UNDER_BN = {"linear_1.bias": "linear_1.weight", "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}
NODE_MLP_UNDER_BN = {"lin1.bias": "lin1.weight", "lin2.bias": "lin2.weight"}      # K = 0: BatchNorm cancels the Linear's bias


def _cmp_grads(got, ref, tol, what, under_bn):
    """The family's step rule: tol of the tensor's largest reference magnitude (an analytically zero gradient: of the weight
    gradient named for it, as test_gpu_gcn_bn.UNDER_BN does)."""
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[under_bn.get(k, k)], np.float64))))
        err = float(np.max(np.abs(g - r)))
        assert err <= tol * scale, (what, k, err, scale)
        _worst("step gradient err / tol", err / (tol * scale) if scale > 0 else 0.0)


# name -> (batch, hidden, K, alpha, GCNX_APPNP_RESIDENT, inputs, readout, norm)
STEP_CASES = {
    "tiny-16-resident": ("tiny", 16, 10, 0.1, "1", "device", "max", "batch"),
    "tiny-64-resident": ("tiny", 64, 10, 0.1, "1", "device", "max", "batch"),
    "tiny-64-streamed": ("tiny", 64, 10, 0.1, "0", "device", "max", "batch"),
    "tiny-64-resident-host": ("tiny", 64, 10, 0.1, "1", "host", "max", "batch"),
    "tiny-64-streamed-host": ("tiny", 64, 10, 0.1, "0", "host", "max", "batch"),
    "ecoli-64-resident": ("ecoli", 64, 10, 0.1, "1", "device", "max", "batch"),
    "ecoli-64-streamed": ("ecoli", 64, 10, 0.1, "0", "device", "max", "batch"),
    "node-mlp": ("tiny", 64, 0, 0.1, "1", "device", "max", "batch"),
    "one-hop": ("tiny", 64, 1, 0.1, "1", "device", "max", "batch"),
    "attention": ("tiny", 64, 10, 0.1, "1", "device", "attention", "batch"),
    "graph-norm": ("tiny", 64, 10, 0.1, "1", "device", "max", "graph"),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_appnp_step_against_restatement(ctx, monkeypatch, case):
    import gcnx
    from gcnx import device as D, synth
    kind, h, K, alpha, resident, route, readout, norm = STEP_CASES[case]
    hb = _tiny_host(16, 16, seed=4) if kind == "tiny" else synth.ecoli_batch(3, 16)
    a = _scipy_adj(hb)
    monkeypatch.setenv("GCNX_APPNP_RESIDENT", resident)
    m = gcnx.APPNP(ctx, hidden_channels=h, K=K, alpha=alpha, seed=0, readout=readout, norm=norm)
    assert m._col_block == (0 if resident == "1" else -1)
    p0 = {k: v.astype(np.float32) for k, v in AP.init_params(16, h, seed=7, readout=readout, norm=norm).items()}
    m.load_state_dict(p0)
    assert list(m.state_dict()) == list(AP.keys(readout, norm))
    inputs = _device_batch(ctx, hb) if route == "device" else (hb.x, a, hb.ids())
    target = None if route == "device" else hb.y
    under = dict(HEAD_UNDER_BN, **(NODE_MLP_UNDER_BN if K == 0 else {}))
    al = np.float64(np.float32(alpha))
    for step in range(2):
        p = m.state_dict()
        pos = {}
        if norm == "graph":                                  # the PReLU sides: the signs of y1 / y2 of a forward of its own
            m(inputs)
            pos = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
        m.loss_and_grads(inputs, target)
        batch, b = m._last_batch, m._bufs
        assert batch.a.max_block_rows == int(np.diff(hb.graph_ptr).max()) and D.appnp_resident_ok(ctx, batch.a.max_block_rows, h)
        if norm == "batch":
            pos = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), p[f"batch_norm_{i}.weight"],
                                                 p[f"batch_norm_{i}.bias"]) for i in (1, 2)}
        arg = b["arg"].numpy().astype(np.int64) if readout == "max" else None
        r = AP.model(hb.x, a, hb.graph_ptr, p, K, al, hb.y, masks=pos, argmax=arg, readout=readout, norm=norm)
        what = f"{case} step {step}"
        assert_close(b["z1"].numpy(), r["z1"], STEP, f"{what} z1")
        assert_close(b["out"].numpy(), r["out"], STEP, f"{what} logits")
        la = m.loss_acc.numpy()
        assert rel_err(la[0], r["loss"]) < STEP and la[1] == r["hits"], (what, la, r["loss"], r["hits"])
        got = m.gradients()
        assert list(got) == list(AP.keys(readout, norm))
        _cmp_grads(got, r["grads"], STEP, what, under)
        if K > 0:                            # P (1 b^T) is not constant over rows: the Linears' biases have genuine gradients
            assert all(np.abs(r["grads"][k]).max() > 1e-3 * np.abs(r["grads"][k.replace("bias", "weight")]).max()
                       for k in ("lin1.bias", "lin2.bias")), what
        m._apply_sgd(0.05)
    print("worst:", WORST)


def test_both_routes_give_the_model_the_same_bits(ctx, monkeypatch):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    p0 = {k: v.astype(np.float32) for k, v in AP.init_params(16, 64, seed=7).items()}
    grads = []
    for resident in ("1", "0"):
        monkeypatch.setenv("GCNX_APPNP_RESIDENT", resident)
        m = gcnx.APPNP(ctx, hidden_channels=64, K=10, alpha=0.1, seed=0)
        m.load_state_dict(p0)
        m.loss_and_grads(_device_batch(ctx, hb))
        grads.append(m.flat_g.numpy())
    assert np.array_equal(bits(grads[0]), bits(grads[1]))


# ---- 9. state, single graphs, fit ---------------------------------------------------------------------------------------------------
def test_appnp_state_dict_round_trip_single_graph_and_forward(ctx):
    import gcnx
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.APPNP(ctx, seed=1)
    ids, a = hb.ids(), _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1) and np.all(np.isfinite(logits))
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    sd = m.state_dict()
    assert list(sd) == list(AP.KEYS) and sd["lin1.weight"].shape == (64, 16) and sd["lin2.bias"].shape == (64,)
    assert np.max(np.abs(sd["lin1.weight"])) <= 0.25 and np.max(np.abs(sd["lin2.weight"])) <= 0.125   # U(+-1/sqrt(fan_in))
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    m2 = gcnx.APPNP(ctx, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(bits(v), bits(sd[k])), k
    assert np.array_equal(bits(m2((hb.x, a, ids))), bits(logits))
    r = AP.model(hb.x, a, hb.graph_ptr, sd, 10, np.float64(np.float32(0.1)), masks={
        f"m{i}": R.device_prelu_sides(m._bufs[f"z{i}"].numpy(), m._bufs[f"m{i}"].numpy(), m._bufs[f"i{i}"].numpy(),
                                      sd[f"batch_norm_{i}.weight"], sd[f"batch_norm_{i}.bias"]) for i in (1, 2)},
        argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert_close(logits, r["out"], STEP, "forward logits")
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


def test_fit_runs_the_appnp_model(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:12]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[12:]])
    m = gcnx.APPNP(ctx, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=4, epochs=1, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=4, shuffle=False), epochs=1, verbose=False)           # three steps
    assert len(out["history"]) == 1 and all(np.all(np.isfinite(h)) for h in out["history"])


# ---- 10. sync-BN over graph shards --------------------------------------------------------------------------------------------------
def test_appnp_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in AP.init_params(16, 64, seed=7).items()}

    def step(ctx, part, comm, gb):
        m = gcnx.APPNP(ctx, hidden_channels=64, K=10, alpha=0.1, seed=0, comm=comm)
        m.build(hb.f)
        m.load_state_dict(p)
        loss, acc = m.train_step(_device_batch(ctx, part), lr=0.05, global_batch=gb)
        return {"loss": loss, "acc": acc, "g": m.flat_g.numpy()[:m.n_params], "w": m.flat_p.numpy(), "b": part.n_graphs}

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
    for r in ranks:      # the tolerances of test_gpu_gcn_sync_bn._check_sharded for the same comparison
        assert abs(r["loss"] - whole["loss"]) < 1e-5 * max(1.0, abs(whole["loss"])), (r["loss"], whole["loss"])
        assert r["acc"] == whole["acc"]
        assert rel_err(r["g"], whole["g"]) < 1e-4, rel_err(r["g"], whole["g"])
        assert rel_err(r["w"], whole["w"]) < 1e-4
    assert np.array_equal(bits(ranks[0]["w"]), bits(ranks[1]["w"]))

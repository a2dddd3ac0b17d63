"""GPU tests of the Chebyshev convolution: gcnx_cheb_norm, gcnx_cheb_basis and gcnx_cheb_sum (csrc/cheb.hip) on their one-launch
(resident) and one-launch-per-gather (streamed) routes, the layer gcnx.ChebConv and the model gcnx.Cheb on both routes
(GCNX_CHEB_RESIDENT) -- each against the float64 restatement tests/cheb_ref.py, the model on the device's side of every kink.
Tolerances: 1e-6 for the operator's values (the bar of the graph-prep tests), TIGHT = 2e-5 for a single fp32 kernel up to K = 5,
1e-4 for a whole step; K = 16 is held to a bound computed from the recurrence itself (test_sixteen_terms_within_the_rounding_bound).
Both routes and every column block evaluate one expression per element, so they are compared bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import cheb_ref as CH
import gcn_bn_ref as R
from gpu_frames import SENTINEL, Frame, bits, same
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
STEP = 1e-4
NORM = 1e-6
CBS = (128, 64, 48, 32, 16, 8, 4)
# (K, lambda_max): below the spectrum's edge (1.5) the terms grow, so K <= 3 there
CASES = [(K, lam) for K in (1, 2, 3, 5) for lam in (2.0, 3.0)] + [(K, 1.5) for K in (1, 2, 3)]
WORST = {}                                       # what -> the worst error / tolerance ratio seen


def _worst(what, value):
    WORST[what] = max(WORST.get(what, 0.0), float(value))


def _fits(rows, cb):
    """include/gcnx.h: two buffers of rows x cb floats and the row pointers (rows + 1, padded to 4) within 128 KiB; cb <= 256."""
    return 0 < cb <= 256 and cb % 4 == 0 and 2 * rows * cb * 4 + 4 * ((rows + 1 + 3) // 4 * 4) <= 128 * 1024


@functools.lru_cache(maxsize=None)
def _host(kind):
    """The batch's pattern, asymmetric random weights on it, and the float64 operators: S of the pattern, S of the weighted
    matrix and its transpose -- computed once."""
    import scipy.sparse as sp
    from gcnx import synth
    hb = _tiny_host(16, 4) if kind == "tiny" else synth.ecoli_batch(3, 4)
    sizes = np.diff(hb.graph_ptr)
    if kind == "tiny":
        assert sizes.min() >= 8 and sizes.max() <= 64 and hb.n_graphs == 16
        assert np.all(_scipy_adj(hb).diagonal() == 1)                                  # stored loops
    else:
        assert list(sizes) == [808, 525, 326] and int(np.diff(hb.rowptr).max()) == 22
    w = np.random.default_rng(7).uniform(0.2, 1.5, len(hb.colidx)).astype(np.float32)
    weighted = sp.csr_matrix((w.astype(np.float64), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    refs = {"S": CH.operator(_scipy_adj(hb), hb.n), "Sw": CH.operator(weighted, hb.n)}
    refs["Sw_t"] = refs["Sw"].T.tocsr()
    assert (abs(refs["Sw"] - refs["Sw_t"]) > 1e-6).nnz > 0
    return hb, w, refs


@functools.lru_cache(maxsize=None)
def _x(n, f, seed=0):
    x = np.random.default_rng(1000 * f + seed).standard_normal((n, f)).astype(np.float32)
    x[x == 0] = 1.0
    return x


def _dev_ops(ctx, hb, w):
    from gcnx.device import DeviceCSR
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    aw = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, w, hb.graph_ptr)
    assert a.symmetric and not aw.symmetric and a.max_block_rows == int(np.diff(hb.graph_ptr).max())
    sw = aw.cheb_norm()
    ops = {"S": a.cheb_norm(), "Sw": sw, "Sw_t": sw.transpose()}
    assert ops["Sw_t"] is not sw and ops["S"].transpose() is ops["S"] and aw.cheb_norm() is sw
    return ops


def _basis(ctx, a, xd, k, lam, col_block=0):
    from gcnx import device as D
    n, f = xd.shape
    out = ctx.empty((n, k * f))
    D.cheb_basis(ctx, a, xd, out, k, lam, col_block=col_block)
    return out.numpy()


def _sum(ctx, a, hd, bias, k, lam, col_block=0, scratch=True):
    from gcnx import device as D
    n, f = hd.shape[0], hd.shape[1] // k
    out = ctx.empty((n, f))
    D.cheb_sum(ctx, a, hd, bias, out, k, lam, scratch=ctx.empty((max(n * f, 4),)) if scratch else None, col_block=col_block)
    return out.numpy()


def _forced(fn, *args, cb, **kw):
    """The forced resident call, or None where the library answers GCNX_ERR_UNSUPPORTED."""
    from gcnx import _lib
    try:
        return fn(*args, col_block=cb, **kw)
    except _lib.GcnxError as e:
        assert e.code == _lib.ERR_UNSUPPORTED, e
        return None


# ---- 1. the operator -----------------------------------------------------------------------------------------------------------
def _check_norm(ctx, rowptr, colidx, vals, gp, what):
    from gcnx.device import DeviceCSR
    n = len(rowptr) - 1
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    s = a.cheb_norm()
    got, ref = s.vals.numpy()[:a.nnz], CH.operator_values(rowptr, colidx, vals, n)
    assert s.rowptr is a.rowptr and s.colidx is a.colidx and s.max_block_rows == a.max_block_rows and s.symmetric == a.symmetric
    err = rel_err(got, ref)
    assert err < NORM, (what, err)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    diag = rows == colidx
    assert diag.any() and np.array_equal(bits(got[diag]), bits(np.zeros(int(diag.sum()), np.float32))), (what, "a stored diagonal is +0")
    deg = np.bincount(colidx[~diag], weights=(np.ones(len(colidx)) if vals is None else vals)[~diag], minlength=n)
    assert not got[(deg[rows] == 0) | (deg[colidx] == 0)].any(), (what, "entries of a node without incoming weight are 0")
    again = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp).cheb_norm()
    assert same(again.vals.numpy(), s.vals.numpy()), (what, "a second call")
    _worst("norm err / 1e-6", err / NORM)
    return err


def test_cheb_norm_against_the_restatement(ctx):
    errs = []
    for kind in ("tiny", "ecoli"):
        hb, w, _ = _host(kind)
        errs.append(_check_norm(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr, kind))
        errs.append(_check_norm(ctx, hb.rowptr, hb.colidx, w, hb.graph_ptr, kind + " weighted"))
    rowptr, colidx, vals, gp = CH.hand_batch()
    errs.append(_check_norm(ctx, rowptr, colidx, None, gp, "hand"))
    errs.append(_check_norm(ctx, rowptr, colidx, vals, gp, "hand weighted"))
    from gcnx.device import DeviceCSR
    s = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp).cheb_norm().vals.numpy()
    assert not s[rowptr[4]:rowptr[6]].size and s[rowptr[11]] == 0 and s[rowptr[9] + 2] != 0        # rows 4, 5 empty; (9, 11) lives
    # values on one side only are refused; n = 0 launches nothing
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    t, out = a.transpose(), Frame(ctx, 1, a.nnz, a.nnz, 0)
    call = lambda v, vt, n: ctx.lib.gcnx_cheb_norm(ctx.h, a.rowptr.ptr, a.colidx.ptr, v, t.rowptr.ptr, t.colidx.ptr, vt, n, out.view.ptr)
    assert call(a.vals.ptr, None, a.n) == 1 and call(None, t.vals.ptr, a.n) == 1 and call(a.vals.ptr, t.vals.ptr, -1) == 1
    assert call(a.vals.ptr, t.vals.ptr, 0) == 0
    ctx.sync()
    out.untouched("refused and empty calls write nothing")
    print(f"cheb_norm: worst rel_err {max(errs):.2e} = {max(errs) / NORM:.3f} of 1e-6")


# ---- 2. basis and sum against float64, and the same bits on every route ----------------------------------------------------------
@pytest.mark.parametrize("kind,f", [("tiny", 4), ("tiny", 16), ("tiny", 48), ("tiny", 64), ("tiny", 128), ("ecoli", 16), ("ecoli", 64)])
def test_basis_and_sum_against_float64_and_same_bits_on_every_route(ctx, kind, f):
    from gcnx import device as D
    hb, w, refs = _host(kind)
    ops = _dev_ops(ctx, hb, w)
    rows = int(np.diff(hb.graph_ptr).max())
    x = _x(hb.n, f)
    xd = ctx.to_device(x)
    bias = np.random.default_rng(f).uniform(-0.5, 0.5, f).astype(np.float32)
    bd = ctx.to_device(bias)
    assert D.cheb_resident_ok(ctx, rows, f)
    worst, n_forced = 0.0, 0
    for name, a in ops.items():
        for K, lam in CASES:
            h = _x(hb.n, K * f, seed=K)
            hd = ctx.to_device(h)
            runs = (("basis", lambda col_block: _basis(ctx, a, xd, K, lam, col_block=col_block), CH.basis(refs[name], x, K, lam, fp32=True)),
                    ("sum", lambda col_block: _sum(ctx, a, hd, bd, K, lam, col_block=col_block), CH.cheb_sum(refs[name], h, bias, K, lam, fp32=True)))
            for what, run, ref in runs:
                got = run(0)
                err = rel_err(got, ref)
                worst = max(worst, err)
                assert err < TIGHT, (name, what, K, lam, err)
                assert same(run(-1), got), (name, what, K, lam, "streamed")
                for cb in CBS:
                    res = _forced(run, cb=cb)
                    assert (res is not None) == (cb <= f and _fits(rows, cb)), (name, what, K, lam, cb)
                    if res is not None:
                        n_forced += 1
                        assert same(res, got), (name, what, K, lam, cb)
            if K == 1:
                assert same(_basis(ctx, a, xd, 1, lam), x) and same(_sum(ctx, a, hd, None, 1, lam), h)
        assert same(_basis(ctx, a, xd, 5, 2.0), _basis(ctx, a, xd, 5, 2.0)), (name, "a second call")
        h5 = ctx.to_device(_x(hb.n, 5 * f, seed=5))
        assert same(_sum(ctx, a, h5, bd, 5, 3.0), _sum(ctx, a, h5, bd, 5, 3.0)), (name, "a second call")
    assert n_forced >= len(ops) * len(CASES) * 2 * (1 if f == 4 else 2)
    # K = 2, lambda_max = 2: T_1 = L^ = -S, one aggregation: gcnx_spmm_csr on the same operator
    out = ctx.empty((hb.n, f))
    D.spmm(ctx, ops["Sw"], xd, None, out)
    assert rel_err(_basis(ctx, ops["Sw"], xd, 2, 2.0)[:, f:], -out.numpy()) < TIGHT
    print(f"cheb basis / sum {kind} f={f}: worst rel_err {worst:.2e} = {worst / TIGHT:.3f} of TIGHT")
    _worst("kernel err / TIGHT", worst / TIGHT)


# ---- 3. K = 16: a bound from the recurrence itself ----------------------------------------------------------------------------------
def _dev_operator(a, n):
    """The device's own fp32 values of an operator as a float64 scipy CSR."""
    import scipy.sparse as sp
    return sp.csr_matrix((a.vals.numpy()[:a.nnz].astype(np.float64), a.colidx.numpy()[:a.nnz], a.rowptr.numpy()), shape=(n, n))


def _bounded(S, start, inj, K, lam, bias=None):
    """The float64 recurrence of gcnx_cheb_basis (inj None) or gcnx_cheb_sum and, beside it, a bound on what the fp32 kernel may
    be off by: the same recurrence on absolute values.  A step's (row entries + 4) rounded operations -- the fmaf chain, the
    subtraction, the two fmaf of the recurrence, the bias add -- each add at most 2^-24 of the sum of the step's absolute terms;
    the error already in the two previous terms passes through |a| |S| + |b| and + 1.  Returns [(term, bound)] per step."""
    cs, cd = CH.coefs(lam, fp32=True)
    A = abs(S)
    u = ((np.diff(S.indptr) + 4) * 2.0 ** -24)[:, None]
    cur, e_cur = np.asarray(start, np.float64), np.zeros_like(start, dtype=np.float64)
    prev, e_prev = np.zeros_like(cur), np.zeros_like(cur)
    out = [(cur, e_cur)]
    for s in range(1, K):
        single = (s == K - 1) if inj is not None else (s == 1)
        a, b = (cs, cd) if single else (2 * cs, 2 * cd)
        h = inj(K - 1 - s) if inj is not None else 0.0
        new = a * (S @ cur) + b * cur + h - prev
        mag = abs(a) * (A @ (np.abs(cur) + e_cur)) + abs(b) * (np.abs(cur) + e_cur) + np.abs(h) + np.abs(prev) + e_prev
        if bias is not None and s == K - 1:
            new, mag = new + bias, mag + np.abs(bias)
        e_new = abs(a) * (A @ e_cur) + abs(b) * e_cur + e_prev + u * mag
        prev, e_prev, cur, e_cur = cur, e_cur, new, e_new
        out.append((cur, e_cur))
    return out


def test_sixteen_terms_within_the_rounding_bound(ctx):
    """K = 16 at f = 64 on ecoli: no tolerance is fixed in advance; every element is held to the bound of _bounded."""
    hb, w, _ = _host("ecoli")
    ops = _dev_ops(ctx, hb, w)
    K, f = 16, 64
    x, h = _x(hb.n, f), _x(hb.n, K * f, seed=16)
    bias = np.random.default_rng(16).uniform(-0.5, 0.5, f).astype(np.float32)
    xd, hd, bd = ctx.to_device(x), ctx.to_device(h), ctx.to_device(bias)
    share = 0.0
    for name in ("S", "Sw_t"):
        a = ops[name]
        S = _dev_operator(a, hb.n)
        for lam in (2.0, 3.0):
            got = _basis(ctx, a, xd, K, lam).astype(np.float64)
            steps = _bounded(S, x, None, K, lam)
            for j, (t, e) in enumerate(steps):
                d = np.abs(got[:, j * f:(j + 1) * f] - t)
                assert np.all(d <= e), (name, lam, "basis", j, float(d.max()), float(e.max()))
                share = max(share, float(np.max(d[e > 0] / e[e > 0])) if (e > 0).any() else 0.0)
            assert same(_basis(ctx, a, xd, K, lam, col_block=-1), got.astype(np.float32)) and same(_forced(_basis, ctx, a, xd, K, lam, cb=16), got.astype(np.float32))
            got = _sum(ctx, a, hd, bd, K, lam).astype(np.float64)
            t, e = _bounded(S, h[:, (K - 1) * f:], lambda j: h[:, j * f:(j + 1) * f].astype(np.float64), K, lam, bias.astype(np.float64))[-1]
            d = np.abs(got - t)
            assert np.all(d <= e), (name, lam, "sum", float(d.max()), float(e.max()))
            share = max(share, float(np.max(d / e)))
            assert same(_sum(ctx, a, hd, bd, K, lam, col_block=-1), got.astype(np.float32)) and same(_forced(_sum, ctx, a, hd, bd, K, lam, cb=16), got.astype(np.float32))
    print(f"cheb K=16 f=64 ecoli: worst |error| / bound {share:.3f}")
    _worst("K=16 err / bound", share)


# ---- 4. routes and operands ----------------------------------------------------------------------------------------------------------
def _hand_ring(sizes, seed=5):
    """Ring graphs (self-loop, both neighbours) of the given sizes with random values."""
    rng = np.random.default_rng(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows, cols = [], []
    for g, m in enumerate(sizes):
        for i in range(m):
            for c in sorted({(i - 1) % m, i, (i + 1) % m}):
                rows.append(gp[g] + i); cols.append(gp[g] + c)
    n = int(gp[-1])
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rowptr, np.asarray(cols, np.int32), rng.uniform(0.1, 0.6, len(cols)).astype(np.float32), gp


def test_hand_made_batch_and_empty_calls(ctx):
    from gcnx import _lib
    from gcnx.device import DeviceCSR
    import scipy.sparse as sp
    rowptr, colidx, vals, gp = CH.hand_batch()
    n, f = 12, 8
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    assert not a.symmetric and a.max_block_rows == 6 and a.n_blocks == 4
    s = a.cheb_norm()
    S = CH.operator(sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n)), n)
    x = _x(n, f, seed=1)
    xd = ctx.to_device(x)
    for op, ref_op in ((s, S), (s.transpose(), S.T.tocsr())):
        for K, lam in ((2, 2.0), (3, 3.0), (5, 2.0)):
            h = _x(n, K * f, seed=K)
            hd = ctx.to_device(h)
            got = _basis(ctx, op, xd, K, lam)
            assert rel_err(got, CH.basis(ref_op, x, K, lam, fp32=True)) < TIGHT
            gs = _sum(ctx, op, hd, None, K, lam)
            assert rel_err(gs, CH.cheb_sum(ref_op, h, None, K, lam, fp32=True)) < TIGHT
            for cb in (-1, 8, 4):
                assert same(_basis(ctx, op, xd, K, lam, col_block=cb), got) and same(_sum(ctx, op, hd, None, K, lam, col_block=cb), gs)
            for i in (4, 5):                 # the isolated node and the one-node graph: L^ z = c_d z, exactly
                cd = np.float32(CH.coefs(lam, fp32=True)[1])
                assert same(got[i, f:2 * f], cd * x[i]) if lam != 2.0 else not got[i, f:2 * f].any()
                if lam == 2.0 and K >= 3:    # c_d = 0: T_2 = -T_0
                    assert same(got[i, 2 * f:3 * f], -x[i])
    # n = 0 and b = 0: nothing is launched, whatever the pointers
    out = Frame(ctx, n, 3 * f, 3 * f, 0)
    args = lambda nn, bb: (ctx.h, s.rowptr.ptr, s.colidx.ptr, s.vals.ptr, s.block_ptr.ptr, bb, 6, xd.ptr, f, nn, f, 3, 2.0, 0,
                           out.view.ptr, 3 * f, None)
    assert ctx.lib.gcnx_cheb_basis(*args(0, 4)) == _lib.OK and ctx.lib.gcnx_cheb_basis(*args(n, 0)) == _lib.OK
    ctx.sync()
    out.untouched("n = 0 / b = 0")


def test_a_graph_too_tall_for_lds_is_streamed(ctx):
    import scipy.sparse as sp
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    rowptr, colidx, vals, gp = _hand_ring([5000, 10])
    n, f, K = 5010, 4, 5
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False).cheb_norm()
    S = CH.operator(sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n)), n)
    assert a.max_block_rows == 5000 and not D.cheb_resident_ok(ctx, 5000, f) and not _fits(5000, 4)
    x, h = _x(n, f, seed=2), _x(n, K * f, seed=3)
    xd, hd = ctx.to_device(x), ctx.to_device(h)
    got = _basis(ctx, a, xd, K, 2.0)
    assert rel_err(got, CH.basis(S, x, K, 2.0, fp32=True)) < TIGHT
    gs = _sum(ctx, a, hd, None, K, 2.0)
    assert rel_err(gs, CH.cheb_sum(S, h, None, K, 2.0, fp32=True)) < TIGHT
    assert same(_basis(ctx, a, xd, K, 2.0, col_block=-1), got) and same(_sum(ctx, a, hd, None, K, 2.0, col_block=-1), gs)
    assert _forced(_basis, ctx, a, xd, K, 2.0, cb=4) is None and _forced(_sum, ctx, a, hd, None, K, 2.0, cb=4) is None
    # max_graph_rows understated and the resident route forced: the tall graph's rows are left untouched, the others are correct
    low = DeviceCSR(ctx, n, a.nnz, a.rowptr, a.colidx, a.vals, a.block_ptr, 2, False, max_block_rows=10)
    out = Frame(ctx, n, f, f, 0)
    D.cheb_sum(ctx, low, hd, None, out.view, K, 2.0, col_block=4)
    res = out.numpy()
    assert (res[:5000] == SENTINEL).all() and same(res[5000:], gs[5000:])


@pytest.mark.parametrize("col_block", [0, 16, -1])
def test_strided_operands_inside_sentinel_frames(ctx, col_block):
    from gcnx import device as D
    hb, w, refs = _host("tiny")
    a = _dev_ops(ctx, hb, w)["Sw_t"]
    f, K, lam = 32, 4, 3.0
    x, h = _x(hb.n, f, seed=3), _x(hb.n, K * f, seed=4)
    bias = np.random.default_rng(3).uniform(-0.5, 0.5, f).astype(np.float32)
    want_b = _basis(ctx, a, ctx.to_device(x), K, lam, col_block=col_block)
    want_s = _sum(ctx, a, ctx.to_device(h), ctx.to_device(bias), K, lam, col_block=col_block)
    assert rel_err(want_b, CH.basis(refs["Sw_t"], x, K, lam, fp32=True)) < TIGHT
    assert rel_err(want_s, CH.cheb_sum(refs["Sw_t"], h, bias, K, lam, fp32=True)) < TIGHT
    fx, fo = Frame(ctx, hb.n, f, 2 * f, 4, data=x), Frame(ctx, hb.n, K * f, K * f + 8, 8)
    assert fx.aligned() and fo.aligned()
    D.cheb_basis(ctx, a, fx.view, fo.view, K, lam, col_block=col_block)
    fo.check(want_b, "basis out")
    fx.untouched("x")
    fh, fo, fb = Frame(ctx, hb.n, K * f, K * f + 12, 4, data=h), Frame(ctx, hb.n, f, f + 8, 8), Frame(ctx, 1, f, f, 4, data=bias)
    assert fh.aligned() and fo.aligned()
    D.cheb_sum(ctx, a, fh.view, fb.row(0), fo.view, K, lam, scratch=ctx.empty((hb.n * f,)), col_block=col_block)
    fo.check(want_s, "sum out")
    fh.untouched("h")
    fb.untouched("bias")


@pytest.mark.parametrize("f", [1, 3, 50])
def test_streamed_route_serves_any_width_and_alignment(ctx, f):
    from gcnx import device as D
    hb, w, refs = _host("tiny")
    a = _dev_ops(ctx, hb, w)["Sw"]
    x = _x(hb.n, f, seed=4)
    bias = np.random.default_rng(f).uniform(-0.5, 0.5, f).astype(np.float32)
    assert not D.cheb_resident_ok(ctx, a.max_block_rows, f)
    for K in (1, 2, 3, 4):
        h = _x(hb.n, K * f, seed=10 + K)
        fx, fo = Frame(ctx, hb.n, f, f + 3, 1, data=x), Frame(ctx, hb.n, K * f, K * f + 1, 3)
        assert fx.view.ptr % 16 == 4 and fo.view.ptr % 16 == 12
        fh, fs, fb = Frame(ctx, hb.n, K * f, K * f + 2, 1, data=h), Frame(ctx, hb.n, f, f + 1, 3), Frame(ctx, 1, f, f, 1, data=bias)
        fscr = Frame(ctx, 1, hb.n * f, hb.n * f, 1)
        for cb in (0, -1):
            D.cheb_basis(ctx, a, fx.view, fo.view, K, 2.0, col_block=cb)
            got = fo.numpy()
            assert rel_err(got, CH.basis(refs["Sw"], x, K, 2.0, fp32=True)) < TIGHT, (f, K, cb)
            D.cheb_sum(ctx, a, fh.view, fb.row(0), fs.view, K, 2.0, scratch=fscr.row(0), col_block=cb)
            gs = fs.numpy()
            assert rel_err(gs, CH.cheb_sum(refs["Sw"], h, bias, K, 2.0, fp32=True)) < TIGHT, (f, K, cb)
        fscr.numpy()                         # (nothing behind the scratch was written)
        fx.untouched("x"); fh.untouched("h"); fb.untouched("bias")
    if f == 50:                              # an aligned f % 4 != 0 batch is streamed too, with the same bits as off the boundary
        assert same(_basis(ctx, a, ctx.to_device(x), 4, 2.0), got) and same(_sum(ctx, a, ctx.to_device(h), ctx.to_device(bias), 4, 2.0), gs)


def test_refusals(ctx):
    from gcnx import _lib, device as D
    hb, w, _ = _host("ecoli")
    a = _dev_ops(ctx, hb, w)["Sw"]
    n, f, rows, K = hb.n, 64, 808, 4
    xd, hd = ctx.to_device(_x(n, f)), ctx.to_device(_x(n, K * f, seed=4))
    bd = ctx.to_device(np.ones(f, np.float32))
    ob, osum = Frame(ctx, n, K * f, K * f, 0), Frame(ctx, n, f, f, 0)
    scratch = ctx.empty((n * f,))

    def basis(k=K, lam=2.0, cb=0, x=xd.ptr, o=ob.view.ptr, s=None, gptr=a.block_ptr.ptr, mgr=rows, ldx=f, ldo=K * f, width=f):
        return ctx.lib.gcnx_cheb_basis(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, gptr, 3, mgr, x, ldx, n, width, k, lam, cb, o, ldo, s)

    def csum(k=K, lam=2.0, cb=0, h=hd.ptr, bias=bd.ptr, o=osum.view.ptr, s=scratch.ptr, gptr=a.block_ptr.ptr, mgr=rows, ldh=K * f, ldo=f,
             width=f):
        return ctx.lib.gcnx_cheb_sum(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, gptr, 3, mgr, h, ldh, bias, n, width, k, lam, cb, o,
                                     ldo, s)

    INVALID = 1
    for bad in (dict(k=0), dict(k=17), dict(k=-1), dict(lam=0.0), dict(lam=-2.0), dict(lam=float("nan")), dict(lam=float("inf")),
                dict(cb=-2)):
        assert basis(**bad) == INVALID and csum(**bad) == INVALID, bad
    for bad in (dict(o=xd.ptr), dict(x=ob.view.ptr + 4 * (K * f * (n - 1))), dict(ldx=f - 4), dict(ldo=K * f - 4)):
        assert basis(**bad) == INVALID, bad
    for bad in (dict(o=hd.ptr), dict(o=hd.ptr + 4 * (K * f * (n - 1))), dict(s=osum.view.ptr), dict(s=hd.ptr, cb=-1), dict(o=bd.ptr, ldo=f),
                dict(cb=-1, s=None), dict(gptr=None, s=None), dict(mgr=0, s=None), dict(ldh=K * f - 4), dict(ldo=f - 4)):
        assert csum(**bad) == INVALID, bad
    assert csum(cb=-1, s=None, k=2, ldh=K * f) == _lib.OK                                 # K <= 2 needs no scratch
    assert same(osum.numpy(), _sum(ctx, a, hd.cols(0, 2 * f), bd, 2, 2.0))
    assert basis(cb=-1, s=None) == _lib.OK                                               # the basis never reads scratch
    assert same(ob.numpy(), _basis(ctx, a, xd, K, 2.0))
    ob, osum = Frame(ctx, n, K * f, K * f, 0), Frame(ctx, n, f, f, 0)
    for cb in (6, 128, 32, 2):               # not float4 groups; wider than f; 2 * 808 * 32 * 4 B over the LDS budget
        assert not (_fits(rows, cb) and cb <= f)
        assert basis(cb=cb, o=ob.view.ptr) == _lib.ERR_UNSUPPORTED and csum(cb=cb, o=osum.view.ptr) == _lib.ERR_UNSUPPORTED, cb
    for bad in (dict(gptr=None), dict(mgr=0), dict(mgr=5000), dict(width=62)):
        assert basis(cb=4, o=ob.view.ptr, **bad) == _lib.ERR_UNSUPPORTED and csum(cb=4, o=osum.view.ptr, **bad) == _lib.ERR_UNSUPPORTED, bad
    assert basis(cb=4, o=ob.view.ptr, x=xd.ptr + 4) == _lib.ERR_UNSUPPORTED and csum(cb=4, o=osum.view.ptr, h=hd.ptr + 4, ldh=K * f) == _lib.ERR_UNSUPPORTED
    ctx.sync()
    ob.untouched("refused calls write nothing")
    osum.untouched("refused calls write nothing")
    # gcnx_cheb_resident_ok says what a forced call of the narrowest block accepts
    for mgr, width in ((808, 64), (3640, 64), (3641, 64), (808, 62), (0, 64)):
        ok = D.cheb_resident_ok(ctx, mgr, width)
        assert ok == (mgr > 0 and width % 4 == 0 and _fits(mgr, 4))
        assert (csum(cb=4, mgr=mgr, width=width, k=2, ldh=K * f) == _lib.OK) == ok, (mgr, width)
    assert not D.cheb_resident_ok(ctx, 808, 64, 66) and D.cheb_resident_ok(ctx, 808, 64, 256)


@pytest.mark.parametrize("col_block", [0, -1])
def test_captured_replay_is_bit_identical(ctx, col_block):
    from gcnx import device as D
    hb, w, _ = _host("ecoli")
    a = _dev_ops(ctx, hb, w)["Sw"]
    f, K, lam = 64, 5, 2.0
    xd, hd = ctx.to_device(_x(hb.n, f)), ctx.to_device(_x(hb.n, K * f, seed=5))
    bd = ctx.to_device(np.full(f, 0.25, np.float32))
    eager_b, eager_s = _basis(ctx, a, xd, K, lam, col_block=col_block), _sum(ctx, a, hd, bd, K, lam, col_block=col_block)
    ob, osum, scratch = ctx.zeros((hb.n, K * f)), ctx.zeros((hb.n, f)), ctx.zeros((hb.n * f,))

    def both():
        D.cheb_basis(ctx, a, xd, ob, K, lam, col_block=col_block)
        D.cheb_sum(ctx, a, hd, bd, osum, K, lam, scratch=scratch, col_block=col_block)
    g = ctx.capture(both)
    try:
        assert not ob.numpy().any() and not osum.numpy().any()                # captured, not yet executed
        for _ in range(2):
            ob.fill_zero(); osum.fill_zero()
            g.launch()
            assert same(ob.numpy(), eager_b) and same(osum.numpy(), eager_s)
    finally:
        g.destroy()


@pytest.mark.parametrize("col_block", [0, -1])
def test_adjoint_identity_on_the_device(ctx, col_block):
    """<cheb_sum(S, H), dZ> = sum_k <H_k, basis(S^T, dZ)_k>: what the backward rests on."""
    hb, w, refs = _host("tiny")
    ops = _dev_ops(ctx, hb, w)
    f, K, lam = 16, 5, 3.0
    h, dz = _x(hb.n, K * f, seed=5), _x(hb.n, f, seed=6)
    zs = _sum(ctx, ops["Sw"], ctx.to_device(h), None, K, lam, col_block=col_block).astype(np.float64)
    g = _basis(ctx, ops["Sw_t"], ctx.to_device(dz), K, lam, col_block=col_block).astype(np.float64)
    ref_g = CH.basis(refs["Sw_t"], dz, K, lam, fp32=True)
    ref = float(np.sum(h * ref_g))
    terms = float(np.sum(np.abs(h * ref_g)))
    lhs, rhs = float(np.sum(zs * dz)), float(np.sum(h.astype(np.float64) * g))
    print(f"adjoint: <sum(H), dZ> {lhs:.9g}  <H, basis^T(dZ)> {rhs:.9g}  float64 {ref:.9g}  sum |terms| {terms:.3g}")
    assert abs(lhs - ref) <= TIGHT * terms and abs(rhs - ref) <= TIGHT * terms
    _worst("adjoint err / (TIGHT sum |terms|)", max(abs(lhs - ref), abs(rhs - ref)) / (TIGHT * terms))


# ---- 5. the layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [16, 50])
@pytest.mark.parametrize("K", [1, 3])
def test_chebconv_layer_forward_and_backward(ctx, channels, K):
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    from gcnx.layers import ChebConv
    hb, w, refs = _host("tiny")
    a = ChebConv.preprocess(DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, w, hb.graph_ptr))       # S^T is another matrix
    S = refs["Sw"]
    assert D.cheb_resident_ok(ctx, a.max_block_rows, channels) == (channels == 16)       # 50 takes the streamed route
    x = _x(hb.n, 16, seed=7)
    xd = ctx.to_device(x)
    dy = np.random.default_rng(9).standard_normal((hb.n, channels)).astype(np.float32)
    for use_bias in (True, False):
        lay = ChebConv(channels, K=K, lambda_max=3.0, use_bias=use_bias, seed=3)
        lay([xd, a])
        names = [f"lins.{k}.weight" for k in range(K)]
        assert list(lay.params) == names + (["bias"] if use_bias else []) and lay.weight.shape == (16, K * channels)
        bias = None
        if use_bias:
            assert not lay.params["bias"].numpy().any()
            bias = np.random.default_rng(1).uniform(-0.5, 0.5, channels).astype(np.float32)
            lay.params["bias"].copy_from_host(bias)
        y = lay([xd, a]).numpy()
        ws = [lay.params[k].numpy().astype(np.float64).T for k in names]
        r_y = CH.conv_fwd(S, x, ws, bias, K, 3.0, fp32=True)
        assert rel_err(y, r_y) < TIGHT
        dx = lay.backward(ctx.to_device(dy), need_dx=True)
        r_dx, r_dws, r_db = CH.conv_bwd(S, x, ws, dy, K, 3.0, fp32=True)
        errs = [rel_err(dx.numpy(), r_dx)] + [rel_err(lay.grads[k].numpy(), r_dws[j].T) for j, k in enumerate(names)]
        if use_bias:
            errs.append(rel_err(lay.grads["bias"].numpy(), r_db))
        print(f"ChebConv channels={channels} K={K} bias={use_bias}: rel_err y {rel_err(y, r_y):.2e} dx {errs[0]:.2e} dW {max(errs[1:K + 1]):.2e}")
        assert max(errs) < TIGHT
        _worst("layer err / TIGHT", max(errs + [rel_err(y, r_y)]) / TIGHT)
        gw = lay.weight_grad.numpy().copy()
        assert lay.backward(ctx.to_device(dy), need_dx=False) is None and same(lay.weight_grad.numpy(), gw)
        if channels == 16:                   # the layer on the streamed route: the same bits
            lay2 = ChebConv(channels, K=K, lambda_max=3.0, use_bias=use_bias, seed=3, col_block=-1)
            lay2([xd, a])
            if use_bias:
                lay2.params["bias"].copy_from_host(bias)
            assert same(lay2([xd, a]).numpy(), y)


# ---- 6. gcnx.Cheb: a whole step against the kink-separated restatement ---------------------------------------------------------------
HEAD_UNDER_BN = {"linear_1.bias": "linear_1.weight", "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _under_bn(norm):
    """Gradients that are analytically zero are compared on the scale of the weight gradient named for them (as
    test_gpu_gcn_bn.UNDER_BN does): BatchNorm cancels a bias added to every row right ahead of it -- the head's, and with
    norm="batch" the convolutions' (GraphNorm with a learned mean_scale does not cancel them: they are compared on their own)."""
    conv = {"conv1.bias": "conv1.lins.0.weight", "conv2.bias": "conv2.lins.0.weight"} if norm == "batch" else {}
    return dict(HEAD_UNDER_BN, **conv)


def _cmp_grads(got, ref, tol, what, under_bn):
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[under_bn.get(k, k)], np.float64))))
        err = float(np.max(np.abs(g - r)))
        assert err <= tol * scale, (what, k, err, scale)
        _worst("step gradient err / tol", err / (tol * scale) if scale > 0 else 0.0)


# name -> (hidden, K, lambda_max, GCNX_CHEB_RESIDENT, inputs, readout, norm)
STEP_CASES = {
    "64-K3": (64, 3, 2.0, "1", "device", "max", "batch"),
    "64-K3-streamed-host": (64, 3, 2.0, "0", "host", "max", "batch"),
    "16-K5": (16, 5, 2.0, "1", "device", "max", "batch"),
    "attention": (64, 3, 2.0, "1", "device", "attention", "batch"),
    "graph-norm": (64, 3, 2.0, "1", "device", "max", "graph"),
    "lambda-3": (64, 3, 3.0, "1", "device", "max", "batch"),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_cheb_step_against_restatement(ctx, monkeypatch, case):
    import gcnx
    from gcnx import device as D
    h, K, lam, resident, route, readout, norm = STEP_CASES[case]
    hb = _tiny_host(16, 16, seed=4)
    a = _scipy_adj(hb)
    monkeypatch.setenv("GCNX_CHEB_RESIDENT", resident)
    m = gcnx.Cheb(ctx, hidden_channels=h, K=K, lambda_max=lam, seed=0, readout=readout, norm=norm)
    assert m._col_block == (0 if resident == "1" else -1)
    p0 = {k: v.astype(np.float32) for k, v in CH.init_params(16, h, K, seed=7, readout=readout, norm=norm).items()}
    m.load_state_dict(p0)
    assert list(m.state_dict()) == list(CH.keys(K, readout, norm))
    inputs = _device_batch(ctx, hb) if route == "device" else (hb.x, a, hb.ids())
    target = None if route == "device" else hb.y
    for step in range(2):
        p = m.state_dict()
        pos = {}
        if norm == "graph":                                  # the PReLU sides: the signs of y1 / y2 of a forward of its own
            m(inputs)
            pos = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
        m.loss_and_grads(inputs, target)
        batch, b = m._last_batch, m._bufs
        assert batch.a.max_block_rows == int(np.diff(hb.graph_ptr).max()) and D.cheb_resident_ok(ctx, batch.a.max_block_rows, h, K * h)
        if norm == "batch":
            pos = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), p[f"batch_norm_{i}.weight"],
                                                 p[f"batch_norm_{i}.bias"]) for i in (1, 2)}
        arg = b["arg"].numpy().astype(np.int64) if readout == "max" else None
        r = CH.model(hb.x, a, hb.graph_ptr, p, K, lam, hb.y, masks=pos, argmax=arg, readout=readout, norm=norm, fp32=True)
        what = f"{case} step {step}"
        assert_close(b["z1"].numpy(), r["z1"], STEP, f"{what} z1")
        assert_close(b["out"].numpy(), r["out"], STEP, f"{what} logits")
        la = m.loss_acc.numpy()
        assert rel_err(la[0], r["loss"]) < STEP and la[1] == r["hits"], (what, la, r["loss"], r["hits"])
        got = m.gradients()
        assert list(got) == list(CH.keys(K, readout, norm))
        _cmp_grads(got, r["grads"], STEP, what, _under_bn(norm))
        m._apply_sgd(0.05)
    print("worst:", WORST)


def test_both_routes_give_the_model_the_same_bits(ctx, monkeypatch):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    p0 = {k: v.astype(np.float32) for k, v in CH.init_params(16, 64, 3, seed=7).items()}
    grads = []
    for resident in ("1", "0"):
        monkeypatch.setenv("GCNX_CHEB_RESIDENT", resident)
        m = gcnx.Cheb(ctx, hidden_channels=64, K=3, seed=0)
        m.load_state_dict(p0)
        m.loss_and_grads(_device_batch(ctx, hb))
        grads.append(m.flat_g.numpy())
    assert np.array_equal(bits(grads[0]), bits(grads[1]))


def test_cheb_state_dict_round_trip_single_graph_and_forward(ctx):
    import gcnx
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.Cheb(ctx, seed=1)
    ids, a = hb.ids(), _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1) and np.all(np.isfinite(logits))
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    sd = m.state_dict()
    assert list(sd) == list(CH.keys(3)) and sd["conv1.lins.2.weight"].shape == (64, 16) and sd["conv2.bias"].shape == (64,)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    m2 = gcnx.Cheb(ctx, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(bits(v), bits(sd[k])), k
    assert np.array_equal(bits(m2((hb.x, a, ids))), bits(logits))
    r = CH.model(hb.x, a, hb.graph_ptr, sd, 3, 2.0, masks={
        f"m{i}": R.device_prelu_sides(m._bufs[f"z{i}"].numpy(), m._bufs[f"m{i}"].numpy(), m._bufs[f"i{i}"].numpy(),
                                      sd[f"batch_norm_{i}.weight"], sd[f"batch_norm_{i}.bias"]) for i in (1, 2)},
        argmax=m._bufs["arg"].numpy().astype(np.int64), fp32=True)
    assert_close(logits, r["out"], STEP, "forward logits")
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


def test_fit_runs_the_cheb_model(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:12]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[12:]])
    m = gcnx.Cheb(ctx, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=4, epochs=1, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=4, shuffle=False), epochs=1, verbose=False)           # three steps
    assert len(out["history"]) == 1 and all(np.all(np.isfinite(h)) for h in out["history"])


def test_cheb_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in CH.init_params(16, 64, 3, seed=7).items()}

    def step(ctx, part, comm, gb):
        m = gcnx.Cheb(ctx, hidden_channels=64, K=3, seed=0, comm=comm)
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

"""GPU tests of GINConv: the one-launch kernel gcnx_gin_conv (csrc/gin.hip) in both directions and both forms,
gcnx_gin_aggregate, gcnx_gin_eps_grad, the layer gcnx.GINConv and the model gcnx.GIN on both of its routes (GCNX_GIN_FUSED)
with and without train_eps -- each against the float64 oracle tests/gin_ref.py, the model on the device's side of every kink.
Tolerances: TIGHT = 2e-5 for a single fp32 kernel, 1e-4 for a whole step and for the weights after five SGD steps."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import gin_ref as GR
from gpu_frames import SENTINEL, Frame
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host
from test_gpu_sage import _edge_case_csr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5

# gradients that are analytically zero (see test_gpu_gcn_bn.UNDER_BN): compared relative to the weight gradient named here
UNDER_BN = {"conv1.nn.2.bias": "conv1.nn.2.weight", "conv2.nn.2.bias": "conv2.nn.2.weight", "linear_1.bias": "linear_1.weight",
            "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _cmp_grads(got, ref, tol, what, keys=None):
    for k in keys or got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        if k in UNDER_BN:
            scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN[k]], np.float64))))
            assert float(np.max(np.abs(g - r))) <= tol * scale, (what, k, float(np.max(np.abs(g - r))), scale)
        else:
            assert_close(g, r, tol, f"{what} {k}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ecoli3(f):
    """synth.ecoli_batch(3, f) and its float64 all-ones operator (computed once, never modified)."""
    from gcnx import synth
    hb = synth.ecoli_batch(3, f)
    assert hb.n % 32 != 0 and hb.n > 32
    return hb, GR.sum_operator(_scipy_adj(hb), hb.n)


def _csr(ctx, hb):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)


def _weights(rng, k0, k1, k2, wt):
    """(w_a, b_a, w_b, b_b) as the call takes them (wt: [out, in]; k2 = 0: no second stage) and the two weights as float64
    [in, out] matrices."""
    mk = lambda fi, fo: (rng.standard_normal((fo, fi) if wt else (fi, fo)) / np.sqrt(fi)).astype(np.float32)
    m = lambda w: (w.T if wt else w).astype(np.float64)
    w_a, b_a = mk(k0, k1), rng.standard_normal(k1).astype(np.float32)
    if not k2:
        return w_a, b_a, None, None, m(w_a), None
    w_b, b_b = mk(k1, k2), rng.standard_normal(k2).astype(np.float32)
    return w_a, b_a, w_b, b_b, m(w_a), m(w_b)


def _ref(A, x, eps, m_a, b_a, m_b, b_b):
    """(out, T, U) in float64 from the float32 inputs (eps: a float32 value or None)."""
    x = x.astype(np.float64)
    t = (1.0 + (float(eps) if eps is not None else 0.0)) * x + A @ x
    v = t @ m_a + (b_a.astype(np.float64) if b_a is not None else 0.0)
    if m_b is None:
        return v, t, None
    u = np.maximum(v, 0.0)
    return u @ m_b + (b_b.astype(np.float64) if b_b is not None else 0.0), t, u


def _dev(ctx, a):
    return ctx.to_device(a) if a is not None else None


def _run(ctx, a, x, eps, w_a, b_a, w_b, b_b, wt, keep=True):
    from gcnx import device as D
    n, k0 = x.shape
    k1 = w_a.shape[0] if wt else w_a.shape[1]
    k2 = 0 if w_b is None else (w_b.shape[0] if wt else w_b.shape[1])
    out = ctx.empty((n, k2 or k1))
    t = ctx.empty((n, k0)) if keep else None
    u = ctx.empty((n, k1)) if keep and k2 else None
    D.gin_conv(ctx, a, ctx.to_device(x), _dev(ctx, None if eps is None else np.full(1, eps, np.float32)), ctx.to_device(w_a), _dev(ctx, b_a),
               _dev(ctx, w_b), _dev(ctx, b_b), out, t=t, u=u, w_transposed=wt)
    return out.numpy(), (t.numpy() if t is not None else None), (u.numpy() if u is not None else None)


# ---- 1. the kernel, both directions, both forms ----------------------------------------------------------------------------
TWO_STAGE = [(16, 64, 64), (64, 64, 64), (32, 48, 16), (128, 128, 128), (128, 16, 112), (16, 128, 32)]
ONE_STAGE = [(64, 16, 0), (64, 64, 0), (128, 128, 0), (32, 48, 0)]


@pytest.mark.parametrize("eps", [None, -0.3])
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("k0,k1,k2", TWO_STAGE + ONE_STAGE)
def test_gin_conv_against_float64(ctx, k0, k1, k2, wt, eps):
    from gcnx import device as D
    hb, A = _ecoli3(k0)
    a = _csr(ctx, hb).unweighted()
    op = a.transpose() if wt else a
    assert op.vals is None
    Aref = A.T.tocsr() if wt else A
    assert D.gin_conv_ok(ctx, hb.n, k0, k1, k2)
    rng = np.random.default_rng(10000 * k0 + 100 * k1 + k2 + wt)
    w_a, b_a, w_b, b_b, m_a, m_b = _weights(rng, k0, k1, k2, wt)
    e32 = None if eps is None else np.float32(eps)
    out, t, u = _run(ctx, op, hb.x, e32, w_a, b_a, w_b, b_b, wt)
    r_out, r_t, r_u = _ref(Aref, hb.x, e32, m_a, b_a, m_b, b_b)
    e_out, e_t = rel_err(out, r_out), rel_err(t, r_t)
    e_u = rel_err(u, r_u) if k2 else 0.0
    print(f"gin_conv k=({k0},{k1},{k2}) wt={wt} eps={eps}: rel_err out {e_out:.2e} t {e_t:.2e} u {e_u:.2e}")
    assert e_out < TIGHT and e_t < TIGHT and e_u < TIGHT
    assert (u is None) == (k2 == 0) and (k2 == 0 or (u >= 0).all())
    # no atomics: a second call leaves the same bits
    out2, t2, u2 = _run(ctx, op, hb.x, e32, w_a, b_a, w_b, b_b, wt)
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(t2), _bits(t))
    assert k2 == 0 or np.array_equal(_bits(u2), _bits(u))
    # t = u = NULL gives the same out; without the last bias the same out minus that bias
    out3, _, _ = _run(ctx, op, hb.x, e32, w_a, b_a, w_b, b_b, wt, keep=False)
    assert np.array_equal(_bits(out3), _bits(out))
    if k2:
        out4, _, _ = _run(ctx, op, hb.x, e32, w_a, b_a, w_b, None, wt, keep=False)
        assert np.array_equal(_bits(out4 + b_b), _bits(out))
        out5, _, u5 = _run(ctx, op, hb.x, e32, w_a, None, w_b, b_b, wt)             # no first bias: U = relu(T w_a)
        r_out5, _, r_u5 = _ref(Aref, hb.x, e32, m_a, None, m_b, b_b)
        assert rel_err(out5, r_out5) < TIGHT and rel_err(u5, r_u5) < TIGHT
    else:
        out4, _, _ = _run(ctx, op, hb.x, e32, w_a, None, None, None, wt, keep=False)
        assert np.array_equal(_bits(out4 + b_a), _bits(out))
    # T is gcnx_gin_aggregate's, bit for bit (the same additions in the same order)
    t6 = ctx.empty((hb.n, k0))
    D.gin_aggregate(ctx, op, ctx.to_device(hb.x), _dev(ctx, None if eps is None else np.full(1, eps, np.float32)), t6)
    assert np.array_equal(_bits(t6.numpy()), _bits(t))


# ---- 2. degenerate inputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wt", [0, 1])
def test_gin_conv_degenerate_inputs(ctx, wt):
    import scipy.sparse as sp
    from gcnx.device import DeviceCSR
    rowptr, colidx, vals, gp = _edge_case_csr()
    n, k0, k1, k2 = 56, 32, 48, 16
    rng = np.random.default_rng(7 + wt)
    x = rng.standard_normal((n, k0), dtype=np.float32)
    w_a, b_a, w_b, b_b, m_a, m_b = _weights(rng, k0, k1, k2, wt)
    A = sp.csr_matrix((np.ones(len(colidx)), colidx, rowptr), shape=(n, n))
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)      # the values are there and are not read
    for eps in (None, np.float32(-0.3)):
        out, t, u = _run(ctx, a, x, eps, w_a, b_a, w_b, b_b, wt)
        r_out, r_t, r_u = _ref(A, x, eps, m_a, b_a, m_b, b_b)
        assert rel_err(out, r_out) < TIGHT and rel_err(t, r_t) < TIGHT and rel_err(u, r_u) < TIGHT
        scale = np.float32(1.0) + (eps if eps is not None else np.float32(0.0))
        assert np.array_equal(_bits(t[[4, 20]]), _bits(scale * x[[4, 20]]))          # rows without entries: T = (1 + eps) x exactly
        # the transposed pattern of the same matrix (row 4 of A^T is empty too: a single-node graph nobody lists)
        out_t, t_t, u_t = _run(ctx, a.transpose(), x, eps, w_a, b_a, w_b, b_b, wt)
        r_out_t, r_t_t, r_u_t = _ref(A.T.tocsr(), x, eps, m_a, b_a, m_b, b_b)
        assert rel_err(out_t, r_out_t) < TIGHT and rel_err(t_t, r_t_t) < TIGHT and rel_err(u_t, r_u_t) < TIGHT
        assert np.array_equal(_bits(t_t[4]), _bits(scale * x[4])) and not np.array_equal(t_t[20], scale * x[20])
    r_out, r_t, r_u = _ref(A, x, None, m_a, b_a, m_b, b_b)
    # the single-stage form on the same rows
    out_s, t_s, _ = _run(ctx, a, x, None, w_a, b_a, None, None, wt)
    assert rel_err(out_s, r_t @ m_a + b_a) < TIGHT and np.array_equal(_bits(t_s[[4, 20]]), _bits(x[[4, 20]]))
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:rowptr[5]], vals[:rowptr[5]], gp[:4].copy(), symmetric=False)
    out5, t5, u5 = _run(ctx, a5, x[:5], None, w_a, b_a, w_b, None, wt)
    assert rel_err(out5, r_out[:5] - b_b) < TIGHT and rel_err(t5, r_t[:5]) < TIGHT and rel_err(u5, r_u[:5]) < TIGHT
    # one row: with its self-loop (one more neighbour), and without any entry
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), np.array([0.75], np.float32), one, symmetric=True)
    out1, t1, _ = _run(ctx, a1, x[:1], None, w_a, b_a, w_b, b_b, wt)
    assert np.array_equal(t1, np.float32(2.0) * x[:1])
    assert rel_err(out1, np.maximum((2.0 * x[:1].astype(np.float64)) @ m_a + b_a, 0) @ m_b + b_b) < TIGHT
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), one, symmetric=True)   # (the entry is in no row)
    out0, t0, _ = _run(ctx, a0, x[:1], None, w_a, b_a, w_b, b_b, wt)
    assert np.array_equal(_bits(t0), _bits(x[:1])) and rel_err(out0, np.maximum(x[:1].astype(np.float64) @ m_a + b_a, 0) @ m_b + b_b) < TIGHT


# ---- 3. rows longer than the staged entries ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hub():
    from gcnx import synth
    hb = synth.power_law_batch(n_graphs=1, graph_size=8192, f=64, seed=3)
    assert int(np.diff(hb.rowptr).max()) >= 4096                         # past the 1024 staged entries of a tile
    return hb, GR.sum_operator(_scipy_adj(hb), hb.n)


@pytest.mark.parametrize("wt", [0, 1])
def test_gin_conv_long_rows(ctx, wt):
    hb, A = _hub()
    a = _csr(ctx, hb).unweighted()
    op = a.transpose() if wt else a
    k0, k1, k2 = 64, 32, 48
    rng = np.random.default_rng(11 + wt)
    w_a, b_a, w_b, b_b, m_a, m_b = _weights(rng, k0, k1, k2, wt)
    eps = np.float32(-0.3)
    out, t, u = _run(ctx, op, hb.x, eps, w_a, b_a, w_b, b_b, wt)
    r_out, r_t, r_u = _ref(A.T.tocsr() if wt else A, hb.x, eps, m_a, b_a, m_b, b_b)     # float64 sums of the float32 inputs
    e_out, e_t, e_u = rel_err(out, r_out), rel_err(t, r_t), rel_err(u, r_u)
    print(f"gin_conv hub wt={wt}: rel_err out {e_out:.2e} t {e_t:.2e} u {e_u:.2e}")
    assert e_out < TIGHT and e_t < TIGHT and e_u < TIGHT
    out_s, t_s, _ = _run(ctx, op, hb.x, eps, w_a, b_a, None, None, wt)
    assert rel_err(out_s, r_t @ m_a + b_a) < TIGHT and np.array_equal(_bits(t_s), _bits(t))


# ---- 4. strided operands ------------------------------------------------------------------------------------------------
def _frame_check(fr, want, tol, what):
    got = fr.buf.numpy()
    body = fr._body(got)
    assert rel_err(body[:, :fr.f], want) < tol, (what, rel_err(body[:, :fr.f], want))
    assert (body[:, fr.f:] == SENTINEL).all() and (got[:fr.lead] == SENTINEL).all() \
        and (got[fr.lead + fr.n * fr.ld:] == SENTINEL).all(), (what, "written outside the view")


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("k2", [16, 0])
def test_gin_conv_strided_operands(ctx, wt, k2):
    from gcnx import device as D
    k0, k1 = 32, 48
    hb, A = _ecoli3(k0)
    a = _csr(ctx, hb).unweighted()
    op = a.transpose() if wt else a
    rng = np.random.default_rng(21 + wt)
    w_a, b_a, w_b, b_b, m_a, m_b = _weights(rng, k0, k1, k2, wt)
    ko = k2 or k1
    fx = Frame(ctx, hb.n, k0, 2 * k0, 4, data=hb.x)                     # x: a column slice of an array twice as wide
    fo_, ft, fu = Frame(ctx, hb.n, ko, ko + 8, 8), Frame(ctx, hb.n, k0, k0 + 4, 12), Frame(ctx, hb.n, k1, k1 + 12, 4)
    assert fx.aligned() and fo_.aligned() and ft.aligned() and fu.aligned()
    assert D.gin_conv_ok(ctx, hb.n, k0, k1, k2, fx.view.ld)
    eps = np.float32(-0.3)
    D.gin_conv(ctx, op, fx.view, ctx.to_device(np.full(1, eps, np.float32)), ctx.to_device(w_a), ctx.to_device(b_a), _dev(ctx, w_b),
               _dev(ctx, b_b), fo_.view, t=ft.view, u=fu.view if k2 else None, w_transposed=wt)
    r_out, r_t, r_u = _ref(A.T.tocsr() if wt else A, hb.x, eps, m_a, b_a, m_b, b_b)
    _frame_check(fo_, r_out, TIGHT, "out")
    _frame_check(ft, r_t, TIGHT, "t")
    if k2:
        _frame_check(fu, r_u, TIGHT, "u")
    else:
        fu.untouched("u is not an operand of the single-stage form")
    fx.untouched("x is not written")


# ---- 5. gcnx_gin_aggregate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 3, 16, 20, 130])
def test_gin_aggregate_any_width(ctx, f):
    import scipy.sparse as sp
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    hb, A = _ecoli3(16)
    a = _csr(ctx, hb).unweighted()
    rng = np.random.default_rng(40 + f)
    x = rng.standard_normal((hb.n, f), dtype=np.float32)
    e32 = np.float32(0.45)
    for eps in (None, e32):
        want = (1.0 + (float(eps) if eps is not None else 0.0)) * x.astype(np.float64) + A @ x.astype(np.float64)
        dev_eps = _dev(ctx, None if eps is None else np.full(1, eps, np.float32))
        # contiguous; padded leading dimensions a multiple of 4 (float4 lanes where f allows); odd ones and an odd start (scalar)
        for ldx, ldo, lead in ((f, f, 0), (f + (-f) % 4 + 4, f + (-f) % 4 + 8, 4), (f + 3, f + 5, 1)):
            fx, fo_ = Frame(ctx, hb.n, f, ldx, lead, data=x), Frame(ctx, hb.n, f, ldo, lead)
            D.gin_aggregate(ctx, a, fx.view, dev_eps, fo_.view)
            got = fo_.numpy()                                                           # (asserts nothing outside the view is written)
            assert rel_err(got, want) < TIGHT, (f, ldx, ldo, lead, rel_err(got, want))
            fx.untouched("x")
            fo2 = Frame(ctx, hb.n, f, ldo, lead)
            D.gin_aggregate(ctx, a, fx.view, dev_eps, fo2.view)
            assert np.array_equal(_bits(fo2.numpy()), _bits(got))                       # bits repeat
    # the degenerate CSR and its transpose: every row is written, rows without entries hold (1 + eps) x exactly
    rowptr, colidx, vals, gp = _edge_case_csr()
    ad = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    Ad = sp.csr_matrix((np.ones(len(colidx)), colidx, rowptr), shape=(56, 56))
    xd = rng.standard_normal((56, f), dtype=np.float32)
    for op, Aop, empty in ((ad, Ad, [4, 20]), (ad.transpose(), Ad.T.tocsr(), [4])):
        fo_ = Frame(ctx, 56, f, f, 0)
        D.gin_aggregate(ctx, op, ctx.to_device(xd), ctx.to_device(np.full(1, e32, np.float32)), fo_.view)
        got = fo_.numpy()
        assert rel_err(got, (1.0 + float(e32)) * xd.astype(np.float64) + Aop @ xd.astype(np.float64)) < TIGHT
        assert np.array_equal(_bits(got[empty]), _bits((np.float32(1.0) + e32) * xd[empty]))


# ---- 6. gcnx_gin_eps_grad ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [3, 16, 128])
@pytest.mark.parametrize("n", [1, 33, "ecoli"])
def test_gin_eps_grad_against_float64(ctx, n, f):
    from gcnx import device as D
    n = _ecoli3(16)[0].n if n == "ecoli" else n
    rng = np.random.default_rng(1000 * f + n)
    x = rng.standard_normal((n, f), dtype=np.float32)
    dt = (0.5 * x + rng.standard_normal((n, f), dtype=np.float32)).astype(np.float32)     # correlated: the sum does not cancel
    want = float(np.sum(x.astype(np.float64) * dt.astype(np.float64)))
    fx, fd = Frame(ctx, n, f, f + 3, 1, data=x), Frame(ctx, n, f, f + 8, 4, data=dt)       # any leading dimensions
    parts, deps = ctx.zeros(D.gin_eps_grad_parts(n)), Frame(ctx, 1, 1, 1, 3, data=np.full(1, 77.0, np.float32))
    D.gin_eps_grad(ctx, fx.view, fd.view, parts, deps.row(0))
    got = deps.numpy()[0, 0]
    err = abs(float(got) - want) / abs(want)
    print(f"gin_eps_grad n={n} f={f}: got {got:.8e} want {want:.8e} rel {err:.2e}")
    assert err <= TIGHT                                                  # written, not accumulated onto the 77
    D.gin_eps_grad(ctx, fx.view, fd.view, parts, deps.row(0))
    assert deps.numpy()[0, 0].view(np.uint32) == got.view(np.uint32)     # bits repeat
    fx.untouched("x"); fd.untouched("dt")
    # n = 0 writes 0
    rc = ctx.lib.gcnx_gin_eps_grad(ctx.h, None, f, None, f, 0, f, None, deps.row(0).ptr)
    assert rc == 0 and deps.numpy()[0, 0] == 0.0 and not np.signbit(deps.numpy()[0, 0])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_gin_conv_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb, _ = _ecoli3(16)
    a = _csr(ctx, hb).unweighted()
    n = hb.n

    def refused(x, k0, k1, k2, code=_lib.ERR_UNSUPPORTED, u_single=False):
        w_a, w_b = ctx.zeros((k0, k1)), (ctx.zeros((k1, k2)) if k2 else None)
        out, t, u = Frame(ctx, n, k2 or k1, k2 or k1, 0), Frame(ctx, n, k0, k0, 0), Frame(ctx, n, k1, k1, 0)
        with pytest.raises(_lib.GcnxError) as e:
            D.gin_conv(ctx, a, x, None, w_a, None, w_b, None, out.view, t=t.view, u=u.view if (k2 or u_single) else None)
        assert e.value.code == code, (k0, k1, k2, e.value.code)
        out.untouched("out"); t.untouched("t"); u.untouched("u")

    assert not D.gin_conv_ok(ctx, n, 96, 64, 64) and not D.gin_conv_ok(ctx, n, 16, 256, 64) and not D.gin_conv_ok(ctx, n, 16, 64, 24)
    assert not D.gin_conv_ok(ctx, n, 16, 64, 64, 18)
    refused(ctx.zeros((n, 96)), 96, 64, 64)
    refused(ctx.zeros((n, 16)), 16, 256, 64)
    refused(ctx.zeros((n, 16)), 16, 64, 24)
    wide = ctx.zeros((n, 18))
    refused(DeviceArray(ctx, wide.ptr, (n, 16), np.float32, ld=18, base=wide), 16, 64, 64)       # ldx % 4 != 0
    off = Frame(ctx, n, 16, 16, 1, data=hb.x)                                                    # x one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4
    refused(off.view, 16, 64, 64)
    refused(off.view, 16, 64, 0)
    refused(ctx.zeros((n, 16)), 16, 64, 0, code=1, u_single=True)                  # u in the single-stage form
    # outputs off a 16-byte boundary or with a leading dimension that is no multiple of 4 floats
    x, w_a, w_b = ctx.to_device(hb.x), ctx.zeros((16, 64)), ctx.zeros((64, 64))
    for which in ("out", "t", "u"):
        fr = {k: Frame(ctx, n, f, f + (2 if k == which else 0), 0) for k, f in (("out", 64), ("t", 16), ("u", 64))}
        with pytest.raises(_lib.GcnxError) as e:
            D.gin_conv(ctx, a, x, None, w_a, None, w_b, None, fr["out"].view, t=fr["t"].view, u=fr["u"].view)
        assert e.value.code == _lib.ERR_UNSUPPORTED, which
        for k in fr:
            fr[k].untouched(k)
    # n = 0: nothing to do, no error -- whatever the pointers
    x, out = ctx.zeros((4, 16)), Frame(ctx, 4, 64, 64, 0)
    call = lambda **kw: ctx.lib.gcnx_gin_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, kw.get("x", x.ptr), 16, kw.get("n", 4), 16, None,
                                              kw.get("w_a", w_a.ptr), None, 64, kw.get("w_b", w_b.ptr), None, kw.get("k2", 64), 0, None, 0,
                                              None, 0, out.view.ptr, 64)
    assert call(n=0) == _lib.OK
    out.untouched("n = 0 writes nothing")
    # negative sizes, NULL mandatory pointers, w_b and k2 that do not go together: invalid arguments
    for bad in (dict(n=-1), dict(w_a=None), dict(x=None), dict(w_b=None), dict(k2=0)):
        assert call(**bad) == 1, bad                                                              # GCNX_ERR_INVALID
    out.untouched("refused calls write nothing")
    # gcnx_gin_aggregate: out must not alias x
    xn = ctx.zeros((n, 16))
    with pytest.raises(_lib.GcnxError) as e:
        D.gin_aggregate(ctx, a, xn, None, xn)
    assert e.value.code == 1


# ---- 8. capture -----------------------------------------------------------------------------------------------------------
def test_gin_conv_captured_replay_reads_eps_on_the_device(ctx):
    from gcnx import device as D
    k0, k1, k2 = 64, 64, 64
    hb, _ = _ecoli3(k0)
    op = _csr(ctx, hb).unweighted()
    rng = np.random.default_rng(5)
    w_a, b_a, w_b, b_b, _, _ = _weights(rng, k0, k1, k2, 0)
    eager = {e: _run(ctx, op, hb.x, np.float32(e), w_a, b_a, w_b, b_b, 0) for e in (-0.3, 0.6)}
    assert not np.array_equal(eager[-0.3][0], eager[0.6][0])
    x, wa, ba, wb, bb = (ctx.to_device(v) for v in (hb.x, w_a, b_a, w_b, b_b))
    eps = ctx.to_device(np.full(1, -0.3, np.float32))
    out, t, u = ctx.zeros((hb.n, k2)), ctx.zeros((hb.n, k0)), ctx.zeros((hb.n, k1))
    parts, deps = ctx.zeros(D.gin_eps_grad_parts(hb.n)), ctx.zeros(1)

    def seq():
        D.gin_conv(ctx, op, x, eps, wa, ba, wb, bb, out, t=t, u=u)
        D.gin_eps_grad(ctx, x, t, parts, deps)                           # (any [n, k0] pair: here <x, T>)

    g = ctx.capture(seq)
    try:
        assert not out.numpy().any()                                     # captured, not yet executed
        for e in (-0.3, -0.3, 0.6):                                      # twice the same bits, then the replay follows the new value
            eps.copy_from_host(np.full(1, e, np.float32))
            out.fill_zero(); t.fill_zero(); u.fill_zero()
            g.launch()
            for got, want in zip((out, t, u), eager[e]):
                assert np.array_equal(_bits(got.numpy()), _bits(want)), e
            want = np.sum(hb.x.astype(np.float64) * eager[e][1].astype(np.float64))
            assert abs(float(deps.numpy()[0]) - float(want)) <= TIGHT * abs(float(want))
    finally:
        g.destroy()


# ---- 9. the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mlp_hidden", [32, 48])         # 48: the forward launch serves it, the dX gather (k0 = 48) does not
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("train_eps", [False, True])
def test_ginconv_layer_forward_and_backward(ctx, train_eps, fused, mlp_hidden):
    from gcnx import device as D
    from gcnx.layers import GINConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    A = GR.sum_operator(_scipy_adj(hb), hb.n)
    lay = GINConv(64, mlp_hidden=mlp_hidden, eps=-0.3, train_eps=train_eps, fused=fused, seed=3)
    x = ctx.to_device(hb.x)
    y = lay([x, GINConv.preprocess(a)])
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    assert list(p) == (["eps"] if train_eps else []) + ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    assert all(v.ptr % 16 == 0 for v in lay.params.values())
    assert lay._one_launch(x, mlp_hidden, 64, y) == fused and D.gin_conv_ok(ctx, hb.n, mlp_hidden, 16, 0) == (mlp_hidden == 32)
    eps = np.float32(-0.3)
    w_a, w_b = p["nn.0.weight"].T, p["nn.2.weight"].T
    r_y, r_t, r_u, _ = GR.gin_conv_fwd(A, hb.x, eps, w_a, p["nn.0.bias"], w_b, p["nn.2.bias"])
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    mask = lay._saved[3].numpy() > 0                                      # the device's side of the inner ReLU
    r_dx, r_deps, r_dwa, r_dba, r_dwb, r_dbb = GR.gin_conv_bwd(A, hb.x, eps, r_t, r_u, mask, w_a, w_b, dy)
    g = {k: v.numpy() for k, v in lay.grads.items()}
    assert rel_err(dx.numpy(), r_dx) < TIGHT
    assert rel_err(g["nn.0.weight"], r_dwa.T) < TIGHT and rel_err(g["nn.0.bias"], r_dba) < TIGHT
    assert rel_err(g["nn.2.weight"], r_dwb.T) < TIGHT and rel_err(g["nn.2.bias"], r_dbb) < TIGHT
    if train_eps:
        e_eps = abs(float(g["eps"][0]) - float(r_deps[0])) / abs(float(r_deps[0]))
        print(f"GINConv layer mlp_hidden={mlp_hidden} fused={fused}: d eps {g['eps'][0]:.8e} want {r_deps[0]:.8e} rel {e_eps:.2e}")
        assert e_eps < TIGHT
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    g2 = {k: v.numpy() for k, v in lay.grads.items()}
    assert all(np.array_equal(_bits(g2[k]), _bits(g[k])) for k in g)      # need_dx=False leaves the same gradients


@pytest.mark.parametrize("fused", [True, False])
def test_ginconv_layer_without_biases(ctx, fused):
    from gcnx.layers import GINConv
    hb = _tiny_host(16, 16)
    A = GR.sum_operator(_scipy_adj(hb), hb.n)
    lay = GINConv(32, use_bias=False, fused=fused, seed=5)
    y = lay([ctx.to_device(hb.x), GINConv.preprocess(_csr(ctx, hb))])
    assert list(lay.params) == ["nn.0.weight", "nn.2.weight"] and lay._eps() is None
    w_a, w_b = lay.params["nn.0.weight"].numpy().astype(np.float64).T, lay.params["nn.2.weight"].numpy().astype(np.float64).T
    r_y, r_t, r_u, _ = GR.gin_conv_fwd(A, hb.x, 0.0, w_a, None, w_b, None)
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(10).standard_normal((hb.n, 32)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy))
    r_dx, _, r_dwa, _, r_dwb, _ = GR.gin_conv_bwd(A, hb.x, 0.0, r_t, r_u, lay._saved[3].numpy() > 0, w_a, w_b, dy)
    assert rel_err(dx.numpy(), r_dx) < TIGHT
    assert rel_err(lay.grads["nn.0.weight"].numpy(), r_dwa.T) < TIGHT and rel_err(lay.grads["nn.2.weight"].numpy(), r_dwb.T) < TIGHT


# ---- 10. gcnx.GIN: a full step on either route against the kink-separated oracle ----------------------------------------------
def _sides(m, pre=None, relu=True):
    """The device's side of every kink of the last call.  relu=False after a forward-only call: the one launch keeps U only for
    a step that goes on to the gradients, and the logits, continuous in the ReLU input, do not depend on the side taken."""
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    s = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
         for i in (1, 2)}
    if relu:
        s.update(relu1=b["u1"].numpy() > 0, relu2=b["u2"].numpy() > 0)
    return s


def _keys(m):
    return [k for k, _, _ in m.TORCH_KEYS]


def _check_step(m, batch, hb, p, tol, what):
    m.loss_and_grads(batch)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = GR.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, hb.y, masks=_sides(m), argmax=arg)
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol and la[1] == r["hits"], (la, r["loss"], r["hits"])
    got = m.gradients()
    assert list(got) == _keys(m) and (("conv1.eps" in got) == ("conv2.eps" in got) == m.train_eps)
    _cmp_grads(got, r["grads"], tol, what)
    return r


@pytest.mark.parametrize("shape", ["config1", "config2"])
@pytest.mark.parametrize("train_eps", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_gin_step_against_oracle(ctx, monkeypatch, fused, train_eps, shape):
    import gcnx
    from gcnx import synth
    hb = _tiny_host(16, 16, seed=4) if shape == "config1" else synth.ecoli_batch(f=16)
    batch = _device_batch(ctx, hb)
    monkeypatch.setenv("GCNX_GIN_FUSED", fused)
    m = gcnx.GIN(ctx, hidden_channels=64, train_eps=train_eps, seed=0)
    assert m._fused == (fused == "1")
    p = {k: v.astype(np.float32) for k, v in GR.init_params(16, 64, seed=7, eps=(-0.3, 0.2)).items()}
    m.load_state_dict(p)
    what = f"{shape} fused={fused} train_eps={train_eps}"
    _check_step(m, batch, hb, p, 1e-4, what)
    # five SGD steps, each oracle step on the device's kink sides of that step (taken with the step's own weights)
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    a = _scipy_adj(hb)
    for _ in range(5):
        pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
        m.train_step(batch, lr=0.02)
        arg = m._bufs["arg"].numpy().astype(np.int64)
        r = GR.model(hb.x, a, hb.graph_ptr, ph, hb.y, masks=_sides(m, pre), argmax=arg)
        grads = {k: (r["grads"][k] if train_eps or k not in GR.EPS_KEYS else 0.0 * r["grads"][k]) for k in ph}   # a fixed eps stays
        ph = GR.sgd(ph, grads, 0.02)
    sd = m.state_dict()
    assert list(sd) == list(GR.KEYS)
    for k in GR.KEYS:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after 5 steps {k}")
    if train_eps:
        assert sd["conv1.eps"][0] != np.float32(-0.3) and sd["conv2.eps"][0] != np.float32(0.2)
    else:
        assert sd["conv1.eps"][0] == np.float32(-0.3) and sd["conv2.eps"][0] == np.float32(0.2)


# ---- 11. torch-style surface ---------------------------------------------------------------------------------------------
def _logits_match_oracle(m, x, a, gp, what):
    r = GR.model(x, a, gp, m.state_dict(), masks=_sides(m, relu=False), argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, what)


def test_gin_forward_state_dict_and_single_graph(ctx):
    import gcnx
    import scipy.sparse as sp
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.GIN(ctx, seed=1)
    ids, a = hb.ids(), _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1)
    _logits_match_oracle(m, hb.x, a, hb.graph_ptr, "stored loops")
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    sd = m.state_dict()
    assert list(sd) == list(GR.KEYS)                                     # eps is there although it is not trained
    assert sd["conv1.eps"].shape == (1,) and sd["conv1.eps"][0] == 0 and sd["conv2.eps"][0] == 0
    assert sd["conv1.nn.0.weight"].shape == (64, 16) and sd["conv1.nn.2.weight"].shape == (64, 64) and sd["conv1.nn.0.bias"].shape == (64,)
    assert sd["conv2.nn.0.weight"].shape == (64, 64) and sd["linear_2.weight"].shape == (1, 64)
    assert np.max(np.abs(sd["conv1.nn.0.weight"])) <= 0.25 and np.max(np.abs(sd["conv2.nn.2.weight"])) <= 0.125   # U(+-1/sqrt(fan_in))
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    assert [w.shape for w in m.get_weights()] == [sd[k].shape for k in GR.KEYS if k not in GR.EPS_KEYS]
    sd["conv1.eps"] = np.array([0.4], np.float32)                         # a checkpoint's eps is honoured, trained or not
    for te in (False, True):
        m2 = gcnx.GIN(ctx, train_eps=te, seed=9)
        m2.load_state_dict(sd)
        for k, v in m2.state_dict().items():
            assert np.array_equal(_bits(v), _bits(sd[k])), k
        assert len(m2.get_weights()) == len(GR.KEYS) - (0 if te else 2)
        l2 = m2((hb.x, a, ids))
        assert not np.allclose(l2, logits, rtol=1e-3, atol=1e-3)
        _logits_match_oracle(m2, hb.x, a, hb.graph_ptr, f"loaded eps, train_eps={te}")
    with pytest.raises(KeyError):
        gcnx.GIN(ctx).load_state_dict({k: v for k, v in sd.items() if k != "conv2.eps"})
    # no loop is re-added: a graph stripped of its stored self-loops is another graph
    a_noloop = sp.csr_matrix(a - sp.diags(a.diagonal()))
    a_noloop.eliminate_zeros()
    stripped = m((hb.x, a_noloop, ids))
    assert not np.allclose(stripped, logits, rtol=1e-3, atol=1e-3)
    _logits_match_oracle(m, hb.x, a_noloop, hb.graph_ptr, "stripped loops")
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


@pytest.mark.parametrize("train_eps", [False, True])
def test_gin_hidden_256_takes_the_composed_route(ctx, train_eps):
    import gcnx
    from gcnx import device as D
    hb = _tiny_host(16, 16, seed=8)
    m = gcnx.GIN(ctx, hidden_channels=256, train_eps=train_eps, seed=0)
    assert m._fused and not D.gin_conv_ok(ctx, hb.n, 16, 256, 256) and not D.gin_conv_ok(ctx, hb.n, 256, 256, 0)
    p = {k: v.astype(np.float32) for k, v in GR.init_params(16, 256, seed=2, eps=(0.1, -0.2)).items()}
    m.load_state_dict(p)
    _check_step(m, _device_batch(ctx, hb), hb, p, 1e-4, f"hidden 256 train_eps={train_eps}")


# ---- 12. sync-BN over graph shards ----------------------------------------------------------------------------------------
def test_gin_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in GR.init_params(16, 64, seed=7, eps=(-0.3, 0.2)).items()}

    def step(ctx, part, comm, gb):
        m = gcnx.GIN(ctx, hidden_channels=64, train_eps=True, seed=0, comm=comm)
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
    assert np.array_equal(_bits(ranks[0]["w"]), _bits(ranks[1]["w"]))


# ---- 13. gcnx.fit and the optimizers ------------------------------------------------------------------------------------------
def test_fit_runs_the_gin_model(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:10]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[10:]])
    m = gcnx.GIN(ctx, train_eps=True, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])


@pytest.mark.parametrize("train_eps", [True, False])
def test_adam_step_moves_eps_only_when_it_is_trained(ctx, train_eps):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    m = gcnx.GIN(ctx, train_eps=train_eps, seed=0)
    m.build(hb.f)
    opt = gcnx.Adam()
    m.set_optimizer(opt)
    assert opt.flat("m").size == m.n_params
    before = m.state_dict()
    m.train_step(_device_batch(ctx, hb), lr=0.01)
    after = m.state_dict()
    assert not np.array_equal(after["conv1.nn.0.weight"], before["conv1.nn.0.weight"])
    for k in GR.EPS_KEYS:
        assert before[k][0] == 0 and (after[k][0] != 0) == train_eps, (k, after[k])
        assert not train_eps or abs(abs(after[k][0]) - 0.01) < 1e-3      # Adam's first step: lr * sign(gradient)

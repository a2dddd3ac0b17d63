"""GPU tests of SAGEConv: the one-launch kernel gcnx_sage_conv (csrc/sage.hip) in both directions, the layer gcnx.SAGEConv
and the model gcnx.SAGE on both of its routes (GCNX_SAGE_FUSED) -- each against the float64 oracle tests/sage_ref.py, the
model on the device's side of every kink.  Tolerances: TIGHT = 2e-5 for the single fp32 kernel, 1e-4 for a whole step."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import sage_ref as SR
from gpu_frames import SENTINEL, Frame
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5

# gradients that are analytically zero (see test_gpu_gcn_bn.UNDER_BN): compared relative to the weight gradient named here
UNDER_BN = {"conv1.lin_l.bias": "conv1.lin_l.weight", "conv2.lin_l.bias": "conv2.lin_l.weight", "linear_1.bias": "linear_1.weight",
            "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _cmp_grads(got, ref, tol, what, keys=None):
    for k in keys or ref:
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
    """synth.ecoli_batch(3, f) and its float64 row-mean operator (computed once, never modified)."""
    from gcnx import synth
    hb = synth.ecoli_batch(3, f)
    assert hb.n % 32 != 0 and hb.n > 32
    return hb, SR.mean_operator(_scipy_adj(hb), hb.n)


def _csr(ctx, hb):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)


def _weights(rng, fi, fo, wt):
    """(w_nb, w_root, bias) as the call takes them (wt: [fo, fi]) and as float64 [fi, fo] matrices."""
    shape = (fo, fi) if wt else (fi, fo)
    w_nb, w_root = (rng.standard_normal(shape) / np.sqrt(fi)).astype(np.float32), (rng.standard_normal(shape) / np.sqrt(fi)).astype(np.float32)
    bias = rng.standard_normal(fo).astype(np.float32)
    m = lambda w: (w.T if wt else w).astype(np.float64)
    return w_nb, w_root, bias, m(w_nb), m(w_root)


def _ref(A, x, m_nb, m_root, bias):
    s = A @ x.astype(np.float64)
    out = s @ m_nb + x.astype(np.float64) @ m_root
    return (out + bias.astype(np.float64) if bias is not None else out), s


def _run(ctx, a, x, w_nb, w_root, bias, fo, wt, with_s=True):
    from gcnx import device as D
    n, fi = x.shape
    out, s = ctx.empty((n, fo)), (ctx.empty((n, fi)) if with_s else None)
    D.sage_conv(ctx, a, ctx.to_device(x), ctx.to_device(w_nb), ctx.to_device(w_root), ctx.to_device(bias) if bias is not None else None,
                out, s=s, w_transposed=wt)
    return out.numpy(), (s.numpy() if with_s else None)


# ---- 1. the kernel, both directions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("fi,fo", [(16, 64), (64, 64), (32, 16), (128, 128), (128, 48)])
def test_sage_conv_against_float64(ctx, fi, fo, wt):
    from gcnx import device as D
    hb, A = _ecoli3(fi)
    a = _csr(ctx, hb)
    op = a.row_mean().transpose() if wt else a.row_mean()
    assert op.vals is not None and op is not a
    Aref = A.T.tocsr() if wt else A
    if wt:      # the transposed operator's values differ from the forward's although the pattern is symmetric
        assert not np.array_equal(op.vals.numpy(), a.row_mean().vals.numpy())
    assert D.sage_conv_ok(ctx, hb.n, fi, fo)
    rng = np.random.default_rng(100 * fi + fo + wt)
    w_nb, w_root, bias, m_nb, m_root = _weights(rng, fi, fo, wt)
    out, s = _run(ctx, op, hb.x, w_nb, w_root, bias, fo, wt)
    r_out, r_s = _ref(Aref, hb.x, m_nb, m_root, bias)
    e_out, e_s = rel_err(out, r_out), rel_err(s, r_s)
    print(f"sage_conv fi={fi} fo={fo} wt={wt}: rel_err out {e_out:.2e} s {e_s:.2e}")
    assert e_out < TIGHT and e_s < TIGHT
    # no atomics: a second call leaves the same bits
    out2, s2 = _run(ctx, op, hb.x, w_nb, w_root, bias, fo, wt)
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(s2), _bits(s))
    # s = None and bias = None give the same out (minus the bias)
    out3, _ = _run(ctx, op, hb.x, w_nb, w_root, bias, fo, wt, with_s=False)
    assert np.array_equal(_bits(out3), _bits(out))
    out4, _ = _run(ctx, op, hb.x, w_nb, w_root, None, fo, wt, with_s=False)
    assert np.array_equal(_bits(out4 + bias), _bits(out))
    # vals = NULL: the all-ones sum
    ones = _scipy_adj(hb)
    out5, s5 = _run(ctx, a.unweighted(), hb.x, w_nb, w_root, bias, fo, wt)
    r_out5, r_s5 = _ref(ones, hb.x, m_nb, m_root, bias)
    assert a.unweighted().vals is None and rel_err(out5, r_out5) < TIGHT and rel_err(s5, r_s5) < TIGHT


# ---- 2. degenerate inputs -------------------------------------------------------------------------------------------------
def _edge_case_csr():
    """The 56-row construction of test_gcn_conv_fused_edge_cases: graphs of [1, 3, 1, 7, 2, 1, 40, 1] rows, rows 4 and 20
    without entries, directed values."""
    rng = np.random.default_rng(3)
    sizes = np.array([1, 3, 1, 7, 2, 1, 40, 1], np.int64)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(gp[-1])
    rows, cols = [], []
    for g in range(len(sizes)):
        for i in range(gp[g], gp[g + 1]):
            if i in (4, 20):
                continue
            rows.append(i); cols.append(i)
            if sizes[g] > 2 and i + 1 < gp[g + 1]:
                rows += [i, i + 1]; cols += [i + 1, i]
    order = np.lexsort((cols, rows))
    rows, cols = np.asarray(rows)[order], np.asarray(cols)[order]
    keep = ~np.isin(rows, (4, 20))
    rows, cols = rows[keep], cols[keep]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    vals = (rng.random(len(cols)) + 0.5).astype(np.float32)
    assert rowptr[5] == rowptr[4] and rowptr[21] == rowptr[20] and n == 56
    return rowptr, cols.astype(np.int32), vals, gp


@pytest.mark.parametrize("wt", [0, 1])
def test_sage_conv_degenerate_inputs(ctx, wt):
    import scipy.sparse as sp
    from gcnx.device import DeviceCSR
    rowptr, colidx, vals, gp = _edge_case_csr()
    n, fi, fo = 56, 32, 48
    rng = np.random.default_rng(7 + wt)
    x = rng.standard_normal((n, fi), dtype=np.float32)
    w_nb, w_root, bias, m_nb, m_root = _weights(rng, fi, fo, wt)
    A = sp.csr_matrix((vals.astype(np.float64), colidx, rowptr), shape=(n, n))
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    out, s = _run(ctx, a, x, w_nb, w_root, bias, fo, wt)
    r_out, r_s = _ref(A, x, m_nb, m_root, bias)
    assert rel_err(out, r_out) < TIGHT and rel_err(s, r_s) < TIGHT
    assert not s[[4, 20]].any() and not np.signbit(s[[4, 20]]).any()          # rows without entries: exact zeros
    assert rel_err(out[[4, 20]], x[[4, 20]].astype(np.float64) @ m_root + bias) < TIGHT
    # the transposed operator of the same matrix (row 4 of A^T is empty too: a single-node graph nobody lists)
    out_t, s_t = _run(ctx, a.transpose(), x, w_nb, w_root, bias, fo, wt)
    r_out_t, r_s_t = _ref(A.T.tocsr(), x, m_nb, m_root, bias)
    assert rel_err(out_t, r_out_t) < TIGHT and rel_err(s_t, r_s_t) < TIGHT
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:rowptr[5]], vals[:rowptr[5]], gp[:4].copy(), symmetric=False)
    out5, s5 = _run(ctx, a5, x[:5], w_nb, w_root, None, fo, wt)
    assert rel_err(out5, r_out[:5] - bias) < TIGHT and rel_err(s5, r_s[:5]) < TIGHT
    # one row: with its self-loop, and without any entry
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), np.array([0.75], np.float32), one, symmetric=True)
    out1, s1 = _run(ctx, a1, x[:1], w_nb, w_root, bias, fo, wt)
    assert np.array_equal(s1, np.float32(0.75) * x[:1])
    assert rel_err(out1, (0.75 * x[:1].astype(np.float64)) @ m_nb + x[:1].astype(np.float64) @ m_root + bias) < TIGHT
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32), one, symmetric=True)   # (the entry is in no row)
    out0, s0 = _run(ctx, a0, x[:1], w_nb, w_root, bias, fo, wt)
    assert not s0.any() and rel_err(out0, x[:1].astype(np.float64) @ m_root + bias) < TIGHT


# ---- 3. rows longer than the staged entries ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hub():
    from gcnx import synth
    hb = synth.power_law_batch(n_graphs=1, graph_size=8192, f=64, seed=3)
    assert int(np.diff(hb.rowptr).max()) >= 4096                         # past the 1024 staged entries of a tile
    return hb, SR.mean_operator(_scipy_adj(hb), hb.n)


@pytest.mark.parametrize("wt", [0, 1])
def test_sage_conv_long_rows(ctx, wt):
    hb, A = _hub()
    a = _csr(ctx, hb)
    op = a.row_mean().transpose() if wt else a.row_mean()
    fi, fo = 64, 32
    rng = np.random.default_rng(11 + wt)
    w_nb, w_root, bias, m_nb, m_root = _weights(rng, fi, fo, wt)
    out, s = _run(ctx, op, hb.x, w_nb, w_root, bias, fo, wt)
    r_out, r_s = _ref(A.T.tocsr() if wt else A, hb.x, m_nb, m_root, bias)
    e_out, e_s = rel_err(out, r_out), rel_err(s, r_s)
    print(f"sage_conv hub wt={wt}: rel_err out {e_out:.2e} s {e_s:.2e}")
    assert e_out < TIGHT and e_s < TIGHT


# ---- 4. strided operands ------------------------------------------------------------------------------------------------
def _frame_check(fr, want, tol, what):
    got = fr.buf.numpy()
    body = fr._body(got)
    assert rel_err(body[:, :fr.f], want) < tol, (what, rel_err(body[:, :fr.f], want))
    assert (body[:, fr.f:] == SENTINEL).all() and (got[:fr.lead] == SENTINEL).all() \
        and (got[fr.lead + fr.n * fr.ld:] == SENTINEL).all(), (what, "written outside the view")


@pytest.mark.parametrize("wt", [0, 1])
def test_sage_conv_strided_operands(ctx, wt):
    from gcnx import device as D
    fi, fo = 32, 48
    hb, A = _ecoli3(fi)
    a = _csr(ctx, hb)
    op = a.row_mean().transpose() if wt else a.row_mean()
    rng = np.random.default_rng(21 + wt)
    w_nb, w_root, bias, m_nb, m_root = _weights(rng, fi, fo, wt)
    fx = Frame(ctx, hb.n, fi, 2 * fi, 4, data=hb.x)                     # x: a column slice of an array twice as wide
    fo_, fs = Frame(ctx, hb.n, fo, fo + 8, 8), Frame(ctx, hb.n, fi, fi + 4, 12)
    assert fx.aligned() and fo_.aligned() and fs.aligned()
    assert D.sage_conv_ok(ctx, hb.n, fi, fo, fx.view.ld)
    D.sage_conv(ctx, op, fx.view, ctx.to_device(w_nb), ctx.to_device(w_root), ctx.to_device(bias), fo_.view, s=fs.view, w_transposed=wt)
    r_out, r_s = _ref(A.T.tocsr() if wt else A, hb.x, m_nb, m_root, bias)
    _frame_check(fo_, r_out, TIGHT, "out")
    _frame_check(fs, r_s, TIGHT, "s")
    fx.check(hb.x, "x is not written")


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_sage_conv_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb, _ = _ecoli3(16)
    a = _csr(ctx, hb).row_mean()
    n = hb.n

    def refused(x, fi, fo):
        w = ctx.zeros((fi, fo))
        out, s = Frame(ctx, n, fo, fo, 0), Frame(ctx, n, fi, fi, 0)
        with pytest.raises(_lib.GcnxError) as e:
            D.sage_conv(ctx, a, x, w, w, None, out.view, s=s.view)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        out.check(np.full((n, fo), SENTINEL), "out"); s.check(np.full((n, fi), SENTINEL), "s")

    assert not D.sage_conv_ok(ctx, n, 96, 64) and not D.sage_conv_ok(ctx, n, 16, 256) and not D.sage_conv_ok(ctx, n, 16, 64, 18)
    refused(ctx.zeros((n, 96)), 96, 64)
    refused(ctx.zeros((n, 16)), 16, 256)
    wide = ctx.zeros((n, 18))
    refused(DeviceArray(ctx, wide.ptr, (n, 16), np.float32, ld=18, base=wide), 16, 64)          # ldx % 4 != 0
    off = Frame(ctx, n, 16, 16, 1, data=hb.x)                                                    # x one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4
    refused(off.view, 16, 64)
    # n = 0: nothing to do, no error -- whatever the pointers
    x, w, out = ctx.zeros((4, 16)), ctx.zeros((16, 64)), Frame(ctx, 4, 64, 64, 0)
    rc = ctx.lib.gcnx_sage_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, x.ptr, 16, 0, 16, w.ptr, w.ptr, 64, 0, None, None, 0,
                                out.view.ptr, 64)
    assert rc == _lib.OK
    out.check(np.full((4, 64), SENTINEL), "n = 0 writes nothing")
    # negative sizes and NULL mandatory pointers: invalid arguments
    for bad in (dict(n=-1), dict(w=None), dict(x=None)):
        rc = ctx.lib.gcnx_sage_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, x.ptr if "x" not in bad else None, 16, bad.get("n", 4),
                                    16, w.ptr if "w" not in bad else None, w.ptr, 64, 0, None, None, 0, out.view.ptr, 64)
        assert rc == 1, bad                                                                       # GCNX_ERR_INVALID
    out.check(np.full((4, 64), SENTINEL), "refused calls write nothing")


# ---- 6. capture -----------------------------------------------------------------------------------------------------------
def test_sage_conv_captured_replay_is_bit_identical(ctx):
    from gcnx import device as D
    fi, fo = 64, 64
    hb, _ = _ecoli3(fi)
    op = _csr(ctx, hb).row_mean()
    rng = np.random.default_rng(5)
    w_nb, w_root, bias, _, _ = _weights(rng, fi, fo, 0)
    out_e, s_e = _run(ctx, op, hb.x, w_nb, w_root, bias, fo, 0)
    x, wn, wr, b = ctx.to_device(hb.x), ctx.to_device(w_nb), ctx.to_device(w_root), ctx.to_device(bias)
    out, s = ctx.zeros((hb.n, fo)), ctx.zeros((hb.n, fi))
    g = ctx.capture(lambda: D.sage_conv(ctx, op, x, wn, wr, b, out, s=s))
    try:
        assert not out.numpy().any()                                     # captured, not yet executed
        for _ in range(2):
            out.fill_zero(); s.fill_zero()
            g.launch()
            assert np.array_equal(_bits(out.numpy()), _bits(out_e)) and np.array_equal(_bits(s.numpy()), _bits(s_e))
    finally:
        g.destroy()


# ---- 7. the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("root_weight", [True, False])
def test_sageconv_layer_forward_and_backward(ctx, root_weight):
    from gcnx.layers import SAGEConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    A = SR.mean_operator(_scipy_adj(hb), hb.n)
    lay = SAGEConv(64, root_weight=root_weight, seed=3)
    a_mean = SAGEConv.preprocess(a)
    x = ctx.to_device(hb.x)
    y = lay([x, a_mean])
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    assert list(p) == (["lin_l.weight", "lin_l.bias", "lin_r.weight"] if root_weight else ["lin_l.weight", "lin_l.bias"])
    w_l, w_r = p["lin_l.weight"].T, (p["lin_r.weight"].T if root_weight else None)
    r_y, r_s = SR.sage_conv_fwd(A, hb.x, w_l, w_r, p["lin_l.bias"])
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r_dx, r_dwl, r_dwr, r_db = SR.sage_conv_bwd(A, hb.x, r_s, w_l, w_r, dy)
    assert rel_err(dx.numpy(), r_dx) < TIGHT
    assert rel_err(lay.grads["lin_l.weight"].numpy(), r_dwl.T) < TIGHT and rel_err(lay.grads["lin_l.bias"].numpy(), r_db) < TIGHT
    if root_weight:
        assert rel_err(lay.grads["lin_r.weight"].numpy(), r_dwr.T) < TIGHT
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None


# ---- 8. gcnx.SAGE: a full step on either route against the kink-separated oracle ---------------------------------------------
def _sides(m, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    return {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
            for i in (1, 2)}


def _check_step(m, batch, hb, p, tol, what):
    m.loss_and_grads(batch)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = SR.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, hb.y, masks=_sides(m), argmax=arg)
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol and la[1] == r["hits"], (la, r["loss"], r["hits"])
    _cmp_grads(m.gradients(), r["grads"], tol, what)
    return r


@pytest.mark.parametrize("shape", ["config1", "config2"])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_sage_step_against_oracle(ctx, monkeypatch, fused, shape):
    import gcnx
    from gcnx import synth
    hb = _tiny_host(16, 16, seed=4) if shape == "config1" else synth.ecoli_batch(f=16)
    batch = _device_batch(ctx, hb)
    monkeypatch.setenv("GCNX_SAGE_FUSED", fused)
    m = gcnx.SAGE(ctx, hidden_channels=64, seed=0)
    assert m._fused == (fused == "1")
    p = {k: v.astype(np.float32) for k, v in SR.init_params(16, 64, seed=7).items()}
    m.load_state_dict(p)
    _check_step(m, batch, hb, p, 1e-4, f"{shape} fused={fused}")
    # five SGD steps, each oracle step on the device's kink sides of that step (taken with the step's own weights)
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    a = _scipy_adj(hb)
    for _ in range(5):
        pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
        m.train_step(batch, lr=0.02)
        arg = m._bufs["arg"].numpy().astype(np.int64)
        r = SR.model(hb.x, a, hb.graph_ptr, ph, hb.y, masks=_sides(m, pre), argmax=arg)
        ph = SR.sgd(ph, r["grads"], 0.02)
    sd = m.state_dict()
    for k in SR.KEYS:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{shape} fused={fused} after 5 steps {k}")


# ---- 9. torch-style surface ---------------------------------------------------------------------------------------------
def _logits_match_oracle(m, x, a, gp, what):
    r = SR.model(x, a, gp, m.state_dict(), masks=_sides(m), argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, what)


def test_sage_forward_state_dict_and_single_graph(ctx):
    import gcnx
    import scipy.sparse as sp
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.SAGE(ctx, seed=1)
    ids, a = hb.ids(), _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1)
    _logits_match_oracle(m, hb.x, a, hb.graph_ptr, "stored loops")
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    sd = m.state_dict()
    assert list(sd) == list(SR.KEYS)
    assert sd["conv1.lin_l.weight"].shape == (64, 16) and sd["conv1.lin_r.weight"].shape == (64, 16) and sd["conv1.lin_l.bias"].shape == (64,)
    assert sd["conv2.lin_l.weight"].shape == (64, 64) and sd["linear_2.weight"].shape == (1, 64)
    assert np.max(np.abs(sd["conv1.lin_l.weight"])) <= 0.25 and np.max(np.abs(sd["conv2.lin_r.weight"])) <= 0.125   # U(+-1/sqrt(fan_in))
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    m2 = gcnx.SAGE(ctx, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(_bits(v), _bits(sd[k])), k
    assert np.array_equal(m2((hb.x, a, ids)), logits)
    assert [w.shape for w in m.get_weights()] == [sd[k].shape for k in SR.KEYS]
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


def test_sage_hidden_256_takes_the_composed_route(ctx):
    import gcnx
    from gcnx import device as D
    hb = _tiny_host(16, 16, seed=8)
    m = gcnx.SAGE(ctx, hidden_channels=256, seed=0)
    assert m._fused and not D.sage_conv_ok(ctx, hb.n, 16, 256) and not D.sage_conv_ok(ctx, hb.n, 256, 256)
    p = {k: v.astype(np.float32) for k, v in SR.init_params(16, 256, seed=2).items()}
    m.load_state_dict(p)
    _check_step(m, _device_batch(ctx, hb), hb, p, 1e-4, "hidden 256")


# ---- 10. sync-BN over graph shards ----------------------------------------------------------------------------------------
def test_sage_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in SR.init_params(16, 64, seed=7).items()}

    def step(ctx, part, comm, gb):
        m = gcnx.SAGE(ctx, hidden_channels=64, seed=0, comm=comm)
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


# ---- 11. gcnx.fit -----------------------------------------------------------------------------------------------------------
def test_fit_runs_the_sage_model(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:10]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[10:]])
    m = gcnx.SAGE(ctx, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])

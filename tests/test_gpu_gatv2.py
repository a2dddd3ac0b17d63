"""GPU tests of GATv2Conv: the kernels of csrc/gatv2.hip (gcnx_gatv2_aggregate, gcnx_gatv2_bwd_edges, gcnx_gatv2_bwd_nodes), the
layer gcnx.GATv2Conv and the model gcnx.GATv2 -- each against the float64 oracle tests/gatv2_ref.py on the device's side of every
kink: the nnz H C LeakyReLU sides come from gatv2_ref.device_sides, which recomputes s in float32 by the contract of
include/gcnx.h from the stored operands.  Bound: test_gpu_gat.TIGHT = 2e-5 (max-norm relative against float64) for every kernel,
the layer, a whole step of the model and the two loader routes."""
import functools

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import gatv2_ref as GV
from gpu_frames import SENTINEL, Frame
from test_gpu_gat import TIGHT, UNDER_BN, _bits, _csr, _ecoli3, _edge_case_csr, _frame_check
from test_gpu_gcn_bn import _tiny_host

pytestmark = pytest.mark.gpu

STEP = TIGHT                        # a whole step of the model is held to the kernels' bound
SHAPES = [(1, 16), (1, 64), (4, 16), (8, 16), (2, 32), (1, 128), (4, 32)]
EDGE_DIMS = [0, 1, 2, 8]
UNDER_BN_V2 = {"conv1.bias": "conv1.lin_l.weight", "conv2.bias": "conv2.lin_l.weight", "linear_1.bias": "linear_1.weight",
               "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}
assert set(UNDER_BN_V2) == set(UNDER_BN)


def _operands(n, nnz, heads, c, d, seed, xl=None, scale=1.0, shift=0.0):
    """Xl | Xr (unit scale; xl: given left half), att ~ N(0, 1) / sqrt(c) (the softmax neither flat nor saturated), a bias, e in
    (0, 1) as dca / proximity are, W_e ~ N(0, 1) / 2, dout."""
    rng = np.random.default_rng(seed)
    hc = heads * c
    xlr = rng.standard_normal((n, 2 * hc)).astype(np.float32)
    if xl is not None:
        xlr[:, :hc] = xl
    xlr[:, hc:] += np.float32(shift)
    att = (scale * rng.standard_normal((heads, c)) / np.sqrt(c)).astype(np.float32)
    bias = rng.standard_normal(hc).astype(np.float32)
    e = rng.uniform(0, 1, (nnz, d)).astype(np.float32) if d else None
    w_e = (rng.standard_normal((d, hc)) / 2).astype(np.float32) if d else None
    dout = rng.standard_normal((n, hc)).astype(np.float32)
    return dict(xlr=xlr, att=att, bias=bias, e=e, w_e=w_e, dout=dout)


class _Dev:
    """The device side of one layer evaluation: operands uploaded once (or given as device views), every kernel callable."""

    def __init__(self, ctx, a, ops, slope=0.2):
        up = lambda t: t if t is None or hasattr(t, "ptr") else ctx.to_device(t)
        self.ctx, self.a, self.slope = ctx, a, slope
        self.xlr, self.att, self.bias, self.e, self.w_e, self.dout = (up(ops[k]) for k in ("xlr", "att", "bias", "e", "w_e", "dout"))
        self.heads, self.c = self.att.shape
        self.n, self.hc = self.xlr.shape[0], self.heads * self.c
        self.d = 0 if self.e is None else self.e.shape[1]

    def aggregate(self, alpha=True, o_pre=True, bias=True, out=None, o=None):
        from gcnx import device as D
        ctx = self.ctx
        self.out = out if out is not None else ctx.empty((self.n, self.hc))
        self.alpha = ctx.zeros((self.a.nnz, self.heads)) if alpha else None
        self.o = (o if o is not None else ctx.empty((self.n, self.hc))) if o_pre else None
        D.gatv2_aggregate(ctx, self.a, self.xlr, self.att, self.bias if bias else None, self.out, e=self.e, w_e=self.w_e, alpha=self.alpha,
                          o_pre=self.o, slope=self.slope)
        return self.out.numpy(), (self.alpha.numpy() if alpha else None), (self.o.numpy() if o_pre else None)

    def bwd_edges(self, dxr=None):
        from gcnx import device as D
        ctx = self.ctx
        self.dscore = ctx.zeros((self.a.nnz, self.heads))
        self.dxr = dxr if dxr is not None else ctx.empty((self.n, self.hc))
        self.datt = ctx.empty((self.heads, self.c))
        self.dwe = ctx.empty((self.d, self.hc)) if self.d else None
        scratch = ctx.empty(max(D.gatv2_bwd_scratch_floats(ctx, self.n, self.heads, self.c, self.d), 1))
        D.gatv2_bwd_edges(ctx, self.a, self.xlr, self.att, self.alpha, self.dout, self.o, self.dscore, self.dxr, self.datt, scratch, e=self.e,
                          w_e=self.w_e, dw_e=self.dwe, slope=self.slope)
        return self.dscore.numpy(), self.dxr.numpy(), self.datt.numpy(), (self.dwe.numpy() if self.d else None)

    def bwd_nodes(self, dxl=None):
        from gcnx import device as D
        self.dxl = dxl if dxl is not None else self.ctx.empty((self.n, self.hc))
        D.gatv2_bwd_nodes(self.ctx, self.a, self.xlr, self.att, self.alpha, self.dscore, self.dout, self.dxl, e=self.e, w_e=self.w_e,
                          slope=self.slope)
        return self.dxl.numpy()


def _oracle(rowptr, colidx, ops, sides, slope=0.2):
    """gatv2_ref on Xl | Xr directly (x = Xl | Xr, W_l = [I; 0], W_r = [0; I], no lin biases): the gradient of x is dXl | dXr."""
    hc = ops["xlr"].shape[1] // 2
    eye, zero = np.eye(hc), np.zeros((hc, hc))
    out, cache = GV.conv_fwd(rowptr, colidx, ops["xlr"], np.vstack([eye, zero]), None, np.vstack([zero, eye]), None, ops["att"], ops["bias"],
                             ops["e"], ops["w_e"], slope, sides)
    cache["grads"] = GV.conv_bwd(cache, ops["dout"])
    return out, cache


def _check_all(ctx, a, rowptr, colidx, ops, what, tol=TIGHT, cancelling=False):
    """Every kernel on one input against the oracle; returns the device object with the host copies (errors printed first).
    cancelling: dxr = sum_j ds_ij and datt = sum_ij dscore_ij g_ij are measured against the largest sum of the MAGNITUDES of
    their terms instead of the largest result -- for inputs on which every s of a row lies on one side of the kink, so that
    dxr[i] = att * sum_j dscore_ij is analytically ZERO (a softmax's score gradients sum to zero over its row) and datt loses
    the common part of g the same way.  The rounding error of an fp32 sum is bounded by eps times the sum of its terms'
    magnitudes, whatever cancels; relative to a result that is zero no bound can hold."""
    d = _Dev(ctx, a, ops)
    out, alpha, o = d.aggregate()
    dscore, dxr, datt, dwe = d.bwd_edges()
    dxl = d.bwd_nodes()
    sides = GV.device_sides(ops["xlr"], ops["e"], ops["w_e"], rowptr, colidx)
    r_out, k = _oracle(rowptr, colidx, ops, sides)
    n, hc = d.n, d.hc
    g = k["grads"]
    errs = {"out": rel_err(out, r_out), "alpha": rel_err(alpha, k["alpha"]), "o_pre": rel_err(o, k["O"].reshape(n, hc)),
            "dscore": rel_err(dscore, k["dscore"]), "dxr": rel_err(dxr, g["x"][:, hc:]), "dxl": rel_err(dxl, g["x"][:, :hc]),
            "datt": rel_err(datt, g["att"])}
    if d.d:
        errs["dw_e"] = rel_err(dwe, g["We"])
    if cancelling:
        row = np.repeat(np.arange(n), np.diff(np.asarray(rowptr, np.int64)))
        terms = np.zeros((n, hc))
        np.add.at(terms, row, np.abs(k["ds"]))
        errs["dxr"] = float(np.max(np.abs(dxr - g["x"][:, hc:]))) / float(terms.max())
        errs["datt"] = float(np.max(np.abs(datt - g["att"]))) / float(np.abs(k["dscore"][:, :, None] * k["g"]).sum(0).max())
    print(f"gatv2 {what} heads={d.heads} c={d.c} edge_dim={d.d}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert np.isfinite(out).all() and np.isfinite(alpha).all() and np.isfinite(dxl).all() and np.isfinite(dxr).all()
    for key, v in errs.items():
        assert v < tol, (what, key, v)
    d.host = dict(out=out, alpha=alpha, o=o, dscore=dscore, dxr=dxr, datt=datt, dwe=dwe, dxl=dxl, ref=k, r_out=r_out, sides=sides)
    return d


# ---- 1. the kernels against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("heads,c", SHAPES)
def test_gatv2_kernels_against_float64(ctx, heads, c, edge_dim):
    from gcnx import device as D
    hb = _ecoli3(heads * c)
    a = _csr(ctx, hb)
    assert D.gatv2_conv_ok(ctx, hb.n, heads, c, edge_dim=edge_dim) and hb.n % 32 != 0
    ops = _operands(hb.n, hb.nnz, heads, c, edge_dim, 1000 * edge_dim + 100 * heads + c, xl=hb.x)
    d = _check_all(ctx, a, hb.rowptr, hb.colidx, ops, "ecoli-3")
    h = d.host
    frac = h["sides"].mean()
    assert 0.2 < frac < 0.8, frac                                       # both sides of the kink are exercised
    sums = np.add.reduceat(h["alpha"].astype(np.float64), hb.rowptr[:-1].astype(np.int64))
    assert np.diff(hb.rowptr).min() > 0 and np.max(np.abs(sums - 1.0)) < 1e-6, np.max(np.abs(sums - 1.0))
    # no atomics: a second call of each leaves the same bits
    out2, alpha2, o2 = d.aggregate()
    second = (out2, alpha2, o2) + d.bwd_edges() + (d.bwd_nodes(),)
    first = tuple(h[k] for k in ("out", "alpha", "o", "dscore", "dxr", "datt", "dwe", "dxl"))
    for k, (x, y) in enumerate(zip(first, second)):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), k
    # alpha = NULL, o_pre = NULL and bias = NULL give the same out bits (minus the bias)
    out3, alpha3, o3 = d.aggregate(alpha=False, o_pre=False)
    assert alpha3 is None and o3 is None and np.array_equal(_bits(out3), _bits(h["out"]))
    out4, _, _ = d.aggregate(alpha=False, o_pre=False, bias=False)
    assert np.array_equal(_bits(out4 + ops["bias"]), _bits(h["out"])) and np.array_equal(_bits(out4), _bits(h["o"]))


# ---- 2. the smallest shapes that can still go wrong -----------------------------------------------------------------------------
@pytest.mark.parametrize("heads,c,edge_dim", [(4, 8, 2), (1, 16, 0), (1, 128, 2)])
def test_gatv2_kernels_degenerate_inputs(ctx, heads, c, edge_dim):
    """Rows without entries, a directed pattern (the transposed pattern differs), fewer rows than a tile, a row with only its
    loop, a row whose only entry is in no row.  (1, 128): the backward kernels' 16-row workgroups."""
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _edge_case_csr()
    n, hc = 56, heads * c
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp, symmetric=False)
    assert not a.symmetric
    ops = _operands(n, len(colidx), heads, c, edge_dim, 7 + heads)
    d = _check_all(ctx, a, rowptr, colidx, ops, "56 rows")
    h = d.host
    assert np.array_equal(_bits(h["out"][[4, 20]]), _bits(np.broadcast_to(ops["bias"], (2, hc))))       # no entries: the bias, bit for bit
    assert not h["o"][[4, 20]].any() and not h["dxr"][[4, 20]].any()
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    nnz5 = int(rowptr[5])
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:nnz5], None, gp[:4].copy(), symmetric=False)
    _check_all(ctx, a5, rowptr[:6], colidx[:nnz5], _operands(5, nnz5, heads, c, edge_dim, 32), "5 rows")
    # one row with only its self-loop: alpha == 1 exactly, out == Xl + bias bit for bit
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), None, one, symmetric=True)
    ops1 = _operands(1, 1, heads, c, edge_dim, 33)
    d1 = _check_all(ctx, a1, one, np.zeros(1, np.int32), ops1, "1 row, self-loop")
    assert np.array_equal(d1.host["alpha"], np.ones((1, heads), np.float32))
    assert np.array_equal(_bits(d1.host["out"]), _bits(ops1["xlr"][:, :hc] + ops1["bias"]))
    # one row without any entry (the stored entry is in no row)
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), None, one, symmetric=True)
    d0 = _Dev(ctx, a0, ops1)
    out0, _, o0 = d0.aggregate()
    assert np.array_equal(_bits(out0), _bits(ops1["bias"][None])) and not o0.any()
    _, dxr0, datt0, dwe0 = d0.bwd_edges()                                # (no transposed pattern of a CSR whose entry is in no row)
    assert not dxr0.any() and not datt0.any() and (dwe0 is None or not dwe0.any())


@functools.lru_cache(maxsize=None)
def _one_long_row():
    """One graph of 1 300 rows (not a multiple of 32): every loop, a ring, and row 7 <-> columns 0 .. 1 099 -- a single row of
    more than the 1 024 entries a tile stages in LDS, in the forward CSR and, the pattern being symmetric, in the transposed one."""
    import scipy.sparse as sp
    n = 1300
    i = np.arange(n)
    hub = np.arange(1100)
    rows = np.concatenate([i, i, (i + 1) % n, np.full(hub.size, 7), hub])
    cols = np.concatenate([i, (i + 1) % n, i, hub, np.full(hub.size, 7)])
    a = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    deg = np.diff(a.indptr)
    assert deg[7] > 1024 and np.sum(deg > 1024) == 1 and n % 32 != 0
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.array([0, n], np.int32)


@pytest.mark.parametrize("heads,edge_dim", [(1, 2), (4, 0)])
def test_gatv2_kernels_one_row_beyond_the_staged_entries(ctx, heads, edge_dim):
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _one_long_row()
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp)
    assert a.symmetric
    _check_all(ctx, a, rowptr, colidx, _operands(1300, len(colidx), heads, 64 // heads, edge_dim, 11 + heads), "long row")


def test_gatv2_no_rows(ctx):
    """n = 0 succeeds and writes nothing."""
    from gcnx import _lib
    lib = ctx.lib
    out, al, big = Frame(ctx, 4, 16, 16, 0), Frame(ctx, 16, 1, 1, 0), ctx.zeros(64)
    x, att = ctx.zeros((4, 32)), ctx.zeros((1, 16))
    rp = ctx.to_device(np.zeros(1, np.int32))
    rcs = (lib.gcnx_gatv2_aggregate(ctx.h, rp.ptr, rp.ptr, x.ptr, 32, 0, 1, 16, None, 0, 0, None, att.ptr, None, 0.2, out.view.ptr, 16,
                                    al.view.ptr, None, 0),
           lib.gcnx_gatv2_bwd_edges(ctx.h, rp.ptr, rp.ptr, x.ptr, 32, 0, 1, 16, None, 0, 0, None, att.ptr, 0.2, al.view.ptr, x.ptr, 32, x.ptr, 32,
                                    al.view.ptr, out.view.ptr, 16, big.ptr, None, big.ptr),
           lib.gcnx_gatv2_bwd_nodes(ctx.h, rp.ptr, rp.ptr, rp.ptr, x.ptr, 32, 0, 1, 16, None, 0, 0, None, att.ptr, 0.2, al.view.ptr, al.view.ptr,
                                    x.ptr, 32, out.view.ptr, 16))
    assert rcs == (_lib.OK,) * 3
    for fr in (out, al):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "n = 0 writes nothing")
    assert not big.numpy().any()


def test_gatv2_strided_operands(ctx):
    """ldx > 2 HC, a strided e, strided out / o_pre / d_out, and dXl | dXr written as the halves of ONE wider array."""
    from gcnx import device as D
    heads, c, ed = 4, 8, 2
    hc = heads * c
    hb = _ecoli3(hc)
    a = _csr(ctx, hb)
    ops = _operands(hb.n, hb.nnz, heads, c, ed, 51, xl=hb.x)
    fx = Frame(ctx, hb.n, 2 * hc, 2 * hc + 8, 4, data=ops["xlr"])
    fe = Frame(ctx, hb.nnz, ed, ed + 3, 1, data=ops["e"])               # (e is read with scalar loads: no alignment rule)
    f_out, f_o = Frame(ctx, hb.n, hc, hc + 8, 8), Frame(ctx, hb.n, hc, hc + 4, 12)
    f_do = Frame(ctx, hb.n, hc, hc + 4, 4, data=ops["dout"])
    f_dx = Frame(ctx, hb.n, 2 * hc, 2 * hc + 4, 4)
    assert all(f.aligned() for f in (fx, f_out, f_o, f_do, f_dx)) and D.gatv2_conv_ok(ctx, hb.n, heads, c, fx.view.ld, ed)
    d = _Dev(ctx, a, dict(ops, xlr=fx.view, e=fe.view, dout=f_do.view))
    d.aggregate(out=f_out.view, o=f_o.view)
    d.bwd_edges(dxr=f_dx.view.cols(hc, 2 * hc))
    d.bwd_nodes(dxl=f_dx.view.cols(0, hc))
    r_out, k = _oracle(hb.rowptr, hb.colidx, ops, GV.device_sides(ops["xlr"], ops["e"], ops["w_e"], hb.rowptr, hb.colidx))
    g = k["grads"]
    assert rel_err(d.alpha.numpy(), k["alpha"]) < TIGHT and rel_err(d.dscore.numpy(), k["dscore"]) < TIGHT
    assert rel_err(d.datt.numpy(), g["att"]) < TIGHT and rel_err(d.dwe.numpy(), g["We"]) < TIGHT
    _frame_check(f_out, r_out, TIGHT, "out")
    _frame_check(f_o, k["O"].reshape(hb.n, hc), TIGHT, "o_pre")
    _frame_check(f_dx, g["x"], TIGHT, "dXl | dXr")
    fx.check(ops["xlr"], "xlr is not written")
    fe.check(ops["e"], "e is not written")
    f_do.check(ops["dout"], "d_out is not written")


# ---- 3. the range of the exponential ----------------------------------------------------------------------------------------
def test_gatv2_scaled_scores_give_near_one_hot_rows(ctx):
    hb = _ecoli3(64)
    ops = _operands(hb.n, hb.nnz, 4, 16, 2, 41, xl=hb.x, scale=30.0)
    d = _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, "att x 30")
    top = np.maximum.reduceat(d.host["alpha"], hb.rowptr[:-1].astype(np.int64))
    assert np.median(top) > 0.99                                          # near one-hot


@pytest.mark.parametrize("shift", [200.0, -200.0])
def test_gatv2_shifted_xr_stays_finite(ctx, shift):
    """Xr shifted by +-200: every s, and with it every score, moves by hundreds.  The running maximum is subtracted before each
    exponential, so nothing overflows (asserted below for fp32: what a kernel without the subtraction would sum) and no row
    divides 0 by 0.  Every s then lies on one side of the kink: dxr and datt are cancelling sums (_check_all)."""
    hb = _ecoli3(64)
    ops = _operands(hb.n, hb.nnz, 4, 16, 2, 43, xl=hb.x, shift=shift)
    d = _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, f"Xr {shift:+.0f}", cancelling=True)
    sides = d.host["sides"]
    assert sides.all() if shift > 0 else not sides.any()                  # one side for every entry: what makes the sums cancel
    top = np.abs(d.host["ref"]["score"]).max()
    assert top > (100.0 if shift > 0 else 20.0), top                      # (the negative side is scaled by the slope 0.2)
    with np.errstate(over="ignore"):
        assert shift < 0 or np.exp(np.float32(top)) == np.inf


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_gatv2_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb = _ecoli3(16)
    a = _csr(ctx, hb)
    n, nnz = hb.n, a.nnz

    def refused(xlr, heads, c, ed=0):
        hc = heads * c
        att, w_e, e = ctx.zeros((heads, c)), (ctx.zeros((ed, hc)) if ed else None), (ctx.zeros((nnz, ed)) if ed else None)
        out, o, dxl, dxr = (Frame(ctx, n, hc, hc, 0) for _ in range(4))
        alpha, ds = Frame(ctx, nnz, heads, heads, 0), Frame(ctx, nnz, heads, heads, 0)
        datt, dwe = Frame(ctx, heads, c, c, 0), (Frame(ctx, ed, hc, hc, 0) if ed else None)
        dense = ctx.zeros((n, hc))
        scratch = ctx.zeros(max(D.gatv2_bwd_scratch_floats(ctx, n, heads, c, ed), 1) + 16 * n)
        calls = (lambda: D.gatv2_aggregate(ctx, a, xlr, att, None, out.view, e=e, w_e=w_e, alpha=alpha.view, o_pre=o.view),
                 lambda: D.gatv2_bwd_edges(ctx, a, xlr, att, alpha.view, dense, dense, ds.view, dxr.view, datt.view, scratch, e=e, w_e=w_e,
                                           dw_e=dwe.view if ed else None),
                 lambda: D.gatv2_bwd_nodes(ctx, a, xlr, att, alpha.view, ds.view, dense, dxl.view, e=e, w_e=w_e))
        for call in calls:
            with pytest.raises(_lib.GcnxError) as err:
                call()
            assert err.value.code == _lib.ERR_UNSUPPORTED
        for fr in (out, o, dxl, dxr, alpha, ds, datt) + ((dwe,) if ed else ()):
            fr.check(np.full((fr.n, fr.f), SENTINEL), "a refused call writes nothing")

    for heads, c in ((3, 16), (1, 96), (8, 32), (8, 2)):
        assert not D.gatv2_conv_ok(ctx, n, heads, c)
        refused(ctx.zeros((n, 2 * heads * c)), heads, c)
    assert not D.gatv2_conv_ok(ctx, n, 1, 16, edge_dim=9)
    refused(ctx.zeros((n, 32)), 1, 16, ed=9)
    wide = ctx.zeros((n, 34))
    assert not D.gatv2_conv_ok(ctx, n, 1, 16, 34)
    refused(DeviceArray(ctx, wide.ptr, (n, 32), np.float32, ld=34, base=wide), 1, 16)            # ldx % 4 != 0
    off = Frame(ctx, n, 32, 32, 1)                                                              # one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4 and D.gatv2_conv_ok(ctx, n, 1, 16)
    refused(off.view, 1, 16)
    # negative sizes and NULL mandatory pointers: invalid arguments; e = NULL with edge_dim > 0 too
    lib = ctx.lib
    x, att, out = ctx.zeros((4, 32)), ctx.zeros((1, 16)), Frame(ctx, 4, 16, 16, 0)
    al, big, we = Frame(ctx, 16, 1, 1, 0), ctx.zeros(256), ctx.zeros((2, 16))
    rp, ci = a.rowptr.ptr, a.colidx.ptr

    def call_all(nn, xp, ed=0, ep=None):
        return (lib.gcnx_gatv2_aggregate(ctx.h, rp, ci, xp, 32, nn, 1, 16, ep, ed, ed, we.ptr, att.ptr, None, 0.2, out.view.ptr, 16, al.view.ptr,
                                         None, 0),
                lib.gcnx_gatv2_bwd_edges(ctx.h, rp, ci, xp, 32, nn, 1, 16, ep, ed, ed, we.ptr, att.ptr, 0.2, al.view.ptr, x.ptr, 32, x.ptr, 32,
                                         al.view.ptr, out.view.ptr, 16, big.ptr, big.ptr, big.ptr),
                lib.gcnx_gatv2_bwd_nodes(ctx.h, rp, ci, ci, xp, 32, nn, 1, 16, ep, ed, ed, we.ptr, att.ptr, 0.2, al.view.ptr, al.view.ptr, x.ptr,
                                         32, out.view.ptr, 16))

    assert call_all(-1, x.ptr) == (1,) * 3                                                      # GCNX_ERR_INVALID
    assert call_all(4, None) == (1,) * 3
    assert call_all(4, x.ptr, ed=2, ep=None) == (1,) * 3
    for fr in (out, al):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "invalid calls write nothing")
    assert not big.numpy().any()


# ---- 5. the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dim", [None, 2])
def test_gatv2conv_layer_forward_and_backward(ctx, edge_dim):
    from gcnx.layers import GATv2Conv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    lay = GATv2Conv(16, heads=4, edge_dim=edge_dim, seed=3)
    pre = GATv2Conv.preprocess(a)
    assert pre.vals is None and pre.nnz == a.nnz
    lay.build(ctx, 16)
    names = ["att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias"] + (["lin_edge.weight"] if edge_dim else [])
    assert list(lay.params) == names == list(lay.grads)
    assert lay.lin_weight.shape == (16, 128) and lay.lin_bias.shape == (128,) and all(v.ptr % 16 == 0 for v in lay.params.values())
    assert lay.params["lin_r.weight"].ptr == lay.lin_weight.ptr + 4 * 64 and lay.params["lin_r.weight"].ld == 128       # views of ONE tensor
    assert not lay.params["bias"].numpy().any() and not lay.lin_bias.numpy().any()
    rng = np.random.default_rng(1)
    w = lay.get_weights()
    for i, k in enumerate(names):
        if k.endswith("bias"):
            w[i] = rng.standard_normal(64).astype(np.float32)
    lay.set_weights(w)
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    assert all(np.array_equal(p[k], np.asarray(w[i], np.float64)) for i, k in enumerate(names))
    sd = lay.state_dict()
    assert sd["att"].shape == (1, 4, 16) and sd["lin_l.weight"].shape == sd["lin_r.weight"].shape == (64, 16) and sd["bias"].shape == (64,)
    assert sd["lin_l.bias"].shape == (64,) and (not edge_dim or sd["lin_edge.weight"].shape == (64, 2))
    assert np.array_equal(sd["lin_r.weight"].T, lay.params["lin_r.weight"].numpy())
    x = ctx.to_device(hb.x)
    e_host = rng.uniform(0, 1, (hb.nnz, 2)).astype(np.float32) if edge_dim else None
    e = ctx.to_device(e_host) if edge_dim else None
    y = lay([x, pre, e] if edge_dim else [x, pre])
    xlr = lay._saved[3].numpy()
    sides = GV.device_sides(xlr, e_host, p.get("lin_edge.weight"), hb.rowptr, hb.colidx)
    r_y, k = GV.conv_fwd(hb.rowptr, hb.colidx, hb.x, p["lin_l.weight"], p["lin_l.bias"], p["lin_r.weight"], p["lin_r.bias"], p["att"],
                         p["bias"], e_host, p.get("lin_edge.weight"), 0.2, sides)
    assert rel_err(xlr, np.hstack([k["Xl"].reshape(hb.n, 64), k["Xr"].reshape(hb.n, 64)])) < TIGHT      # ONE gcnx_gemm, stacked bias
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = rng.standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r = GV.conv_bwd(k, dy)
    g = lay.grads
    errs = {"dx": rel_err(dx.numpy(), r["x"]), "att": rel_err(g["att"].numpy(), r["att"]), "bias": rel_err(g["bias"].numpy(), r["bias"]),
            "lin_l.weight": rel_err(g["lin_l.weight"].numpy(), r["Wl"]), "lin_l.bias": rel_err(g["lin_l.bias"].numpy(), r["bl"]),
            "lin_r.weight": rel_err(g["lin_r.weight"].numpy(), r["Wr"]), "lin_r.bias": rel_err(g["lin_r.bias"].numpy(), r["br"])}
    if edge_dim:
        errs["lin_edge.weight"] = rel_err(g["lin_edge.weight"].numpy(), r["We"])
    print(f"gatv2 layer edge_dim={edge_dim}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert max(errs.values()) < TIGHT, errs
    before = {k: v.numpy() for k, v in g.items()}
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    assert all(np.array_equal(_bits(before[k]), _bits(g[k].numpy())) for k in before)              # the same gradients without dx
    with pytest.raises(NotImplementedError):
        GATv2Conv(24, heads=4)([x, pre])                                 # HC = 96: no kernel and no composed route
    with pytest.raises(ValueError):
        lay([x, pre] if edge_dim else [x, pre, ctx.zeros((hb.nnz, 2))])  # e missing with edge_dim / given without
    if edge_dim:
        with pytest.raises(ValueError):
            lay([x, pre, ctx.zeros((hb.nnz, 3))])                        # a wrong width


# ---- 6. gcnx.GATv2: a full step against the kink-separated oracle -------------------------------------------------------------
def _loop_mean_features(rowptr, colidx, d, seed):
    """e [nnz, d] in (0, 1), float32, every loop's row the mean of its row's other entries (zeros if none): what the host
    route's add_self_loops(fill_value="mean") writes, so it changes neither pattern nor values on graphs that carry every loop."""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    e = rng.uniform(0, 1, (len(colidx), d)).astype(np.float32)
    loop = row == colidx
    assert loop.sum() == len(rowptr) - 1
    s, cnt = np.zeros((len(rowptr) - 1, d)), np.bincount(row[~loop], minlength=len(rowptr) - 1)
    np.add.at(s, row[~loop], e[~loop].astype(np.float64))
    e[loop] = (s / np.maximum(cnt, 1)[:, None]).astype(np.float32)
    return e


def _sides(m, hb, e, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    s = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
         for i in (1, 2)}
    for i in (1, 2):
        we = m.p[f"we{i}"].numpy() if m.edge_dim else None
        s[f"s{i}"] = GV.device_sides(b[f"xlr{i}"].numpy(), e, we, hb.rowptr, hb.colidx)
    return s


def _cmp_grads(got, ref, tol, what):
    worst = 0.0
    for k in ref:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN_V2.get(k, k)], np.float64))))
        diff = float(np.max(np.abs(g - r)))
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)      # (a gradient that is exactly zero on both sides)
        worst = max(worst, err)
        assert err <= tol, (what, k, err)
    return worst


def _device_batch(ctx, hb, e):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), e=None if e is None else ctx.to_device(e))


@pytest.mark.parametrize("edge_dim", [None, 2])
@pytest.mark.parametrize("heads", [1, 4])
def test_gatv2_step_against_oracle(ctx, heads, edge_dim):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    e = _loop_mean_features(hb.rowptr, hb.colidx, 2, 5) if edge_dim else None
    batch = _device_batch(ctx, hb, e)
    m = gcnx.GATv2(ctx, hidden_channels=64, heads=heads, edge_dim=edge_dim, seed=0)
    assert m.uses_edge_features is bool(edge_dim)
    p = {k: v.astype(np.float32) for k, v in GV.init_params(16, 64, heads, edge_dim, seed=7).items()}
    m.load_state_dict(p)
    sd = m.state_dict()
    assert list(sd) == list(GV.keys(edge_dim)) and all(np.array_equal(_bits(sd[k]), _bits(p[k])) for k in p)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    what = f"heads={heads} edge_dim={edge_dim}"
    m.loss_and_grads(batch)
    for k in ("xlr1", "xlr2", "alpha1", "alpha2", "o1", "o2", "dscore", "dxlr", "scratch"):
        assert k in m._bufs, k
    assert m._bufs["alpha1"].shape == (hb.nnz, heads) and m._bufs["xlr1"].shape == (hb.n, 128)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = GV.model(hb.x, hb.rowptr, hb.colidx, e, hb.graph_ptr, p, hb.y, masks=_sides(m, hb, e), argmax=arg, heads=heads)
    la = m.loss_acc.numpy()
    e_out, e_loss = rel_err(m._bufs["out"].numpy(), r["out"]), rel_err(la[0], r["loss"])
    print(f"gatv2 step {what}: logits {e_out:.2e} loss {e_loss:.2e}")
    assert_close(m._bufs["out"].numpy(), r["out"], STEP, f"{what} logits")
    assert e_loss < STEP and la[1] == r["hits"], (la, r["loss"], r["hits"])
    print(f"gatv2 step {what}: worst gradient {_cmp_grads(m.gradients(), r['grads'], STEP, what):.2e}")
    # three steps with gcnx.Adam run and lower the loss
    m.set_optimizer(gcnx.Adam())
    losses = [m.train_step(batch, lr=0.01)[0] for _ in range(3)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_gatv2_host_and_device_loader_routes_agree(ctx):
    """The same model fed (a) DisjointLoader batches (host route: add_self_loops with fill_value="mean", which changes nothing
    on these graphs) and (b) DeviceDisjointLoader batches of DeviceDataset(edge_features=True) over the same graphs in the same
    order: the same loss and gradients to TIGHT.  On route (b) the transposed pattern is the loader's preset: no host sort."""
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(12, 16, seed=3)
    graphs = []
    for k, (x, a, y) in enumerate(raw):
        a = a.tocsr()
        a.sort_indices()
        graphs.append(Graph(x=x, a=a, y=y, e=_loop_mean_features(a.indptr, a.indices, 2, 100 + k)))
    ds = ListDataset(graphs)
    dsd = gcnx.DeviceDataset(ctx, ds, edge_features=True)
    dev = gcnx.DeviceDisjointLoader(dsd, batch_size=4, epochs=1, shuffle=True, seed=8)
    host = gcnx.DisjointLoader(ds, batch_size=4, epochs=1, shuffle=True, seed=8)
    m = gcnx.GATv2(ctx, hidden_channels=64, heads=4, edge_dim=2, seed=2)
    seen = 0
    for (inputs, target), (db, none) in zip(host, dev):
        assert none is None and len(inputs) == 4
        m.loss_and_grads(inputs, target)
        hbatch = m._last_batch
        la_h, g_h = m.loss_acc.numpy(), m.gradients()
        assert hbatch.a.nnz == db.a.nnz and np.array_equal(hbatch.a.colidx.numpy()[:db.a.nnz], db.a.colidx.numpy()[:db.a.nnz])
        assert np.array_equal(_bits(hbatch.e.numpy()), _bits(db.e.numpy()))                         # the rule changed no value
        preset = [v.ptr for v in db.a.transpose_perm()]
        assert preset == [dev._bufs.rowptr_t.ptr, dev._bufs.colidx_t.ptr, dev._bufs.perm_t.ptr]
        m.loss_and_grads(db)
        assert [v.ptr for v in m._op(db)[1].transpose_perm()] == preset                             # the preset views are used
        la_d, g_d = m.loss_acc.numpy(), m.gradients()
        assert rel_err(la_d[0], la_h[0]) < TIGHT and la_d[1] == la_h[1]
        worst = _cmp_grads(g_d, g_h, TIGHT, "device loader vs host loader")
        print(f"gatv2 loader routes batch {seen}: loss {rel_err(la_d[0], la_h[0]):.2e} worst gradient {worst:.2e}")
        seen += 1
    assert seen == 3


def test_fit_runs_the_gatv2_model_from_device_batches(ctx):
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    mk = lambda part: ListDataset([Graph(x=x, a=a.tocsr(), y=y, e=_loop_mean_features(a.tocsr().indptr, a.tocsr().indices, 2, 7))
                                   for x, a, y in part])
    tr, te = gcnx.DeviceDataset(ctx, mk(raw[:10]), edge_features=True), gcnx.DeviceDataset(ctx, mk(raw[10:]), edge_features=True)
    m = gcnx.GATv2(ctx, heads=4, edge_dim=2, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])

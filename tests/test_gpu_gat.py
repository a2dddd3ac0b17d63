"""GPU tests of GATConv: the kernels of csrc/gat.hip (gcnx_gat_scores, gcnx_gat_aggregate, gcnx_gat_bwd_edges, gcnx_gat_bwd_nodes),
the layer gcnx.GATConv and the model gcnx.GAT -- each against the float64 oracle tests/gat_ref.py, the backward and the model
on the device's side of every kink (the LeakyReLU of the scores included).  Tolerances: TIGHT = 2e-5 for a single fp32 kernel,
1e-4 for a whole step."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import gat_ref as GR
from gpu_frames import SENTINEL, Frame
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SHAPES = [(1, 16), (1, 64), (1, 128), (4, 16), (8, 16), (2, 8), (8, 4)]

# gradients that are analytically zero (see test_gpu_gcn_bn.UNDER_BN): compared relative to the weight gradient named here
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ecoli3(f):
    """synth.ecoli_batch(3, f): 1 659 rows, degrees 8-22 (computed once, never modified); x serves as Hf, unit scale."""
    from gcnx import synth
    hb = synth.ecoli_batch(3, f)
    assert hb.n % 32 != 0 and hb.n > 32
    return hb


def _csr(ctx, hb):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)


def _params(heads, c, seed, scale=1.0):
    """att_src, att_dst ~ N(0, 1) / sqrt(c) (the softmax neither flat nor saturated at unit-scale Hf), a bias, dout."""
    rng = np.random.default_rng(seed)
    att_src, att_dst = ((scale * rng.standard_normal((heads, c)) / np.sqrt(c)).astype(np.float32) for _ in range(2))
    return att_src, att_dst, rng.standard_normal(heads * c).astype(np.float32)


class _Dev:
    """The device side of one layer evaluation: operands uploaded once, every kernel callable on them."""

    def __init__(self, ctx, a, hf, att_src, att_dst, bias, slope=0.2):
        self.ctx, self.a, self.slope = ctx, a, slope
        self.heads, self.c = att_src.shape
        self.n, self.hc = hf.shape
        self.hf = hf if hasattr(hf, "ptr") else ctx.to_device(hf)
        self.att_src, self.att_dst = ctx.to_device(att_src), ctx.to_device(att_dst)
        self.bias = ctx.to_device(bias) if bias is not None else None
        self.asrc, self.adst = ctx.empty((self.n, self.heads)), ctx.empty((self.n, self.heads))

    def scores(self):
        from gcnx import device as D
        D.gat_scores(self.ctx, self.hf, self.att_src, self.att_dst, self.asrc, self.adst)
        return self.asrc.numpy(), self.adst.numpy()

    def aggregate(self, alpha=True, o_pre=True, bias=True, out=None, o=None):
        from gcnx import device as D
        ctx = self.ctx
        self.out = out if out is not None else ctx.empty((self.n, self.hc))
        self.alpha = ctx.zeros((self.a.nnz, self.heads)) if alpha else None
        self.o = (o if o is not None else ctx.empty((self.n, self.hc))) if o_pre else None
        D.gat_aggregate(ctx, self.a, self.hf, self.asrc, self.adst, self.bias if bias else None, self.out, alpha=self.alpha, o_pre=self.o,
                        slope=self.slope)
        return self.out.numpy(), (self.alpha.numpy() if self.alpha is not None else None), (self.o.numpy() if self.o is not None else None)

    def bwd_edges(self, dout, from_out=False):
        from gcnx import device as D
        ctx = self.ctx
        self.dout = dout if hasattr(dout, "ptr") else ctx.to_device(dout)
        self.dz, self.dadst = ctx.zeros((self.a.nnz, self.heads)), ctx.empty((self.n, self.heads))
        D.gat_bwd_edges(ctx, self.a, self.hf, self.asrc, self.adst, self.alpha, self.dout, self.out if from_out else self.o, self.dz,
                        self.dadst, o_bias=self.bias if from_out else None, slope=self.slope)
        return self.dz.numpy(), self.dadst.numpy()

    def bwd_nodes(self, dhf=None):
        from gcnx import device as D
        ctx = self.ctx
        self.dhf = dhf if dhf is not None else ctx.empty((self.n, self.hc))
        self.dasrc = ctx.empty((self.n, self.heads))
        self.datt_src, self.datt_dst = ctx.empty((self.heads, self.c)), ctx.empty((self.heads, self.c))
        scratch = ctx.empty(max(D.gat_bwd_scratch_floats(ctx, self.n, self.heads, self.c), 1))
        D.gat_bwd_nodes(ctx, self.a, self.alpha, self.dz, self.dout, self.hf, self.dadst, self.att_src, self.att_dst, self.dhf, self.dasrc,
                        self.datt_src, self.datt_dst, scratch)
        return self.dhf.numpy(), self.dasrc.numpy(), self.datt_src.numpy(), self.datt_dst.numpy()


def _oracle(rowptr, colidx, hf, att_src, att_dst, bias, dout=None, sides=None, slope=0.2):
    """gat_ref on Hf directly (x = Hf, W = I); with dout the backward too (its pieces are left in the cache)."""
    out, cache = GR.gat_conv_fwd(rowptr, colidx, hf, np.eye(hf.shape[1]), att_src, att_dst, bias, slope, sides)
    if dout is not None:
        cache["grads"] = GR.gat_conv_bwd(cache, dout)
    return out, cache


def _check_all(ctx, a, rowptr, colidx, hf, heads, c, seed, what, tol=TIGHT, scale=1.0):
    """Every kernel on one input against the oracle; returns the device object and the errors (printed before asserting)."""
    att_src, att_dst, bias = _params(heads, c, seed, scale)
    dout = np.random.default_rng(seed + 1).standard_normal(hf.shape).astype(np.float32)
    d = _Dev(ctx, a, hf, att_src, att_dst, bias)
    asrc, adst = d.scores()
    out, alpha, o = d.aggregate()
    dz, dadst = d.bwd_edges(dout)
    dhf, dasrc, das, dad = d.bwd_nodes()
    sides = GR.device_score_sides(asrc, adst, rowptr, colidx)
    r_out, k = _oracle(rowptr, colidx, hf, att_src, att_dst, bias, dout, sides)
    n, hc = hf.shape
    errs = {"a_src": rel_err(asrc, k["a_src"]), "a_dst": rel_err(adst, k["a_dst"]), "out": rel_err(out, r_out),
            "alpha": rel_err(alpha, k["alpha"]), "o_pre": rel_err(o, k["O"].reshape(n, hc)), "dz": rel_err(dz, k["dz"]),
            "da_dst": rel_err(dadst, k["da_dst"]), "dhf": rel_err(dhf, k["dHf"]), "da_src": rel_err(dasrc, k["da_src"]),
            "datt_src": rel_err(das, k["grads"][2]), "datt_dst": rel_err(dad, k["grads"][3])}
    print(f"gat {what} heads={heads} c={c}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert np.isfinite(out).all() and np.isfinite(alpha).all() and np.isfinite(dhf).all()
    for key, v in errs.items():
        assert v < tol, (what, key, v)
    d.host = dict(asrc=asrc, adst=adst, out=out, alpha=alpha, o=o, dz=dz, dadst=dadst, dhf=dhf, dasrc=dasrc, das=das, dad=dad,
                  att_src=att_src, att_dst=att_dst, bias=bias, dout=dout, ref=k, r_out=r_out)
    return d


# ---- 1. the kernels against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,c", SHAPES)
def test_gat_kernels_against_float64(ctx, heads, c):
    from gcnx import device as D
    hb = _ecoli3(heads * c)
    a = _csr(ctx, hb)
    assert D.gat_conv_ok(ctx, hb.n, heads, c)
    d = _check_all(ctx, a, hb.rowptr, hb.colidx, hb.x, heads, c, 100 * heads + c, "ecoli-3")
    h = d.host
    sums = np.add.reduceat(h["alpha"].astype(np.float64), hb.rowptr[:-1].astype(np.int64))
    assert np.diff(hb.rowptr).min() > 0 and np.max(np.abs(sums - 1.0)) < 1e-6, np.max(np.abs(sums - 1.0))
    # no atomics: a second call of each leaves the same bits
    asrc2, adst2 = d.scores()
    out2, alpha2, o2 = d.aggregate()
    dz2, dadst2 = d.bwd_edges(h["dout"])
    second = (asrc2, adst2, out2, alpha2, o2, dz2, dadst2) + d.bwd_nodes()
    first = tuple(h[k] for k in ("asrc", "adst", "out", "alpha", "o", "dz", "dadst", "dhf", "dasrc", "das", "dad"))
    for k, (x, y) in enumerate(zip(first, second)):
        assert np.array_equal(_bits(x), _bits(y)), k
    # alpha = NULL, o_pre = NULL and bias = NULL give the same out bits (minus the bias)
    out3, alpha3, o3 = d.aggregate(alpha=False, o_pre=False)
    assert alpha3 is None and o3 is None and np.array_equal(_bits(out3), _bits(h["out"]))
    out4, _, _ = d.aggregate(alpha=False, o_pre=False, bias=False)
    assert np.array_equal(_bits(out4 + h["bias"]), _bits(h["out"])) and np.array_equal(_bits(out4), _bits(h["o"]))
    # without o_pre the backward takes out and the bias
    d.aggregate()
    dz5, dadst5 = d.bwd_edges(h["dout"], from_out=True)
    assert rel_err(dz5, h["ref"]["dz"]) < TIGHT and rel_err(dadst5, h["ref"]["da_dst"]) < TIGHT


# ---- 2. degenerate inputs -------------------------------------------------------------------------------------------------
def _edge_case_csr():
    """The 56-row construction of test_gpu_sage._edge_case_csr: graphs of [1, 3, 1, 7, 2, 1, 40, 1] rows, rows 4 and 20
    without entries, a directed pattern."""
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
    assert rowptr[5] == rowptr[4] and rowptr[21] == rowptr[20] and n == 56
    return rowptr, cols.astype(np.int32), gp


@pytest.mark.parametrize("heads,c", [(4, 8), (1, 16)])
def test_gat_kernels_degenerate_inputs(ctx, heads, c):
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _edge_case_csr()
    n, hc = 56, heads * c
    hf = np.random.default_rng(7 + heads).standard_normal((n, hc), dtype=np.float32)
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp, symmetric=False)
    assert not a.symmetric
    d = _check_all(ctx, a, rowptr, colidx, hf, heads, c, 31, "56 rows")
    h = d.host
    assert np.array_equal(_bits(h["out"][[4, 20]]), _bits(np.broadcast_to(h["bias"], (2, hc))))      # no entries: the bias, bit for bit
    assert not h["o"][[4, 20]].any() and not h["dadst"][[4, 20]].any()
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:rowptr[5]], None, gp[:4].copy(), symmetric=False)
    _check_all(ctx, a5, rowptr[:6], colidx[:rowptr[5]], hf[:5], heads, c, 32, "5 rows")
    # one row with only its self-loop: alpha == 1 exactly, out == Hf + bias bit for bit
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), None, one, symmetric=True)
    d1 = _check_all(ctx, a1, one, np.zeros(1, np.int32), hf[:1], heads, c, 33, "1 row, self-loop")
    assert np.array_equal(d1.host["alpha"], np.ones((1, heads), np.float32))
    assert np.array_equal(_bits(d1.host["out"]), _bits(hf[:1] + d1.host["bias"]))
    # one row without any entry (the stored entry is in no row)
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), None, one, symmetric=True)
    att_src, att_dst, bias = _params(heads, c, 34)
    d0 = _Dev(ctx, a0, hf[:1], att_src, att_dst, bias)
    d0.scores()
    out0, _, o0 = d0.aggregate()
    assert np.array_equal(_bits(out0), _bits(bias[None])) and not o0.any()
    _, dadst0 = d0.bwd_edges(hf[:1])                                    # (no transposed pattern of a CSR whose entry is in no row)
    assert not dadst0.any()


# ---- 3. rows longer than the staged entries ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hub():
    from gcnx import synth
    hb = synth.power_law_batch(n_graphs=1, graph_size=8192, f=64, seed=3)
    assert int(np.diff(hb.rowptr).max()) >= 4096                         # past the 1024 staged entries of a tile
    return hb


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_kernels_long_rows(ctx, heads):
    hb = _hub()
    a = _csr(ctx, hb)
    _check_all(ctx, a, hb.rowptr, hb.colidx, hb.x, heads, 64 // heads, 11 + heads, "hub")     # (the transposed pattern has the same hub rows)


# ---- 4. the range of the exponential ----------------------------------------------------------------------------------------
def test_gat_scaled_scores_give_near_one_hot_rows(ctx):
    hb = _ecoli3(64)
    d = _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, hb.x, 4, 16, 41, "scores x 30", scale=30.0)
    top = np.maximum.reduceat(d.host["alpha"], hb.rowptr[:-1].astype(np.int64))
    assert np.median(top) > 0.99                                          # near one-hot


@pytest.mark.parametrize("shift", [200.0, -200.0])
def test_gat_shifted_scores_stay_finite(ctx, shift):
    """a_src shifted by +-200 between the two launches.  Without the max subtraction +200 overflows exp to inf (asserted below
    for fp32); -200 puts every score at e = 0.2 z near -40, where a sum of un-shifted weights keeps 1e-18 of its range."""
    hb = _ecoli3(64)
    heads, c = 4, 16
    att_src, att_dst, bias = _params(heads, c, 43)
    d = _Dev(ctx, _csr(ctx, hb), hb.x, att_src, att_dst, bias)
    asrc, adst = d.scores()
    asrc_s = (asrc + np.float32(shift)).astype(np.float32)
    d.asrc = ctx.to_device(asrc_s)
    out, alpha, o = d.aggregate()
    hf3 = hb.x.astype(np.float64).reshape(hb.n, heads, c)
    r_o, r_alpha, _, _ = GR.softmax_aggregate(hb.rowptr, hb.colidx, hf3, asrc_s, adst)
    r_out = r_o.reshape(hb.n, -1) + bias
    errs = rel_err(out, r_out), rel_err(alpha, r_alpha), rel_err(o, r_o.reshape(hb.n, -1))
    print(f"gat shift {shift}: out {errs[0]:.2e} alpha {errs[1]:.2e} o_pre {errs[2]:.2e}")
    assert np.isfinite(out).all() and np.isfinite(alpha).all() and np.isfinite(o).all()
    assert max(errs) < TIGHT, errs
    with np.errstate(over="ignore"):
        assert shift < 0 or np.exp(np.float32(150.0)) == np.inf            # what a kernel without the subtraction would sum


# ---- 5. strided operands ------------------------------------------------------------------------------------------------
def _frame_check(fr, want, tol, what):
    got = fr.buf.numpy()
    body = fr._body(got)
    assert rel_err(body[:, :fr.f], want) < tol, (what, rel_err(body[:, :fr.f], want))
    assert (body[:, fr.f:] == SENTINEL).all() and (got[:fr.lead] == SENTINEL).all() \
        and (got[fr.lead + fr.n * fr.ld:] == SENTINEL).all(), (what, "written outside the view")


def test_gat_strided_operands(ctx):
    from gcnx import device as D
    heads, c = 4, 8
    hc = heads * c
    hb = _ecoli3(hc)
    a = _csr(ctx, hb)
    att_src, att_dst, bias = _params(heads, c, 51)
    dout = np.random.default_rng(52).standard_normal(hb.x.shape).astype(np.float32)
    fh = Frame(ctx, hb.n, hc, 2 * hc, 4, data=hb.x)                     # Hf: a column slice of an array twice as wide
    f_out, f_o, f_dhf = Frame(ctx, hb.n, hc, hc + 8, 8), Frame(ctx, hb.n, hc, hc + 4, 12), Frame(ctx, hb.n, hc, hc + 12, 4)
    f_do = Frame(ctx, hb.n, hc, hc + 4, 4, data=dout)
    assert all(f.aligned() for f in (fh, f_out, f_o, f_dhf, f_do)) and D.gat_conv_ok(ctx, hb.n, heads, c, fh.view.ld)
    d = _Dev(ctx, a, fh.view, att_src, att_dst, bias)
    asrc, adst = d.scores()
    _, alpha, _ = d.aggregate(out=f_out.view, o=f_o.view)
    dz, dadst = d.bwd_edges(f_do.view)
    d.bwd_nodes(dhf=f_dhf.view)
    r_out, k = _oracle(hb.rowptr, hb.colidx, hb.x, att_src, att_dst, bias, dout, GR.device_score_sides(asrc, adst, hb.rowptr, hb.colidx))
    assert rel_err(asrc, k["a_src"]) < TIGHT and rel_err(alpha, k["alpha"]) < TIGHT and rel_err(dz, k["dz"]) < TIGHT
    _frame_check(f_out, r_out, TIGHT, "out")
    _frame_check(f_o, k["O"].reshape(hb.n, hc), TIGHT, "o_pre")
    _frame_check(f_dhf, k["dHf"], TIGHT, "dhf")
    assert rel_err(d.datt_src.numpy(), k["grads"][2]) < TIGHT and rel_err(d.dasrc.numpy(), k["da_src"]) < TIGHT
    fh.check(hb.x, "hf is not written")
    f_do.check(dout, "d_out is not written")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_gat_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb = _ecoli3(16)
    a = _csr(ctx, hb)
    n, nnz = hb.n, a.nnz

    def refused(hf, heads, c):
        hc = heads * c
        att = ctx.zeros((heads, c))
        s1, s2 = Frame(ctx, n, heads, heads, 0), Frame(ctx, n, heads, heads, 0)
        out, o, dhf = Frame(ctx, n, hc, hc, 0), Frame(ctx, n, hc, hc, 0), Frame(ctx, n, hc, hc, 0)
        alpha, dz = Frame(ctx, nnz, heads, heads, 0), Frame(ctx, nnz, heads, heads, 0)
        datt = Frame(ctx, heads, c, c, 0)
        dense = ctx.zeros((n, hc))
        scratch = ctx.zeros(max(D.gat_bwd_scratch_floats(ctx, n, heads, c), 1) + 4 * n)
        calls = (lambda: D.gat_scores(ctx, hf, att, att, s1.view, s2.view),
                 lambda: D.gat_aggregate(ctx, a, hf, s1.view, s2.view, None, out.view, alpha=alpha.view, o_pre=o.view),
                 lambda: D.gat_bwd_edges(ctx, a, hf, s1.view, s2.view, alpha.view, dense, dense, dz.view, s1.view),
                 lambda: D.gat_bwd_nodes(ctx, a, alpha.view, dz.view, hf, dense, s1.view, att, att, dhf.view, s2.view, datt.view, datt.view,
                                         scratch))
        for call in calls:
            with pytest.raises(_lib.GcnxError) as e:
                call()
            assert e.value.code == _lib.ERR_UNSUPPORTED
        for fr in (s1, s2, out, o, dhf, alpha, dz, datt):
            fr.check(np.full((fr.n, fr.f), SENTINEL), "a refused call writes nothing")

    for heads, c in ((3, 16), (1, 96), (8, 32), (8, 2)):
        assert not D.gat_conv_ok(ctx, n, heads, c)
        refused(ctx.zeros((n, heads * c)), heads, c)
    wide = ctx.zeros((n, 18))
    assert not D.gat_conv_ok(ctx, n, 1, 16, 18)
    refused(DeviceArray(ctx, wide.ptr, (n, 16), np.float32, ld=18, base=wide), 1, 16)            # ld % 4 != 0
    off = Frame(ctx, n, 16, 16, 1, data=hb.x)                                                    # one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4 and D.gat_conv_ok(ctx, n, 1, 16)
    refused(off.view, 1, 16)
    # n = 0: nothing to do, no error; n = -1 and NULL mandatory pointers: invalid arguments
    lib = ctx.lib
    hf, att, s, out = ctx.zeros((4, 16)), ctx.zeros((1, 16)), Frame(ctx, 4, 1, 1, 0), Frame(ctx, 4, 16, 16, 0)
    al, big = Frame(ctx, 16, 1, 1, 0), ctx.zeros(64)
    rp, ci = a.rowptr.ptr, a.colidx.ptr

    def call_all(nn, hfp):
        return (lib.gcnx_gat_scores(ctx.h, hfp, 16, nn, 1, 16, att.ptr, att.ptr, s.view.ptr, s.view.ptr),
                lib.gcnx_gat_aggregate(ctx.h, rp, ci, hfp, 16, nn, 1, 16, s.view.ptr, s.view.ptr, None, 0.2, out.view.ptr, 16, al.view.ptr,
                                       None, 0),
                lib.gcnx_gat_bwd_edges(ctx.h, rp, ci, hfp, 16, nn, 1, 16, s.view.ptr, s.view.ptr, 0.2, al.view.ptr, hf.ptr, 16, hf.ptr, 16,
                                       None, al.view.ptr, s.view.ptr),
                lib.gcnx_gat_bwd_nodes(ctx.h, rp, ci, ci, nn, 1, 16, al.view.ptr, al.view.ptr, hf.ptr, 16, hfp, 16, s.view.ptr, att.ptr,
                                       att.ptr, out.view.ptr, 16, s.view.ptr, big.ptr, big.ptr, big.ptr))

    assert call_all(0, hf.ptr) == (_lib.OK,) * 4
    assert call_all(-1, hf.ptr) == (1,) * 4                                                     # GCNX_ERR_INVALID
    assert call_all(4, None) == (1,) * 4
    for fr in (s, out, al):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "n = 0 and invalid calls write nothing")
    assert not big.numpy().any()


# ---- 7. capture -----------------------------------------------------------------------------------------------------------
def test_gat_captured_replay_is_bit_identical(ctx):
    from gcnx import device as D
    heads, c = 4, 16
    hb = _ecoli3(64)
    a = _csr(ctx, hb)
    att_src, att_dst, bias = _params(heads, c, 61)
    d = _Dev(ctx, a, hb.x, att_src, att_dst, bias)
    d.scores()
    out_e, alpha_e, o_e = d.aggregate()
    out, alpha, o = ctx.zeros((hb.n, 64)), ctx.zeros((a.nnz, heads)), ctx.zeros((hb.n, 64))
    asrc, adst = ctx.zeros((hb.n, heads)), ctx.zeros((hb.n, heads))

    def seq():                                                           # a linear graph: two launches, no parallel branch
        D.gat_scores(ctx, d.hf, d.att_src, d.att_dst, asrc, adst)
        D.gat_aggregate(ctx, a, d.hf, asrc, adst, d.bias, out, alpha=alpha, o_pre=o)

    g = ctx.capture(seq)
    try:
        assert not out.numpy().any()                                     # captured, not yet executed
        for _ in range(2):
            for t in (out, alpha, o, asrc, adst):
                t.fill_zero()
            g.launch()
            assert np.array_equal(_bits(out.numpy()), _bits(out_e)) and np.array_equal(_bits(alpha.numpy()), _bits(alpha_e))
            assert np.array_equal(_bits(o.numpy()), _bits(o_e)) and np.array_equal(_bits(asrc.numpy()), _bits(d.asrc.numpy()))
    finally:
        g.destroy()


# ---- 8. the layer ---------------------------------------------------------------------------------------------------------
def test_gatconv_layer_forward_and_backward(ctx):
    from gcnx.layers import GATConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    lay = GATConv(16, heads=4, seed=3)
    pre = GATConv.preprocess(a)
    assert pre.vals is None and pre.nnz == a.nnz
    lay.build(ctx, 16)
    assert list(lay.params) == ["att_src", "att_dst", "bias", "lin.weight"]
    assert not lay.params["bias"].numpy().any()
    lay.params["bias"].copy_from_host(np.random.default_rng(1).standard_normal(64).astype(np.float32))
    x = ctx.to_device(hb.x)
    y = lay([x, pre])
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    sd = lay.state_dict()
    assert sd["att_src"].shape == sd["att_dst"].shape == (1, 4, 16) and sd["lin.weight"].shape == (64, 16) and sd["bias"].shape == (64,)
    _, _, _, asrc, adst, _, _ = lay._saved
    sides = GR.device_score_sides(asrc.numpy(), adst.numpy(), hb.rowptr, hb.colidx)
    r_y, k = GR.gat_conv_fwd(hb.rowptr, hb.colidx, hb.x, p["lin.weight"], p["att_src"], p["att_dst"], p["bias"], 0.2, sides)
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r_dx, r_dw, r_das, r_dad, r_db = GR.gat_conv_bwd(k, dy)
    assert rel_err(dx.numpy(), r_dx) < TIGHT
    g = lay.grads
    assert rel_err(g["lin.weight"].numpy(), r_dw) < TIGHT and rel_err(g["bias"].numpy(), r_db) < TIGHT
    assert rel_err(g["att_src"].numpy(), r_das) < TIGHT and rel_err(g["att_dst"].numpy(), r_dad) < TIGHT
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    with pytest.raises(NotImplementedError):
        GATConv(24, heads=4)([x, pre])                                   # HC = 96: no kernel and no composed route


# ---- 9. gcnx.GAT: a full step against the kink-separated oracle -------------------------------------------------------------
def _sides(m, hb, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    s = {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
         for i in (1, 2)}
    s.update({f"e{i}": GR.device_score_sides(b[f"asrc{i}"].numpy(), b[f"adst{i}"].numpy(), hb.rowptr, hb.colidx) for i in (1, 2)})
    return s


@pytest.mark.parametrize("shape", ["config1", "config2"])
@pytest.mark.parametrize("heads", [1, 4])
def test_gat_step_against_oracle(ctx, heads, shape):
    import gcnx
    from gcnx import synth
    hb = _tiny_host(16, 16, seed=4) if shape == "config1" else synth.ecoli_batch(f=16)
    batch = _device_batch(ctx, hb)
    m = gcnx.GAT(ctx, hidden_channels=64, heads=heads, seed=0)
    p = {k: v.astype(np.float32) for k, v in GR.init_params(16, 64, heads, seed=7).items()}
    m.load_state_dict(p)
    a = _scipy_adj(hb)
    what = f"{shape} heads={heads}"
    m.loss_and_grads(batch)
    for k in ("hf1", "hf2", "asrc1", "adst1", "asrc2", "adst2", "alpha1", "alpha2", "o1", "o2", "dz", "dadst", "dasrc", "dhf", "scratch"):
        assert k in m._bufs, k
    assert m._bufs["alpha1"].shape == (hb.nnz, heads) and m._bufs["dz"].shape == (hb.nnz, heads)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = GR.model(hb.x, a, hb.graph_ptr, p, hb.y, masks=_sides(m, hb), argmax=arg, heads=heads)
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < 1e-4 and la[1] == r["hits"], (la, r["loss"], r["hits"])
    _cmp_grads(m.gradients(), r["grads"], 1e-4, what)
    # five SGD steps, each oracle step on the device's kink sides of that step (taken with the step's own weights)
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    for _ in range(5):
        pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
        m.train_step(batch, lr=0.02)
        arg = m._bufs["arg"].numpy().astype(np.int64)
        r = GR.model(hb.x, a, hb.graph_ptr, ph, hb.y, masks=_sides(m, hb, pre), argmax=arg, heads=heads)
        ph = GR.sgd(ph, r["grads"], 0.02)
    sd = m.state_dict()
    for k in GR.KEYS:
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after 5 steps {k}")


# ---- 10. torch-style surface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [1, 4])
def test_gat_forward_state_dict_and_single_graph(ctx, heads):
    import gcnx
    import scipy.sparse as sp
    hb = _tiny_host(8, 16, seed=6)
    m = gcnx.GAT(ctx, heads=heads, seed=1)
    ids, a = hb.ids(), _scipy_adj(hb)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1)
    r = GR.model(hb.x, a, hb.graph_ptr, m.state_dict(), masks=_sides(m, hb), argmax=m._bufs["arg"].numpy().astype(np.int64), heads=heads)
    assert_close(logits, r["out"], 1e-4, "logits")
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    sd = m.state_dict()
    assert list(sd) == list(GR.KEYS)
    c = 64 // heads
    assert sd["conv1.att_src"].shape == sd["conv2.att_dst"].shape == (1, heads, c) and sd["conv1.bias"].shape == (64,)
    assert sd["conv1.lin.weight"].shape == (64, 16) and sd["conv2.lin.weight"].shape == (64, 64) and sd["linear_2.weight"].shape == (1, 64)
    assert not sd["conv1.bias"].any() and np.max(np.abs(sd["conv1.att_src"])) <= np.sqrt(6 / (heads + c))      # zero bias, glorot
    assert np.max(np.abs(sd["conv1.lin.weight"])) <= np.sqrt(6 / 80) and np.max(np.abs(sd["conv2.lin.weight"])) <= np.sqrt(6 / 128)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    m2 = gcnx.GAT(ctx, heads=heads, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(_bits(v), _bits(sd[k])), k
    assert np.array_equal(m2((hb.x, a, ids)), logits)
    assert [w.shape for w in m.get_weights()] == [sd[k].shape for k in GR.KEYS]
    assert [g.shape for g in m.gradients().values()] == [sd[k].shape for k in GR.KEYS]
    # the loops are re-added (unlike SAGE): a host matrix stripped of its stored self-loops is the same graph
    a_noloop = sp.csr_matrix(a - sp.diags(a.diagonal()))
    a_noloop.eliminate_zeros()
    assert a_noloop.nnz < a.nnz and np.array_equal(m((hb.x, a_noloop, ids)), logits)
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


# ---- 11. sync-BN over graph shards ----------------------------------------------------------------------------------------
def test_gat_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in GR.init_params(16, 64, 4, seed=7).items()}

    def step(ctx, part, comm, gb):
        m = gcnx.GAT(ctx, hidden_channels=64, heads=4, seed=0, comm=comm)
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


# ---- 12. gcnx.fit -----------------------------------------------------------------------------------------------------------
def test_fit_runs_the_gat_model(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:10]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[10:]])
    m = gcnx.GAT(ctx, heads=4, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])

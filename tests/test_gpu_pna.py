"""GPU tests of PNAConv: gcnx_pna_aggregate and gcnx_pna_bwd (csrc/pna.hip), the layer gcnx.PNAConv and the model gcnx.PNA,
each against the float64 oracle tests/pna_ref.py, the model on the device's side of every PReLU and pooling kink.
Every bound is TIGHT = 2e-5, max-norm relative against float64, taken per output block (a block of C, of the statistics, dP,
dQ, one parameter's gradient)."""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
import gcn_bn_ref as R
import pna_ref as PR
from gpu_frames import Frame
from test_gpu_gcn_bn import _device_batch, _scipy_adj, _tiny_host
from test_gpu_gin import _hub

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from thread_comm import ThreadWorld  # noqa: E402

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
STD0 = np.sqrt(np.float32(1e-5))                           # the std of a row whose entries are all equal, in fp32

# gradients that are analytically zero (a bias in front of a BatchNorm; see test_gpu_gcn_bn.UNDER_BN): compared relative to
# the weight gradient named here
UNDER_BN = {"conv1.lin.bias": "conv1.lin.weight", "conv2.lin.bias": "conv2.lin.weight",
            "conv1.post_nns.0.0.bias": "conv1.post_nns.0.0.weight", "conv2.post_nns.0.0.bias": "conv2.post_nns.0.0.weight",
            "linear_1.bias": "linear_1.weight", "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _blocks(a, f):
    return [a[:, k * f:(k + 1) * f] for k in range(a.shape[1] // f)]


@functools.lru_cache(maxsize=None)
def _host(kind, f):
    """A small batch of pna_ref.graphs as (HostBatch, rowptr, colidx): empty rows, d = 1 rows, a single-node graph and
    duplicated feature rows (computed once, never modified)."""
    from gcnx import synth
    x, a, gp, y = PR.graphs(kind, n_graphs=6, f=f, seed=11 if kind == "directed" else 12, lo=8, hi=24)
    rp, ci = PR.pattern(a, x.shape[0])
    hb = synth.HostBatch(x.astype(np.float32), rp.astype(np.int32), ci.astype(np.int32), None, gp.astype(np.int32), y.astype(np.float32))
    d = np.diff(rp)
    assert (d == 0).any() and (d == 1).any() and 1 in np.diff(gp) and hb.n > 32
    return hb, rp, ci


def _csr(ctx, hb):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr).unweighted()


def _tied_pq(rng, x, f, offset=0.0):
    """pq [n, 2f] in fp32 whose Q rows repeat wherever the rows of x repeat: exact ties of minima and maxima."""
    _, inv = np.unique(x, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    q = (offset + rng.standard_normal((int(inv.max()) + 1, f)))[inv]
    return np.concatenate([rng.standard_normal((x.shape[0], f)), q], axis=1).astype(np.float32)


def _fwd(ctx, a, x, pq, delta, keep=True):
    from gcnx import device as D
    n, f = x.shape
    c, stats = ctx.empty((n, 13 * f)), ctx.empty((n, 6 * f)) if keep else None
    D.pna_aggregate(ctx, a, ctx.to_device(x), ctx.to_device(pq), delta, c, stats)
    return c.numpy(), (stats.numpy() if keep else None)


def _bwd(ctx, a, pq, stats, dc, delta):
    from gcnx import device as D
    n, f = pq.shape[0], pq.shape[1] // 2
    dpq = ctx.empty((n, 2 * f))
    ns = D.pna_bwd_scratch_floats(ctx, n, f)
    assert ns == 4 * n * f
    D.pna_bwd(ctx, a, a.transpose(), ctx.to_device(pq), ctx.to_device(stats), ctx.to_device(dc), delta, dpq, ctx.empty(ns))
    return dpq.numpy()


def _check_fwd(c, stats, r_c, r_stats, f, what):
    errs = [rel_err(g, r) for g, r in zip(_blocks(c, f), _blocks(r_c, f))]
    e_st = [rel_err(g, r) for g, r in zip(_blocks(stats, f)[:4], _blocks(r_stats, f)[:4])]
    print(f"{what}: C blocks max {max(errs):.2e} (std blocks {errs[4]:.2e} {errs[8]:.2e} {errs[12]:.2e}), stats {max(e_st):.2e}")
    assert max(errs) < TIGHT and max(e_st) < TIGHT, (what, errs, e_st)
    assert np.array_equal(stats[:, 4 * f:], r_stats[:, 4 * f:]), (what, "tie counts")


# ---- 1. the two entry points against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["symmetric", "directed"])
@pytest.mark.parametrize("f", [1, 3, 16, 64, 70, 128])
def test_pna_aggregate_and_bwd_against_float64(ctx, f, kind):
    hb, rp, ci = _host(kind, f)
    a = _csr(ctx, hb)
    rng = np.random.default_rng(100 * f + (kind == "directed"))
    pq, delta = _tied_pq(rng, hb.x, f), np.float32(1.7)
    c, stats = _fwd(ctx, a, hb.x, pq, delta)
    r_c, r_stats = PR.aggregate(rp, ci, hb.x, pq, delta)
    _check_fwd(c, stats, r_c, r_stats, f, f"pna_aggregate f={f} {kind}")
    d = np.diff(rp)
    assert r_stats[:, 4 * f:].max() >= 2                                  # ties are exercised
    assert np.array_equal(_bits(c[:, :f]), _bits(hb.x))                    # block 0: the copy of x
    assert np.array_equal(_bits(stats[d <= 1, 3 * f:4 * f]), _bits(np.full(((d <= 1).sum(), f), STD0)))   # d = 0, 1: sqrt(1e-5) exactly
    assert np.all(c[d == 0, f:4 * f] == 0) and np.all(stats[d == 0, :3 * f] == 0) and np.all(stats[d == 0, 4 * f:] == 0)
    c2, none = _fwd(ctx, a, hb.x, pq, delta, keep=False)                  # stats = NULL: the same C bits
    assert none is None and np.array_equal(_bits(c2), _bits(c))
    dc = rng.standard_normal((hb.n, 13 * f)).astype(np.float32)
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    r_dpq, _ = PR.aggregate_bwd(rp, ci, pq, r_stats, dc, delta)
    e_dp, e_dq = rel_err(dpq[:, :f], r_dpq[:, :f]), rel_err(dpq[:, f:], r_dpq[:, f:])
    print(f"pna_bwd f={f} {kind}: dP {e_dp:.2e} dQ {e_dq:.2e}")
    assert e_dp < TIGHT and e_dq < TIGHT
    assert np.all(dpq[d == 0, :f] == 0)
    assert np.array_equal(_bits(_bwd(ctx, a, pq, stats, dc, delta)), _bits(dpq))      # no atomics: the same bits again
    dc[:, :f] = 7.0                                                       # block 0 of dC is not an operand
    assert np.array_equal(_bits(_bwd(ctx, a, pq, stats, dc, delta)), _bits(dpq))


# ---- 2. exact ties ---------------------------------------------------------------------------------------------------------
def test_pna_exact_ties_share_the_gradient_evenly(ctx):
    from gcnx.device import DeviceCSR
    n, f = 7, 8
    # row 0 gathers rows 1 .. 5: rows 1, 2 tie for the minimum, rows 3, 4, 5 for the maximum; row 6 gathers 1 and 2 (all tied)
    rp = np.array([0, 5, 5, 5, 5, 5, 5, 7], np.int32)
    ci = np.array([1, 2, 3, 4, 5, 1, 2], np.int32)
    rng = np.random.default_rng(3)
    lo, hi = rng.standard_normal(f).astype(np.float32) - 3, rng.standard_normal(f).astype(np.float32) + 3
    pq = rng.standard_normal((n, 2 * f)).astype(np.float32)
    pq[1:3, f:], pq[3:6, f:] = lo, hi
    x = rng.standard_normal((n, f)).astype(np.float32)
    a = DeviceCSR.from_host_csr(ctx, rp, ci, None, np.array([0, n], np.int32)).unweighted()
    delta = np.float32(1.1)
    c, stats = _fwd(ctx, a, x, pq, delta)
    r_c, r_stats = PR.aggregate(rp.astype(np.int64), ci.astype(np.int64), x, pq, delta)
    _check_fwd(c, stats, r_c, r_stats, f, "pna_aggregate ties")
    cmin, cmax = stats[:, 4 * f:5 * f], stats[:, 5 * f:]
    assert np.all(cmin[0] == 2) and np.all(cmax[0] == 3) and np.all(cmin[6] == 2) and np.all(cmax[6] == 2) and np.all(cmin[1:6] == 0)
    assert np.array_equal(_bits(stats[6, 3 * f:4 * f]), _bits(np.full(f, STD0)))       # all entries equal: var = 0 exactly
    dc = np.zeros((n, 13 * f), np.float32)
    g_min, g_max = rng.standard_normal(f).astype(np.float32), rng.standard_normal(f).astype(np.float32)
    dc[0, 2 * f:3 * f], dc[0, 3 * f:4 * f] = g_min, g_max                  # the identity scaler's min and max blocks of row 0
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    dq = dpq[:, f:]
    assert np.array_equal(_bits(dq[1]), _bits(g_min / np.float32(2))) and np.array_equal(_bits(dq[2]), _bits(dq[1]))
    assert np.array_equal(_bits(dq[3]), _bits(g_max / np.float32(3))) and np.array_equal(_bits(dq[4]), _bits(dq[3])) \
        and np.array_equal(_bits(dq[5]), _bits(dq[3]))
    assert np.all(dq[0] == 0) and np.all(dq[6] == 0) and np.array_equal(_bits(dpq[0, :f]), _bits(g_min + g_max)) and np.all(dpq[1:, :f] == 0)
    r_dpq, _ = PR.aggregate_bwd(rp.astype(np.int64), ci.astype(np.int64), pq, r_stats, dc, delta)
    assert rel_err(dpq, r_dpq) < TIGHT
    # row 6 (all entries equal): the std carries no gradient, the tied minimum and maximum split theirs
    dc[:] = rng.standard_normal(dc.shape).astype(np.float32)
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    r_dpq, _ = PR.aggregate_bwd(rp.astype(np.int64), ci.astype(np.int64), pq, r_stats, dc, delta)
    assert rel_err(dpq[:, :f], r_dpq[:, :f]) < TIGHT and rel_err(dpq[:, f:], r_dpq[:, f:]) < TIGHT


# ---- 3. a large common offset --------------------------------------------------------------------------------------------------
def _emulate_dq_f32(rp, ci, pq, r_stats, dc, delta):
    """The contract expression of dQ evaluated in NumPy float32 from the best statistics fp32 can store (the float64 ones,
    rounded): dQ_j = sum_i g_mean / d + g_min [Q_j = minQ] / cmin + g_max [Q_j = maxQ] / cmax + g_std [max > min] (Q_j - meanQ) / (d std),
    the terms of a source added in the transposed pattern's stored order."""
    f32 = np.float32
    n, f = pq.shape[0], pq.shape[1] // 2
    st = r_stats.astype(f32)
    mean, mn, mx, std, cmin, cmax = (st[:, k * f:(k + 1) * f] for k in range(6))
    d = np.diff(rp)
    amp, att = (v.astype(f32)[:, None] for v in PR.scalers(d, float(delta)))
    g = dc[:, f:5 * f] + amp * dc[:, 5 * f:9 * f] + att * dc[:, 9 * f:13 * f]
    t = np.repeat(np.arange(n), d)
    qe, dd = pq[ci, f:], d[t].astype(f32)[:, None]
    term = g[t, :f] / dd + np.where(qe == mn[t], g[t, f:2 * f] / np.maximum(cmin[t], f32(1)), f32(0)) \
        + np.where(qe == mx[t], g[t, 2 * f:3 * f] / np.maximum(cmax[t], f32(1)), f32(0)) \
        + np.where(mx[t] > mn[t], g[t, 3 * f:] / (dd * std[t]), f32(0)) * (qe - mean[t])
    assert term.dtype == f32
    dq = np.zeros((n, f), f32)
    order = np.argsort(ci, kind="stable")                                   # per source, its targets in ascending order
    for e in order:
        dq[ci[e]] += term[e]
    return dq


def test_pna_offset_case_keeps_the_std(ctx):
    """Q = 100 + N(0, 1): the std block is held to TIGHT (the plain E[q^2] - E[q]^2 form is off by 1e-3 here); the mean, min
    and max blocks are measured against max |Q|, dQ against the largest term of its sum.  dQ does not meet TIGHT on this
    data and cannot from fp32 statistics: meanQ near 100 is stored to 4e-6, and a target whose entries lie close together
    (std 0.006) scales that by g_std / (d std).  The float32 emulation of the contract expression from correctly rounded
    statistics measures 2.13e-04 here and the kernel, on an MI355X, the same 2.13e-04 (the same worst element); the kernel is
    held to 4 x the emulation's error (PNAConv)."""
    f = 64
    hb, rp, ci = _host("symmetric", f)
    a = _csr(ctx, hb)
    rng = np.random.default_rng(5)
    pq, delta = _tied_pq(rng, hb.x, f, offset=100.0), np.float32(1.7)
    c, stats = _fwd(ctx, a, hb.x, pq, delta)
    r_c, r_stats = PR.aggregate(rp, ci, hb.x, pq, delta)
    top = float(np.max(np.abs(pq[:, f:])))
    e_std = rel_err(stats[:, 3 * f:4 * f], r_stats[:, 3 * f:4 * f])
    e_c_std = max(rel_err(c[:, k * f:(k + 1) * f], r_c[:, k * f:(k + 1) * f]) for k in (4, 8, 12))
    e_stat = [float(np.max(np.abs(stats[:, k * f:(k + 1) * f] - r_stats[:, k * f:(k + 1) * f]))) / top for k in range(3)]
    e_c = [rel_err(c[:, k * f:(k + 1) * f], r_c[:, k * f:(k + 1) * f]) for k in (1, 2, 3, 5, 6, 7, 9, 10, 11)]
    print(f"pna offset: std {e_std:.2e} (C blocks {e_c_std:.2e}); meanQ / minQ / maxQ against max|Q| {e_stat}; C mean/min/max blocks {max(e_c):.2e}")
    assert e_std < TIGHT and e_c_std < TIGHT
    assert max(e_stat) < TIGHT and max(e_c) < TIGHT
    assert np.array_equal(stats[:, 4 * f:], r_stats[:, 4 * f:])
    dc = rng.standard_normal((hb.n, 13 * f)).astype(np.float32)
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    r_dpq, big = PR.aggregate_bwd(rp, ci, pq, r_stats, dc, delta)
    e_dq = float(np.max(np.abs(dpq[:, f:] - r_dpq[:, f:]))) / float(np.max(big))
    e_dp = rel_err(dpq[:, :f], r_dpq[:, :f])
    e_emu = float(np.max(np.abs(_emulate_dq_f32(rp, ci, pq, r_stats, dc, delta) - r_dpq[:, f:]))) / float(np.max(big))
    print(f"pna offset: dQ against its largest term {e_dq:.2e} (float32 emulation of the contract: {e_emu:.2e}), dP {e_dp:.2e}")
    assert e_dp < TIGHT and e_dq < max(TIGHT, 4 * e_emu)


# ---- 4. long rows -----------------------------------------------------------------------------------------------------------
def test_pna_long_rows(ctx):
    hb, _ = _hub()                                                         # one row of at least 4096 entries
    f = 64
    rp, ci = hb.rowptr.astype(np.int64), hb.colidx.astype(np.int64)
    assert int(np.diff(rp).max()) >= 4096 and hb.x.shape[1] == f
    a = _csr(ctx, hb)
    rng = np.random.default_rng(6)
    pq, delta = rng.standard_normal((hb.n, 2 * f)).astype(np.float32), np.float32(2.0)
    c, stats = _fwd(ctx, a, hb.x, pq, delta)
    r_c, r_stats = PR.aggregate(rp, ci, hb.x, pq, delta)
    _check_fwd(c, stats, r_c, r_stats, f, "pna_aggregate hub")
    dc = rng.standard_normal((hb.n, 13 * f)).astype(np.float32)
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    r_dpq, _ = PR.aggregate_bwd(rp, ci, pq, r_stats, dc, delta)
    e_dp, e_dq = rel_err(dpq[:, :f], r_dpq[:, :f]), rel_err(dpq[:, f:], r_dpq[:, f:])
    print(f"pna_bwd hub: dP {e_dp:.2e} dQ {e_dq:.2e}")
    assert e_dp < TIGHT and e_dq < TIGHT


# ---- 5. rows with one entry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [3, 16])
def test_pna_single_entry_rows_have_the_floor_std_and_no_std_gradient(ctx, f):
    from gcnx.device import DeviceCSR
    n = 70
    rng = np.random.default_rng(7 + f)
    rp, ci = np.arange(n + 1, dtype=np.int32), rng.permutation(n).astype(np.int32)      # every row gathers exactly one row
    a = DeviceCSR.from_host_csr(ctx, rp, ci, None, np.array([0, n], np.int32)).unweighted()
    x, pq = rng.standard_normal((n, f)).astype(np.float32), (50 + rng.standard_normal((n, 2 * f))).astype(np.float32)
    delta = np.float32(0.8)
    c, stats = _fwd(ctx, a, x, pq, delta)
    for k in (3, ):
        assert np.array_equal(_bits(stats[:, k * f:(k + 1) * f]), _bits(np.full((n, f), STD0)))
    assert np.array_equal(_bits(c[:, 4 * f:5 * f]), _bits(np.full((n, f), STD0)))
    assert np.array_equal(_bits(stats[:, :f]), _bits(pq[ci, f:])) and np.all(stats[:, 4 * f:] == 1)      # mean = min = max = the entry
    r_c, r_stats = PR.aggregate(rp.astype(np.int64), ci.astype(np.int64), x, pq, delta)
    _check_fwd(c, stats, r_c, r_stats, f, f"pna_aggregate d=1 f={f}")
    dc = np.zeros((n, 13 * f), np.float32)
    for k in (4, 8, 12):                                                   # a gradient on the three std blocks only
        dc[:, k * f:(k + 1) * f] = rng.standard_normal((n, f))
    dpq = _bwd(ctx, a, pq, stats, dc, delta)
    assert np.all(dpq == 0)


# ---- 6. strided operands inside sentinel frames --------------------------------------------------------------------------------
@pytest.mark.parametrize("f,pad,lead", [(16, 4, 4), (16, 3, 1), (3, 2, 1)])      # float4 lanes; the same width unaligned; scalar
def test_pna_strided_operands_in_frames(ctx, f, pad, lead):
    from gcnx import device as D
    hb, rp, ci = _host("directed", f)
    a = _csr(ctx, hb)
    n = hb.n
    rng = np.random.default_rng(8)
    pq, delta = _tied_pq(rng, hb.x, f), np.float32(1.3)
    dc = rng.standard_normal((n, 13 * f)).astype(np.float32)
    fx, fpq = Frame(ctx, n, f, f + pad, lead, data=hb.x), Frame(ctx, n, 2 * f, 2 * f + pad, lead, data=pq)
    fc, fs = Frame(ctx, n, 13 * f, 13 * f + 2 * pad, lead), Frame(ctx, n, 6 * f, 6 * f + pad, lead)
    fdc, fd = Frame(ctx, n, 13 * f, 13 * f + pad, lead, data=dc), Frame(ctx, n, 2 * f, 2 * f + 3 * pad, lead)
    assert all(fr.aligned() for fr in (fx, fpq, fc, fs, fdc, fd)) == (pad == 4)
    D.pna_aggregate(ctx, a, fx.view, fpq.view, delta, fc.view, fs.view)
    c, stats = fc.numpy(), fs.numpy()                                      # (asserts that nothing outside the views was written)
    r_c, r_stats = PR.aggregate(rp, ci, hb.x, pq, delta)
    _check_fwd(c, stats, r_c, r_stats, f, f"pna_aggregate frames f={f} pad={pad}")
    c0, s0 = _fwd(ctx, a, hb.x, pq, delta)                                 # the same bits as on packed operands
    assert np.array_equal(_bits(c), _bits(c0)) and np.array_equal(_bits(stats), _bits(s0))
    scratch = ctx.empty(D.pna_bwd_scratch_floats(ctx, n, f))
    D.pna_bwd(ctx, a, a.transpose(), fpq.view, fs.view, fdc.view, delta, fd.view, scratch)
    dpq = fd.numpy()
    r_dpq, _ = PR.aggregate_bwd(rp, ci, pq, r_stats, dc, delta)
    assert rel_err(dpq[:, :f], r_dpq[:, :f]) < TIGHT and rel_err(dpq[:, f:], r_dpq[:, f:]) < TIGHT
    assert np.array_equal(_bits(dpq), _bits(_bwd(ctx, a, pq, stats, dc, delta)))
    fx.untouched("x"), fpq.untouched("pq"), fdc.untouched("dC, block 0 included")
    fc.check(c, "C after the backward"), fs.check(stats, "stats after the backward")


def test_pna_entry_points_refuse_bad_arguments(ctx):
    from gcnx import _lib, device as D
    hb, rp, ci = _host("directed", 16)
    a = _csr(ctx, hb)
    n, f = hb.n, 16
    x, pq, c = ctx.to_device(hb.x), ctx.zeros((n, 2 * f)), Frame(ctx, n, 13 * f, 13 * f, 0)
    with pytest.raises(_lib.GcnxError):
        D.pna_aggregate(ctx, a, x, pq, 0.0, c.view)                        # avg_deg_log must be positive
    bad = D.DeviceArray(ctx, pq.ptr, (n, 2 * f), np.float32, ld=2 * f - 1, base=pq)
    with pytest.raises(_lib.GcnxError):
        D.pna_aggregate(ctx, a, x, bad, 1.0, c.view)                       # ldpq < 2f
    alias = D.DeviceArray(ctx, c.view.ptr, (n, f), np.float32, ld=13 * f, base=c.buf)
    with pytest.raises(_lib.GcnxError):
        D.pna_aggregate(ctx, a, alias, pq, 1.0, c.view)                    # c aliases x
    c.untouched("a refused call writes nothing")


# ---- 7. the layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("fi,fo", [(16, 32), (64, 64)])
def test_pnaconv_layer_forward_and_backward(ctx, fi, fo, use_bias):
    from gcnx.layers import PNAConv
    hb, rp, ci = _host("symmetric", fi)
    a = _csr(ctx, hb)
    hist = np.bincount(np.diff(rp))
    lay = PNAConv(fo, deg=hist, use_bias=use_bias, seed=3)
    assert abs(lay.avg_deg_log - PR.avg_deg_log(hist)) < 1e-12
    x = ctx.to_device(hb.x)
    y = lay([x, PNAConv.preprocess(a)])
    names = ["pre_nns.0.0.weight", "pre_nns.0.0.bias", "post_nns.0.0.weight", "post_nns.0.0.bias", "lin.weight", "lin.bias"]
    assert list(lay.params) == [k for k in names if use_bias or k.endswith("weight")]
    assert all(v.ptr % 16 == 0 for v in lay.params.values())
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    w = [p[k].T if k.endswith("weight") else p[k] for k in names if k in p]                # torch's layouts
    args = w if use_bias else [w[0], None, w[1], None, w[2], None]
    delta = np.float32(lay.avg_deg_log)                                    # what the kernels receive
    r_y, cache = PR.pna_conv_fwd(rp, ci, hb.x, *args, delta)
    e_y = rel_err(y.numpy(), r_y)
    dy = np.random.default_rng(9).standard_normal((hb.n, fo)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r = PR.pna_conv_bwd(rp, ci, cache, args[0], args[2], args[4], delta, dy)
    g = {k: v.numpy() for k, v in lay.grads.items()}
    errs = {"dx": rel_err(dx.numpy(), r[0]), "pre_nns.0.0.weight": rel_err(g["pre_nns.0.0.weight"], r[1].T),
            "post_nns.0.0.weight": rel_err(g["post_nns.0.0.weight"], r[3].T), "lin.weight": rel_err(g["lin.weight"], r[5].T)}
    if use_bias:
        errs.update({"pre_nns.0.0.bias": rel_err(g["pre_nns.0.0.bias"], r[2]), "post_nns.0.0.bias": rel_err(g["post_nns.0.0.bias"], r[4]),
                     "lin.bias": rel_err(g["lin.bias"], r[6])})
    print(f"PNAConv {fi}->{fo} bias={use_bias}: y {e_y:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_y < TIGHT and max(errs.values()) < TIGHT, errs
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    g2 = {k: v.numpy() for k, v in lay.grads.items()}
    assert all(np.array_equal(_bits(g2[k]), _bits(g[k])) for k in g)      # need_dx=False leaves the same gradients
    y_eval = lay([x, a], training=False).numpy()                           # no statistics stored: the same output
    assert np.array_equal(_bits(y_eval), _bits(y.numpy()))
    with pytest.raises(RuntimeError):
        lay.backward(ctx.to_device(dy))


# ---- 8. gcnx.PNA: a full step against the kink-separated oracle ----------------------------------------------------------------
def _sides(m, pre=None):
    """The device's side of both PReLUs of the last call."""
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    return {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
            for i in (1, 2)}


def _cmp_grads(got, ref, tol, what):
    worst = {}
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        if k in UNDER_BN:
            scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN[k]], np.float64))))
            worst[k] = float(np.max(np.abs(g - r))) / scale
        else:
            worst[k] = rel_err(g, r)
    top = sorted(worst, key=worst.get, reverse=True)
    print(f"{what}: worst gradient blocks " + ", ".join(f"{k} {worst[k]:.2e}" for k in top[:6]))
    assert worst[top[0]] < tol, (what, [(k, worst[k]) for k in top[:6]])


def _alpha4_condition(r, p, y):
    """sum |terms| / |sum terms| of the oracle's prelu_4.weight gradient, a single scalar: the factor by which its relative
    error exceeds that of the logits it is summed from."""
    out, a4 = r["out"].ravel(), float(p["prelu_4.weight"][0])
    terms = (1 / (1 + np.exp(-out)) - R.targets(y)) * np.minimum(np.where(out < 0, out / a4, out), 0)
    return float(np.abs(terms).sum() / abs(terms.sum()))


def _delta_of(hb):
    return PR.avg_deg_log(np.bincount(np.diff(hb.rowptr)))


@pytest.mark.parametrize("shape", ["config1", "config2"])
def test_pna_step_against_oracle(ctx, shape):
    import gcnx
    from gcnx import synth
    hb = _tiny_host(16, 16, seed=4) if shape == "config1" else synth.ecoli_batch(f=16)
    batch = _device_batch(ctx, hb)
    hist = gcnx.PNA.degree_histogram([_scipy_adj(hb)])
    m = gcnx.PNA(ctx, hidden_channels=64, deg=hist, seed=0)
    delta = np.float32(m.avg_deg_log[0])
    assert abs(m.avg_deg_log[0] - _delta_of(hb)) < 1e-12
    p = {k: v.astype(np.float32) for k, v in PR.init_params(16, 64, seed=10).items()}
    m.load_state_dict(p)
    m.loss_and_grads(batch)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = PR.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, delta, hb.y, masks=_sides(m), argmax=arg)
    # the parameters are chosen so that no one-element block is a cancelling sum in the ORACLE (with seed 7 the 32 terms of
    # prelu_4.weight cancel to 1 / 357 of their size at config 2, and a relative error of that scalar measures the cancellation)
    assert _alpha4_condition(r, p, hb.y) < 8
    e_out = rel_err(m._bufs["out"].numpy(), r["out"])
    la = m.loss_acc.numpy()
    print(f"PNA step {shape}: logits {e_out:.2e} loss {rel_err(la[0], r['loss']):.2e}")
    assert e_out < TIGHT and rel_err(la[0], r["loss"]) < TIGHT and la[1] == r["hits"], (la, r["loss"], r["hits"])
    got = m.gradients()
    assert list(got) == list(PR.KEYS)
    _cmp_grads(got, r["grads"], TIGHT, f"PNA step {shape}")
    before = m.state_dict()
    loss, acc = m.train_step(batch, lr=0.02)                               # the update moves every convolution tensor
    after = m.state_dict()
    assert np.isfinite(loss) and all(not np.array_equal(after[k], before[k]) for k in PR.CONV_KEYS if k not in UNDER_BN)
    assert all(after[k][0] == before[k][0] for k in PR.DELTA_KEYS)          # a constant


# ---- 9. the model's surface -----------------------------------------------------------------------------------------------------
def test_pna_forward_state_dict_and_single_graph(ctx):
    import gcnx
    hb = _tiny_host(8, 16, seed=6)
    ids, a = hb.ids(), _scipy_adj(hb)
    m = gcnx.PNA(ctx, avg_deg_log=_delta_of(hb), seed=1)
    logits = m((hb.x, a, ids))
    assert logits.shape == (8, 1) and m._bufs["st1"] is not None
    sd = m.state_dict()
    assert list(sd) == list(PR.STATE_KEYS)
    r = PR.model(hb.x, a, hb.graph_ptr, {k: sd[k] for k in PR.KEYS}, np.float32(m.avg_deg_log[0]), masks=_sides(m),
                 argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert rel_err(logits, r["out"]) < TIGHT
    coo = a.tocoo()
    assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)     # PyG: source -> target = CSR row
    assert sd["conv1.pre_nns.0.0.weight"].shape == (16, 32) and sd["conv1.post_nns.0.0.weight"].shape == (64, 208)
    assert sd["conv2.pre_nns.0.0.weight"].shape == (64, 128) and sd["conv2.post_nns.0.0.weight"].shape == (64, 832)
    assert np.max(np.abs(sd["conv1.pre_nns.0.0.weight"])) <= 1 / np.sqrt(32) and np.max(np.abs(sd["conv2.post_nns.0.0.weight"])) <= 1 / np.sqrt(832)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    assert [w.shape for w in m.get_weights()] == [sd[k].shape for k in PR.KEYS]
    sd["conv2.aggr_module.avg_deg_log"] = np.array([0.9], np.float32)      # a checkpoint's constant is honoured
    m2 = gcnx.PNA(ctx, avg_deg_log=5.0, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(_bits(v), _bits(sd[k])), k
    l2 = m2((hb.x, a, ids))
    assert not np.allclose(l2, logits, rtol=1e-3, atol=1e-3)
    r2 = PR.model(hb.x, a, hb.graph_ptr, {k: sd[k] for k in PR.KEYS}, [np.float32(m2.avg_deg_log[0]), np.float32(0.9)],
                  masks=_sides(m2), argmax=m2._bufs["arg"].numpy().astype(np.int64))
    assert rel_err(l2, r2["out"]) < TIGHT
    loss, acc, probs = m.evaluate_batch((hb.x, a, ids), hb.y)              # evaluate_batch: the oracle's loss and hits
    ry = PR.model(hb.x, a, hb.graph_ptr, {k: m.state_dict()[k] for k in PR.KEYS}, np.float32(m.avg_deg_log[0]), hb.y, masks=_sides(m),
                  argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert rel_err(loss, ry["loss"]) < TIGHT and acc == ry["hits"] / 8 and probs.shape == (8, 1)
    assert rel_err(probs, 1 / (1 + np.exp(-ry["out"]))) < TIGHT
    one = hb.slice_graphs(0, 1)
    with pytest.raises(ValueError):
        m((one.x, _scipy_adj(one), one.ids()))
    with pytest.raises(ValueError):
        m.train_step(_device_batch(ctx, one), lr=0.01)


# ---- 10. what the model inherits --------------------------------------------------------------------------------------------------
def test_pna_sync_bn_step_equals_the_whole_batch():
    import gcnx
    from gcnx import shard
    hb = _tiny_host(16, 16)
    p = {k: v.astype(np.float32) for k, v in PR.init_params(16, 64, seed=7).items()}
    delta = _delta_of(hb)

    def step(ctx, part, comm, gb):
        m = gcnx.PNA(ctx, hidden_channels=64, avg_deg_log=delta, seed=0, comm=comm)
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
    for r in ranks:
        print(f"PNA sync-BN: loss {abs(r['loss'] - whole['loss']):.2e} g {rel_err(r['g'], whole['g']):.2e} w {rel_err(r['w'], whole['w']):.2e}")
        assert abs(r["loss"] - whole["loss"]) < TIGHT * max(1.0, abs(whole["loss"])), (r["loss"], whole["loss"])
        assert r["acc"] == whole["acc"]
        assert rel_err(r["g"], whole["g"]) < TIGHT and rel_err(r["w"], whole["w"]) < TIGHT
    assert np.array_equal(_bits(ranks[0]["w"]), _bits(ranks[1]["w"]))


def _tiny_datasets():
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    mk = lambda part: ListDataset([Graph(x=x, a=a.tocsr(), y=y) for x, a, y in part])
    return mk(raw[:10]), mk(raw[10:])


def test_fit_runs_the_pna_model_with_adam(ctx):
    import gcnx
    tr, te = _tiny_datasets()
    m = gcnx.PNA(ctx, deg=gcnx.PNA.degree_histogram(tr), seed=0)
    opt = gcnx.Adam()
    m.set_optimizer(opt)
    out = gcnx.fit(m, gcnx.DisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   gcnx.DisjointLoader(te, batch_size=3, shuffle=False), epochs=2, verbose=False)
    assert len(out["history"]) == 2 and all(np.all(np.isfinite(h)) for h in out["history"])
    assert opt.flat("m").size == m.n_params


def test_pna_trains_from_device_loader_batches(ctx):
    import gcnx
    tr, _ = _tiny_datasets()
    m = gcnx.PNA(ctx, deg=gcnx.PNA.degree_histogram(tr), seed=2)
    dev = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, tr), batch_size=4, epochs=1, shuffle=True, seed=8)
    host = gcnx.DisjointLoader(tr, batch_size=4, epochs=1, shuffle=True, seed=8)
    seen = 0
    for (inputs, target), (db, none) in zip(host, dev):
        assert none is None
        m.loss_and_grads(inputs, target)                                   # the same graphs from the host loader
        la_h, g_h = m.loss_acc.numpy(), m.gradients()
        m.loss_and_grads(db)
        la_d, g_d = m.loss_acc.numpy(), m.gradients()
        assert rel_err(la_d[0], la_h[0]) < TIGHT and la_d[1] == la_h[1]
        assert all(rel_err(g_d[k], g_h[k]) < TIGHT for k in g_h if k not in UNDER_BN)
        before = m.flat_p.numpy()
        loss, acc = m.train_step(db, lr=0.01)
        assert np.isfinite(loss) and not np.array_equal(m.flat_p.numpy(), before)
        seen += 1
    assert seen == 3

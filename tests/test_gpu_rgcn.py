"""GPU tests of RGCNConv (csrc/rgcn.hip): gcnx_rgcn_operator, the one launch gcnx_rgcn_conv in both directions
and the composed route gcnx_rgcn_aggregate + gcnx_gemm, the layer gcnx.RGCNConv and the model gcnx.RGCN on both routes
(GCNX_RGCN_FUSED) -- each against the float64 restatement tests/rgcn_ref.py, the model on the device's side of every kink.
Tolerances (tests/test_gpu_sage.py's): TIGHT = 2e-5 for one fp32 kernel, 1e-4 for a whole step; 1e-6 for the operator's values
(the graph-preparation bar).  Every test builds its own edge features and asserts on the host, before the upload, that every
relation holds an entry, that every relation is missing from some row, and that some row holds no entry at all."""
import functools

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import rgcn_ref as RR
from gpu_frames import SENTINEL, Frame
from test_gpu_gcn_bn import _tiny_host

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
SHAPES = [(16, 64), (64, 64), (32, 16), (128, 128)]
UNDER_BN = {"conv1.bias": "conv1.weight", "conv2.bias": "conv2.weight", "linear_1.bias": "linear_1.weight",
            "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
class _Case:
    """A pattern (rowptr, colidx, graph_ptr, n), node features, labels and edge features for one rule; rel: the restatement's."""

    def __init__(self, rowptr, colidx, gp, x, y, e, rule, R_):
        self.rowptr, self.colidx, self.gp, self.x, self.y, self.e, self.rule, self.R = rowptr, colidx, gp, x, y, e, rule, R_
        self.n, self.nnz = len(rowptr) - 1, len(colidx)
        self.rel = RR.relations(e, rule, R_)
        self.rows = np.repeat(np.arange(self.n), np.diff(rowptr))
        # the three conditions on the inputs, on the host: no test passes by never meeting a case
        assert all((self.rel == r).any() for r in range(R_)), "every relation holds at least one entry"
        has = np.zeros((self.n, R_), bool)
        has[self.rows, self.rel] = True
        assert (~has).any(0).all(), "at least one row lacks each relation"
        assert (np.diff(rowptr) == 0).any(), "at least one row has none"
        self.ops = RR.operators(rowptr, colidx, self.rel, R_)

    def csr(self, ctx):
        from gcnx.device import DeviceCSR
        return DeviceCSR.from_host_csr(ctx, self.rowptr, self.colidx, None, self.gp)


def _features(rowptr, colidx, R_, seed):
    """(e, rule): R = 3: reference-style (dca, proximity) -- dca on a few entries, proximity on most, a share (every stored loop
    among it) with neither; otherwise one index column with the same proportions folded into R relations."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    rng = np.random.default_rng(seed)
    u = rng.random(len(colidx))
    kind = np.where(rows == colidx, 2, np.where(u < 0.08, 0, np.where(u < 0.85, 1, 2)))
    if R_ == 3:
        e = np.zeros((len(colidx), 2), np.float32)
        e[kind == 0, 0] = rng.uniform(0.2, 1.5, (kind == 0).sum())
        e[kind == 1, 1] = rng.uniform(0.2, 1.5, (kind == 1).sum())
        return e, "nonzero"
    if R_ == 4:
        kind = np.where((kind == 1) & (rng.random(len(colidx)) < 0.3), 3, kind)
    return np.minimum(kind, R_ - 1).astype(np.float32)[:, None], "index"


def _drop_rows(rowptr, colidx, drop):
    """The pattern without the entries of the rows ``drop`` (their columns keep theirs: the pattern becomes asymmetric)."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    keep = ~np.isin(rows, drop)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(rowptr) - 1))]).astype(np.int32)
    return rp, colidx[keep].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(shape, f, R_):
    """"hand": rgcn_ref.hand_batch (R = 3: its own features); "tiny": the tiny host batch; "ecoli": synth.ecoli_batch(2) -- the
    last two with the entries of three rows removed.  Built once per (shape, f, R), never modified."""
    from gcnx import synth
    rng = np.random.default_rng(17)
    if shape == "hand":
        rowptr, colidx, e3, gp = RR.hand_batch()
        x = rng.standard_normal((12, f)).astype(np.float32)
        y = np.array([1, 0, 1, 0], np.float32)
        e, rule = (e3, "nonzero") if R_ == 3 else _features(rowptr, colidx, R_, 3)
        return _Case(rowptr, colidx, gp, x, y, e, rule, R_)
    hb = _tiny_host(16, f) if shape == "tiny" else synth.ecoli_batch(2, f)
    rowptr, colidx = _drop_rows(hb.rowptr, hb.colidx, [3, 40, hb.n - 2])
    e, rule = _features(rowptr, colidx, R_, 5)
    c = _Case(rowptr, colidx, hb.graph_ptr, hb.x.astype(np.float32), hb.y, e, rule, R_)
    assert shape == "tiny" or (c.n % 32 != 0 and c.n > 1000)
    return c


def _operator(ctx, a, c):
    return a.rgcn_operator(ctx.to_device(c.e), c.rule, c.R)


# ---- 1. the operator -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", ["hand", "tiny", "ecoli"])
def test_rgcn_operator(ctx, shape, R_):
    c = _case(shape, 16, R_)
    a = c.csr(ctx)
    rel, val, rel_t, val_t = _operator(ctx, a, c)
    assert rel.dtype == np.uint8 and rel_t.dtype == np.uint8
    g_rel, g_val = rel.numpy()[:c.nnz], val.numpy()[:c.nnz]
    assert np.array_equal(g_rel, c.rel)
    want = RR.values(c.rowptr, c.rel, c.R)
    err = float(np.max(np.abs(g_val - want) / want))
    print(f"rgcn_operator {shape} R={R_}: val rel. error {err:.2e} ({err / 1e-6:.2f} of the bound)")
    assert err <= 1e-6
    perm = a.transpose_perm()[2].numpy()[:c.nnz]
    assert np.array_equal(rel_t.numpy()[:c.nnz], g_rel[perm]) and np.array_equal(_bits(val_t.numpy()[:c.nnz]), _bits(g_val[perm]))
    # no atomics: the same bits on a second call
    rel2, val2, _, _ = _operator(ctx, a, c)
    assert np.array_equal(rel2.numpy(), rel.numpy()) and np.array_equal(_bits(val2.numpy()[:c.nnz]), _bits(g_val))


def test_rgcn_operator_index_rule_clamps_on_the_device(ctx):
    c = _case("hand", 16, 3)
    a = c.csr(ctx)
    col = np.array([-2.0, 0.0, 1.0, 2.0, 3.0, 9.0, np.nan, 1.5], np.float32)
    e = np.resize(col, c.nnz).astype(np.float32)[:, None]
    rel = a.rgcn_operator(ctx.to_device(e), "index", 3)[0].numpy()[:c.nnz]
    assert np.array_equal(rel, RR.relations(e, "index", 3)) and list(rel[:8]) == [0, 0, 1, 2, 2, 2, 0, 1]


# ---- 2. both routes against float64 ------------------------------------------------------------------------------------------
def _weights(rng, fi, fo, nb, wt):
    """w as the call takes it (nb blocks, [fi, fo] each; wt: [fo, fi] each) and as float64 [nb, fi, fo]."""
    shape = (nb, fo, fi) if wt else (nb, fi, fo)
    w = (rng.standard_normal(shape) / np.sqrt(fi * nb)).astype(np.float32)
    return w, (w.transpose(0, 2, 1) if wt else w).astype(np.float64), rng.standard_normal(fo).astype(np.float32)


def _ref(ops, x, w64, bias, R_, root, wt):
    """(out, M) in float64.  wt: the operators transposed -- out = x W_root + sum_r A_r^T (x W_r), the backward's form."""
    x = x.astype(np.float64)
    m = np.concatenate([(A.T if wt else A) @ x for A in ops], axis=1)
    out = m @ w64[:R_].reshape(-1, w64.shape[2])
    if root:
        out = out + x @ w64[R_]
    return (out + bias.astype(np.float64) if bias is not None else out), m


def _sides(ctx, a, ops_dev, wt):
    """(rowptr, colidx, rel, val) of the direction."""
    if wt:
        rp, ci, _ = a.transpose_perm()
        return rp, ci, ops_dev[2], ops_dev[3]
    return a.rowptr, a.colidx, ops_dev[0], ops_dev[1]


def _run_fused(ctx, side, x, w, bias, fo, R_, root, wt, with_m=True):
    from gcnx import device as D
    n, fi = x.shape
    out, m = ctx.empty((n, fo)), (ctx.empty((n, R_ * fi)) if with_m else None)
    D.rgcn_conv(ctx, *side, ctx.to_device(x), ctx.to_device(w.reshape(-1, w.shape[2])), ctx.to_device(bias) if bias is not None else None,
                out, R_, root, m=m, w_transposed=bool(wt))
    return out.numpy(), (m.numpy() if with_m else None)


def _run_composed(ctx, side, x, w, bias, fo, R_, root, wt):
    """gcnx_rgcn_aggregate, then gcnx_gemm over the panel and over x (wt: gcnx_gemm_dx per block, the weights as stored)."""
    from gcnx import device as D
    n, fi = x.shape
    dx, dw = ctx.to_device(x), ctx.to_device(w.reshape(-1, w.shape[2]))
    m, out, tmp = ctx.empty((n, R_ * fi)), ctx.empty((n, fo)), ctx.empty((n, fo))
    D.rgcn_aggregate(ctx, *side, dx, m, R_)
    db = ctx.to_device(bias) if bias is not None else None
    if not wt:
        D.gemm(ctx, m, dw.flat(0, R_ * fi * fo, (R_ * fi, fo)), db, out)
        if root:
            D.gemm(ctx, dx, dw.flat(R_ * fi * fo, fi * fo, (fi, fo)), None, tmp)
            D.add(ctx, out, tmp, out)
        return out.numpy(), m.numpy()
    for q in range(R_ + (1 if root else 0)):
        src = dx if q == R_ else m.cols(q * fi, (q + 1) * fi)
        D.gemm_dx(ctx, src, dw.flat(q * fi * fo, fi * fo, (fo, fi)), out, accumulate=q > 0)
    res = out.numpy()
    return (res + bias if bias is not None else res), m.numpy()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("R_", [1, 2, 4])
@pytest.mark.parametrize("fi,fo", SHAPES)
def test_rgcn_conv_both_routes_against_float64(ctx, fi, fo, R_, wt):
    from gcnx import device as D
    worst = 0.0
    for shape in ("hand", "tiny", "ecoli"):
        c = _case(shape, fi, R_)
        a = c.csr(ctx)
        side = _sides(ctx, a, _operator(ctx, a, c), wt)
        assert D.rgcn_conv_ok(ctx, c.n, fi, fo, R_)
        rng = np.random.default_rng(100 * fi + fo + 10 * R_ + wt)
        w, w64, bias = _weights(rng, fi, fo, R_ + 1, wt)
        r_out, r_m = _ref(c.ops, c.x, w64, bias, R_, True, wt)
        out, m = _run_fused(ctx, side, c.x, w, bias, fo, R_, True, wt)
        out_c, m_c = _run_composed(ctx, side, c.x, w, bias, fo, R_, True, wt)
        errs = (rel_err(out, r_out), rel_err(m, r_m), rel_err(out_c, r_out))
        worst = max(worst, *errs)
        assert max(errs) < TIGHT, (shape, errs)
        assert np.array_equal(_bits(m), _bits(m_c)), (shape, "the panel M differs between the routes")
        empty = np.diff(c.rowptr if not wt else np.concatenate([[0], np.cumsum(np.bincount(c.colidx, minlength=c.n))])) == 0
        assert not m[empty].any() and not np.signbit(m[empty]).any()                  # the mean over no entry: +0
        # no atomics: a second call leaves the same bits; m = NULL and bias = NULL change nothing else
        out2, m2 = _run_fused(ctx, side, c.x, w, bias, fo, R_, True, wt)
        assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(m2), _bits(m))
        out3, _ = _run_fused(ctx, side, c.x, w, None, fo, R_, True, wt, with_m=False)
        assert np.array_equal(_bits(out3 + bias), _bits(out))
        # root_weight = 0: R blocks, the own rows are not read into the product
        out4, m4 = _run_fused(ctx, side, c.x, w[:R_], bias, fo, R_, False, wt)
        r_out4, _ = _ref(c.ops, c.x, w64, bias, R_, False, wt)
        assert rel_err(out4, r_out4) < TIGHT and np.array_equal(_bits(m4), _bits(m))
    print(f"rgcn_conv fi={fi} fo={fo} R={R_} wt={wt}: worst rel_err {worst:.2e} ({worst / TIGHT:.2f} of TIGHT)")


@pytest.mark.parametrize("wt", [0, 1])
def test_rgcn_one_relation_is_sage_conv(ctx, wt):
    """R = 1: within TIGHT of gcnx_sage_conv on the row-mean operator with the same weights."""
    from gcnx import device as D
    fi, fo = 64, 64
    c = _case("ecoli", fi, 1)
    a = c.csr(ctx)
    side = _sides(ctx, a, _operator(ctx, a, c), wt)
    rng = np.random.default_rng(3 + wt)
    w, _, bias = _weights(rng, fi, fo, 2, wt)
    out, m = _run_fused(ctx, side, c.x, w, bias, fo, 1, True, wt)
    op = a.row_mean().transpose() if wt else a.row_mean()
    s_out, s = ctx.empty((c.n, fo)), ctx.empty((c.n, fi))
    D.sage_conv(ctx, op, ctx.to_device(c.x), ctx.to_device(w[0]), ctx.to_device(w[1]), ctx.to_device(bias), s_out, s=s, w_transposed=bool(wt))
    assert rel_err(out, s_out.numpy()) < TIGHT and rel_err(m, s.numpy()) < TIGHT


# ---- 3. degenerate inputs, long rows -----------------------------------------------------------------------------------------
def _csr_of(ctx, rowptr, colidx, n):
    """One graph of n rows on the device, with the true entry count (also 0) and no symmetry claimed."""
    from gcnx.device import DeviceCSR
    rp, ci = ctx.to_device(np.asarray(rowptr, np.int32)), ctx.to_device(np.asarray(colidx if len(colidx) else [0], np.int32))
    return DeviceCSR(ctx, n, len(colidx), rp, ci, None, ctx.to_device(np.array([0, n], np.int32)), 1, False, n)


@pytest.mark.parametrize("wt", [0, 1])
def test_rgcn_degenerate_inputs(ctx, wt):
    from gcnx import _lib
    fi, fo, R_ = 32, 16, 3
    rng = np.random.default_rng(7 + wt)
    w, w64, bias = _weights(rng, fi, fo, R_ + 1, wt)
    # n = 33 (one row past a tile) on a ring with loops, relation 1 absent from the whole batch
    n = 33
    rows = np.repeat(np.arange(n), 3)
    cols = np.stack([(np.arange(n) - 1) % n, np.arange(n), (np.arange(n) + 1) % n], 1).ravel()
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    e = np.where(rows == cols, 2.0, 0.0).astype(np.float32)[:, None]
    rel = RR.relations(e, "index", R_)
    assert not (rel == 1).any() and (rel == 0).any() and (rel == 2).any()
    x = rng.standard_normal((n, fi)).astype(np.float32)
    a = _csr_of(ctx, rowptr, cols, n)
    side = _sides(ctx, a, a.rgcn_operator(ctx.to_device(e), "index", R_), wt)
    ops = RR.operators(rowptr, cols, rel, R_)
    out, m = _run_fused(ctx, side, x, w, bias, fo, R_, True, wt)
    out_c, m_c = _run_composed(ctx, side, x, w, bias, fo, R_, True, wt)
    r_out, r_m = _ref(ops, x, w64, bias, R_, True, wt)
    assert rel_err(out, r_out) < TIGHT and rel_err(out_c, r_out) < TIGHT and np.array_equal(_bits(m), _bits(m_c)) and rel_err(m, r_m) < TIGHT
    assert not m[:, fi:2 * fi].any() and not np.signbit(m[:, fi:2 * fi]).any()        # the absent relation: exact +0
    # nnz = 0 on 5 rows, and n = 1 without entries: the root term and the bias alone
    for k in (5, 1):
        a0 = _csr_of(ctx, np.zeros(k + 1, np.int32), [], k)
        ops0 = a0.rgcn_operator(ctx.zeros((1, 1)), "index", R_)
        side0 = _sides(ctx, a0, ops0, wt)
        out0, m0 = _run_fused(ctx, side0, x[:k], w, bias, fo, R_, True, wt)
        out0c, m0c = _run_composed(ctx, side0, x[:k], w, bias, fo, R_, True, wt)
        want = x[:k].astype(np.float64) @ w64[R_] + bias
        assert rel_err(out0, want) < TIGHT and rel_err(out0c, want) < TIGHT and not m0.any() and not m0c.any()
    # n = 0: nothing to do, no error, nothing written
    fr = Frame(ctx, 4, fo, fo, 0)
    dw = ctx.zeros(((R_ + 1) * fi, fo))
    rc = ctx.lib.gcnx_rgcn_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, side[2].ptr, side[3].ptr, ctx.zeros((4, fi)).ptr, fi, 0, fi, dw.ptr, 1, fo,
                                R_, wt, None, None, 0, fr.view.ptr, fo)
    assert rc == _lib.OK
    rc = ctx.lib.gcnx_rgcn_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, side[2].ptr, side[3].ptr, ctx.zeros((4, fi)).ptr, fi, 0, fi, R_,
                                     fr.view.ptr, R_ * fi)
    assert rc == _lib.OK
    fr.check(np.full((4, fo), SENTINEL), "n = 0 writes nothing")


@pytest.mark.parametrize("wt", [0, 1])
def test_rgcn_long_rows_beyond_the_staged_entries(ctx, wt):
    """40 nodes, complete graph with loops: a 32-row tile holds 1280 entries, more than the 1024 staged in LDS; one row is emptied."""
    n, fi, fo, R_ = 40, 64, 32, 3
    rowptr = (np.arange(n + 1) * n).astype(np.int32)
    colidx = np.tile(np.arange(n), n).astype(np.int32)
    rowptr, colidx = _drop_rows(rowptr, colidx, [37])
    assert rowptr[32] > 1024
    e, rule = _features(rowptr, colidx, R_, 9)
    e[(np.repeat(np.arange(n), np.diff(rowptr)) == 5), 0] = 0.0                        # row 5 lacks relation 0 ...
    e[(np.repeat(np.arange(n), np.diff(rowptr)) == 6), 1] = 0.0                        # ... row 6 relation 1; the loops make 2
    e[:3] = 0.0
    e[3:8, 0], e[3:8, 1] = 0.7, 0.0                                                    # row 0: relation 0 and 2 only
    gp = np.array([0, n], np.int32)
    rng = np.random.default_rng(11 + wt)
    c = _Case(rowptr, colidx, gp, rng.standard_normal((n, fi)).astype(np.float32), None, e, rule, R_)
    a = _csr_of(ctx, rowptr, colidx, n)
    side = _sides(ctx, a, _operator(ctx, a, c), wt)
    w, w64, bias = _weights(rng, fi, fo, R_ + 1, wt)
    out, m = _run_fused(ctx, side, c.x, w, bias, fo, R_, True, wt)
    _, m_c = _run_composed(ctx, side, c.x, w, bias, fo, R_, True, wt)
    r_out, r_m = _ref(c.ops, c.x, w64, bias, R_, True, wt)
    e_out, e_m = rel_err(out, r_out), rel_err(m, r_m)
    print(f"rgcn_conv long rows wt={wt}: rel_err out {e_out:.2e} M {e_m:.2e}")
    assert e_out < TIGHT and e_m < TIGHT and np.array_equal(_bits(m), _bits(m_c))


def test_rgcn_a_column_outside_the_rows_adds_nothing_on_both_routes(ctx):
    """include/gcnx.h: an entry whose column lies outside [0, n) adds nothing -- also one whose byte offset column * ldx * 4 wraps
    modulo 2^32 back into the rows (2^26 + 1 at ldx = 16 lands on row 1), a negative one, and n itself; the panel keeps its bits
    between the routes.  (No transposed pattern is built of such a CSR: the operator is called without perm_t.)"""
    fi, fo, R_ = 16, 64, 2
    c = _case("tiny", fi, R_)
    colidx = c.colidx.copy()
    bad = {5: (1 << 26) + 1, 17: -1, 40: c.n, c.nnz - 3: (1 << 28) + 2}
    for k, v in bad.items():
        colidx[k] = v
    a = _csr_of(ctx, c.rowptr, colidx, c.n)
    rel, val = ctx.empty(c.nnz, np.uint8), ctx.empty(c.nnz)
    ctx._ck(ctx.lib.gcnx_rgcn_operator(ctx.h, a.rowptr.ptr, ctx.to_device(c.e).ptr, 1, 1, 1, R_, None, c.n, c.nnz, rel.ptr, val.ptr, None, None))
    side = (a.rowptr, a.colidx, rel, val)
    w, w64, bias = _weights(np.random.default_rng(4), fi, fo, R_ + 1, 0)
    out, m = _run_fused(ctx, side, c.x, w, bias, fo, R_, True, 0)
    out_c, m_c = _run_composed(ctx, side, c.x, w, bias, fo, R_, True, 0)
    # float64: the means keep their denominators (val counts every stored entry of the row), the bad entries' terms are absent
    keep = np.ones(c.nnz, bool)
    keep[list(bad)] = False
    vals = RR.values(c.rowptr, c.rel, R_)
    r_m = np.zeros((c.n, R_ * fi))
    for k in np.nonzero(keep)[0]:
        r_m[c.rows[k], c.rel[k] * fi:(c.rel[k] + 1) * fi] += vals[k] * c.x[c.colidx[k]].astype(np.float64)
    r_out = r_m @ w64[:R_].reshape(-1, fo) + c.x.astype(np.float64) @ w64[R_] + bias
    assert rel_err(m, r_m) < TIGHT and rel_err(out, r_out) < TIGHT and rel_err(out_c, r_out) < TIGHT
    assert np.array_equal(_bits(m), _bits(m_c))


# ---- 4. strided operands, any width ----------------------------------------------------------------------------------------
def _frame_close(fr, want, tol, what):
    got = fr.numpy()                                                                   # (asserts that nothing outside the view was written)
    assert rel_err(got, want) < tol, (what, rel_err(got, want))
    return got


@pytest.mark.parametrize("wt", [0, 1])
def test_rgcn_strided_operands_on_both_routes(ctx, wt):
    from gcnx import device as D
    fi, fo, R_ = 32, 64, 3
    c = _case("tiny", fi, R_)
    a = c.csr(ctx)
    side = _sides(ctx, a, _operator(ctx, a, c), wt)
    rng = np.random.default_rng(21 + wt)
    w, w64, bias = _weights(rng, fi, fo, R_ + 1, wt)
    r_out, r_m = _ref(c.ops, c.x, w64, bias, R_, True, wt)
    fx = Frame(ctx, c.n, fi, 2 * fi, 4, data=c.x)                       # x: a column slice of an array twice as wide
    fo_, fm = Frame(ctx, c.n, fo, fo + 8, 8), Frame(ctx, c.n, R_ * fi, R_ * fi + 4, 12)
    assert fx.aligned() and fo_.aligned() and fm.aligned() and D.rgcn_conv_ok(ctx, c.n, fi, fo, R_, fx.view.ld)
    D.rgcn_conv(ctx, *side, fx.view, ctx.to_device(w.reshape(-1, w.shape[2])), ctx.to_device(bias), fo_.view, R_, True, m=fm.view,
                w_transposed=bool(wt))
    _frame_close(fo_, r_out, TIGHT, "out")
    m_f = _frame_close(fm, r_m, TIGHT, "M")
    fx.untouched("x is not written")
    # the composed route's panel: unaligned start, odd strides -- the scalar kernel -- and the same bits
    fx2, fm2 = Frame(ctx, c.n, fi, fi + 3, 1, data=c.x), Frame(ctx, c.n, R_ * fi, R_ * fi + 5, 3)
    assert not fx2.aligned() and not fm2.aligned()
    D.rgcn_aggregate(ctx, *side, fx2.view, fm2.view, R_)
    assert np.array_equal(_bits(fm2.numpy()), _bits(m_f))
    fx2.untouched("x is not written")
    # ... and aligned frames: the 16-byte kernel, the same bits again
    fm3 = Frame(ctx, c.n, R_ * fi, R_ * fi + 4, 12)
    D.rgcn_aggregate(ctx, *side, fx.view, fm3.view, R_)
    assert np.array_equal(_bits(fm3.numpy()), _bits(m_f))


@pytest.mark.parametrize("f", [1, 3, 50])
def test_rgcn_aggregate_any_width_and_alignment(ctx, f):
    from gcnx import device as D
    for R_ in (2, 4):
        c = _case("tiny", 16, R_)
        a = c.csr(ctx)
        ops_dev = _operator(ctx, a, c)
        x = np.random.default_rng(f).standard_normal((c.n, f)).astype(np.float32)
        for wt in (0, 1):
            side = _sides(ctx, a, ops_dev, wt)
            fx, fm = Frame(ctx, c.n, f, f + 2, 1, data=x), Frame(ctx, c.n, R_ * f, R_ * f + 1, 5)
            D.rgcn_aggregate(ctx, *side, fx.view, fm.view, R_)
            _, r_m = _ref(c.ops, x, np.zeros((R_ + 1, f, 1)), None, R_, False, wt)
            _frame_close(fm, r_m, TIGHT, f"M f={f} R={R_} wt={wt}")
            fx.untouched()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def test_rgcn_refusals_launch_and_write_nothing(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    c = _case("tiny", 16, 3)
    a = c.csr(ctx)
    ops_dev = _operator(ctx, a, c)
    side = _sides(ctx, a, ops_dev, 0)
    n = c.n

    def refused(x, fi, fo, R_, text, code=_lib.ERR_UNSUPPORTED, m_ld=None, out_lead=0):
        w = ctx.zeros(((R_ + 1) * fi, fo))
        out, m = Frame(ctx, n, fo, fo, out_lead), Frame(ctx, n, max(R_, 1) * fi, m_ld or max(R_, 1) * fi, 0)
        with pytest.raises(_lib.GcnxError, match=text) as err:
            D.rgcn_conv(ctx, *side, x, w, None, out.view, R_, True, m=m.view)
        assert err.value.code == code
        out.untouched("out"); m.untouched("m")

    assert not D.rgcn_conv_ok(ctx, n, 96, 64, 3) and not D.rgcn_conv_ok(ctx, n, 16, 256, 3) and not D.rgcn_conv_ok(ctx, n, 16, 48, 3)
    assert not D.rgcn_conv_ok(ctx, n, 16, 64, 5) and not D.rgcn_conv_ok(ctx, n, 16, 64, 0) and not D.rgcn_conv_ok(ctx, n, 16, 64, 3, 18)
    shape_text = "fi and fo in \\{16, 32, 64, 128\\}, num_relations in 1 .. 4"
    refused(ctx.zeros((n, 96)), 96, 64, 3, shape_text)
    refused(ctx.zeros((n, 16)), 16, 256, 3, shape_text)
    refused(ctx.zeros((n, 16)), 16, 48, 3, shape_text)
    wide = ctx.zeros((n, 18))
    refused(DeviceArray(ctx, wide.ptr, (n, 16), np.float32, ld=18, base=wide), 16, 64, 3, shape_text)      # ldx % 4 != 0
    off = Frame(ctx, n, 16, 16, 1, data=c.x)                                                               # x one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4
    refused(off.view, 16, 64, 3, "16-byte aligned")
    refused(ctx.zeros((n, 16)), 16, 64, 3, "16-byte aligned", m_ld=3 * 16 + 2)                             # ldm % 4 != 0
    refused(ctx.zeros((n, 16)), 16, 64, 3, "16-byte aligned", out_lead=1)                                  # out off a boundary
    # num_relations outside 1 .. 4 through the C ABI (the wrapper's own shape assertions aside)
    x, w, out = ctx.zeros((n, 16)), ctx.zeros((6 * 16, 64)), Frame(ctx, n, 64, 64, 0)
    for bad in (0, 5):
        rc = ctx.lib.gcnx_rgcn_conv(ctx.h, side[0].ptr, side[1].ptr, side[2].ptr, side[3].ptr, x.ptr, 16, n, 16, w.ptr, 1, 64, bad, 0, None,
                                    None, 0, out.view.ptr, 64)
        assert rc == _lib.ERR_UNSUPPORTED
        rc = ctx.lib.gcnx_rgcn_aggregate(ctx.h, side[0].ptr, side[1].ptr, side[2].ptr, side[3].ptr, x.ptr, 16, n, 16, bad, out.view.ptr, 64)
        assert rc == 1                                                                                     # GCNX_ERR_INVALID
    # NULL mandatory pointers, negative n, aliasing: invalid arguments
    for kw in (dict(x=None), dict(w=None), dict(n=-1), dict(rel=None), dict(alias=True)):
        xp = None if "x" in kw else x.ptr
        rc = ctx.lib.gcnx_rgcn_conv(ctx.h, side[0].ptr, side[1].ptr, None if "rel" in kw else side[2].ptr, side[3].ptr, xp, 16,
                                    kw.get("n", n), 16, None if "w" in kw else w.ptr, 1, 64, 3, 0, None, None, 0,
                                    x.ptr if "alias" in kw else out.view.ptr, 64)
        assert rc in (1, _lib.ERR_UNSUPPORTED) and (rc == 1 or "alias" in kw), kw
    out.untouched("refused calls write nothing")
    # the operator's refusals
    e = ctx.to_device(c.e)
    perm = a.transpose_perm()[2]
    bufs = [ctx.empty(c.nnz, np.uint8), ctx.empty(c.nnz), ctx.empty(c.nnz, np.uint8), ctx.empty(c.nnz)]
    call = lambda edge_dim, rule, r, pm=perm.ptr: ctx.lib.gcnx_rgcn_operator(ctx.h, a.rowptr.ptr, e.ptr, 2, edge_dim, rule, r, pm, n, c.nnz,
                                                                            bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
    assert call(2, 0, 3) == _lib.OK
    for args, text in (((2, 0, 2), "edge_dim \\+ 1"), ((2, 2, 3), "rule"), ((1, 1, 5), "num_relations"), ((1, 1, 0), "num_relations"),
                       ((0, 1, 2), "edge_dim >= 1"), ((3, 1, 2), "lde >= edge_dim"), ((2, 0, 3, None), "perm_t, rel_t and val_t")):
        assert call(*args) == 1, args
        assert text.replace("\\", "") in ctx.lib.gcnx_last_error(ctx.h).decode(), (args, ctx.lib.gcnx_last_error(ctx.h))


# ---- 6. capture -----------------------------------------------------------------------------------------------------------
def test_rgcn_conv_captured_replay_is_bit_identical(ctx):
    from gcnx import device as D
    fi, fo, R_ = 64, 64, 3
    c = _case("ecoli", fi, R_)
    a = c.csr(ctx)
    side = _sides(ctx, a, _operator(ctx, a, c), 0)
    rng = np.random.default_rng(5)
    w, _, bias = _weights(rng, fi, fo, R_ + 1, 0)
    out_e, m_e = _run_fused(ctx, side, c.x, w, bias, fo, R_, True, 0)
    x, dw, b, e = ctx.to_device(c.x), ctx.to_device(w.reshape(-1, fo)), ctx.to_device(bias), ctx.to_device(c.e)
    out, m, m2 = ctx.zeros((c.n, fo)), ctx.zeros((c.n, R_ * fi)), ctx.zeros((c.n, R_ * fi))
    rel, val = ctx.zeros(c.nnz, np.uint8), ctx.zeros(c.nnz)
    perm = a.transpose_perm()[2]
    rel_t, val_t = ctx.zeros(c.nnz, np.uint8), ctx.zeros(c.nnz)

    def step():                                                                        # operator, one launch, panel alone
        ctx._ck(ctx.lib.gcnx_rgcn_operator(ctx.h, a.rowptr.ptr, e.ptr, 2, 2, 0, R_, perm.ptr, c.n, c.nnz, rel.ptr, val.ptr, rel_t.ptr, val_t.ptr))
        D.rgcn_conv(ctx, a.rowptr, a.colidx, rel, val, x, dw, b, out, R_, True, m=m)
        D.rgcn_aggregate(ctx, a.rowptr, a.colidx, rel, val, x, m2, R_)
    g = ctx.capture(step)
    try:
        assert not out.numpy().any()                                                   # captured, not yet executed
        for _ in range(2):
            out.fill_zero(); m.fill_zero(); m2.fill_zero()
            g.launch()
            assert np.array_equal(_bits(out.numpy()), _bits(out_e)) and np.array_equal(_bits(m.numpy()), _bits(m_e))
            assert np.array_equal(_bits(m2.numpy()), _bits(m_e)) and np.array_equal(rel.numpy(), c.rel.astype(np.uint8))
    finally:
        g.destroy()


# ---- 7. the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("R_,root_weight", [(3, True), (2, False)])
def test_rgcnconv_layer_forward_and_backward(ctx, R_, root_weight, fused):
    from gcnx.layers import RGCNConv
    c = _case("tiny", 16, R_)
    a = RGCNConv.preprocess(c.csr(ctx))
    lay = RGCNConv(64, num_relations=None if R_ == 3 else R_, relations=c.rule, root_weight=root_weight, seed=3, fused=fused)
    x, e = ctx.to_device(c.x), ctx.to_device(c.e)
    y = lay([x, a, e])
    assert lay.R == R_ and list(lay.params) == (["weight", "root", "bias"] if root_weight else ["weight", "bias"])
    assert lay._one_launch(x, 64, y) == fused
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    w = p["weight"].reshape(R_, 16, 64)
    r_y, r_m = RR.conv_fwd(c.ops, c.x, w, p.get("root"), p["bias"])
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((c.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r_dx, r_dw, r_droot, r_db = RR.conv_bwd(c.ops, c.x, w, p.get("root"), dy)
    assert rel_err(dx.numpy(), r_dx) < TIGHT
    assert rel_err(lay.grads["weight"].numpy(), r_dw.reshape(R_ * 16, 64)) < TIGHT and rel_err(lay.grads["bias"].numpy(), r_db) < TIGHT
    if root_weight:
        assert rel_err(lay.grads["root"].numpy(), r_droot) < TIGHT
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    # e refilled in place: the next call reads the new relations (the layer keeps none across calls)
    e2 = np.roll(c.e, 7, axis=0)
    assert not np.array_equal(RR.relations(e2, c.rule, R_), c.rel)
    e.copy_from_host(e2)
    y2 = lay([x, a, e])
    r_y2, _ = RR.conv_fwd(RR.operators(c.rowptr, c.colidx, RR.relations(e2, c.rule, R_), R_), c.x, w, p.get("root"), p["bias"])
    assert rel_err(y2.numpy(), r_y2) < TIGHT and not rel_err(r_y, r_y2) < 1e-3
    with pytest.raises(ValueError):
        lay([x, a])
    with pytest.raises(ValueError):
        lay([x, a, ctx.zeros((c.nnz - 1, c.e.shape[1]))])


# ---- 8. gcnx.RGCN: a full step on either route against the kink-separated restatement ------------------------------------------
def _device_batch(ctx, c, e=None):
    from gcnx.device import Segments
    from gcnx.models import DeviceBatch
    return DeviceBatch(ctx, ctx.to_device(c.x), c.csr(ctx), Segments(ctx, c.gp), ctx.to_device(c.y), e=ctx.to_device(c.e if e is None else e))


def _kinks(m, pre=None):
    b = m._bufs
    if m.norm != "batch":
        return {}
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    return {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
            for i in (1, 2)}


def _oracle(m, c, p, sides):
    arg = m._bufs["arg"].numpy().astype(np.int64) if m.readout == "max" else None
    return RR.model(c.x, c.rowptr, c.colidx, c.e, c.gp, p, c.y, rule=c.rule, num_relations=c.R, masks=sides, argmax=arg,
                    readout=m.readout, norm=m.norm)


def _cmp_grads(got, ref, tol, what):
    worst = 0.0
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN.get(k, k)], np.float64))))
        diff = float(np.max(np.abs(g - r)))
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)
        worst = max(worst, err)
        assert err <= tol, (what, k, err)
    return worst


def _check_step(m, batch, c, p, tol, what):
    sides = {}
    if m.norm == "graph":       # GraphNorm·PReLU: the sides are the signs of y1 / y2 of a forward of its own (the max readout's backward overwrites y2)
        m(batch)
        sides = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
    m.loss_and_grads(batch)
    sides.update(_kinks(m))
    r = _oracle(m, c, p, sides)
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol and la[1] == r["hits"], (la, r["loss"], r["hits"])
    got = m.gradients()
    assert list(got) == [k for k, _, _ in m.TORCH_KEYS]
    worst = _cmp_grads(got, r["grads"], tol, what)
    print(f"RGCN step {what}: logits {rel_err(m._bufs['out'].numpy(), r['out']):.2e} worst gradient {worst:.2e} ({worst / tol:.2f} of the bound)")
    return r


STEP_CASES = {"R3-nonzero": (3, {}), "R2-index": (2, {}), "no-root": (3, dict(root_weight=False)), "graph-norm": (3, dict(norm="graph")),
              "attention": (3, dict(readout="attention"))}


@pytest.mark.parametrize("case", list(STEP_CASES))
@pytest.mark.parametrize("fused", ["1", "0"])
def test_rgcn_step_against_the_restatement(ctx, monkeypatch, fused, case):
    import gcnx
    R_, kw = STEP_CASES[case]
    c = _case("tiny", 16, R_)
    batch = _device_batch(ctx, c)
    monkeypatch.setenv("GCNX_RGCN_FUSED", fused)
    mk = dict(relations="index", num_relations=R_) if c.rule == "index" else {}
    m = gcnx.RGCN(ctx, hidden_channels=64, seed=0, **mk, **kw)
    assert m._fused == (fused == "1") and m.uses_edge_features and m.R == R_
    p = {k: v.astype(np.float32) for k, v in RR.init_params(16, 64, R_, seed=7, **kw).items()}
    m.load_state_dict(p)
    sd = m.state_dict()
    assert list(sd) == list(RR.keys(**kw)) and all(np.array_equal(_bits(sd[k]), _bits(p[k])) for k in p)
    what = f"{case} fused={fused}"
    _check_step(m, batch, c, p, 1e-4, what)
    b = m._bufs
    assert m._one_launch(batch.x, 64, b["z1"], b["pm1"]) == (fused == "1") and m._one_launch(b["dz2"], 64, b["dy1"]) == (fused == "1")
    # five SGD steps, each restated step on the kink sides of that step (taken with the step's own weights; GraphNorm·PReLU:
    # the signs of y1 / y2 of a forward of its own before the step, as in _check_step)
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    for _ in range(5):
        pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
        sides = {}
        if m.norm == "graph":
            m(batch)
            sides = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
        m.train_step(batch, lr=0.02)
        sides.update(_kinks(m, pre))
        r = _oracle(m, c, ph, sides)
        ph = RR.sgd(ph, r["grads"], 0.02)
    sd = m.state_dict()
    worst = 0.0
    for k in ph:
        worst = max(worst, rel_err(sd[k], ph[k].reshape(sd[k].shape)))
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after 5 steps {k}")
    print(f"RGCN {what}: worst weight after 5 SGD steps {worst:.2e}")


def test_rgcn_hidden_256_and_an_unaligned_input_take_the_composed_route(ctx):
    import gcnx
    from gcnx import device as D
    c = _case("tiny", 16, 3)
    m = gcnx.RGCN(ctx, hidden_channels=256, seed=0)
    assert m._fused and not D.rgcn_conv_ok(ctx, c.n, 16, 256, 3) and not D.rgcn_conv_ok(ctx, c.n, 256, 256, 3)
    p = {k: v.astype(np.float32) for k, v in RR.init_params(16, 256, 3, seed=2).items()}
    m.load_state_dict(p)
    batch = _device_batch(ctx, c)
    _check_step(m, batch, c, p, 1e-4, "hidden 256")
    assert not m._one_launch(batch.x, 256, m._bufs["z1"], m._bufs["pm1"])
    # 7 input features: conv1 composed (any width), conv2 one launch
    c7 = _case("tiny", 7, 3)
    m7 = gcnx.RGCN(ctx, hidden_channels=32, seed=0)
    p7 = {k: v.astype(np.float32) for k, v in RR.init_params(7, 32, 3, seed=2).items()}
    m7.load_state_dict(p7)
    b7 = _device_batch(ctx, c7)
    _check_step(m7, b7, c7, p7, 1e-4, "F = 7")
    assert not m7._one_launch(b7.x, 32, m7._bufs["z1"], m7._bufs["pm1"]) and m7._one_launch(m7._bufs["y1"], 32, m7._bufs["z2"], m7._bufs["pm2"])


# ---- 9. batch sources, fit, the torch-style surface ----------------------------------------------------------------------------
def _graphs(n_graphs, seed, R_=3):
    from gcnx import Graph, synth
    graphs = []
    for k, (x, a, y) in enumerate(synth.tiny_graphs(n_graphs, 16, seed=seed)):
        a = a.tocsr()
        a.sort_indices()
        graphs.append(Graph(x=x, a=a, y=y, e=_features(a.indptr, a.indices, R_, 100 + k)[0]))
    return graphs


def test_rgcn_batch_sources_give_the_same_bits_and_the_logits_read_e(ctx):
    """The same step from a host batch (x, a, e, i), a DeviceBatch that carries e and a DeviceDisjointLoader(DeviceDataset(
    edge_features=True)) batch: the same loss, hits and gradients bit for bit."""
    import gcnx
    from gcnx import ListDataset
    from gcnx.device import Segments
    from gcnx.models import DeviceBatch
    ds = ListDataset(_graphs(6, 3))
    dev = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, ds, edge_features=True), batch_size=6, epochs=1, shuffle=False)
    host = gcnx.DisjointLoader(ds, batch_size=6, epochs=1, shuffle=False)
    m = gcnx.RGCN(ctx, hidden_channels=64, seed=2)
    (inputs, target), (db, none) = next(iter(host)), next(iter(dev))
    assert none is None and len(inputs) == 4
    m.loss_and_grads(inputs, target)
    hbatch = m._last_batch
    la_h, g_h, out_h = m.loss_acc.numpy(), m.gradients(), m._bufs["out"].numpy()
    assert hbatch.a.nnz == db.a.nnz and np.array_equal(_bits(hbatch.e.numpy()), _bits(db.e.numpy()))
    rel_h = m._rel_ops[0].numpy()[:db.a.nnz]
    assert set(rel_h) == {0, 1, 2}
    preset = [v.ptr for v in db.a.transpose_perm()]
    m.loss_and_grads(db)
    assert [v.ptr for v in m._op(db)[1].transpose_perm()] == preset      # the loader's transposed pattern is used
    assert np.array_equal(m._rel_ops[0].numpy()[:db.a.nnz], rel_h)
    la_d, g_d = m.loss_acc.numpy(), m.gradients()
    gp = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(inputs[3])))]).astype(np.int32)
    mine = DeviceBatch(ctx, ctx.to_device(hbatch.x.numpy()), hbatch.a, Segments(ctx, gp), ctx.to_device(hbatch.y.numpy()),
                       e=ctx.to_device(hbatch.e.numpy()))
    m.loss_and_grads(mine)
    la_m, g_m = m.loss_acc.numpy(), m.gradients()
    for la, g in ((la_d, g_d), (la_m, g_m)):
        assert np.array_equal(_bits(la), _bits(la_h))
        assert all(np.array_equal(_bits(g[k]), _bits(g_h[k])) for k in g_h)
    assert all(np.max(np.abs(g_h[f"conv{k}.weight"][r])) > 0 for k in (1, 2) for r in range(3))
    # the logits read the relations: moving the bridges to the contacts changes them; scaling a feature does not
    x, a, e, i = inputs
    e = np.asarray(e)
    assert np.array_equal(_bits(m(inputs)), _bits(out_h)) and np.array_equal(_bits(m((x, a, 3.0 * e, i))), _bits(out_h))
    assert not np.allclose(m((x, a, e[:, ::-1].copy(), i)), out_h, rtol=1e-3, atol=1e-3)
    with pytest.raises(ValueError):
        m.loss_and_grads(inputs[:2] + inputs[3:], target)                 # (x, a, i) for a model that reads e
    with pytest.raises(ValueError):
        m((x, a, np.zeros((e.shape[0], 3), np.float32), i))               # another edge_dim
    mi = gcnx.RGCN(ctx, hidden_channels=64, relations="index", num_relations=2, seed=2)
    with pytest.raises(ValueError, match="integers in 0 .. 1"):
        mi((x, a, np.full((e.shape[0], 1), 2.0, np.float32), i))


def test_fit_and_evaluate_run_the_rgcn_model_from_device_batches(ctx):
    import gcnx
    from gcnx import ListDataset
    gs = _graphs(8, 3)
    tr, te = gcnx.DeviceDataset(ctx, ListDataset(gs[:5]), edge_features=True), gcnx.DeviceDataset(ctx, ListDataset(gs[5:]), edge_features=True)
    m = gcnx.RGCN(ctx, hidden_channels=32, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=1, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=1, schedule=lambda it: 0.01, verbose=False)
    assert len(out["history"]) == 1 and np.all(np.isfinite(out["history"][0]))
    (loss, acc), preds = gcnx.models.evaluate(m, gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False))
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and len(preds) == 1


def test_rgcn_state_dict_round_trip_and_a_single_graph(ctx):
    import gcnx
    c = _case("tiny", 16, 3)
    batch = _device_batch(ctx, c)
    m = gcnx.RGCN(ctx, seed=1)
    logits = m(batch)
    assert logits.shape == (16, 1)
    sd = m.state_dict()
    assert list(sd) == list(RR.keys()) and sd["conv1.weight"].shape == (3, 16, 64) and sd["conv2.root"].shape == (64, 64)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER) and m.p["wo1"].ptr == m.p["w1"].ptr + 4 * 3 * 16 * 64
    r = RR.model(c.x, c.rowptr, c.colidx, c.e, c.gp, sd, masks=_kinks(m), argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert_close(logits, r["out"], 1e-4, "logits of the initial weights")
    m2 = gcnx.RGCN(ctx, seed=9)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert np.array_equal(_bits(v), _bits(sd[k])), k
    assert np.array_equal(m2(batch), logits)
    assert [w.shape for w in m.get_weights()] == [sd[k].shape for k in RR.keys()]
    # a single graph: BatchNorm over one pooled row raises, as torch does
    n1 = int(c.gp[1])
    e1 = int(c.rowptr[n1])
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    gp1 = np.array([0, n1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, c.rowptr[:n1 + 1].copy(), c.colidx[:e1].copy(), None, gp1)
    b1 = DeviceBatch(ctx, ctx.to_device(c.x[:n1]), a1, Segments(ctx, gp1), ctx.to_device(c.y[:1]), e=ctx.to_device(c.e[:e1]))
    with pytest.raises(ValueError):
        m(b1)
    with pytest.raises(ValueError):
        m.train_step(b1, lr=0.01)

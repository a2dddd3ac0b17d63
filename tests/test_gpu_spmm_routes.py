"""Every launch route of csrc/spmm.hip (and the aggregations of spmm_bf16.hip / elementwise.hip) on column-slice views inside
sentinel frames, the way the models call them: GeneralGNN writes every aggregation into a slice of its concat buffer
(ldo > f) and its backward gathers from slices (ldh > f).

For every route and every layout:
  * the result inside the output frame equals, BIT FOR BIT, the same call on contiguous operands under the same knobs -- the
    route, the chunking and the summation order are functions of (n, f, plan, knobs), never of a leading dimension;
  * every element outside the view is still the sentinel, and every input frame (h, bias, y, dpooled) is untouched;
  * the contiguous result is within TIGHT (rel_err) of the float64 product (tests/spmm_route_batches.py);
  * an operand that breaks spmm_vec_ok (a pointer off a 16-byte boundary, a leading dimension that is no multiple of 4
    floats, the bias alone 4 bytes off) takes spmm_scalar_kernel whatever plan or knob is set: the bits of that kernel run
    on its own.
No route was found whose bits depend on a leading dimension.

The batches hold every scheduling class at minimum size (tests/spmm_route_batches.py, pinned on the host by
tests/test_spmm_route_batches_host.py); each case restates the dispatch rule that sends it to the kernel it names as an assert
on its own shape (cus from ctx.info()), so on any chip it reaches that kernel or fails loudly.  Every frame has a tail of
n * (ld - f) + 64 elements: a store that took f for the row stride, or ran a slab past the view, lands in the sentinels."""
import contextlib

import numpy as np
import pytest

import spmm_route_batches as B
from conftest import assert_close, rel_err
from gpu_frames import Frame, same as _same

pytestmark = pytest.mark.gpu

TIGHT = 2e-5                       # as tests/test_gpu_kernels.py
LAYOUTS = ["contiguous", "aligned", "unaligned", "bias4"]
KNOB_DEFAULTS = {"spmm_kernel": "auto", "spmm_cap1": 0, "spmm_sg": 0, "spmm_conc": 0, "spmm_cb": 1}
_CACHE = {}


def O():
    from oracle import gcn_oracle
    return gcn_oracle


@contextlib.contextmanager
def _knobs(ctx, **kw):
    try:
        for k, v in kw.items():
            ctx.set_tuning(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_tuning(k, KNOB_DEFAULTS[k])


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frame(ctx, n, f, ld, lead, data=None, dtype=np.float32):
    return Frame(ctx, n, f, ld, lead, data, tail=n * (ld - f) + 64, dtype=dtype)


def _place(ctx, n, f, layout, role, data=None):
    """An [n, f] float32 operand in its frame.  aligned: lead % 4 == 0, ld % 4 == 0, ld > f, ldh != ldo, sentinel columns on
    both sides.  unaligned: h one float off a 16-byte boundary, out with a leading dimension that is no multiple of 4."""
    f4 = (f + 3) // 4 * 4
    if layout == "contiguous":
        ld, lead = f, 0
    elif layout in ("aligned", "bias4"):
        ld, lead = (f4 + 8, 4) if role == "in" else (f4 + 16, 8)
    else:
        ld, lead = (f4 + 8, 1) if role == "in" else (f4 + 13, 4)
    fr = _frame(ctx, n, f, ld, lead, data)
    assert fr.aligned() == (layout != "unaligned" and ld % 4 == 0)
    return fr


def _place_bias(ctx, f, layout, data):
    fr = _frame(ctx, 1, f, f, {"contiguous": 0, "aligned": 4, "unaligned": 1, "bias4": 1}[layout], data)
    assert (fr.view.ptr % 16 == 4) == (layout in ("unaligned", "bias4"))
    return fr


def _vals(b, kind):
    return {"none": lambda: None, "gcn": lambda: B.gcn_vals(b), "skew": lambda: B.skew_vals(b)}[kind]()


def _csr(ctx, b, kind, symmetric=None):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, b.rowptr, b.colidx, _vals(b, kind), b.gp, symmetric=symmetric)


def _h1():
    return _memo("h1", lambda: B.features(B.batch1().n))


def _bias():
    return _memo("bias", lambda: np.random.default_rng(5).standard_normal(B.FMAX).astype(np.float32))


def _ref1(kind):
    """A h of batch 1 in float64 at the full width, computed once; the batch without the column-block graph is its leading
    rows (block diagonal), a narrower h its leading columns."""
    return _memo(("ref1", kind), lambda: B.ref_spmm(B.batch1(), _vals(B.batch1(), kind), _h1()))


def _want(ref, f, act):
    return np.maximum(ref[:, :f] + _bias()[:f], 0) if act else ref[:, :f]


def _units(cus, n1, n2, f):
    """tile_units_fill: whether gcnx_spmm_csr takes the tile kernels without being asked to."""
    return (n1 + 2 * n2) * (f // 32) >= 4 * cus


def _spmm(ctx, a, h, bias, f, act, layout):
    """One gcnx_spmm_csr call in `layout`; asserts the frames and returns the result."""
    from gcnx import device as D
    n = a.n
    hf, of = _place(ctx, n, f, layout, "in", h), _place(ctx, n, f, layout, "out")
    bf = _place_bias(ctx, f, layout, bias) if act else None
    D.spmm(ctx, a, hf.view, bf.row(0) if bf else None, of.view, act="relu" if act else None)
    got = of.numpy()                                               # (asserts the sentinels around the view)
    hf.untouched((layout, "h"))
    if bf:
        bf.untouched((layout, "bias"))
    return got


def _scalar_alone(ctx, b, bkey, kind, f, act):
    """spmm_scalar_kernel on its own: an operator without a plan, dense rows, h one float off a 16-byte boundary."""
    def run():
        from gcnx import device as D
        from gcnx.device import DeviceCSR
        a = DeviceCSR.from_host_csr(ctx, b.rowptr, b.colidx, _vals(b, kind), None)
        assert a.plan is None
        hf, of = _frame(ctx, b.n, f, f, 1, _h1()[:b.n, :f]), _frame(ctx, b.n, f, f, 0)
        assert hf.view.ptr % 16 == 4
        bias = ctx.to_device(_bias()[:f]) if act else None
        D.spmm(ctx, a, hf.view, bias, of.view, act="relu" if act else None)
        return of.numpy()
    return _memo(("scalar", bkey, kind, f, act), run)


def _forward(ctx, b, bkey, f, layout, route, plan, kinds=("none", "gcn")):
    """The four calls (plain / bias + ReLU, unweighted / weighted) of one route in one layout."""
    ref_rows = b.n
    for kind in kinds:
        a = _csr(ctx, b, kind)
        assert (a.plan is not None) == plan, "the route's precondition on the plan"
        ref = _ref1(kind)[:ref_rows]
        for act in (False, True):
            what = (route, f, kind, act, layout)
            h, bias = _h1()[:b.n, :f], _bias()[:f]
            base = _spmm(ctx, a, h, bias, f, act, "contiguous")
            assert_close(base, _want(ref, f, act), TIGHT, f"spmm route {route} f={f} {kind} relu={act}")
            if layout == "contiguous":
                assert _same(_spmm(ctx, a, h, bias, f, act, "contiguous"), base), (what, "not deterministic")
                continue
            if layout == "bias4" and not act:
                continue
            got = _spmm(ctx, a, h, bias, f, act, layout)
            if layout == "aligned":
                assert _same(got, base), (what, "strided operands change the bits")
            else:                                                  # !vec is decided first: the scalar kernel's bits
                scal = _scalar_alone(ctx, b, bkey, kind, f, act)
                assert rel_err(scal, _want(ref, f, act)) < TIGHT, what
                assert _same(got, scal), (what, "not the scalar kernel's result")


# ------------------------------------------------------------------------------------------- gcnx_spmm_csr
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", [10, 8])
def test_scalar_kernel(ctx, f, layout):
    """spmm_scalar_kernel: f = 10 is no multiple of 4 (spmm_vec_ok fails in every layout); f = 8 reaches it only through an
    unaligned operand (the other layouts take the row gather at the 4-lane split, which the bit comparison then holds to its
    own contiguous result).  All of batch 1, plan bound: !vec is decided before any plan is looked at."""
    b = B.batch1()
    assert f % 4 != 0 or f == 8
    _forward(ctx, b, "b1", f, layout, "scalar", plan=True)
    if f == 10:                                                    # every layout is the scalar kernel's
        a = _csr(ctx, b, "gcn")
        got = _spmm(ctx, a, _h1()[:, :f], _bias()[:f], f, True, layout)
        assert _same(got, _scalar_alone(ctx, b, "b1", "gcn", f, True))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", [16, 32, 64, 128, 256, 512])
def test_row_gather_without_a_plan(ctx, f, layout):
    """spmm_rows_kernel over all rows in order (launch_gather without a plan: dispatch_rows(NULL list)), knob "rows", on batch 1
    without its 4 096-row graph -- fewer than 128 graphs, no graph of 4 096 rows: DeviceCSR.plan is None.  f / 4 lanes per row:
    4, 8, 16, 32, 64 lanes, and at f = 512 the second col0 pass of the 64-lane split.  n < 128k rows: 8-row chunks; the hub
    graph's eight 300-entry rows are split over the workgroup's waves (more than kLongRowSmall entries) and together overflow
    the chunk's LDS staging (2 400 > kStageCap)."""
    b = B.batch1(with_cb=False)
    assert b.n < 16 * 1024 * 32 // 4 and {16: 4, 32: 8, 64: 16, 128: 32, 256: 64, 512: 128}[f] == f // 4
    hub = B.degrees(b, B.HUB1)
    assert (hub > 256).sum() == 8 and hub[B.DENSE8:B.DENSE8 + 8].sum() > 2048 and (b.gp[B.HUB1] + B.DENSE8) % 8 == 0
    with _knobs(ctx, spmm_kernel="rows"):
        _forward(ctx, b, "b1-", f, layout, "rows/no plan", plan=False)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f,cb", [(128, 1), (256, 1), (64, 1), (256, 0)])
def test_gather_with_a_bound_plan(ctx, f, cb, layout):
    """launch_gather with a bound plan, knob "auto": the 4 096-row graph makes DeviceCSR.plan build a plan, the batch has too
    few tile units for tiles_worth_it.  f >= kCbMinF = 128 and spmm_cb = 1 (cb_path_ok): plan->rest chunks on spmm_rows_kernel
    (HUBS), the hub graph's rows as spmm_hub_seg_kernel + spmm_hub_combine_kernel, the 4 096-row graph on spmm_cb_kernel in
    one (f = 128) and two (f = 256) sets of 64-column blocks -- short rows, rows of 33 .. 256 entries, the hub row and the
    2 500-entry row.  f = 64, or spmm_cb = 0: no column blocks, all rows in order on the row gather and every hub row of both
    graphs as segments."""
    b = B.batch1()
    cus = ctx.info()["cus"]
    n2 = sum(0 < m <= B.SOLO_CAP for m in b.sizes)
    assert not _units(cus, 0, n2, f) and max(b.sizes) >= B.CB_MIN_ROWS
    assert (f >= B.CB_MIN_F and f % 64 == 0) == (f != 64) and b.n * (f + 8) * 4 < 0xFFFFFF00
    cbd = B.degrees(b, B.CB1)
    assert (cbd <= 32).any() and ((cbd > 32) & (cbd <= 256)).any() and (cbd > 256).sum() == 2 and (cbd > 2048).sum() == 1
    with _knobs(ctx, spmm_cb=cb):
        _forward(ctx, b, "b1", f, layout, f"gather/plan cb={cb}", plan=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f,cap1,sg,conc", [(32, -1, 0, 0), (64, -1, 0, 0), (256, -1, 0, 0), (64, 0, 0, 0), (256, 0, 0, 0),
                                            (256, -1, 1, 0), (256, -1, 4, 0), (256, -1, 0, 1), (256, 0, 0, 1)])
def test_tile_tiers(ctx, f, cap1, sg, conc, layout):
    """Knob "tile" (tiles_worth_it by force) on all of batch 1, in one call: spmm_duo_kernel<512> (tier 1: graphs up to 632
    rows, with spmm_cap1 = -1) and spmm_duo_kernel<1024> (tier 2: up to 1 276 rows; double-buffered up to 624) side by side,
    the 1 277-row graph and the hub graph as plan-listed 8-row chunks on spmm_rows_kernel, the hub rows as segments (launch_hubs, tall only), the
    4 096-row graph on spmm_cb_kernel (f >= 128) or on the row chunks (narrower).  spmm_cap1 = 0, the default: every tile
    graph on the 1024-thread shape.  spmm_sg: slab groups of 1 and 4.  spmm_conc = 1: the launches as concurrent branches on
    the auxiliary streams."""
    b = B.batch1()
    tier1 = sum(0 < m <= B.DUO_CAP for m in b.sizes) if cap1 == -1 else 0
    tier2 = sum(0 < m <= B.SOLO_CAP for m in b.sizes) - tier1
    assert (tier1 > 0) == (cap1 == -1) and tier2 > 0 and [m for m in b.sizes if m > B.SOLO_CAP] == [1277, 1400, 4096]
    assert sg == 0 or (f // 32) % sg == 0
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=cap1, spmm_sg=sg, spmm_conc=conc):
        _forward(ctx, b, "b1", f, layout, f"tile cap1={cap1} sg={sg} conc={conc}", plan=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("f", [32, 128, 256])
def test_pipelined_kernel(ctx, f, layout):
    """Knob "pipe": spmm_pipe_kernel<32> for the graphs up to kPipeCap32 = 624 rows, spmm_pipe_kernel<16> for 625 .. 1 024 rows
    (kPipeCap16), and the taller graphs (1 025, 1 276, 1 277, 1 400, 4 096 rows) as 32-row chunks on spmm_rows_kernel.
    f <= kPipeMaxF = 512 and n * ldo * 4 < 2^32 (pipe_ok)."""
    b = B.batch1()
    assert any(0 < m <= 624 for m in b.sizes) and any(624 < m <= 1024 for m in b.sizes) and any(m > 1024 for m in b.sizes)
    assert f <= 512 and b.n * (f + 16) * 4 < 0xFFFFFFF0
    with _knobs(ctx, spmm_kernel="pipe"):
        _forward(ctx, b, "b1", f, layout, "pipe", plan=True)


# ------------------------------------------------------------------------------------------- gcnx_spmm_csr_relu_bits
def _unpack(words, f):
    """[f / 32, rows] words -> [rows, f] booleans."""
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).transpose(1, 0, 2).reshape(w.shape[1], f)


def _clear_bias(ref, f):
    """A bias that keeps every value of ref + bias further than 1e-6 max|ref| from zero (asserted): the sign of a device
    result that is a few fp32 roundings of max|ref| off is then the reference's."""
    bias = _bias()[:f].copy()
    top = np.abs(ref).max()
    for _ in range(8):
        close = np.abs(ref + bias) < 1e-6 * top
        if not close.any():
            break
        bias[close.any(0)] += np.float32(3e-4)
    assert not (np.abs(ref + bias) < 1e-6 * top).any()
    return bias


@pytest.mark.parametrize("layout", ["contiguous", "aligned", "unaligned"])
@pytest.mark.parametrize("f,cap1", [(64, -1), (256, 0)])
def test_relu_bits_on_the_tile_route(ctx, f, cap1, layout):
    """gcnx_spmm_csr_relu_bits under the knob "tile" on batch 1: spmm_duo_kernel in mode kDuoBitsOut (both tiers with
    spmm_cap1 = -1).  The image sits in a frame of exactly (f / 32) * n 32-bit words.  Rows of tile graphs: bit c of word
    [slab, row] is [out > 0], and equals [ref > 0] (the bias keeps every reference value further than 1e-6 max|ref| from
    zero).  Rows of the three graphs taller than a tile: "graphs taller than a tile get no bits" (include/gcnx.h) -- their words
    are not written, `out` holds their rows.  A call the tile kernels do not serve -- knob "rows", knob "pipe", or an
    unaligned operand, for which gcnx_spmm_csr takes spmm_scalar_kernel (before this test such a call ran that kernel and
    answered "served" without a bit image) -- answers ERR_UNSUPPORTED and writes nothing at all."""
    from gcnx import device as D, _lib as L
    b = B.batch1()
    n = b.n
    a = _csr(ctx, b, "gcn")
    ref = _ref1("gcn")[:, :f]
    bias = _clear_bias(ref, f)
    want = np.maximum(ref + bias, 0)
    tile_rows, tall_rows = B.rows_of(b, lambda m: 0 < m <= B.SOLO_CAP), B.rows_of(b, lambda m: m > B.SOLO_CAP)
    assert len(tile_rows) + len(tall_rows) == n and len(tall_rows) == 1277 + 1400 + 4096

    def call(lay):
        hf, of, bf = _place(ctx, n, f, lay, "in", _h1()[:, :f]), _place(ctx, n, f, lay, "out"), _place_bias(ctx, f, lay, bias)
        img = _frame(ctx, 1, (f // 32) * n, (f // 32) * n, 4, dtype=np.int32)
        served = D.spmm_relu_bits(ctx, a, hf.view, bf.row(0), of.view, img.row(0))
        hf.untouched("h"), bf.untouched("bias")
        return served, of, img

    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=cap1):
        assert a.plan is not None
        served, of0, img0 = call("contiguous")
        assert served
        base, words0 = of0.numpy(), img0.numpy().reshape(f // 32, n)
        assert_close(base, want, TIGHT, f"spmm_relu_bits tile f={f} cap1={cap1}")
        assert np.array_equal(_unpack(words0[:, tile_rows], f), base[tile_rows] > 0)
        assert np.array_equal(_unpack(words0[:, tile_rows], f), want[tile_rows] > 0)   # (no reference value within 1e-6 max|ref| of 0)
        assert (words0[:, tall_rows] == img0.sentinel).all()       # no bits for graphs taller than a tile
        if layout == "aligned":
            served, of1, img1 = call(layout)
            assert served
            of1.check(base, "out")
            img1.check(words0.reshape(1, -1), "bit image")
        if layout == "unaligned":                                  # gcnx_spmm_csr would take the scalar kernel, which writes no bits
            served, of1, img1 = call(layout)
            assert not served
            of1.untouched("out"), img1.untouched("bit image")
            return
    for knob in ("rows", "pipe"):
        with _knobs(ctx, spmm_kernel=knob):
            if knob == "rows":
                assert a.plan is not None                          # (the 4 096-row graph)
            hf, of, img = _place(ctx, n, f, layout, "in", _h1()[:, :f]), _place(ctx, n, f, layout, "out"), \
                _frame(ctx, 1, (f // 32) * n, (f // 32) * n, 4, dtype=np.int32)
            rc = ctx.lib.gcnx_spmm_csr_relu_bits(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.vals.ptr, hf.view.ptr, hf.view.ld, None,
                                                 of.view.ptr, of.view.ld, n, f, a.plan, img.view.ptr)
            assert rc == L.ERR_UNSUPPORTED, knob
            of.untouched("out"), img.untouched("bit image"), hf.untouched("h")


# ------------------------------------------------------------------------------------------- gcnx_spmm_csr_relu_bits_pool
def _b2(ctx, f=256, hub=False):
    return B.batch2(ctx.info()["cus"], f, hub)


def _h2(b):
    return _memo(("h2", b.n), lambda: B.features(b.n, seed=13))


def _ref2(b, kind, hub=False):
    return _memo(("ref2", b.n, kind, hub), lambda: B.ref_spmm(b, _vals(b, kind), _h2(b)[:, :256]))


@pytest.mark.parametrize("layout", ["contiguous", "aligned"])
@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_relu_bits_pool_defines_every_pooled_row(ctx, mode, layout):
    """gcnx_spmm_csr_relu_bits_pool on batch 2 (knob "tile" for the plan of a batch of fewer than 128 graphs; spmm_cap1 = 0
    before the plan is created: n1 == 0; 2 n2 (f / 32) >= 4 cus): spmm_duo_kernel<1024> in mode kDuoBitsPool +
    pool_parts_reduce_kernel for the tile graphs, 8-row chunks on spmm_rows_kernel + gcnx_pool_graph_list for the two tall
    graphs, pool_empty_rows_kernel for the empty graph BETWEEN the two tall graphs.  The call must be served.  pooled in a
    frame with ldp > f, cnt and out framed.  Pooled rows against the float64 pool of relu(A h + b) at TIGHT, counts exact;
    rows of tile graphs in `out` are NOT written, rows of the tall graphs are and are correct; the empty graph's pooled and
    cnt rows hold what gcnx_segment_pool gives for an empty segment (zeros) -- before this test no launch of the call wrote
    them (the plan lists an empty graph nowhere, and the tall graphs' pool walks the listed graphs only)."""
    from gcnx import device as D
    from gcnx.device import Segments
    f = 256
    b = _b2(ctx)
    cus = ctx.info()["cus"]
    n, nb = b.n, len(b.sizes)
    empty = b.sizes.index(0)
    n2 = sum(0 < m <= B.SOLO_CAP for m in b.sizes)
    assert b.sizes[empty - 1] > B.SOLO_CAP and b.sizes[empty + 1] > B.SOLO_CAP and _units(cus, 0, n2, f)
    ref = _ref2(b, "gcn")
    bias = _clear_bias(ref, f)
    want = np.maximum(ref + bias, 0)
    pooled_ref, _ = O().global_pool_fwd(want, b.gp, mode)
    tile_rows, tall_rows = B.rows_of(b, lambda m: 0 < m <= B.SOLO_CAP), B.rows_of(b, lambda m: m > B.SOLO_CAP)
    seg = Segments(ctx, b.gp)
    # what gcnx_segment_pool gives for the empty segment
    sp = _frame(ctx, nb, f, f, 0)
    D.segment_pool(ctx, seg, ctx.to_device(want.astype(np.float32)), sp.view, mode)
    empty_row = sp.numpy()[empty]
    assert not empty_row.any()
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=0):
        a = _csr(ctx, b, "gcn")
        assert a.plan is not None
        hf, of, bf = _place(ctx, n, f, layout, "in", _h2(b)[:, :f]), _place(ctx, n, f, layout, "out"), _place_bias(ctx, f, layout, bias)
        pf = _frame(ctx, nb, f, f if layout == "contiguous" else f + 12, 0 if layout == "contiguous" else 4)
        cf = _frame(ctx, nb, f, f, 4)
        img = _frame(ctx, 1, (f // 32) * n, (f // 32) * n, 4, dtype=np.int32)
        assert D.spmm_relu_bits_pool(ctx, a, hf.view, bf.row(0), of.view, img.row(0), seg, pf.view, cf.view, mode), "not served"
        hf.untouched("h"), bf.untouched("bias")
        out, pooled, cnt, words = of.numpy(), pf.numpy(), cf.numpy(), img.numpy().reshape(f // 32, n)
        assert (out[tile_rows] == of.sentinel).all()               # "Rows of tile graphs in `out` are NOT written"
        assert rel_err(out[tall_rows], want[tall_rows]) < TIGHT
        assert _same(pooled[empty], empty_row) and _same(cnt[empty], empty_row), "the empty graph's rows"
        assert_close(pooled, pooled_ref, TIGHT, f"spmm_relu_bits_pool {mode} pooled")
        got_y = np.where(np.isin(np.arange(n), tall_rows)[:, None], out > 0, False)
        got_y[tile_rows] = _unpack(words[:, tile_rows], f)
        cnt_dev = np.add.reduceat(got_y.astype(np.float64), np.minimum(b.gp[:-1], n - 1).astype(np.int64), axis=0)
        cnt_dev[np.diff(b.gp) == 0] = 0
        assert np.array_equal(cnt, cnt_dev)                        # exactly the positives of the device's own result ...
        cnt_ref = np.add.reduceat((want > 0).astype(np.float64), np.minimum(b.gp[:-1], n - 1).astype(np.int64), axis=0)
        cnt_ref[np.diff(b.gp) == 0] = 0
        assert np.array_equal(cnt, cnt_ref)                        # ... and of the float64 reference (none within 1e-6 max|ref| of 0)
        assert (words[:, tall_rows] == img.sentinel).all()
        if layout != "contiguous":                                 # bit for bit the contiguous call
            h0, o0, p0, c0 = ctx.to_device(_h2(b)[:, :f]), _frame(ctx, n, f, f, 0), _frame(ctx, nb, f, f, 0), _frame(ctx, nb, f, f, 0)
            i0 = _frame(ctx, 1, (f // 32) * n, (f // 32) * n, 0, dtype=np.int32)
            assert D.spmm_relu_bits_pool(ctx, a, h0, ctx.to_device(bias), o0.view, i0.row(0), seg, p0.view, c0.view, mode)
            assert _same(o0.numpy(), out) and _same(p0.numpy(), pooled) and _same(c0.numpy(), cnt)
            assert np.array_equal(i0.numpy().reshape(f // 32, n), words)


# ------------------------------------------------------------------------------------------- gcnx_spmm_csr_pool_bwd
def _pool_bwd_inputs(b, f, mode, seed, y=None):
    rng = np.random.default_rng(seed)
    if y is None:
        y = np.maximum(rng.standard_normal((b.n, f), dtype=np.float32), 0)    # a saved ReLU output (about half zeros)
    dp = rng.standard_normal((len(b.sizes), f), dtype=np.float32)
    dz = O().global_pool_bwd(dp.astype(np.float64), b.gp, b.n, mode, None) * (y > 0)
    dp_nan = dp.copy()
    dp_nan[np.diff(b.gp) == 0] = np.nan                            # the empty graph's dpooled row: read by nobody
    return y, dp_nan, dz


def _pool_bwd(ctx, at, seg, y, dp, f, mode, layout, bits=None):
    from gcnx import device as D
    n, nb = at.n, seg.n_graphs
    yf, of = _place(ctx, n, f, layout, "in", y), _place(ctx, n, f, layout, "out")
    df = _frame(ctx, nb, f, f if layout == "contiguous" else f + 20, 0 if layout == "contiguous" else 8, dp)
    D.spmm_pool_bwd(ctx, at, yf.view, seg, df.view, of.view, mode, y_bits=bits)
    yf.untouched("y"), df.untouched("dpooled")
    return of.numpy()


def _pool_bwd_case(ctx, b, f, mode, layout, route, seed):
    from gcnx.device import Segments
    seg = Segments(ctx, b.gp)
    for kind in ("skew", "none"):
        a = _csr(ctx, b, kind, symmetric=False if kind == "skew" else None)
        at = a.transpose()
        assert at.plan is not None and (kind == "none") == (at is a)
        y, dp, dz = _pool_bwd_inputs(b, f, mode, seed)
        ref = B.ref_spmm_t(b, _vals(b, kind), dz)
        base = _pool_bwd(ctx, at, seg, y, dp, f, mode, "contiguous")
        assert np.isfinite(base).all(), "the empty graph's dpooled row was read"
        assert_close(base, ref, TIGHT, f"spmm_pool_bwd {route} f={f} {kind} {mode}")
        if layout != "contiguous":
            assert _same(_pool_bwd(ctx, at, seg, y, dp, f, mode, layout), base), (route, f, kind, mode)


@pytest.mark.parametrize("layout", ["contiguous", "aligned"])
@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("f,cb", [(128, 1), (64, 1)])
def test_pool_bwd_on_the_gather_route(ctx, f, cb, mode, layout):
    """gcnx_spmm_csr_pool_bwd on batch 1, knob "auto" (too few tile units): launch_gather with FoldArgs -- f = 128:
    spmm_rows_kernel<FOLD, HUBS> over plan->rest, spmm_hub_seg_kernel<FOLD> + spmm_hub_combine_kernel<FOLD> for the hub graph,
    spmm_cb_kernel<FOLD> for the 4 096-row graph (its dpooled row through plan->cb_gids); f = 64 (< kCbMinF): all rows in
    order, every hub row as folded segments.  Non-symmetric values, the transposed operator."""
    b = B.batch1()
    assert not _units(ctx.info()["cus"], 0, sum(0 < m <= B.SOLO_CAP for m in b.sizes), f)
    with _knobs(ctx, spmm_cb=cb):
        _pool_bwd_case(ctx, b, f, mode, layout, "gather", 21)


@pytest.mark.parametrize("layout", ["contiguous", "aligned"])
@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("f,cap1", [(64, -1), (256, 0)])
def test_pool_bwd_on_the_tile_route(ctx, f, cap1, mode, layout):
    """gcnx_spmm_csr_pool_bwd on batch 1 under the knob "tile": spmm_duo_kernel<512> and <1024> in mode kDuoFold (both with
    spmm_cap1 = -1), every graph taller than a tile -- the 4 096-row graph included, no column blocks on this route -- as
    plan-listed 8-row chunks on spmm_rows_kernel<FOLD, HUBS>, their hub rows as folded segments.  Then the same from the bit
    image of gcnx_spmm_csr_relu_bits (mode kDuoFoldBits on the tiers; the taller graphs' rows from y)."""
    b = B.batch1()
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=cap1):
        _pool_bwd_case(ctx, b, f, mode, layout, f"tile cap1={cap1}", 22)
        _pool_bwd_from_bits(ctx, b, _h1(), f, mode, layout, f"tile cap1={cap1}", 26)     # mode kDuoFoldBits on both tiers


def _pool_bwd_from_bits(ctx, b, hsrc, f, mode, layout, route, seed):
    """The fold from the image gcnx_spmm_csr_relu_bits wrote (the rows of graphs taller than a tile still come from y): the
    bits of the fold from y, in every layout."""
    from gcnx import device as D
    from gcnx.device import Segments
    seg = Segments(ctx, b.gp)
    a = _csr(ctx, b, "skew", symmetric=False)
    at = a.transpose()
    y2 = ctx.empty((b.n, f))
    bits = ctx.zeros((f // 32) * b.n, np.int32)
    assert D.spmm_relu_bits(ctx, a, ctx.to_device(hsrc[:b.n, :f]), ctx.to_device(_bias()[:f]), y2, bits)
    y2h = y2.numpy()
    _, dp, dz = _pool_bwd_inputs(b, f, mode, seed, y=y2h)
    from_y = _pool_bwd(ctx, at, seg, y2h, dp, f, mode, "contiguous")
    assert np.isfinite(from_y).all()
    assert_close(from_y, B.ref_spmm_t(b, _vals(b, "skew"), dz), TIGHT, f"spmm_pool_bwd y_bits {route} f={f} {mode}")
    assert _same(_pool_bwd(ctx, at, seg, y2h, dp, f, mode, layout, bits=bits), from_y)


@pytest.mark.parametrize("layout", ["contiguous", "aligned"])
@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_pool_bwd_on_batch_2_and_from_the_bit_image(ctx, mode, layout):
    """Batch 2 (the empty graph between the two tall ones; knob "tile", spmm_cap1 = 0): mode kDuoFold from y, and mode
    kDuoFoldBits from the image gcnx_spmm_csr_relu_bits wrote (the tall graphs' rows still come from y).  Both give the bits
    of the contiguous call; the fold from the image gives the bits of the fold from y."""
    f = 256
    b = _b2(ctx)
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=0):
        _pool_bwd_case(ctx, b, f, mode, layout, "batch 2", 23)
        _pool_bwd_from_bits(ctx, b, _h2(b), f, mode, layout, "batch 2", 24)


def test_pool_bwd_refuses_an_unaligned_operand_without_a_write(ctx):
    """The folded backward has no scalar form: an operand off a 16-byte boundary, or a leading dimension that is no multiple
    of 4 floats, is refused with the message of spmm_csr_pool_bwd_impl, and nothing is written."""
    from gcnx import device as D
    from gcnx._lib import GcnxError
    from gcnx.device import Segments
    b = B.batch1(with_cb=False)
    f = 64
    seg = Segments(ctx, b.gp)
    a = _csr(ctx, b, "none")
    y, dp, _ = _pool_bwd_inputs(b, f, "sum", 25)
    nb = len(b.sizes)
    for bad in ("y", "out", "dpooled"):
        yf = _place(ctx, b.n, f, "unaligned" if bad == "y" else "aligned", "in", y)
        of = _place(ctx, b.n, f, "unaligned" if bad == "out" else "aligned", "out")
        df = _frame(ctx, nb, f, f + 20, 1 if bad == "dpooled" else 8, dp)
        with pytest.raises(GcnxError, match="multiples of 4 floats and 16-byte aligned"):
            D.spmm_pool_bwd(ctx, a, yf.view, seg, df.view, of.view, "sum")
        of.untouched(bad), yf.untouched(bad), df.untouched(bad)


# ------------------------------------------------------------------------------------------- bf16 result rows
def _ulp_apart(got, want):
    """Distance in bf16 units in the last place between two arrays of bf16 bit patterns (sign-magnitude -> ordered)."""
    def key(u):
        u = u.astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u & 0x7FFF)
    return np.abs(key(got) - key(want))


@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_bf16_result_rows_in_a_frame(ctx, mode):
    """gcnx_spmm_csr_bf16out / gcnx_spmm_csr_pool_bwd_bf16out on batch 2, f = 256, weighted (knob "tile", spmm_cap1 = 0):
    spmm_duo_kernel<1024, OUT16> for the tile graphs, spmm_rows_kernel<64, OUT16> over the 8-row chunks of the two tall
    graphs.  The result sits in a uint16 frame with ldo > f, ldo % 4 == 0: every element within one bf16 unit in the last
    place of the correctly rounded fp32-route result (tests/test_gpu_kernels.py holds these forms to equality with it on a
    large batch), the bits of the contiguous call, the frame intact."""
    from gcnx import device as D
    from gcnx.device import Segments
    o = O()
    f = 256
    b = _b2(ctx)
    n, nb = b.n, len(b.sizes)
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=0):
        a = _csr(ctx, b, "gcn")
        assert a.plan is not None and a.vals is not None
        h, bias = ctx.to_device(_h2(b)[:, :f]), ctx.to_device(_bias()[:f])
        out32 = ctx.empty((n, f))
        for act, bb in ((None, None), ("relu", bias)):
            D.spmm(ctx, a, h, bb, out32, act=act)
            c16, f16 = _frame(ctx, n, f, f, 0, dtype=np.uint16), _frame(ctx, n, f, f + 8, 8, dtype=np.uint16)
            hf = _place(ctx, n, f, "aligned", "in", _h2(b)[:, :f])
            assert D.spmm_bf16out(ctx, a, h, bb, c16.view, act=act) and D.spmm_bf16out(ctx, a, hf.view, bb, f16.view, act=act)
            hf.untouched("h")
            got = f16.numpy()
            assert np.array_equal(got, c16.numpy()), act
            assert _ulp_apart(got, o.bf16_bits(out32.numpy())).max() <= 1, act
        # the folded backward from the bit image
        seg = Segments(ctx, b.gp)
        y2, bits = ctx.empty((n, f)), ctx.zeros((f // 32) * n, np.int32)
        assert D.spmm_relu_bits(ctx, a, h, bias, y2, bits)
        _, dp, _ = _pool_bwd_inputs(b, f, mode, 31, y=y2.numpy())
        at = a.transpose()
        D.spmm_pool_bwd(ctx, at, y2, seg, ctx.to_device(dp), out32, mode, y_bits=bits)
        assert np.isfinite(out32.numpy()).all()
        yf = _place(ctx, n, f, "aligned", "in", y2.numpy())
        df = _frame(ctx, nb, f, f + 20, 8, dp)
        c16, f16 = _frame(ctx, n, f, f, 0, dtype=np.uint16), _frame(ctx, n, f, f + 8, 8, dtype=np.uint16)
        assert D.spmm_pool_bwd_bf16out(ctx, at, y2, seg, ctx.to_device(dp), c16.view, mode, y_bits=bits)
        assert D.spmm_pool_bwd_bf16out(ctx, at, yf.view, seg, df.view, f16.view, mode, y_bits=bits)
        yf.untouched("y"), df.untouched("dpooled")
        got = f16.numpy()
        assert np.array_equal(got, c16.numpy())
        assert _ulp_apart(got, o.bf16_bits(out32.numpy())).max() <= 1


@pytest.mark.parametrize("why", ["unweighted", "f = 128", "n1 > 0", "hub row in a tall graph", "column-block graph", "ldo % 4",
                                 "unaligned out"])
def test_bf16_result_rows_refusals_leave_the_frame_untouched(ctx, why):
    """Every condition of out16_shape_ok (and the hub-row check behind it) that a small batch can violate: ERR_UNSUPPORTED --
    False from the wrapper -- and not one element of the frame written."""
    from gcnx import device as D
    f = 128 if why == "f = 128" else 256
    cap1 = -1 if why == "n1 > 0" else 0
    b = B.batch1() if why == "column-block graph" else _b2(ctx, hub=why == "hub row in a tall graph")
    hsrc = _h1() if why == "column-block graph" else _h2(b)
    with _knobs(ctx, spmm_kernel="tile", spmm_cap1=cap1):
        a = _csr(ctx, b, "none" if why == "unweighted" else "gcn")
        assert a.plan is not None
        h = ctx.to_device(hsrc[:b.n, :f])
        ld, lead = {"ldo % 4": (f + 6, 8), "unaligned out": (f + 8, 2)}.get(why, (f + 8, 8))
        fr = _frame(ctx, b.n, f, ld, lead, dtype=np.uint16)
        assert not D.spmm_bf16out(ctx, a, h, None, fr.view), why
        fr.untouched(why)
        if why == "hub row in a tall graph":                       # ... and the same batch without the hub row is served
            b0 = _b2(ctx)
            a0 = _csr(ctx, b0, "gcn")
            ok = _frame(ctx, b0.n, f, f + 8, 8, dtype=np.uint16)
            assert D.spmm_bf16out(ctx, a0, ctx.to_device(_h2(b0)[:, :f]), None, ok.view)
            ok.numpy()


# ------------------------------------------------------------------------------------------- gcnx_spmm_csr_bf16
@pytest.mark.parametrize("f", [64, 128])
def test_bf16_features_in_frames(ctx, f):
    """gcnx_spmm_csr_bf16 (spmm_bf16_kernel, one route): input and output as uint16 frames with ld % 8 == 0, ld > f -- the bits
    of the contiguous call, which is held to the bound of test_spmm_bf16_features (half a unit of the final rounding plus the
    fp32 accumulation); ld % 8 != 0 or a pointer off a 16-byte boundary is refused without a write."""
    from gcnx import device as D
    from gcnx._lib import GcnxError
    o = O()
    b = B.batch1(with_cb=False)
    n = b.n
    vals = B.gcn_vals(b)
    a = _csr(ctx, b, "gcn")
    h16 = o.bf16_bits(_h1()[:n, :f])
    bias = _bias()[:f]
    rp, ci = b.rowptr.astype(np.int64), b.colidx.astype(np.int64)
    ref = o.spmm_csr_bf16(rp, ci, vals, h16, bias, True)
    mag = o.spmm_csr_bf16(rp, ci, np.abs(vals), o.bf16_bits(np.abs(o.bf16_from_bits(h16))), np.abs(bias))
    c_out = _frame(ctx, n, f, f, 0, dtype=np.uint16)
    D.spmm_bf16(ctx, a, ctx.to_device(h16), ctx.to_device(bias), c_out.view, act="relu")
    base = c_out.numpy()
    assert np.all(np.abs(o.bf16_from_bits(base).astype(np.float64) - ref) <= 2.0 ** -8 * np.abs(ref) + 2.0 ** -19 * mag)
    hf = _frame(ctx, n, f, f + 8, 8, h16, dtype=np.uint16)
    of = _frame(ctx, n, f, f + 24, 16, dtype=np.uint16)
    assert hf.aligned() and of.aligned()
    D.spmm_bf16(ctx, a, hf.view, ctx.to_device(bias), of.view, act="relu")
    of.check(base)
    hf.untouched("h")
    for h_ld, h_lead, o_ld, o_lead in ((f + 4, 8, f + 8, 8), (f + 8, 8, f + 12, 8), (f + 8, 4, f + 8, 8), (f + 8, 8, f + 8, 2)):
        hf, of = _frame(ctx, n, f, h_ld, h_lead, h16, dtype=np.uint16), _frame(ctx, n, f, o_ld, o_lead, dtype=np.uint16)
        with pytest.raises(GcnxError, match="16-byte aligned with leading dimensions in multiples of 8"):
            D.spmm_bf16(ctx, a, hf.view, None, of.view)
        of.untouched(), hf.untouched()


# ------------------------------------------------------------------------------------------- max / min / prod aggregation
def _directed():
    import scipy.sparse as sp
    n = 301
    m = sp.random(n, n, density=0.03, random_state=3, format="csr")
    m.data[:] = 1.0
    m = m.tolil(); m[7, :] = 0; m[200, :] = 0; m = m.tocsr(); m.eliminate_zeros(); m.sort_indices()
    return n, m.indptr.astype(np.int32), m.indices.astype(np.int32)


@pytest.mark.parametrize("mode", ["max", "min", "prod"])
def test_minmax_prod_aggregation_every_operand_in_its_own_frame(ctx, mode):
    """gcnx_spmm_csr_minmax / _minmax_bwd / gcnx_spmm_csr_prod / _prod_bwd (spmm_minmax_kernel, spmm_prod_kernel and their
    backward kernels: one route each, five or six strided operands): n = 301, f = 37, a directed pattern, integer-valued
    messages, every operand with a leading dimension and a lead of its own, every output framed.  Outputs exactly the oracle's
    and the contiguous call's; the gradient at TIGHT, bit for bit the contiguous call's; cnt / aux = NULL leaves its frame
    untouched."""
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    o = O()
    n, rp, ci = _directed()
    f = 37
    rng = np.random.default_rng(17)
    a = DeviceCSR.from_host_csr(ctx, rp, ci, None, None)
    h = rng.integers(-3, 4, (n, f)).astype(np.float32) if mode != "prod" else rng.integers(-2, 3, (n, f)).astype(np.float32)
    dy = rng.standard_normal((n, f), dtype=np.float32)
    rp64, ci64, h64 = rp.astype(np.int64), ci.astype(np.int64), h.astype(np.float64)
    if mode == "prod":
        rout, raux = o.aggregate_prod(rp64, ci64, h64)
        rdh = o.aggregate_prod_bwd(rp64, ci64, h64, rout, raux, dy.astype(np.float64))
    else:
        rout, raux = o.aggregate_minmax(rp64, ci64, h64, mode)
        rdh = o.aggregate_minmax_bwd(rp64, ci64, h64, rout, raux, dy.astype(np.float64))
    # contiguous
    c_out, c_aux, c_dh = ctx.empty((n, f)), ctx.empty((n, f)), ctx.empty((n, f))
    D.spmm_minmax(ctx, a, ctx.to_device(h), c_out, c_aux, mode)
    D.spmm_minmax_bwd(ctx, a.transpose(), ctx.to_device(h), c_out, c_aux, ctx.to_device(dy), c_dh, mode)
    assert np.array_equal(c_out.numpy(), rout.astype(np.float32)) and np.array_equal(c_aux.numpy(), raux.astype(np.float32))
    assert rel_err(c_dh.numpy(), rdh) < TIGHT
    # every operand in its own frame
    hf = _frame(ctx, n, f, f + 3, 1, h)
    of, af = _frame(ctx, n, f, f + 6, 5), _frame(ctx, n, f, f + 1, 2)
    D.spmm_minmax(ctx, a, hf.view, of.view, af.view, mode)
    of.check(c_out.numpy(), "out"), af.check(c_aux.numpy(), "cnt / aux"), hf.untouched("h")
    dyf, dhf = _frame(ctx, n, f, f + 11, 3, dy), _frame(ctx, n, f, f + 2, 7)
    D.spmm_minmax_bwd(ctx, a.transpose(), hf.view, of.view, af.view, dyf.view, dhf.view, mode)
    dhf.check(c_dh.numpy(), "dh")
    hf.untouched("h"), dyf.untouched("dy"), of.check(c_out.numpy(), "out (an input now)"), af.check(c_aux.numpy(), "cnt (an input now)")
    # cnt / aux = NULL
    of2, af2 = _frame(ctx, n, f, f + 6, 5), _frame(ctx, n, f, f + 1, 2)
    D.spmm_minmax(ctx, a, hf.view, of2.view, None, mode)
    of2.check(c_out.numpy(), "out without cnt"), af2.untouched("cnt = NULL")

"""Every launch route of csrc/reduce.hip -- the global pools and their backward, the folded db of the pool backward and the
column sums -- bit for bit against tests/reduce_ref.py.

The kernels choose their launch shape from the problem size relative to the chip's CU count, so every shape below is
derived from cus = ctx.info()["cus"], and every case restates the dispatch rule it relies on as an assert on its own shape:
on any chip a case reaches the route it names or fails loudly.

Inputs are integers in [-3, 3] (as tests/test_gpu_splitk_order.py): every partial sum is exact in fp32, so whatever a route
slices, chunks or re-orders, it has to give the bits of the reference -- a dropped or doubled row, a run that steps into the
wrong graph or a slice that loses its tail shows as a wrong integer.  AVG cases whose result is summed again take graphs of
power-of-two sizes, which keeps the quotients exact.  One run per entry point uses Gaussian data against the float64 oracle at
the suite's TIGHT."""
import numpy as np
import pytest

import reduce_ref as R
from conftest import rel_err
from gpu_frames import SENTINEL, Frame, same as _same

pytestmark = pytest.mark.gpu

TIGHT = 2e-5                       # as tests/test_gpu_kernels.py
SIZES = [0, 1, 15, 16, 0, 17, 63, 64, 65, 700, 0]      # an empty graph at the start, in the middle and at the end
POW2_SIZES = [0, 1, 2, 16, 0, 64, 512, 4, 256, 0]


def O():
    from oracle import gcn_oracle
    return gcn_oracle


def _ints(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float32)


def _cdiv(a, b):
    return -(-a // b)


def _gp(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _layouts(f):
    """(name, ld, lead): contiguous; a column view whose rows stay 16-byte aligned; one that is not aligned (vec = 0)."""
    ld4 = (f + 3) // 4 * 4 + 8
    return [("contiguous", f, 0), ("aligned view", ld4, 4), ("unaligned view", ld4 + 1, 5)]


def _operand(ctx, data, layout):
    """`data` on the device in the given layout; returns (the operand, is it 16-byte aligned, its Frame or None)."""
    name, ld, lead = layout
    n, f = data.shape
    if name == "contiguous":
        a = ctx.to_device(data)
        return a, a.ptr % 16 == 0 and f % 4 == 0, None
    fr = Frame(ctx, n, f, ld, lead, data)
    return fr.view, fr.aligned(), fr


# ------------------------------------------------------------------------------------------- pool forward
def _pool_split(cus, b, f, knob=0):
    """gcnx_pool_split restated: the slice count of a SUM / AVG pool (1: one launch, the division inside)."""
    base = _cdiv(f, 64) * b
    if base >= 2 * cus:
        return 1
    ns = min(16, max(2, _cdiv(4 * cus // 2, base)))
    return knob if 2 <= knob <= 16 else ns


def _run_pool(ctx, seg, x, gp, f, mode):
    from gcnx import device as D
    b = len(gp) - 1
    want, warg = R.pool_fwd(x, gp, mode)
    for layout in _layouts(f):
        xd = _operand(ctx, x, layout)[0]
        out = Frame(ctx, b, f, f, 3)                              # pooled is contiguous by contract: framed to see overruns
        arg = ctx.to_device(np.full((b, f), -7, np.int32)) if mode == "max" else None
        D.segment_pool(ctx, seg, xd, out.view, mode, arg)
        out.check(want, (mode, f, layout[0]))
        if mode == "max":
            nonempty = np.diff(gp) > 0
            assert np.array_equal(arg.numpy()[nonempty], warg[nonempty]), (f, layout[0])


@pytest.mark.parametrize("split", [0, 2, 3, 5, 8, 16])
@pytest.mark.parametrize("f", [4, 64, 70, 130])
def test_pool_forward_split_route(ctx, f, split):
    """Few graphs: the rows of each are sliced over blockIdx.z, pool_combine_kernel adds the slices and divides.  Forced
    slice counts leave slices empty (the 1-row graph; 17 rows over 16 slices are 9 slices of 2)."""
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    gp = _gp(SIZES)
    b = len(SIZES)
    assert b * _cdiv(f, 64) < 2 * cus                             # the split rule
    ns = _pool_split(cus, b, f, split)
    assert 2 <= ns <= 16 and (split == 0 or ns == split)
    per17 = _cdiv(17, ns)
    assert split != 16 or (per17 == 2 and _cdiv(17, per17) == 9)  # seven of sixteen slices are empty
    rng = np.random.default_rng(100 * f + split)
    x = _ints(rng, (int(gp[-1]), f))
    seg = Segments(ctx, gp)
    ctx.set_tuning("pool_split", split)
    try:
        for mode in ("sum", "avg"):
            _run_pool(ctx, seg, x, gp, f, mode)
    finally:
        ctx.set_tuning("pool_split", 0)


@pytest.mark.parametrize("f", [4, 64, 70, 130])
def test_pool_forward_unsplit_route(ctx, f):
    """Many graphs: one launch, the AVG division inside pool_fwd_kernel."""
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    tiles = _cdiv(f, 64)
    b = _cdiv(2 * cus, tiles) + 3
    assert b * tiles >= 2 * cus and _pool_split(cus, b, f) == 1   # the unsplit rule
    rng = np.random.default_rng(200 + f)
    sizes = rng.integers(1, 10, b)
    sizes[0] = sizes[b // 2] = sizes[-1] = 0
    gp = _gp(sizes)
    x = _ints(rng, (int(gp[-1]), f))
    seg = Segments(ctx, gp)
    for mode in ("sum", "avg"):
        _run_pool(ctx, seg, x, gp, f, mode)


@pytest.mark.parametrize("f", [4, 64, 70, 130])
def test_pool_forward_max_first_maximal_row(ctx, f):
    """MAX never splits.  Integer data ties in every column; explicit ties sit in different row groups (rows 5 and 22 of the
    700-row graph), in adjacent rows (40 and 41) and sixteen rows apart (the same row group: 7 and 23)."""
    from gcnx.device import Segments
    gp = _gp(SIZES)
    rng = np.random.default_rng(300 + f)
    x = _ints(rng, (int(gp[-1]), f))
    lo = int(gp[9])
    assert gp[10] - gp[9] == 700
    x[[lo + 5, lo + 22], 0] = 5.0
    x[[lo + 40, lo + 41], 1] = 5.0
    x[[lo + 7, lo + 23], 2] = 5.0
    x[lo + 699, 3] = 5.0                                          # the last row alone
    want, warg = R.pool_fwd(x, gp, "max")
    assert warg[9, 0] == lo + 5 and warg[9, 1] == lo + 40 and warg[9, 2] == lo + 7 and warg[9, 3] == lo + 699
    _run_pool(ctx, Segments(ctx, gp), x, gp, f, "max")


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_pool_forward_gaussian_against_the_oracle(ctx, mode):
    from gcnx import device as D
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    f = 70
    rng = np.random.default_rng(400)
    for route, sizes in (("split", SIZES), ("unsplit", np.concatenate([[0], rng.integers(1, 10, cus + 3), [0]]))):
        gp = _gp(sizes)
        b = len(sizes)
        if route == "split":                                      # MAX never splits
            assert b * _cdiv(f, 64) < 2 * cus and (_pool_split(cus, b, f) > 1 or mode == "max")
        else:
            assert b * _cdiv(f, 64) >= 2 * cus and _pool_split(cus, b, f) == 1
        x = rng.standard_normal((int(gp[-1]), f)).astype(np.float32)
        pooled = ctx.empty((b, f))
        arg = ctx.empty((b, f), np.int32) if mode == "max" else None
        D.segment_pool(ctx, Segments(ctx, gp), ctx.to_device(x), pooled, mode, arg)
        ref, rarg = O().global_pool_fwd(x.astype(np.float64), gp, mode)
        assert rel_err(pooled.numpy(), ref) < TIGHT
        if mode == "max":
            nonempty = np.diff(gp) > 0
            assert np.array_equal(arg.numpy()[nonempty], rarg[nonempty])


# ------------------------------------------------------------------------------------------- pool backward
BWD_PATTERN = [1, 0, 2, 0, 0, 4, 0, 0, 0, 1, 1, 1, 8, 64, 16, 0, 32, 128, 2, 1, 0, 256]     # powers of two; 517 rows


def _bwd_layout(n, rpw, trailing):
    """Graph sizes that sum to n: two leading empty graphs, BWD_PATTERN repeated (517 is odd, so the pattern meets the
    runs at every phase), the rest in powers of two, a last graph of 1, 2 or 4 rows that does not begin on a run boundary (a
    run steps into it), then two trailing empty graphs or none (the last graph is then graph b - 1)."""
    last = next(s for s in (1, 2, 4) if (n - s) % rpw != 0 or rpw == 1)
    body = n - last
    reps = body // sum(BWD_PATTERN)
    sizes = [0, 0] + BWD_PATTERN * reps
    rest = body - reps * sum(BWD_PATTERN)
    sizes += [1 << k for k in range(rest.bit_length()) if rest >> k & 1]
    sizes += [last] + ([0, 0] if trailing else [])
    sizes = np.asarray(sizes, np.int64)
    assert sizes.sum() == n and all(s == 0 or s & (s - 1) == 0 for s in sizes.tolist())
    return sizes


def _rpw(cus, n):
    return min(32, max(1, n // (64 * cus)))                       # gcnx_segment_pool_bwd's rows per wave


def _runs_seen(gp, n, rpw):
    """What the runs of rpw consecutive rows meet: the set of counts of consecutive empty graphs stepped over INSIDE a run
    (between two runs the binary search finds the graph), and the set of counts of graphs a run has rows in."""
    gid = R.graph_of_row(gp)
    step = np.diff(gid)                                            # > 1 where empty graphs lie between two rows
    inside = np.ones(n - 1, bool)
    inside[rpw - 1::rpw] = False
    crossed = set((step[inside & (step > 1)] - 1).tolist())
    nth = np.concatenate([[0], np.cumsum(step > 0)])               # index among the non-empty graphs
    start = np.arange(0, n, rpw)
    spanned = set((nth[np.minimum(start + rpw, n) - 1] - nth[start] + 1).tolist())
    return crossed, spanned


def _bwd_case(ctx, n, f, mode, seed, layouts, trailing=True):
    from gcnx import device as D
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    rpw = _rpw(cus, n)
    sizes = _bwd_layout(n, rpw, trailing)
    assert (sizes[-1] == 0) == trailing
    gp = _gp(sizes)
    b = len(sizes)
    if rpw > 1:
        crossed, spanned = _runs_seen(gp, n, rpw)
        assert {1, 2, 3} <= crossed                               # runs step over one, two and three empty graphs
        assert 1 in spanned and max(spanned) >= min(rpw, 3)       # runs inside one graph and across several
        assert n % rpw != 0                                       # the last run is cut at n
    rng = np.random.default_rng(seed)
    dp = _ints(rng, (b, f))
    y = _ints(rng, (n, f))
    arg = None
    if mode == "max":
        arg = (gp[:-1, None] + rng.integers(0, 1 << 30, (b, f)) % np.maximum(sizes, 1)[:, None]).astype(np.int32)
    seg = Segments(ctx, gp)
    dpd = ctx.to_device(dp)
    argd = ctx.to_device(arg) if arg is not None else None
    plain = R.pool_bwd(dp, gp, n, mode, arg)
    masked = np.where(y > 0, plain, np.float32(0))
    # every partial column sum is exact in fp32: the terms are integers (AVG: multiples of 2^-8, the graphs have power-of-two
    # sizes up to 256) and the sum of their magnitudes stays below 2^24 of that unit
    unit = 256 if mode == "avg" else 1
    assert sizes.max() <= 256 and np.abs(plain).sum(0, dtype=np.float64).max() * unit < 2 ** 24
    wdb = masked.sum(0, dtype=np.float64).astype(np.float32)
    wdb_plain = plain.sum(0, dtype=np.float64).astype(np.float32)
    for layout in layouts:
        name, ld, lead = layout
        yd = _operand(ctx, y, layout)[0]
        for with_y, with_db in ((False, False), (True, True), (False, True), (True, False)):
            dx = Frame(ctx, n, f, ld, lead)
            db = ctx.to_device(np.full(f, SENTINEL, np.float32)) if with_db else None
            D.segment_pool_bwd(ctx, seg, dpd, dx.view, mode, argd, y=yd if with_y else None, db=db)
            dx.check(masked if with_y else plain, (mode, n, f, name, with_y, with_db))
            if with_db:
                assert _same(db.numpy(), wdb if with_y else wdb_plain), (mode, n, f, name, with_y)


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_pool_backward_runs_of_k_rows(ctx, k, mode):
    """n = 64 cus k + 5 rows give runs of k rows per wave; f = 260 is a second 256-column pass with a ragged float4."""
    cus = ctx.info()["cus"]
    n, f = 64 * cus * k + 5, 260
    assert _rpw(cus, n) == k
    _bwd_case(ctx, n, f, mode, 500 + k, [_layouts(f)[k % 3]], trailing=k != 2)      # aligned view, unaligned view, contiguous


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_pool_backward_runs_at_the_cap(ctx, mode):
    """n = 64 cus 32 + 7: runs of kPoolBwdRows = 32 rows, the cap."""
    cus = ctx.info()["cus"]
    n, f = 64 * cus * 32 + 7, 8
    assert n // (64 * cus) == 32 and _rpw(cus, n) == 32
    _bwd_case(ctx, n, f, mode, 540, [_layouts(f)[1], _layouts(f)[2]], trailing=False)


def test_pool_backward_past_the_cap(ctx):
    """n = 64 cus 40 + 3: the quotient is 40, the run stays 32 rows."""
    cus = ctx.info()["cus"]
    n, f = 64 * cus * 40 + 3, 4
    assert n // (64 * cus) > 32 and _rpw(cus, n) == 32
    _bwd_case(ctx, n, f, "avg", 541, [_layouts(f)[0]])


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_pool_backward_gaussian_against_the_oracle(ctx, mode):
    from gcnx import device as D
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    n, f = 64 * cus * 3 + 5, 70
    assert _rpw(cus, n) == 3
    rng = np.random.default_rng(560)
    sizes = np.concatenate([[0], rng.integers(0, 40, n // 16)])
    sizes = sizes[np.cumsum(sizes) <= n]
    sizes = np.concatenate([sizes, [n - sizes.sum(), 0]])
    gp = _gp(sizes)
    b = len(sizes)
    dp = rng.standard_normal((b, f)).astype(np.float32)
    y = rng.standard_normal((n, f)).astype(np.float32)
    arg = (gp[:-1, None] + rng.integers(0, 1 << 30, (b, f)) % np.maximum(sizes, 1)[:, None]).astype(np.int32) if mode == "max" else None
    dx, db = ctx.empty((n, f)), ctx.empty(f)
    D.segment_pool_bwd(ctx, Segments(ctx, gp), ctx.to_device(dp), dx, mode, ctx.to_device(arg) if arg is not None else None,
                       y=ctx.to_device(y), db=db)
    ref = O().global_pool_bwd(dp.astype(np.float64), gp, n, mode, arg) * (y > 0)
    assert rel_err(dx.numpy(), ref) < TIGHT and rel_err(db.numpy(), ref.sum(0)) < TIGHT


# ------------------------------------------------------------------------------------------- folded db of the pool backward
def _colsum_split(cus, b, f):
    base = _cdiv(f, 64) * b
    return 1 if base >= 2 * cus else min(16, _cdiv(2 * cus, base))


@pytest.mark.parametrize("route", ["split", "unsplit"])
@pytest.mark.parametrize("f", [4, 64, 70, 130])
def test_pool_bwd_colsum_routes(ctx, f, route):
    """gcnx_pool_bwd_colsum: per (graph, row slice) the count of positives times the graph's dPooled row, then column sums."""
    from gcnx import device as D
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    tiles = _cdiv(f, 64)
    rng = np.random.default_rng(600 + f)
    for mode in ("sum", "avg"):
        if route == "split":
            sizes = np.asarray(SIZES if mode == "sum" else POW2_SIZES)
            assert len(sizes) * tiles < 2 * cus and _colsum_split(cus, len(sizes), f) > 1
        else:
            b = _cdiv(2 * cus, tiles) + 3
            sizes = rng.integers(1, 10, b) if mode == "sum" else 1 << rng.integers(0, 4, b)
            sizes[0] = sizes[b // 2] = sizes[-1] = 0
            assert b * tiles >= 2 * cus and _colsum_split(cus, b, f) == 1
        gp = _gp(sizes)
        b, n = len(sizes), int(gp[-1])
        dp, y = _ints(rng, (b, f)), _ints(rng, (n, f))
        want = R.pool_bwd_colsum(dp, gp, y, mode)
        assert _same(want, R.pool_bwd(dp, gp, n, mode, y=y).sum(0, dtype=np.float64).astype(np.float32))
        seg = Segments(ctx, gp)
        for layout in _layouts(f):
            yd = _operand(ctx, y, layout)[0]
            dpd = _operand(ctx, dp, layout)[0]
            db = Frame(ctx, 1, f, f, 4 if layout[0] != "unaligned view" else 3)
            D.pool_bwd_colsum(ctx, seg, dpd, yd, db.row(0), mode)
            db.check(want, (mode, f, route, layout[0]))


def test_pool_bwd_colsum_gaussian_against_the_oracle(ctx):
    from gcnx import device as D
    from gcnx.device import Segments
    rng = np.random.default_rng(650)
    cus = ctx.info()["cus"]
    f = 70
    for mode in ("sum", "avg"):
        for route, sizes in (("split", SIZES), ("unsplit", np.concatenate([[0], rng.integers(1, 10, cus + 3), [0]]))):
            gp = _gp(sizes)
            b, n = len(sizes), int(gp[-1])
            assert (_colsum_split(cus, b, f) > 1) == (route == "split")
            assert (b * _cdiv(f, 64) < 2 * cus) == (route == "split")
            dp = rng.standard_normal((b, f)).astype(np.float32)
            y = rng.standard_normal((n, f)).astype(np.float32)
            db = ctx.empty(f)
            D.pool_bwd_colsum(ctx, Segments(ctx, gp), ctx.to_device(dp), ctx.to_device(y), db, mode)
            ref = O().global_pool_bwd(dp.astype(np.float64), gp, n, mode) * (y > 0)
            assert rel_err(db.numpy(), ref.sum(0)) < TIGHT, (mode, len(sizes))


# ------------------------------------------------------------------------------------------- column sums
COL_N = [1, 255, 256, 257, 3 * 256 + 5]          # kColsumRows = 256: one chunk up to 256 rows, two from 257, four at 773
COL_F = [3, 64, 70, 130, 256]


def _act_ref(dy, y, act, alpha):
    if act is None:
        return dy.copy()
    if act == "relu":
        return np.where(y > 0, dy, np.float32(0))
    return np.where(y > 0, dy, alpha[None, :] * dy)


@pytest.mark.parametrize("layout", [0, 1, 2], ids=["contiguous", "aligned", "unaligned"])
@pytest.mark.parametrize("act", [None, "relu", "prelu"])
def test_act_bias_grad_chunks(ctx, act, layout):
    """gcnx_act_bias_grad: one chunk written straight to db (n <= 256), several chunks and the second stage (n > 256); with
    PReLU the second partial array and its own second stage (dalpha), held next to db."""
    from gcnx import device as D
    rng = np.random.default_rng(700 + layout)
    for n in COL_N:
        for f in COL_F:
            lay = _layouts(f)[layout]
            assert _cdiv(n, 256) == {1: 1, 255: 1, 256: 1, 257: 2, 773: 4}[n]
            dy, y = _ints(rng, (n, f)), _ints(rng, (n, f))
            alpha = _ints(rng, f)
            dz_want = _act_ref(dy, y, act, alpha)
            db_want = dz_want.sum(0, dtype=np.float64).astype(np.float32)
            da_want = (dy * np.minimum(y, 0)).sum(0, dtype=np.float64).astype(np.float32)
            dyd, dy_al, _ = _operand(ctx, dy, lay)
            yd, y_al, _ = _operand(ctx, y, lay)
            dz = Frame(ctx, n, f, lay[1], lay[2])
            if lay[0] == "unaligned view":
                assert not (dy_al and y_al and dz.aligned())       # vec = 0
            elif f % 4 == 0:
                assert dy_al and y_al and dz.aligned()             # vec = 1
            out = Frame(ctx, 2, f, f + 2, 4)                       # row 0: db, row 1: dalpha
            db, dal = out.row(0), None
            want = np.full((2, f), SENTINEL, np.float32)
            want[0] = db_want
            if act == "prelu":
                dal = out.row(1)
                want[1] = da_want
            D.act_bias_grad(ctx, dyd, yd if act else None, dz.view, act, db=db, alpha=ctx.to_device(alpha) if act == "prelu" else None,
                            dalpha=dal)
            dz.check(dz_want, (act, n, f, lay[0], "dz"))
            out.check(want, (act, n, f, lay[0], "db / dalpha"))


def test_act_bias_grad_prelu_dalpha_alone(ctx):
    """db = NULL with several chunks: only the second partial array is written and folded."""
    from gcnx import device as D
    rng = np.random.default_rng(720)
    n, f = 773, 70
    dy, y, alpha = _ints(rng, (n, f)), _ints(rng, (n, f)), _ints(rng, f)
    dz, dal = ctx.empty((n, f)), ctx.empty(f)
    D.act_bias_grad(ctx, ctx.to_device(dy), ctx.to_device(y), dz, "prelu", db=None, alpha=ctx.to_device(alpha), dalpha=dal)
    assert _same(dz.numpy(), _act_ref(dy, y, "prelu", alpha))
    assert _same(dal.numpy(), (dy * np.minimum(y, 0)).sum(0, dtype=np.float64).astype(np.float32))


@pytest.mark.parametrize("layout", [0, 1, 2], ids=["contiguous", "aligned", "unaligned"])
def test_colsum_in_place_identity(ctx, layout):
    """dz == dy without an activation: a pure column sum (colsum_kernel<false>, the four-loads-in-flight loop over aligned
    full tiles), nothing written back."""
    from gcnx import device as D
    rng = np.random.default_rng(730 + layout)
    for n in COL_N:
        for f in COL_F:
            lay = _layouts(f)[layout]
            dy = _ints(rng, (n, f))
            dyd, _, frame = _operand(ctx, dy, lay)
            db = Frame(ctx, 1, f, f, 4 if layout != 2 else 1)
            D.act_bias_grad(ctx, dyd, None, dyd, None, db=db.row(0))
            db.check(dy.sum(0, dtype=np.float64).astype(np.float32), (n, f, lay[0]))
            assert _same(dyd.numpy(), dy)
            if frame is not None:
                frame.check(dy, "the operand's frame")


@pytest.mark.parametrize("layout", [0, 2], ids=["contiguous", "unaligned"])
def test_colsum_behind_the_pool_backward(ctx, layout):
    """db of gcnx_segment_pool_bwd is gcnx_colsum of the dx it has just written."""
    from gcnx import device as D
    from gcnx.device import Segments
    rng = np.random.default_rng(740 + layout)
    for n in COL_N:
        gp = np.array([0, 0, n // 3, n // 3, n, n])
        seg = Segments(ctx, gp)
        for f in COL_F:
            lay = _layouts(f)[layout]
            dp, y = _ints(rng, (5, f)), _ints(rng, (n, f))
            want = R.pool_bwd(dp, gp, n, "sum", y=y)
            dx = Frame(ctx, n, f, lay[1], lay[2])
            db = Frame(ctx, 1, f, f, 4)
            D.segment_pool_bwd(ctx, seg, ctx.to_device(dp), dx.view, "sum", None, y=ctx.to_device(y), db=db.row(0))
            dx.check(want, (n, f, lay[0]))
            db.check(want.sum(0, dtype=np.float64).astype(np.float32), (n, f, lay[0], "db"))


def _tiled(rng, n, f, block_rows):
    """n x f integers in [-3, 3] tiled from a block of block_rows rows, and their exact column sums."""
    block = _ints(rng, (block_rows, f))
    reps, rest = divmod(n, block_rows)
    x = np.concatenate([np.tile(block, (reps, 1)), block[:rest]])
    sums = reps * block.sum(0, dtype=np.float64) + block[:rest].sum(0, dtype=np.float64)
    assert 3 * n < 2 ** 24                                         # every partial sum is an exact fp32 integer
    return x, sums.astype(np.float32)


@pytest.mark.parametrize("out_aligned", [True, False])
@pytest.mark.parametrize("f", [16, 256])
@pytest.mark.parametrize("n", [65536, 65537])
def test_colsum_wide_route(ctx, n, f, out_aligned):
    """colsum_wide_kernel (whole rows, 1024-row chunks) + colpart_reduce_kernel; an unaligned db takes colsum_kernel as the
    second stage."""
    from gcnx import device as D
    x, want = _tiled(np.random.default_rng(n + f), n, f, 1031)
    xd = ctx.to_device(x)
    assert n >= 65536 and f in (16, 32, 64, 128, 256) and xd.ptr % 16 == 0          # the wide rule
    assert 1 < _cdiv(n, 1024) <= 4096
    db = Frame(ctx, 1, f, f, 4 if out_aligned else 3)
    assert (db.view.ptr % 16 == 0) == out_aligned
    D.act_bias_grad(ctx, xd, None, xd, None, db=db.row(0))
    db.check(want, (n, f, out_aligned))


def test_colsum_wide_route_with_more_than_4096_chunks(ctx):
    """4098 chunks of 1024 rows: past what one colpart_reduce_kernel launch takes, folded by colsum_kernel."""
    from gcnx import device as D
    n, f = 4096 * 1024 + 1025, 16
    assert _cdiv(n, 1024) > 4096
    x, want = _tiled(np.random.default_rng(7), n, f, 1031)
    xd = ctx.to_device(x)
    assert xd.ptr % 16 == 0
    db = Frame(ctx, 1, f, f, 4)
    D.act_bias_grad(ctx, xd, None, xd, None, db=db.row(0))
    db.check(want)
    xd.free()


@pytest.mark.parametrize("act", [None, "relu", "prelu"])
def test_act_bias_grad_gaussian_against_the_oracle(ctx, act):
    from gcnx import device as D
    rng = np.random.default_rng(760)
    n, f = 773, 70
    dy, y = rng.standard_normal((n, f)).astype(np.float32), rng.standard_normal((n, f)).astype(np.float32)
    al = rng.random(f).astype(np.float32)
    dz, db, dal = ctx.empty((n, f)), ctx.empty(f), ctx.empty(f)
    D.act_bias_grad(ctx, ctx.to_device(dy), ctx.to_device(y), dz, act, db=db, alpha=ctx.to_device(al) if act == "prelu" else None,
                    dalpha=dal if act == "prelu" else None)
    ref = O().act_bwd(dy.astype(np.float64), y.astype(np.float64), act, al.astype(np.float64))
    assert rel_err(dz.numpy(), ref) < TIGHT and rel_err(db.numpy(), ref.sum(0)) < TIGHT
    if act == "prelu":
        assert rel_err(dal.numpy(), (dy.astype(np.float64) * np.minimum(y, 0)).sum(0)) < TIGHT

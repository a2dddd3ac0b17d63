"""The summation order of the deterministic reductions (csrc/gemm.hip splitk_group_sum, csrc/common.h
gcnx_colpart_reduce_sum), bit for bit against a host sum that is independent of the code under test.

Split-K: fi = fo = 64 is one 64 x 64 tile and n = 320 s gives ksteps = 10 s, so nsplit = s and slice j is exactly the
rows [320 j, 320 (j + 1)).  x and dH are integers in [-3, 3] and the rows of slice j of x are scaled by 2^e_j, e_j in
[0, 20]: every entry of a slab is an integer below 2^12 times 2^e_j, exact in fp32 whatever order the MFMA adds in.  The
sum ACROSS slabs is not exact, so it shows the order: four groups of per = ceil(s / 4) consecutive slabs, each summed
ascending from +0.f, combined as (s0 + s1) + (s2 + s3).  s = 17 and 65 are order-sensitive (asserted); s = 2, 3, 5, 7
have short and empty groups and show a dropped or doubled slab.

SGD: lr is a power of two, so lr * g is exact and p - lr * g is one rounding with or without a fused multiply-add.

Column partials: thread group rg adds the rows rg, rg + 128, ... ascending from +0.f, then s[rg] += s[rg + off] for
off = 64, 32, ..., 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 64
LR = np.float32(2.0 ** -6)
SENTINEL = np.float32(12345.0)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(s):
    """x, two dH, and per product the exact fp32 slabs [s][F * F]."""
    if s not in _cache:
        rng = np.random.default_rng(s)
        n = 320 * s
        e = rng.integers(0, 21, s)
        x = rng.integers(-3, 4, (n, F)).astype(np.float64) * np.repeat(2.0 ** e, 320)[:, None]
        dhs = [rng.integers(-3, 4, (n, F)).astype(np.float64) for _ in range(2)]
        slabs = []
        for dh in dhs:
            sl = np.stack([x[320 * j:320 * (j + 1)].T @ dh[320 * j:320 * (j + 1)] for j in range(s)]).reshape(s, F * F)
            assert np.array_equal(sl.astype(np.float32).astype(np.float64), sl)          # exact in fp32
            slabs.append(sl.astype(np.float32))
        _cache[s] = (x.astype(np.float32), [d.astype(np.float32) for d in dhs], slabs)
    return _cache[s]


def _documented_sum(slabs):
    s = len(slabs)
    per = (s + 3) // 4
    grp = []
    for g in range(4):
        acc = np.zeros(slabs.shape[1], np.float32)
        for z in range(g * per, min(s, g * per + per)):
            acc = acc + slabs[z]
        grp.append(acc)
    return (grp[0] + grp[1]) + (grp[2] + grp[3])


def _ascending_sum(slabs):
    acc = np.zeros(slabs.shape[1], np.float32)
    for z in range(len(slabs)):
        acc = acc + slabs[z]
    return acc


def _colpart_sum(part):
    rows, f = part.shape
    acc = np.zeros((128, f), np.float32)
    for r0 in range(0, rows, 128):
        blk = part[r0:r0 + 128]
        acc[:len(blk)] = acc[:len(blk)] + blk
    off = 64
    while off:
        acc[:off] = acc[:off] + acc[off:2 * off]
        off >>= 1
    return acc[0].copy()


@pytest.mark.parametrize("s", [17, 65])
def test_the_inputs_are_order_sensitive(s):
    _, _, slabs = _case(s)
    for sl in slabs:
        differ = np.mean(_bits(_documented_sum(sl)) != _bits(_ascending_sum(sl)))
        print(f"s = {s}: the documented order differs from the ascending sum in {100 * differ:.1f} % of the outputs")
        assert differ > 0.10


def _framed(ctx, layout):
    """A flat buffer of sentinels; layout = [(name, floats)]: the offset of every named interval (the rest are gaps)."""
    off, where = 0, {}
    for name, k in layout:
        where[name] = off
        off += k
    return ctx.to_device(np.full(off, SENTINEL, np.float32)), where, off


@pytest.mark.parametrize("s", [2, 3, 5, 7, 17, 65])
def test_gemm_dw_and_gemm_dw_sgd_sum_in_the_documented_order(ctx, s):
    from gcnx import device as D
    x, dhs, slabs = _case(s)
    want = _documented_sum(slabs[0])
    xd, dhd = ctx.to_device(x), ctx.to_device(dhs[0])
    buf, at, size = _framed(ctx, [("pad0", 12), ("dw", F * F), ("pad1", 20)])
    D.gemm_dw(ctx, xd, dhd, buf.flat(at["dw"], F * F, (F, F)))
    got = buf.numpy()
    assert np.array_equal(_bits(got[at["dw"]:at["dw"] + F * F]), _bits(want))
    assert (got[:at["dw"]] == SENTINEL).all() and (got[at["dw"] + F * F:] == SENTINEL).all()
    # the reduction that also applies the update: every parameter, inside and outside dW's interval
    rng = np.random.default_rng(100 + s)
    p0 = rng.standard_normal(size, dtype=np.float32)
    params = ctx.to_device(p0)
    grads, at, _ = _framed(ctx, [("pad0", 12), ("dw", F * F), ("pad1", 20)])
    D.gemm_dw_sgd(ctx, xd, dhd, grads.flat(at["dw"], F * F, (F, F)), params, grads, float(LR))
    g = grads.numpy()
    assert np.array_equal(_bits(g[at["dw"]:at["dw"] + F * F]), _bits(want))
    assert (g[:at["dw"]] == SENTINEL).all() and (g[at["dw"] + F * F:] == SENTINEL).all()
    assert np.array_equal(_bits(params.numpy()), _bits(p0 - LR * g))


@pytest.mark.parametrize("with_params", [False, True])
@pytest.mark.parametrize("s", [2, 3, 5, 7, 17, 65])
def test_gemm_dw2_sums_in_the_documented_order(ctx, s, with_params):
    from gcnx import device as D
    x, dhs, slabs = _case(s)
    xd = ctx.to_device(x)
    grads, at, size = _framed(ctx, [("pad0", 8), ("dwa", F * F), ("gap", 20), ("dwb", F * F), ("pad1", 12)])
    p0 = np.random.default_rng(200 + s).standard_normal(size, dtype=np.float32)
    params = ctx.to_device(p0) if with_params else None
    D.gemm_dw2(ctx, xd, ctx.to_device(dhs[0]), grads.flat(at["dwa"], F * F, (F, F)), xd, ctx.to_device(dhs[1]),
               grads.flat(at["dwb"], F * F, (F, F)), params=params, grads=grads, lr=float(LR))
    g = grads.numpy()
    inside = np.zeros(size, bool)
    for name, sl in (("dwa", slabs[0]), ("dwb", slabs[1])):
        assert np.array_equal(_bits(g[at[name]:at[name] + F * F]), _bits(_documented_sum(sl))), name
        inside[at[name]:at[name] + F * F] = True
    assert (g[~inside] == SENTINEL).all()
    if with_params:
        assert np.array_equal(_bits(params.numpy()), _bits(p0 - LR * g))


@pytest.mark.parametrize("s", [2, 3, 5, 7, 17, 65])
def test_dense_bwd_sums_dw_in_the_documented_order(ctx, s):
    """gcnx_dense_bwd plans its dW slices by another slot rule than gcnx_gemm_dw: the slices fill the resident-workgroup
    slots (4 per CU) that the dX tiles leave.  With fi = fo = 64 and n = 320 s there are n_dx = 5 s dX tiles and one dW
    tile; spare = 4 CUs - 5 s (1024 - 5 s on the 256-CU device, never under a quarter of the slots, i.e. at least 256
    there), ksteps = 10 s, so nsplit = min(spare, ksteps / 10) = s and kchunk = 320: slice j is exactly the rows
    [320 j, 320 (j + 1)), as above, and dW must carry the bits of the documented sum.  w is an integer matrix in
    [-3, 3] and y_mask = x: every entry of dX is an integer of at most 576 and every partial sum of a column of dX an
    integer below 2^24, so dX and db are exact whatever the order.  Scratch: 2 * 5 s partial rows of 64 floats + s slabs
    of 4096.  The deferred route (gcnx_dense_bwd_deferred, finished by gcnx_gemm_dw_sgd's reduction launch) must give the
    same dW and db bits, and the update p0 - lr g for every parameter."""
    from gcnx import device as D
    x, dhs, slabs = _case(s)
    n = 320 * s
    w = np.random.default_rng(300 + s).integers(-3, 4, (F, F)).astype(np.float32)
    dx64 = (dhs[0].astype(np.float64) @ w.astype(np.float64).T) * (x > 0)
    assert np.abs(dx64).sum(0).max() < 2 ** 24
    want_dw, want_db = _documented_sum(slabs[0]), dx64.sum(0)
    xd, dhd, wd = ctx.to_device(x), ctx.to_device(dhs[0]), ctx.to_device(w)
    layout = [("pad0", 12), ("db", F), ("gap", 20), ("dw", F * F), ("gap2", 8), ("dw0", F * F), ("pad1", 12)]

    def check(g, dxbuf, names):
        assert np.array_equal(_bits(g[at["dw"]:at["dw"] + F * F]), _bits(want_dw))
        assert np.array_equal(g[at["db"]:at["db"] + F].astype(np.float64), want_db)
        inside = np.zeros(size, bool)
        for name in names:
            inside[at[name]:at[name] + (F if name == "db" else F * F)] = True
        assert (g[~inside] == SENTINEL).all()
        dxh = dxbuf.numpy()
        assert np.array_equal(dxh[8:8 + n * F].reshape(n, F).astype(np.float64), dx64)
        assert (dxh[:8] == SENTINEL).all() and (dxh[8 + n * F:] == SENTINEL).all()

    assert D.dense_bwd_scratch_floats(ctx, n, F, F) == 640 * s + 4096 * s
    buf, at, size = _framed(ctx, layout)
    dxbuf = ctx.to_device(np.full(n * F + 16, SENTINEL, np.float32))
    D.dense_bwd(ctx, xd, dhd, wd, dxbuf.flat(8, n * F, (n, F)), buf.flat(at["dw"], F * F, (F, F)), y_mask=xd,
                db_prev=buf.flat(at["db"], F))
    first = buf.numpy()
    check(first, dxbuf, ("db", "dw"))
    # deferred: the partials stay in the caller's scratch until the step's last launch folds them and applies the update
    grads, at, size = _framed(ctx, layout)
    dxbuf = ctx.to_device(np.full(n * F + 16, SENTINEL, np.float32))
    p0 = np.random.default_rng(400 + s).standard_normal(size, dtype=np.float32)
    params = ctx.to_device(p0)
    scratch = ctx.empty(640 * s + 4096 * s)
    pend = D.dense_bwd_deferred(ctx, xd, dhd, wd, dxbuf.flat(8, n * F, (n, F)), grads.flat(at["dw"], F * F, (F, F)), scratch,
                                y_mask=xd, db_prev=grads.flat(at["db"], F))
    assert pend.colpart and pend.crows == 10 * s and pend.slabs and pend.nsplit == s
    D.gemm_dw_sgd(ctx, xd, ctx.to_device(dhs[1]), grads.flat(at["dw0"], F * F, (F, F)), params, grads, float(LR), pending=pend)
    g = grads.numpy()
    check(g, dxbuf, ("db", "dw", "dw0"))
    assert np.array_equal(_bits(g[at["dw"]:at["dw"] + F * F]), _bits(first[at["dw"]:at["dw"] + F * F]))
    assert np.array_equal(_bits(g[at["db"]:at["db"] + F]), _bits(first[at["db"]:at["db"] + F]))
    assert np.array_equal(_bits(g[at["dw0"]:at["dw0"] + F * F]), _bits(_documented_sum(slabs[1])))
    assert np.array_equal(_bits(params.numpy()), _bits(p0 - LR * g))


def _partial_rows(rows, f, seed):
    """Partial rows of ordinary floats: every addition rounds, so the column sums show the order."""
    return np.random.default_rng(seed).standard_normal((rows, f), dtype=np.float32)


@pytest.mark.parametrize("rows", [1, 5, 127, 128, 129, 706])
def test_pending_column_partials_sum_in_the_documented_order(ctx, rows):
    """A pending column-sum reduction over `rows` partial rows, finished by gcnx_gemm_dw_sgd's and by gcnx_gemm_dw2's
    reduction launch (with the update and without), and by the launch of its own that a short dW falls back to."""
    from gcnx import _lib, device as D
    f = 40                                                       # five workgroups of 8 columns
    part = _partial_rows(rows, f, rows)
    want = _colpart_sum(part)
    if rows >= 127:
        plain = np.zeros(f, np.float32)
        for r in range(rows):
            plain = plain + part[r]
        assert np.mean(_bits(plain) != _bits(want)) > 0.10       # the tree shows
    pd = ctx.to_device(part)
    x, dhs, slabs = _case(5)
    xd, dh0, dh1 = ctx.to_device(x), ctx.to_device(dhs[0]), ctx.to_device(dhs[1])

    def pending(grads, at):
        return _lib.PendingReduce(colpart=pd.ptr, crows=rows, cf=f, cout=grads.ptr + 4 * at["db"], slabs=None, total=0, nsplit=0,
                                  out=None)

    layout = [("pad0", 8), ("dwa", F * F), ("gap", 4), ("db", f), ("gap2", 12), ("dwb", F * F), ("pad1", 12)]
    for route in ("dw_sgd", "dw2", "dw2_sgd", "short"):
        grads, at, size = _framed(ctx, layout)
        p0 = np.random.default_rng(rows).standard_normal(size, dtype=np.float32)
        params = ctx.to_device(p0) if route != "dw2" else None
        gwa, gwb = grads.flat(at["dwa"], F * F, (F, F)), grads.flat(at["dwb"], F * F, (F, F))
        if route == "dw_sgd":
            D.gemm_dw_sgd(ctx, xd, dh0, gwa, params, grads, float(LR), pending=pending(grads, at))
        elif route == "short":                                   # 32 rows: one slice, nothing to reduce -- the separate launches
            D.gemm_dw_sgd(ctx, ctx.to_device(x[:32]), ctx.to_device(dhs[0][:32]), gwa, params, grads, float(LR),
                          pending=pending(grads, at))
        else:
            D.gemm_dw2(ctx, xd, dh0, gwa, xd, dh1, gwb, params=params, grads=grads, lr=float(LR), pending=pending(grads, at))
        g = grads.numpy()
        assert np.array_equal(_bits(g[at["db"]:at["db"] + f]), _bits(want)), route
        if route != "short":
            assert np.array_equal(_bits(g[at["dwa"]:at["dwa"] + F * F]), _bits(_documented_sum(slabs[0]))), route
        inside = np.zeros(size, bool)
        for name, k in (("dwa", F * F), ("db", f)) + ((("dwb", F * F),) if route.startswith("dw2") else ()):
            inside[at[name]:at[name] + k] = True
        assert (g[~inside] == SENTINEL).all(), route
        if params is not None:
            assert np.array_equal(_bits(params.numpy()), _bits(p0 - LR * g)), route


def _chain_graphs(n, size):
    """Graphs of `size` rows (the last one shorter): self-loops and a chain inside every graph."""
    gp = np.unique(np.concatenate([np.arange(0, n, size), [n]])).astype(np.int32)
    rows, cols = [], []
    for g in range(len(gp) - 1):
        for i in range(gp[g], gp[g + 1]):
            rows.append(i); cols.append(i)
            if i + 1 < gp[g + 1]:
                rows += [i, i + 1]; cols += [i + 1, i]
    rows, cols = np.asarray(rows), np.asarray(cols)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), gp


@pytest.mark.parametrize("rows", [1, 5, 127, 128, 129, 706])
def test_the_backward_launch_partials_sum_in_the_documented_order(ctx, rows):
    """gcnx_gcn_conv_bwd_pool leaves db1 as one partial row per 32-row tile; gcnx_gemm_dw2(pending) folds them.  The
    partial rows are read back from the scratch and summed on the host in the kernel's order."""
    from gcnx import device as D
    from gcnx.device import DeviceCSR, Segments
    f1 = f2 = 32
    n = 32 * rows - 3
    rowptr, colidx, gp = _chain_graphs(n, 45)
    b = len(gp) - 1
    rng = np.random.default_rng(rows)
    vals = (rng.random(len(colidx)) + 0.25).astype(np.float32)
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    at, seg = a.transpose(), Segments(ctx, gp)
    y2 = ctx.to_device(np.maximum(rng.standard_normal((n, f2), dtype=np.float32), 0))
    y1 = ctx.to_device(np.maximum(rng.standard_normal((n, f1), dtype=np.float32), 0))
    w2 = ctx.to_device((rng.standard_normal((f1, f2)) / np.sqrt(f1)).astype(np.float32))
    dp = ctx.to_device(rng.standard_normal((b, f2), dtype=np.float32))
    dz2, dz1 = ctx.empty((n, f2)), ctx.empty((n, f1))
    s1, s2 = ctx.to_device(rng.standard_normal((n, 32), dtype=np.float32)), ctx.to_device(rng.standard_normal((n, f1), dtype=np.float32))
    for with_params in (False, True):
        grads, where, size = _framed(ctx, [("pad0", 4), ("dwa", 32 * f1), ("dwb", f1 * f2), ("gap", 8), ("db", f1), ("pad1", 4)])
        p0 = rng.standard_normal(size, dtype=np.float32)
        params = ctx.to_device(p0) if with_params else None
        scratch = ctx.zeros(D.gcn_conv_bwd_scratch_floats(ctx, n, f1))
        pend = D.gcn_conv_bwd_pool(ctx, at, y2, seg, dp, w2, y1, dz2, dz1, db1=grads.flat(where["db"], f1), scratch=scratch)
        assert pend.colpart and pend.crows == rows and pend.cf == f1
        first = (pend.colpart - scratch.ptr) // 4
        part = scratch.numpy()[first:first + rows * f1].reshape(rows, f1).copy()
        D.gemm_dw2(ctx, s1, dz1, grads.flat(where["dwa"], 32 * f1, (32, f1)), s2, dz2, grads.flat(where["dwb"], f1 * f2, (f1, f2)),
                   params=params, grads=grads, lr=float(LR), pending=pend)
        g = grads.numpy()
        assert np.any(part != 0)
        assert np.array_equal(_bits(g[where["db"]:where["db"] + f1]), _bits(_colpart_sum(part))), with_params
        assert (g[:where["dwa"]] == SENTINEL).all() and (g[where["db"] + f1:] == SENTINEL).all()
        assert (g[where["gap"]:where["db"]] == SENTINEL).all()
        if with_params:
            assert np.array_equal(_bits(params.numpy()), _bits(p0 - LR * g))

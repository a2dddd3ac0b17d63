"""The lane layout of the byte-mask backward (csrc/fused.hip, the M8 instances): K / 16 mask bytes per lane, 16 lanes per
gathered row, eight entries per trip, and the lane's columns written to the tile in a bank-spreading order.
gcnx_gcn_conv_bwd_pool_mask8 is held bit for bit to gcnx_gcn_conv_bwd_pool on the same operands -- the fp32-row form, which
this layout does not touch -- on dZ1, dZ2 and the db1 partial rows, and to the fp64 oracle at the suite's fp32 tolerance.

Shapes: the smallest at which the lane ownership can go wrong.  K (gathered width) x nc (output width) over {32, 64, 128}
x {16, 64, 128}; n = 1, 31, 33, 70 (a lone row, a ragged tile, one row in a second tile, three tiles); rows of 0, 1, 7, 8,
9, 16 and 17 entries (around the trip of eight); graph boundaries inside a tile and single-node graphs; a hub row that
takes a tile past the 1024 staged entries; the head inside the launch and outside; sum and average pooling; every strided
operand a column view of a wider array of sentinels."""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

TIGHT = 2e-5            # the fp32 bar of tests/test_gpu_kernels.py for this launch
TOL = 1e-4              # the suite's fp32 bar; used for the hub tile only, whose 1080-entry row is one fp32 fma chain (1080 u = 6.4e-5)
ROW_LENGTHS = (0, 1, 7, 8, 9, 16, 17)
SENT = 7.5


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _operator(n, rng, hub=False):
    """The CSR the launch gathers by (the role of A^T) and the graph boundaries: single-node graphs and graphs of 19 - 25
    rows in turn, the entries of a row inside its graph, row lengths cycling through ROW_LENGTHS (cut to the graph)."""
    if hub:
        sizes = [n]
    else:
        sizes, k = [], 0
        while sum(sizes) < n:
            sizes.append(min((1, 1, 19, 1, 25, 22)[k % 6], n - sum(sizes)))
            k += 1
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rowptr, cols = [0], []
    for g in range(len(sizes)):
        lo, hi = int(gp[g]), int(gp[g + 1])
        for i in range(lo, hi):
            want = ROW_LENGTHS[(i + 1) % len(ROW_LENGTHS)]
            if hub:
                want = n - 20 if i == 5 else (3 if i % 3 else 0)
            c = np.sort(rng.choice(np.arange(lo, hi), size=min(want, hi - lo), replace=False))
            cols.extend(c.tolist())
            rowptr.append(len(cols))
    return np.asarray(rowptr, np.int32), np.asarray(cols, np.int32), gp


def _framed(ctx, host, left, right, fill):
    """host [n, k] inside a wider array of `fill`: (the wide device array, the column view)."""
    n, k = host.shape
    wide = np.full((n, left + k + right), fill, host.dtype)
    wide[:, left:left + k] = host
    dev = ctx.to_device(wide)
    return dev, dev.cols(left, left + k)


def _frame_intact(dev, left, k, fill):
    got = dev.numpy()
    return bool((got[:, :left] == fill).all() and (got[:, left + k:] == fill).all())


def _run_case(ctx, n, K, nc, weighted, mode, hub=False):
    from gcnx import device as D
    from gcnx.device import DeviceCSR, Segments
    from oracle import gcn_oracle as o
    rng = np.random.default_rng(1000 * K + 10 * nc + n + int(weighted))
    rowptr, colidx, gp = _operator(n, rng, hub)
    b = len(gp) - 1
    lens = np.diff(rowptr)
    if hub:
        assert np.diff(rowptr[::32]).max() > 1024
    elif n >= 31:
        assert set(ROW_LENGTHS) <= set(lens.tolist())
    vals = (rng.random(len(colidx)) + 0.25).astype(np.float32) if weighted else None
    at = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
    seg = Segments(ctx, gp)
    y2h = np.maximum(rng.standard_normal((n, K), dtype=np.float32), 0)
    y2h[rng.random((n, K)) < 0.05] = 3e-45                                   # positive, however small
    y1h = np.maximum(rng.standard_normal((n, nc), dtype=np.float32), 0)
    w2h = (rng.standard_normal((nc, K)) / np.sqrt(nc)).astype(np.float32)
    dph = rng.standard_normal((b, K), dtype=np.float32)
    _, y2 = _framed(ctx, y2h, 4, 8, np.float32(SENT))
    m8w, m8 = _framed(ctx, (y2h > 0).astype(np.uint8), 16, 16, np.uint8(3))
    _, y1 = _framed(ctx, y1h, 8, 4, np.float32(SENT))
    _, dp = _framed(ctx, dph, 4, 4, np.float32(SENT))
    w2 = ctx.to_device(w2h)
    w2t = ctx.to_device(np.ascontiguousarray(w2h.T))
    # the head's operands: per-tile partial sums as a forward launch leaves them (any operator and any 32-wide input serve)
    tr = D.pool_tile_rows(n, b)
    tp, tc = ctx.zeros((tr, K)), ctx.zeros((tr, K))
    D.gcn_conv_fwd(ctx, at, ctx.to_device(rng.standard_normal((n, 32), dtype=np.float32)),
                   ctx.to_device((rng.standard_normal((32, K)) / np.sqrt(32)).astype(np.float32)), None, ctx.empty((n, K)), act="relu",
                   pool=(seg, tp, tc))
    scale = np.sqrt(K) * (max(n / b, 1.0) if mode == "sum" else 1.0)
    w3 = ctx.to_device((rng.standard_normal((K, 2)) / scale).astype(np.float32))
    b3 = ctx.to_device(rng.standard_normal(2).astype(np.float32))
    yl = ctx.to_device(np.eye(2, dtype=np.float32)[rng.integers(0, 2, b)])
    n_sc = D.gcn_conv_bwd_scratch_floats(ctx, n, nc)

    def run(mask_form, head, pending):
        dz2w, dz2 = _framed(ctx, np.zeros((n, K), np.float32), 8, 4, np.float32(SENT))
        dz1w, dz1 = _framed(ctx, np.zeros((n, nc), np.float32), 4, 12, np.float32(SENT))
        db1, scratch = ctx.zeros(nc), ctx.zeros(n_sc)
        ha = None
        if head:
            ha = D.head_args(seg, tp, tc, ctx.zeros((b, K)), ctx.zeros((b, K)), w3, b3, yl, float(b), ctx.empty((b, 2)), ctx.zeros(2),
                             ctx.empty((K, 2)), ctx.empty(2), ctx.empty(K), ctx.empty((b, K)), ctx.empty((b, K)), mode=mode)
        pend = D.gcn_conv_bwd_pool(ctx, at, None if mask_form else y2, seg, None if head else dp, w2, y1, dz2, dz1, db1=db1, mode=mode,
                                   scratch=scratch if pending else None, w2t=w2t, head=ha, mask8=m8 if mask_form else None)
        assert bool(pend.colpart) == pending
        assert _frame_intact(dz2w, 8, K, np.float32(SENT)) and _frame_intact(dz1w, 4, nc, np.float32(SENT))
        return dz1.numpy(), dz2.numpy(), db1.numpy(), scratch.numpy()

    for head in (False, True):
        for pending in (False, True):
            ref = run(False, head, pending)
            got = run(True, head, pending)
            for k, (g, r) in enumerate(zip(got, ref)):
                assert _same(g, r), (n, K, nc, weighted, mode, head, pending, ("dz1", "dz2", "db1", "partials")[k])
            if not head and not pending:
                rdz2 = o.global_pool_bwd(dph.astype(np.float64), gp, n, mode, None) * (y2h > 0)
                v64 = vals.astype(np.float64) if weighted else np.ones(len(colidx))
                rdh = np.zeros((n, K))
                np.add.at(rdh, np.repeat(np.arange(n), lens), v64[:, None] * rdz2[colidx])
                rdz1 = (rdh @ w2h.astype(np.float64).T) * (y1h > 0)
                tol = TOL if hub else TIGHT
                assert rel_err(got[1], rdz2) < TIGHT and rel_err(got[0], rdz1) < tol and rel_err(got[2], rdz1.sum(0)) < tol
                assert np.any(got[0] != 0) or n == 1
    assert _frame_intact(m8w, 16, K, np.uint8(3))


@pytest.mark.parametrize("nc", [16, 64, 128])
@pytest.mark.parametrize("K", [32, 64, 128])
def test_mask_form_equals_row_form_at_the_layout_edges(ctx, K, nc):
    for n in (1, 31, 33, 70):
        for weighted in (False, True):
            _run_case(ctx, n, K, nc, weighted, "avg" if (n + weighted) % 2 else "sum")


@pytest.mark.parametrize("K,nc,weighted,mode", [(128, 128, True, "sum"), (64, 16, False, "avg"), (32, 64, True, "avg")])
def test_mask_form_equals_row_form_past_the_staged_entries(ctx, K, nc, weighted, mode):
    _run_case(ctx, 1100, K, nc, weighted, mode, hub=True)

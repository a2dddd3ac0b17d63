"""What tests/spmm_route_batches.py has to deliver to tests/test_gpu_spmm_routes.py: every scheduling class of csrc/spmm.hip in
each batch, and a float64 reference that equals scipy's product.  Runs without a GPU."""
import numpy as np
import pytest

import spmm_route_batches as B


def _scipy(b, vals=None):
    import scipy.sparse as sp
    data = np.ones(len(b.colidx)) if vals is None else np.asarray(vals, np.float64)
    return sp.csr_matrix((data, b.colidx.astype(np.int64), b.rowptr.astype(np.int64)), shape=(b.n, b.n))


def _structure_ok(b):
    a = _scipy(b)
    assert (a != a.T).nnz == 0                                           # symmetric pattern
    assert np.all(a.diagonal() == 1)                                     # every row has its self-loop
    assert np.array_equal(b.gp, np.concatenate([[0], np.cumsum(b.sizes)])) and b.n == b.gp[-1] == len(b.rowptr) - 1
    rows = np.repeat(np.arange(b.n), np.diff(b.rowptr))
    gid = np.repeat(np.arange(len(b.sizes)), b.sizes)
    assert np.array_equal(gid[rows], gid[b.colidx])                      # block diagonal
    assert np.all(np.diff(b.colidx)[np.diff(rows) == 0] > 0)             # sorted, no duplicates


def test_batch1_holds_every_scheduling_class():
    b = B.batch1()
    _structure_ok(b)
    s = b.sizes
    assert s == [1, 7, 40, 100, 624, 625, 0, 632, 633, 1024, 1025, 1276, 1277, 1400, 4096]
    assert s[B.EMPTY1] == 0 and 0 < B.EMPTY1 < len(s) - 1 and b.gp[B.EMPTY1] == b.gp[B.EMPTY1 + 1]      # the empty graph, in the middle
    for cap in (B.DBL_CAP, B.PIPE_CAP32, B.DUO_CAP, B.PIPE_CAP16, B.SOLO_CAP):                          # one graph on each side of every limit
        assert cap in s and cap + 1 in s
    assert 12000 < b.n < 14000
    d40, d100 = B.degrees(b, 2), B.degrees(b, 3)
    assert 16 < d40.mean() < 32 and d40.max() > 16 and 32 < d100.mean() < 64              # second register set / tail from global memory
    # the hub graph: taller than a tile, no column-block graph, hub rows, one 8-row chunk that overflows the LDS staging
    hub = B.degrees(b, B.HUB1)
    assert B.SOLO_CAP < s[B.HUB1] < B.CB_MIN_ROWS and (hub > B.HUB_DEG).sum() >= 1 and hub.max() <= B.STAGE_CAP
    assert b.gp[B.HUB1] % 32 == 0 and B.DENSE8 % 32 == 0
    assert hub[B.DENSE8:B.DENSE8 + 8].sum() > B.STAGE_CAP
    # the column-block graph
    cb = B.degrees(b, B.CB1)
    assert s[B.CB1] == B.CB_MIN_ROWS
    assert (cb <= B.CB_SHORT).sum() > 3000 and ((cb > B.CB_SHORT) & (cb <= B.HUB_DEG)).sum() >= 40
    assert ((cb > B.HUB_DEG) & (cb <= B.STAGE_CAP)).sum() == 1 and (cb > B.STAGE_CAP).sum() == 1
    # no other graph has a hub row
    for g in range(len(s)):
        if g not in (B.HUB1, B.CB1) and s[g]:
            assert B.degrees(b, g).max() <= B.HUB_DEG
    # without the column-block graph: the same graphs, nothing of 4 096 rows (DeviceCSR.plan builds no plan)
    b0 = B.batch1(with_cb=False)
    _structure_ok(b0)
    assert b0.sizes == s[:-1] and max(b0.sizes) < B.CB_MIN_ROWS and len(b0.sizes) < 128 and b0.n < 131072
    assert np.array_equal(b0.rowptr, b.rowptr[:b0.n + 1]) and np.array_equal(b0.colidx, b.colidx[:b0.rowptr[-1]])


@pytest.mark.parametrize("cus,f", [(256, 256), (256, 64), (304, 256), (64, 32)])
def test_batch2_fills_the_chip_with_tier_2_alone(cus, f):
    b = B.batch2(cus, f)
    _structure_ok(b)
    sizes, empty = B.batch2_sizes(cus, f)
    assert b.sizes == sizes and sizes[empty] == 0 and sizes[empty - 1] == 1300 and sizes[empty + 1] == 1310   # tall | empty | tall
    small = [m for m in sizes if 0 < m <= B.SOLO_CAP]
    assert len(small) == max(80, -(-4 * cus // (2 * f // 32))) and min(small) >= 5 and max(small) <= 60
    assert 2 * len(small) * (f // 32) >= 4 * cus                         # tile_units_fill(0, n2, f)
    assert sum(m > B.SOLO_CAP for m in sizes) == 2 and max(sizes) < B.CB_MIN_ROWS
    assert max(np.diff(b.rowptr)) <= B.HUB_DEG                           # no hub row ...
    bh = B.batch2(cus, f, hub=True)                                      # ... unless asked for: one, in a tall graph
    _structure_ok(bh)
    assert bh.sizes == sizes
    for g, m in enumerate(sizes):
        if m:
            assert (B.degrees(bh, g) > B.HUB_DEG).sum() == (1 if g == empty - 1 else 0)


def test_the_float64_reference_equals_scipy():
    for b in (B.batch1(), B.batch2(256, 256)):
        h = B.features(b.n)[:, :96].astype(np.float64)
        for vals in (None, B.gcn_vals(b), B.skew_vals(b)):
            a = _scipy(b, vals)
            ref, ref_t = B.ref_spmm(b, vals, h), B.ref_spmm_t(b, vals, h)
            assert ref.shape == h.shape and np.allclose(ref, a @ h, rtol=1e-12, atol=1e-12)
            assert np.allclose(ref_t, a.T @ h, rtol=1e-12, atol=1e-12)
    b = B.batch1()
    v = B.gcn_vals(b).astype(np.float64)
    assert np.allclose(_scipy(b, v).toarray()[:200, :200], _scipy(b, v).T.toarray()[:200, :200])        # gcn_vals is symmetric
    assert (_scipy(b, B.skew_vals(b)) != _scipy(b, B.skew_vals(b)).T).nnz > 0                             # skew_vals is not

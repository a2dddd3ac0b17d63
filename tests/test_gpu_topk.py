"""GPU tests of TopKPool: the kernels of csrc/topk.hip (gcnx_topk_select, gcnx_csr_induce, gcnx_topk_gather, gcnx_topk_bwd),
the layer gcnx.TopKPool between two GCNConv layers, the model gcnx.TopKNet and gcnx.fit on it -- each against the float64
oracle tests/topk_ref.py.  Tolerances: TIGHT = 2e-5 for a single fp32 kernel, 1e-4 for a whole step.

Where a test compares a selection with the oracle's it first asserts that the oracle's selection is unambiguous at fp32
accuracy: either the float64 gap between the k-th and the (k+1)-th score of every graph is at least 1e-4 max|y|, or the
inputs are small integers, for which every fp32 dot product is exact and y = dot / ||p|| keeps their order and their ties."""
import functools

import numpy as np
import pytest

from conftest import assert_close, rel_err
import topk_ref as TR
from gpu_frames import SENTINEL, Frame
from test_gpu_gcn_bn import _scipy_adj, _tiny_host  # noqa: F401
from test_gpu_sage import _bits, _csr, _ecoli3, _edge_case_csr

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
EDGE_SIZES = [1, 3, 1, 7, 2, 1, 40, 1]


def _gp(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _int_frame(ctx, n, lead):
    """An int32 [n] array inside a sentinel frame: (Frame, DeviceArray)."""
    from gcnx.device import DeviceArray
    fr = Frame(ctx, n, 1, 1, lead)
    return fr, DeviceArray(ctx, fr.view.ptr, (n,), np.int32, base=fr.buf)


def _as_f32(ints):
    return np.ascontiguousarray(ints, np.int32).view(np.float32)


def _select(ctx, x, p, gp, ratio, ld=None):
    """gcnx_topk_select with every output inside a sentinel frame; returns (y, idx, pos) after checking the frames and that
    a second call leaves the same bits."""
    from gcnx import device as D
    from gcnx.device import Segments
    n, f = x.shape
    seg = Segments(ctx, gp)
    kp = D.topk_kept_ptr(gp, ratio)
    nk = int(kp[-1])
    dkp = ctx.to_device(kp, np.int32)
    xin = Frame(ctx, n, f, ld or f, 4, data=x)
    dp = ctx.to_device(np.asarray(p, np.float32))
    outs = []
    for _ in range(2):
        fy = Frame(ctx, n, 1, 1, 5)
        fy1 = D.DeviceArray(ctx, fy.view.ptr, (n,), np.float32, base=fy.buf)
        fi, di = _int_frame(ctx, nk, 3)
        fp, dpos = _int_frame(ctx, n, 7)
        D.topk_select(ctx, seg, dkp, nk, xin.view, dp, fy1, di, dpos)
        y, idx, pos = fy1.numpy(), di.numpy(), dpos.numpy()
        fy.check(y, "y frame"); fi.check(_as_f32(idx), "idx frame"); fp.check(_as_f32(pos), "pos frame")
        assert not np.any(y == SENTINEL) and not np.any(_as_f32(idx) == SENTINEL) and not np.any(_as_f32(pos) == SENTINEL)
        outs.append((y, idx, pos))
    xin.check(x, "x untouched")
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1]) \
        and np.array_equal(outs[0][2], outs[1][2])
    return outs[0]


def _check_selection(idx, pos, gp, ratio):
    """What holds whatever the scores are: k_g distinct in-range rows per graph in ascending order, pos their inverse."""
    kp = TR.kept_ptr(gp, ratio)
    assert idx.size == kp[-1] and pos.size == gp[-1]
    for g in range(len(gp) - 1):
        part = idx[kp[g]:kp[g + 1]]
        assert np.all(np.diff(part) > 0) and (part.size == 0 or (part[0] >= gp[g] and part[-1] < gp[g + 1]))
    want = np.full(int(gp[-1]), -1, np.int64)
    want[idx] = np.arange(idx.size)
    assert np.array_equal(pos, want)


# ---- 1. selection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.25, 0.5, 0.8])
@pytest.mark.parametrize("f,s", [(16, 0), (64, 0), (128, 3)])
def test_topk_select_against_float64(ctx, f, s, ratio):
    hb, _ = _ecoli3(f)
    assert np.diff(hb.graph_ptr).tolist() == [808, 525, 326] and hb.n == 1659
    p = np.random.default_rng(1000 + s).standard_normal(f)
    y64 = TR.scores(hb.x, p.astype(np.float32))
    gap = TR.threshold_gap(y64, hb.graph_ptr, ratio)
    print(f"topk_select f={f} ratio={ratio}: threshold gap {gap:.3e} max|y|")
    assert gap >= 1.1e-4                       # ~100 x the error of an fp32 dot product: the oracle's selection is unambiguous
    r_idx, r_pos, _ = TR.select(y64, hb.graph_ptr, ratio)
    y, idx, pos = _select(ctx, hb.x, p, hb.graph_ptr, ratio)
    e = rel_err(y, y64)
    print(f"topk_select f={f} ratio={ratio}: rel_err y {e:.2e}")
    assert np.array_equal(idx, r_idx) and np.array_equal(pos, r_pos)
    assert e < TIGHT
    _check_selection(idx, pos, hb.graph_ptr, ratio)


# ---- 2. ties and shapes ---------------------------------------------------------------------------------------------------
def _int_inputs(sizes, f, seed, span=3):
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    x = rng.integers(-span, span + 1, (n, f)).astype(np.float32)
    p = rng.integers(1, 3, f).astype(np.float32) * rng.choice([-1.0, 1.0], f).astype(np.float32)
    return x, p


def _exact_case(ctx, x, p, sizes, ratio, ld=None):
    gp = _gp(sizes)
    y64 = TR.scores(x, p)
    r_idx, r_pos, _ = TR.select(y64, gp, ratio)
    y, idx, pos = _select(ctx, x, p, gp, ratio, ld)
    assert np.array_equal(idx, r_idx) and np.array_equal(pos, r_pos), (sizes, ratio)
    assert rel_err(y, y64) < TIGHT
    _check_selection(idx, pos, gp, ratio)
    return y, idx, pos


@pytest.mark.parametrize("ratio", [0.5, 1.0])
@pytest.mark.parametrize("f,ld", [(16, 16), (6, 7), (8, 12)])
def test_topk_select_edge_case_batch(ctx, f, ld, ratio):
    x, p = _int_inputs(EDGE_SIZES, f, seed=f)
    _, idx, _ = _exact_case(ctx, x, p, EDGE_SIZES, ratio, ld)
    if ratio == 1.0:
        assert np.array_equal(idx, np.arange(56))
    # all-zero x: every score ties, the first k_g rows win
    _, idx, _ = _exact_case(ctx, np.zeros_like(x), p, EDGE_SIZES, ratio, ld)
    gp, kp = _gp(EDGE_SIZES), TR.kept_ptr(_gp(EDGE_SIZES), ratio)
    assert np.array_equal(idx, np.concatenate([np.arange(gp[g], gp[g] + kp[g + 1] - kp[g]) for g in range(len(EDGE_SIZES))]))


def test_topk_select_duplicates_straddle_the_threshold(ctx):
    """Graph 6 (40 rows, k = 20): 12 rows above, 16 copies of one row of which 8 fit, 12 rows below -- the 8 lowest-numbered
    copies win, wherever they sit."""
    x, p = _int_inputs(EDGE_SIZES, 16, seed=5)
    gp = _gp(EDGE_SIZES)
    rng = np.random.default_rng(6)
    rows = gp[6] + rng.permutation(40)
    p[:] = 1.0
    x[rows[:12]] = 2.0
    x[rows[12:28]] = np.tile(np.array([1, -1, 2, 0, 3, -2, 1, 0], np.float32), 2)      # sums to 8: y = 2
    x[rows[28:]] = -1.0
    _, idx, _ = _exact_case(ctx, x, p, EDGE_SIZES, 0.5)
    kp = TR.kept_ptr(gp, 0.5)
    want = np.sort(np.concatenate([rows[:12], np.sort(rows[12:28])[:8]]))
    assert np.array_equal(idx[kp[6]:kp[7]], want)


def test_topk_select_negative_zero_ties_with_positive_zero(ctx):
    """A score of -0.0 (the smallest negative denormal times 1 / ||p|| = 0.25) next to +0.0 at the threshold: they compare
    equal, so the lower row wins in both arrangements.  The expected selection is the oracle's on the DEVICE's y: in float64
    the product would not round to zero."""
    f, tiny = 16, np.float32(-1e-45)
    assert tiny < 0 and tiny != 0
    x = np.zeros((16, f), np.float32)
    x[0, 0], x[1, 0] = 1.0, tiny                                    # graph 0: rows 1 (-0.0) and 2 (+0.0) at the threshold
    x[3:8, 0] = [-1.0, -2.0, -3.0, -4.0, -5.0]
    x[8, 0], x[10, 0] = 1.0, tiny                                   # graph 1: rows 9 (+0.0) and 10 (-0.0)
    x[11:16, 0] = [-1.0, -2.0, -3.0, -4.0, -5.0]
    p = np.ones(f, np.float32)
    gp = _gp([8, 8])
    y, idx, pos = _select(ctx, x, p, gp, 0.25)
    yb = _bits(y)
    assert yb[1] == 0x80000000 and yb[2] == 0 and yb[9] == 0 and yb[10] == 0x80000000, [hex(v) for v in yb]
    assert np.array_equal(idx, TR.select(y.astype(np.float64), gp, 0.25)[0]) and idx.tolist() == [0, 1, 8, 9]
    _check_selection(idx, pos, gp, 0.25)


@pytest.mark.parametrize("ratio", [0.5, 0.8])
def test_topk_select_padding_edges_and_an_empty_graph(ctx, ratio):
    sizes = [63, 64, 65, 1024, 1025]
    x, p = _int_inputs(sizes, 8, seed=9, span=40)
    _exact_case(ctx, x, p, sizes, ratio)
    sizes = [5, 0, 9, 0]
    x, p = _int_inputs(sizes, 16, seed=10)
    _, idx, _ = _exact_case(ctx, x, p, sizes, ratio)
    assert np.diff(TR.kept_ptr(_gp(sizes), ratio))[[1, 3]].tolist() == [0, 0]


def test_topk_select_one_graph_of_8192_rows(ctx):
    from gcnx import device as D
    x, p = _int_inputs([8192], 16, seed=11, span=60)
    assert D.topk_select_ok(ctx, 8192, 16)
    _exact_case(ctx, x, p, [8192], 0.5)


def test_topk_select_one_graph_at_the_cap_of_16384_rows(ctx):
    """The largest graph served: 128 KiB of keys in LDS, the sort at m = 16384."""
    from gcnx import device as D
    x, p = _int_inputs([16384, 3], 16, seed=12, span=60)
    assert D.topk_select_ok(ctx, 16384, 16)
    _exact_case(ctx, x, p, [16384, 3], 0.5)


def test_topk_select_rejects_an_idx_that_is_too_short(ctx):
    from gcnx import device as D
    from gcnx.device import Segments
    seg = Segments(ctx, _gp([10]))
    kp = ctx.to_device(D.topk_kept_ptr(seg.host, 0.5), np.int32)
    with pytest.raises(AssertionError):
        D.topk_select(ctx, seg, kp, 5, ctx.zeros((10, 4)), ctx.zeros(4), ctx.empty(10), ctx.empty(4, np.int32), ctx.empty(10, np.int32))


def test_topk_select_refuses_a_graph_above_the_cap(ctx):
    from gcnx import device as D
    from gcnx.device import Segments
    n = 16385
    assert not D.topk_select_ok(ctx, n, 16)
    seg = Segments(ctx, _gp([n]))
    kp = ctx.to_device(D.topk_kept_ptr(seg.host, 0.5), np.int32)
    with pytest.raises(NotImplementedError):
        D.topk_select(ctx, seg, kp, n // 2 + 1, ctx.zeros((n, 16)), ctx.zeros(16), ctx.empty(n), ctx.empty(n // 2 + 1, np.int32), ctx.empty(n, np.int32))


# ---- 3. the induced sub-CSR -----------------------------------------------------------------------------------------------
def _induce(ctx, a, idx, pos):
    """gcnx_csr_induce into sentinel frames, twice; returns (rowptr', colidx', vals' or None) cut to nnz'."""
    from gcnx import device as D
    nk = len(idx)
    d_idx, d_pos = ctx.to_device(idx, np.int32), ctx.to_device(pos, np.int32)
    outs = []
    for _ in range(2):
        frp, rp = _int_frame(ctx, nk + 1, 3)
        fci, ci = _int_frame(ctx, max(a.nnz, 1), 5)
        fv = Frame(ctx, max(a.nnz, 1), 1, 1, 6) if a.vals is not None else None
        v = D.DeviceArray(ctx, fv.view.ptr, (max(a.nnz, 1),), np.float32, base=fv.buf) if fv is not None else None
        D.csr_induce(ctx, a, d_idx, d_pos, nk, rp, ci, v)
        nnz2 = D.read_int32(ctx, rp, nk)
        h_rp, h_ci, h_v = rp.numpy(), ci.numpy(), (v.numpy() if v is not None else None)
        frp.check(_as_f32(h_rp), "rowptr' frame")
        assert np.all(_as_f32(h_ci[nnz2:]) == SENTINEL) and (h_v is None or np.all(h_v[nnz2:] == SENTINEL))   # nothing past nnz'
        fci.check(_as_f32(h_ci), "colidx' frame")
        if fv is not None:
            fv.check(h_v, "vals' frame")
        outs.append((h_rp, h_ci[:nnz2], None if h_v is None else h_v[:nnz2]))
    for u, w in zip(*outs):
        assert (u is None and w is None) or np.array_equal(u, w)
    return outs[0]


def _same_csr(got, ref, weighted):
    rp, ci, v = got
    ref.sort_indices()
    assert np.array_equal(rp, ref.indptr) and np.array_equal(ci, ref.indices)
    if weighted:
        assert np.array_equal(_bits(v), _bits(ref.data.astype(np.float32)))
    else:
        assert v is None


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_csr_induce_symmetric_batch(ctx, weighted, ratio):
    import scipy.sparse as sp
    from gcnx import synth
    from gcnx.device import DeviceCSR
    hb, _ = _ecoli3(16)
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx) if weighted else None
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr)
    A = sp.csr_matrix((vals if weighted else np.ones(hb.nnz, np.float32), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    y = TR.scores(hb.x, np.random.default_rng(1000).standard_normal(16))
    idx, pos, _ = TR.select(y, hb.graph_ptr, ratio)
    got = _induce(ctx, a, idx, pos)
    _same_csr(got, A[idx][:, idx].tocsr(), weighted)
    _same_csr(got, TR.induce(A, idx), weighted)
    if ratio == 1.0:                                              # the operator itself
        assert np.array_equal(got[0], hb.rowptr) and np.array_equal(got[1], hb.colidx)
    else:
        assert 0 < len(got[1]) < hb.nnz


@pytest.mark.parametrize("ratio", [0.5, 1.0])
def test_csr_induce_directed_values_and_rows_without_entries(ctx, ratio):
    import scipy.sparse as sp
    from gcnx.device import DeviceCSR
    rowptr, colidx, vals, gp = _edge_case_csr()
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    assert not a.symmetric
    A = sp.csr_matrix((vals, colidx, rowptr), shape=(56, 56))
    x, p = _int_inputs(EDGE_SIZES, 8, seed=2)
    idx, pos, _ = TR.select(TR.scores(x, p), gp, ratio)
    if ratio < 1.0:
        idx = np.union1d(idx, (4, 20))                            # with the two rows without entries, whatever their score
        pos = np.full(56, -1, np.int64)
        pos[idx] = np.arange(idx.size)
    got = _induce(ctx, a, idx, pos)
    _same_csr(got, A[idx][:, idx].tocsr(), True)
    assert np.any(np.diff(got[0]) == 0)
    if ratio == 1.0:
        assert np.array_equal(got[0], rowptr) and np.array_equal(got[1], colidx) and np.array_equal(_bits(got[2]), _bits(vals))


def test_topk_pool_transpose_of_a_directed_operator(ctx):
    """The layer's a' on the directed edge-case batch: not symmetric, block pointers = graph_ptr', and a'.transpose() is the
    transposed oracle."""
    import scipy.sparse as sp
    import gcnx
    from gcnx.device import DeviceCSR, Segments
    rowptr, colidx, vals, gp = _edge_case_csr()
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    A = sp.csr_matrix((vals, colidx, rowptr), shape=(56, 56))
    x, p = _int_inputs(EDGE_SIZES, 8, seed=4)
    lay = gcnx.TopKPool(0.5, return_selection=True, return_score=True)
    lay.build(ctx, 8)
    lay.set_weights([p.reshape(8, 1)])
    x2, a2, seg2, idx, y = lay([ctx.to_device(x), a, Segments(ctx, gp)])
    r = TR.pool_fwd(x, p, gp, 0.5)
    assert np.array_equal(idx.numpy(), r["idx"]) and rel_err(y.numpy(), r["y"]) < TIGHT and rel_err(x2.numpy(), r["out"]) < TIGHT
    ref = TR.induce(A, r["idx"])
    assert not a2.symmetric and a2.n == len(r["idx"]) and a2.nnz == ref.nnz and a2.n_blocks == 8
    assert np.array_equal(a2.block_ptr.numpy(), r["kept_ptr"]) and np.array_equal(seg2.host, r["kept_ptr"]) and seg2.dev is a2.block_ptr
    assert a2.max_block_rows == 20
    t = a2.transpose()
    rt = ref.T.tocsr()
    rt.sort_indices()
    assert t is not a2 and np.array_equal(t.rowptr.numpy(), rt.indptr) and np.array_equal(t.colidx.numpy()[:t.nnz], rt.indices)
    assert np.array_equal(_bits(t.vals.numpy()[:t.nnz]), _bits(rt.data.astype(np.float32)))
    u = a2.unweighted()
    assert u.vals is None and u.rowptr is a2.rowptr and u.nnz == a2.nnz


# ---- 4. gather and backward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("f,ld", [(16, 16), (64, 64), (6, 7), (128, 132)])
def test_topk_gather_and_bwd_against_float64(ctx, f, ld, sigmoid):
    from gcnx import device as D
    hb, _ = _ecoli3(16)
    rng = np.random.default_rng(40 + f)
    n, gp = hb.n, hb.graph_ptr
    x = rng.standard_normal((n, f), dtype=np.float32)
    p = rng.standard_normal(f).astype(np.float32)
    y32 = TR.scores(x, p).astype(np.float32)                     # the kernels under test read y: the reference uses the same values
    idx, pos, _ = TR.select(y32.astype(np.float64), gp, 0.5)
    nk = len(idx)
    dout = rng.standard_normal((nk, f), dtype=np.float32)
    r_out = x[idx].astype(np.float64) * TR.gate(y32[idx].astype(np.float64), sigmoid)[:, None]
    r_dx, r_dp = TR.pool_bwd(x, p, y32.astype(np.float64), idx, dout, sigmoid)
    xin, din = Frame(ctx, n, f, ld, 4, data=x), Frame(ctx, nk, f, ld, 8, data=dout)
    d_y, d_idx, d_pos, d_p = ctx.to_device(y32), ctx.to_device(idx, np.int32), ctx.to_device(pos, np.int32), ctx.to_device(p)
    assert xin.aligned() == (f % 4 == 0)
    res = []
    for _ in range(2):
        fo, fdx, fdp = Frame(ctx, nk, f, ld, 4), Frame(ctx, n, f, ld, 8), Frame(ctx, 1, f, f, 4)
        D.topk_gather(ctx, xin.view, d_y, d_idx, nk, fo.view, sigmoid)
        D.topk_bwd(ctx, xin.view, d_y, d_pos, d_p, din.view, fdx.view, fdp.row(0), sigmoid)
        out, dx, dp = fo.view.numpy(), fdx.view.numpy(), fdp.view.numpy()[0]
        fo.check(out, "out frame"); fdx.check(dx, "dx frame"); fdp.check(dp, "dp frame")
        res.append((out, dx, dp))
    xin.check(x, "x untouched"); din.check(dout, "dout untouched")
    out, dx, dp = res[0]
    assert all(np.array_equal(_bits(u), _bits(w)) for u, w in zip(res[0], res[1]))
    e = rel_err(out, r_out), rel_err(dx, r_dx), rel_err(dp, r_dp)
    print(f"topk gather/bwd f={f} sigmoid={sigmoid}: rel_err out {e[0]:.2e} dx {e[1]:.2e} dp {e[2]:.2e}")
    assert max(e) < TIGHT
    dropped = pos < 0
    assert dropped.sum() == n - nk and np.all(_bits(dx[dropped]) == 0)          # exactly +0.0, written by the kernel
    assert not np.any(dx[~dropped] == SENTINEL)


# ---- 5. the layer in a chain ----------------------------------------------------------------------------------------------
def _norm_csr(ctx, hb):
    """(DeviceCSR, scipy CSR) of hb's pattern with gcn_filter values in fp32 -- the same numbers on both sides."""
    import scipy.sparse as sp
    from gcnx import synth
    from gcnx.device import DeviceCSR
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    return (DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr),
            sp.csr_matrix((vals.astype(np.float64), hb.colidx, hb.rowptr), shape=(hb.n, hb.n)))


def _sides_ok(pre, side, what):
    """The device's ReLU sides may differ from the oracle's own only at pre-activations within 1e-5 of the largest, on at most
    1e-4 of the elements (tests/ecc_ref.py kink_report)."""
    pre = np.asarray(pre, np.float64)
    diff = (pre > 0) != side
    if diff.any():
        assert np.max(np.abs(pre[diff])) <= 1e-5 * np.max(np.abs(pre)) and diff.sum() <= 1e-4 * pre.size, what


@pytest.mark.parametrize("sigmoid", [False, True])
def test_layer_chain_gcnconv_topkpool_gcnconv(ctx, sigmoid):
    import gcnx
    from gcnx.device import Segments
    hb, _ = _ecoli3(16)
    a, A = _norm_csr(ctx, hb)
    assert a.symmetric
    q = {k: v.astype(np.float32) for k, v in TR.init_params(16, 64, 2, seed=0).items()}
    c1, pool, c2 = gcnx.GCNConv(64, activation="relu"), gcnx.TopKPool(0.5, return_selection=True, sigmoid_gating=sigmoid), gcnx.GCNConv(64, activation="relu")
    c1.build(ctx, 16); pool.build(ctx, 64); c2.build(ctx, 64)
    c1.set_weights([q["conv1_kernel"], q["conv1_bias"]]); pool.set_weights([q["pool_kernel"]]); c2.set_weights([q["conv2_kernel"], q["conv2_bias"]])
    seg = Segments(ctx, hb.graph_ptr)
    y1 = c1([ctx.to_device(hb.x), a])
    x2, a2, seg2, idx = pool([y1, a, seg])
    y2 = c2([x2, a2])
    h_y1, h_y2 = y1.numpy(), y2.numpy()
    # oracle on the device's side of every ReLU kink
    gp = hb.graph_ptr
    o1, pre1, _ = TR.gcn_conv_fwd(A, hb.x, q["conv1_kernel"], q["conv1_bias"], h_y1 > 0)
    pl = TR.pool_fwd(o1, q["pool_kernel"], gp, 0.5, sigmoid)
    gap = TR.threshold_gap(pl["y"], gp, 0.5)
    print(f"layer chain sigmoid={sigmoid}: threshold gap {gap:.3e}")
    assert gap >= 1e-4
    assert np.array_equal(idx.numpy(), pl["idx"])                  # required before anything downstream is compared
    A2 = TR.induce(A, pl["idx"])
    o2, pre2, _ = TR.gcn_conv_fwd(A2, pl["out"], q["conv2_kernel"], q["conv2_bias"], h_y2 > 0)
    _sides_ok(pre1, h_y1 > 0, "conv1"); _sides_ok(pre2, h_y2 > 0, "conv2")
    assert a2.symmetric and a2.transpose() is a2 and a2.nnz == A2.nnz and seg2.n == len(pl["idx"])
    assert_close(h_y1, o1, 1e-4, "chain y1"); assert_close(x2.numpy(), pl["out"], 1e-4, "chain x'"); assert_close(h_y2, o2, 1e-4, "chain y2")
    dy2 = np.random.default_rng(3).standard_normal(o2.shape).astype(np.float32)
    dx2 = c2.backward(ctx.to_device(dy2))
    dy1 = pool.backward(dx2)
    dx = c1.backward(dy1)
    r_dx2, r_dw2, r_db2 = TR.gcn_conv_bwd(A2, pl["out"], q["conv2_kernel"], h_y2 > 0, dy2)
    r_dy1, r_dp = TR.pool_bwd(o1, q["pool_kernel"], pl["y"], pl["idx"], r_dx2, sigmoid)
    r_dx, r_dw1, r_db1 = TR.gcn_conv_bwd(A, hb.x, q["conv1_kernel"], h_y1 > 0, r_dy1)
    for got, ref, what in ((dx2.numpy(), r_dx2, "dx'"), (c2.grads["kernel"].numpy(), r_dw2, "dW2"), (c2.grads["bias"].numpy(), r_db2, "db2"),
                           (dy1.numpy(), r_dy1, "dy1"), (pool.grads["kernel"].numpy()[:, 0], r_dp, "dp"), (dx.numpy(), r_dx, "dx"),
                           (c1.grads["kernel"].numpy(), r_dw1, "dW1"), (c1.grads["bias"].numpy(), r_db1, "db1")):
        assert_close(got, ref, 1e-4, f"chain {what} sigmoid={sigmoid}")


# ---- 6. the model ---------------------------------------------------------------------------------------------------------
# per case the first weight seed of 0, 1, 2, ... whose first loss_and_grads and three SGD steps keep the threshold gap on the
# hidden scores >= 1e-4 max|y| in every graph (searched with _model_track on the CPU; the test asserts it again at every step)
MODEL_SEED = {(0.5, "sum"): 0, (0.5, "avg"): 0, (0.8, "sum"): 2, (0.8, "avg"): 2}
MODEL_LR = {"sum": 2e-4, "avg": 0.05}          # the sum over ~400 kept rows gives gradients ~250 x those of the mean


@functools.lru_cache(maxsize=None)
def _model_inputs():
    from gcnx import synth
    hb, _ = _ecoli3(16)
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    return hb, vals


def _model_track(ratio, pool, seed, steps=3):
    """The oracle's own three SGD steps from init_params(seed) on the CPU: the smallest threshold gap on the hidden scores
    along the way.  MODEL_SEED holds, per case, the first seed of 0, 1, 2, ... for which it is >= 1e-4."""
    import scipy.sparse as sp
    hb, vals = _model_inputs()
    A = sp.csr_matrix((vals.astype(np.float64), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    q = {k: v.astype(np.float32).astype(np.float64) for k, v in TR.init_params(16, 64, 2, seed=seed).items()}
    gap = np.inf
    for _ in range(steps + 1):
        r = TR.model(hb.x, A, hb.graph_ptr, q, ratio, hb.y, pool=pool)
        gap = min(gap, r["gap"])
        q = TR.sgd(q, r["grads"], MODEL_LR[pool])
    return gap


@pytest.mark.parametrize("pool", ["sum", "avg"])
@pytest.mark.parametrize("ratio", [0.5, 0.8])
def test_topknet_step_against_float64(ctx, ratio, pool):
    import scipy.sparse as sp
    import gcnx
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    hb, vals = _model_inputs()
    A = sp.csr_matrix((vals.astype(np.float64), hb.colidx, hb.rowptr), shape=(hb.n, hb.n))
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr)
    batch = DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))
    seed = MODEL_SEED[(ratio, pool)]
    q = {k: v.astype(np.float32) for k, v in TR.init_params(16, 64, 2, seed=seed).items()}
    m = gcnx.TopKNet(ctx, n_labels=2, hidden=64, ratio=ratio, pool=pool, seed=1)
    m.build(16)
    m.set_weights(q)
    assert m.use_graph is False and all(np.array_equal(w, q[k]) for k, w in m.get_weights(as_dict=True).items())

    def oracle(params):
        sides = {"m1": m._bufs["y1"].numpy() > 0, "m2": m._bufs["y2"].numpy() > 0}
        r = TR.model(hb.x, A, hb.graph_ptr, params, ratio, hb.y, pool=pool, masks=sides)
        _sides_ok(r["pre1"], sides["m1"], "conv1"); _sides_ok(r["pre2"], sides["m2"], "conv2")
        print(f"TopKNet ratio={ratio} pool={pool}: threshold gap {r['gap']:.3e}")
        assert r["gap"] >= 1e-4                                     # the fixture's precondition: the selection is unambiguous
        assert np.array_equal(m.topk._saved[4].numpy(), r["pool"]["idx"])
        return r

    # loss, probabilities, every gradient
    m.loss_and_grads(batch)
    loss, acc = m.fetch_metrics(hb.n_graphs)
    r = oracle(q)
    assert abs(loss - r["loss"]) <= 1e-4 * max(1.0, abs(r["loss"])) and acc == r["hits"] / hb.n_graphs
    assert_close(m._bufs["probs"].numpy(), r["probs"], 1e-4, "TopKNet probs")
    g = m.gradients()
    assert set(g) == set(TR.KEYS)
    for k in TR.KEYS:
        assert_close(g[k], np.reshape(r["grads"][k], g[k].shape), 1e-4, f"TopKNet grad {k} ratio={ratio} pool={pool}")
    # model(inputs) and evaluate_batch
    assert_close(m(batch), r["probs"], 1e-4, "TopKNet call")
    el, ea, ep = m.evaluate_batch(batch, None)
    assert abs(el - r["loss"]) <= 1e-4 * max(1.0, abs(r["loss"])) and ea == acc
    assert_close(ep, r["probs"], 1e-4, "TopKNet evaluate")
    # three SGD steps track the oracle's
    w = {k: v.astype(np.float64) for k, v in q.items()}
    for step in range(3):
        l_dev, _ = m.train_step(batch, lr=MODEL_LR[pool])
        r = oracle(w)
        assert abs(l_dev - r["loss"]) <= 1e-4 * max(1.0, abs(r["loss"])), step
        w = TR.sgd(w, r["grads"], MODEL_LR[pool])
        for k, got in m.get_weights(as_dict=True).items():
            assert_close(got, w[k], 1e-4, f"TopKNet weights {k} after step {step + 1}")


def test_topknet_takes_host_inputs_and_checks_the_width(ctx):
    import gcnx
    hb = _tiny_host(8, 16, seed=2)
    m = gcnx.TopKNet(ctx, hidden=32, ratio=0.5, seed=0)
    probs = m((hb.x, _scipy_adj(hb), hb.ids()))
    assert probs.shape == (8, 2) and np.allclose(probs.sum(1), 1.0, atol=1e-5)
    loss, acc = m.train_step((hb.x, _scipy_adj(hb), np.zeros((hb.nnz, 2)), hb.ids()), hb.y, lr=0.01)      # an e is dropped
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    other = _tiny_host(4, 8, seed=3)
    with pytest.raises(ValueError):
        m((other.x, _scipy_adj(other), other.ids()))


# ---- 7. the driver --------------------------------------------------------------------------------------------------------
def test_fit_and_evaluate_run_topknet(ctx):
    import gcnx
    from gcnx import DisjointLoader, Graph, ListDataset, synth
    raw = synth.tiny_graphs(40, 16, seed=3)
    tr = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[:32]])
    te = ListDataset([Graph(x=x, a=a, y=y) for x, a, y in raw[32:]])
    m = gcnx.TopKNet(ctx, hidden=32, ratio=0.5, seed=0)
    out = gcnx.fit(m, DisjointLoader(tr, batch_size=4, epochs=2, shuffle=True, seed=1),
                   DisjointLoader(te, batch_size=4, shuffle=False), epochs=2, normalize="spektral", verbose=False)
    hist = out["history"]
    assert len(hist) == 2 and all(np.all(np.isfinite(h)) for h in hist)
    print(f"fit TopKNet: train loss {hist[0][0]:.4f} -> {hist[1][0]:.4f}")
    assert hist[1][0] < hist[0][0]
    (loss, acc), preds = gcnx.evaluate(m, DisjointLoader(te, batch_size=4, shuffle=False), normalize="spektral")
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and sum(p.shape[0] for p in preds) == 8

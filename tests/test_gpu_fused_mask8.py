"""The byte image of [Y2 > 0] in the one-launch GCNConv step (csrc/fused.hip): layer 2's forward launch writes it
(gcnx_gcn_conv_fwd_mask8), the backward launch gathers it in place of the fp32 rows (gcnx_gcn_conv_bwd_pool_mask8).
Every row is accumulated by one lane group in CSR order with acc = fma(w, m, acc), m in {0, 1} -- the operations and the
order of the fp32-row form -- so every comparison here is exact (uint32 views), no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _chains(sizes, skip_rows=()):
    """Self-loops and a chain inside every graph; the rows in skip_rows have no entries at all."""
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows, cols = [], []
    for g in range(len(sizes)):
        for i in range(gp[g], gp[g + 1]):
            rows.append(i); cols.append(i)
            if i + 1 < gp[g + 1]:
                rows += [i, i + 1]; cols += [i + 1, i]
    rows, cols = np.asarray(rows), np.asarray(cols)
    keep = ~np.isin(rows, skip_rows)
    rows, cols = rows[keep], cols[keep]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=int(gp[-1])))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), gp


def _relu_values(rng, n, f):
    """A saved ReLU output with exact zeros, ordinary values and tiny positives (the smallest normal number, and smaller)."""
    y = np.maximum(rng.standard_normal((n, f), dtype=np.float32), 0)
    tiny = rng.random((n, f)) < 0.05
    y[tiny] = rng.choice(np.array([1.17549435e-38, 1e-30, 1e-40, 3e-45], np.float32), int(tiny.sum()))
    y[rng.random((n, f)) < 0.05] = 0.0
    assert (y == 0).any() and (y[y > 0] < 1e-37).any()
    return y


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fo", [16, 64, 128])
def test_forward_writes_the_byte_mask(ctx, fo, weighted, prec):
    """mask8 == (out > 0) beside the fp32 activation; without it (out = NULL) the same mask, S, W^T and pool partials;
    n not a multiple of 32; a strided mask (ld > fo) leaves the bytes between its rows alone."""
    from gcnx import device as D, synth
    from gcnx.device import DeviceCSR, Segments
    fi = 64
    hb = synth.ecoli_batch(3, fi, seed=fo)
    assert hb.n % 32 != 0
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx) if weighted else None
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr)
    seg = Segments(ctx, hb.graph_ptr)
    n, b = hb.n, len(hb.graph_ptr) - 1
    rng = np.random.default_rng(fo)
    x = ctx.to_device(hb.x)
    w = ctx.to_device((rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32))
    bias = ctx.to_device(rng.standard_normal(fo).astype(np.float32))
    tr = D.pool_tile_rows(n, b)

    def run(with_out, mask):
        out = ctx.empty((n, fo)) if with_out else None
        s, wt, tp, tc = ctx.zeros((n, fi)), ctx.zeros((fo, fi)), ctx.zeros((tr, fo)), ctx.zeros((tr, fo))
        D.gcn_conv_fwd(ctx, a, x, w, bias, out, act="relu", s=s, wt=wt, prec=prec, pool=(seg, tp, tc), mask8=mask)
        return (out.numpy() if with_out else None), [t.numpy() for t in (s, wt, tp, tc)]

    ref_out, ref_rest = run(True, None)                              # today's launch
    m1 = ctx.zeros((n, fo), np.uint8)
    out1, rest1 = run(True, m1)
    assert _same(out1, ref_out) and all(_same(g, r) for g, r in zip(rest1, ref_rest))
    assert np.array_equal(m1.numpy(), (ref_out > 0).astype(np.uint8)) and 0 < m1.numpy().mean() < 1
    wide = ctx.to_device(np.full((n, fo + 16), 7, np.uint8))
    m2 = wide.cols(0, fo)
    _, rest2 = run(False, m2)
    assert all(_same(g, r) for g, r in zip(rest2, ref_rest))
    got = wide.numpy()
    assert np.array_equal(got[:, :fo], m1.numpy()) and (got[:, fo:] == 7).all()
    # without the pool's partial sums too
    m3 = ctx.zeros((n, fo), np.uint8)
    D.gcn_conv_fwd(ctx, a, x, w, bias, None, act="relu", prec=prec, mask8=m3)
    assert np.array_equal(m3.numpy(), m1.numpy())


def _backward_case(case, f2):
    from gcnx import synth
    if case == "ecoli":
        hb = synth.ecoli_batch(4, f2, seed=f2)
        return hb.rowptr, hb.colidx, hb.graph_ptr
    if case == "hub":                                                 # a tile with more than 1024 entries: the unstaged tail
        hb = synth.power_law_batch(n_graphs=1, graph_size=4096, f=f2, seed=3)
        assert np.diff(hb.rowptr[::32]).max() > 1024
        return hb.rowptr, hb.colidx, hb.graph_ptr
    # graphs of fewer than 32 rows (several per tile), single-row graphs, rows without entries, a ragged last tile
    return _chains(np.array([1, 1, 1, 2, 1, 50, 1, 1, 1, 1, 3, 1, 70, 1, 1, 9, 31, 5], np.int64), skip_rows=(4, 20, 77))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("case,f1,f2,weighted", [("ecoli", 128, 128, True), ("hub", 64, 128, True), ("ragged", 128, 128, True),
                                                 ("ragged", 32, 64, True), ("ecoli", 64, 32, True), ("ecoli", 128, 128, False),
                                                 ("hub", 32, 64, False), ("ragged", 64, 32, False)])
def test_backward_mask_form_equals_row_form(ctx, case, f1, f2, weighted, mode, prec):
    """gcnx_gcn_conv_bwd_pool_mask8 against gcnx_gcn_conv_bwd_pool on the same operands: dZ1, dZ2, db1 (immediate and
    pending: the per-tile partial sums), pool_sum / pool_cnt bit for bit -- with dpooled given and with the head folded
    in, a contiguous and a strided (ld > K) mask, with and without dZ2, weighted and unweighted operators."""
    from gcnx import device as D
    from gcnx.device import DeviceCSR, Segments
    rowptr, colidx, gp = _backward_case(case, f2)
    n, b = int(gp[-1]), len(gp) - 1
    rng = np.random.default_rng(f1 + f2)
    vals = (rng.random(len(colidx)) + 0.25).astype(np.float32) if weighted else None
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=weighted is False)
    at, seg = a.transpose(), Segments(ctx, gp)
    y2h = _relu_values(rng, n, f2)
    y2 = ctx.to_device(y2h)
    mask = ctx.to_device((y2h > 0).astype(np.uint8))
    wide = ctx.to_device(np.concatenate([(y2h > 0).astype(np.uint8), np.full((n, 32), 3, np.uint8)], axis=1))
    y1 = ctx.to_device(np.maximum(rng.standard_normal((n, f1), dtype=np.float32), 0))
    w2 = ctx.to_device((rng.standard_normal((f1, f2)) / np.sqrt(f1)).astype(np.float32))
    w2t = ctx.to_device(np.ascontiguousarray(w2.numpy().T))
    dp = ctx.to_device(rng.standard_normal((b, f2), dtype=np.float32))
    # the head's operands: the pool's per-tile partial sums as a forward launch leaves them
    tr = D.pool_tile_rows(n, b)
    tp, tc = ctx.zeros((tr, f2)), ctx.zeros((tr, f2))
    D.gcn_conv_fwd(ctx, a, y1, ctx.to_device(np.ascontiguousarray(w2.numpy())), None, ctx.empty((n, f2)), act="relu",
                   pool=(seg, tp, tc))
    scale = np.sqrt(f2) * (n / b if mode == "sum" else 1.0)
    w3 = ctx.to_device((rng.standard_normal((f2, 2)) / scale).astype(np.float32))
    b3 = ctx.to_device(rng.standard_normal(2).astype(np.float32))
    yl = ctx.to_device(np.eye(2, dtype=np.float32)[rng.integers(0, 2, b)])
    n_sc = D.gcn_conv_bwd_scratch_floats(ctx, n, f1)

    def run(form, head, pending, with_dz2=True, transposed=True):
        dz2 = ctx.zeros((n, f2)) if with_dz2 else None
        dz1, db1, scratch = ctx.zeros((n, f1)), ctx.zeros(f1), ctx.zeros(n_sc)
        psum, pcnt = ctx.zeros((b, f2)), ctx.zeros((b, f2))
        ha = None
        if head:
            ha = D.head_args(seg, tp, tc, psum, pcnt, w3, b3, yl, float(b), ctx.empty((b, 2)), ctx.zeros(2), ctx.empty((f2, 2)),
                             ctx.empty(2), ctx.empty(f2), ctx.empty((b, f2)), ctx.empty((b, f2)), mode=mode)
        m8 = {"rows": None, "mask": mask, "strided": wide.cols(0, f2)}[form]
        pend = D.gcn_conv_bwd_pool(ctx, at, y2 if m8 is None else None, seg, None if head else dp, w2, y1, dz2, dz1, db1=db1,
                                   mode=mode, scratch=scratch if pending else None, w2t=w2t if transposed else None, prec=prec,
                                   head=ha, mask8=m8)
        assert bool(pend.colpart) == pending
        return [t.numpy() for t in (dz1, db1, scratch, psum, pcnt)] + ([dz2.numpy()] if with_dz2 else [])

    for head in (False, True):
        for pending in (False, True):
            ref = run("rows", head, pending)
            assert np.any(ref[0] != 0) and np.any(ref[5] != 0)
            assert np.any(ref[2] != 0) == pending and np.any(ref[1] != 0) == (not pending)
            for form in ("mask", "strided"):
                got = run(form, head, pending)
                for k, (g, r) in enumerate(zip(got, ref)):
                    assert _same(g, r), (head, pending, form, k)
        ref = run("rows", head, True, with_dz2=False, transposed=False)
        got = run("mask", head, True, with_dz2=False, transposed=False)
        assert all(_same(g, r) for g, r in zip(got, ref)), head
    assert (wide.numpy()[:, f2:] == 3).all()


def test_mask8_entry_points_zero_sizes_and_argument_errors(ctx):
    """Empty inputs are no-ops that still leave defined outputs, bad arguments are GCNX_ERR_INVALID, shapes without a
    kernel GCNX_ERR_UNSUPPORTED."""
    from gcnx import _lib, device as D, synth
    from gcnx.device import DeviceCSR, Segments
    lib, h = ctx.lib, ctx.h
    hb = synth.ecoli_batch(2, 32, seed=1)
    n, b, f = hb.n, len(hb.graph_ptr) - 1, 32
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    seg = Segments(ctx, hb.graph_ptr)
    x, w, out = ctx.to_device(hb.x), ctx.zeros((f, f)), ctx.empty((n, f))
    m8 = ctx.zeros((n, 48), np.uint8)

    def fwd(n_=n, act=1, out_=out, mask=m8.ptr, ldm=48, fo=f):
        return lib.gcnx_gcn_conv_fwd_mask8(h, a.rowptr.ptr, a.colidx.ptr, None, x.ptr, f, n_, f, w.ptr, fo, None, act, None, 0,
                                           out_.ptr if out_ is not None else None, f, None, 0, None, 0, None, None, mask, ldm)
    assert fwd() == 0
    assert fwd(n_=0) == 0 and fwd(fo=0) == 0                         # nothing to do
    assert fwd(out_=None) == 0                                       # the fp32 activation is optional beside the mask
    assert fwd(out_=None, mask=None) == 1 and "NULL pointer" in _lib.last_error(h)
    assert fwd(act=0) == 1 and "ReLU" in _lib.last_error(h)
    assert fwd(ldm=40) == 1 and "multiples of 16 bytes" in _lib.last_error(h)
    assert fwd(ldm=16) == 1                                          # narrower than fo
    assert fwd(mask=m8.ptr + 4) == 1 and "16-byte aligned" in _lib.last_error(h)
    assert fwd(n_=-1) == 1
    with pytest.raises(_lib.GcnxError, match="ReLU"):
        D.gcn_conv_fwd(ctx, a, x, w, None, out, act=None, mask8=ctx.zeros((n, f), np.uint8))

    at = a.transpose()
    y1, dz1, dz2, dp = ctx.zeros((n, f)), ctx.empty((n, f)), ctx.empty((n, f)), ctx.zeros((b, f))
    db1 = ctx.to_device(np.ones(f, np.float32))

    def bwd(n_=n, mask=m8.ptr, ldm=48, f2=f, f1=f, dp_=dp.ptr, db=None):
        return lib.gcnx_gcn_conv_bwd_pool_mask8(h, at.rowptr.ptr, at.colidx.ptr, None, mask, ldm, seg.ids.ptr, seg.dev.ptr, b, dp_, f, 0,
                                                n_, f2, w.ptr, f1, 0, y1.ptr, f, dz2.ptr, f, dz1.ptr, f, db, None, 0, None, 0, None)
    assert bwd() == 0
    assert bwd(n_=0, db=db1.ptr) == 0 and not db1.numpy().any()      # no rows: db1 is zeroed
    assert bwd(f1=0) == 0
    assert bwd(mask=None) == 1 and "NULL pointer" in _lib.last_error(h)
    assert bwd(ldm=40) == 1 and "multiple of 16 bytes" in _lib.last_error(h)
    assert bwd(ldm=16) == _lib.ERR_UNSUPPORTED                       # narrower than f2
    assert bwd(f2=96) == _lib.ERR_UNSUPPORTED and bwd(f1=24) == _lib.ERR_UNSUPPORTED
    assert bwd(mask=m8.ptr + 4) == 1 and "16-byte aligned" in _lib.last_error(h)
    assert bwd(dp_=None) == 1 and "NULL pointer" in _lib.last_error(h)
    assert bwd(n_=-1) == 1


def _ecoli_device_batch(ctx, n_graphs, f, seed):
    from gcnx import synth
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    hb = synth.ecoli_batch(n_graphs, f, seed=seed)
    hb.vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, hb.vals, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("hidden,pool", [(128, "sum"), (32, "avg")])
def test_gcn2_steps_with_and_without_the_byte_mask_are_identical(ctx, monkeypatch, hidden, pool, prec):
    """Three GCN2.train_steps on an E. coli-shaped batch with the route on and with GCNX_MASK8=0, eager and captured:
    loss, accuracy, every gradient and every weight bit for bit; loss_and_grads (which keeps the fp32 Y2) likewise."""
    from gcnx.models import GCN2
    batch = _ecoli_device_batch(ctx, 8, 128, seed=4)
    runs = {}
    for knob in ("1", "0"):
        for use_graph in (False, True):
            monkeypatch.setenv("GCNX_MASK8", knob)
            m = GCN2(ctx, 2, hidden=hidden, pool=pool, prec=prec, seed=3, use_graph=use_graph)
            m.build(128)
            assert m._knob["mask8"] == (knob == "1")
            steps = [m.train_step(batch, None, lr=0.05) for _ in range(3)]
            assert m._fused(batch) and m._head_late(batch)
            assert (m._bufs["_mask8"] is not None) == (knob == "1")
            g, wts = m.gradients(), m.get_weights()
            m.loss_and_grads(batch, None)
            y2 = m._bufs["y2"].numpy()
            if knob == "1":
                assert np.array_equal(m._bufs["y2m8"].numpy(), (y2 > 0).astype(np.uint8))
            runs[knob, use_graph] = (steps, g, wts, m.gradients(), y2)
    ref = runs["0", False]
    assert np.isfinite(ref[0][-1][0]) and any(np.any(v != 0) for v in ref[1].values())
    for key, (steps, g, wts, g2, y2) in runs.items():
        assert steps == ref[0], key
        assert all(_same(g[k], ref[1][k]) for k in g), key
        assert all(_same(x, r) for x, r in zip(wts, ref[2])), key
        assert all(_same(g2[k], ref[3][k]) for k in g2), key
        assert _same(y2, ref[4]), key


def test_gcn2_two_ranks_with_and_without_the_byte_mask_are_identical(monkeypatch):
    """The sharded step (two thread ranks on one GPU, host-mediated all-reduce): the same weights bit for bit with the
    byte mask and with GCNX_MASK8=0."""
    import os
    import sys
    import gcnx
    from gcnx import shard, synth
    from gcnx.models import DeviceBatch, GCN2
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from thread_comm import ThreadWorld
    hb = synth.ecoli_batch(6, 32, seed=8)
    hb.vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)

    def rank_fn(rank, make_comm):
        ctx = gcnx.Context(0)
        part, global_b = shard.shard_batch(hb, rank, 2)
        a = gcnx.DeviceCSR.from_host_csr(ctx, part.rowptr, part.colidx, part.vals, part.graph_ptr)
        batch = DeviceBatch(ctx, ctx.to_device(part.x), a, gcnx.Segments(ctx, part.graph_ptr), ctx.to_device(part.y, np.float32))
        m = GCN2(ctx, 2, hidden=32, seed=5, use_graph=False, comm=make_comm(ctx))
        out = [m.train_step(batch, None, lr=0.05, global_batch=global_b) for _ in range(2)]
        res = (out, m.gradients(), m.get_weights(), m._bufs["_mask8"] is not None)
        ctx.close()
        return res

    res = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("GCNX_MASK8", knob)
        res[knob] = ThreadWorld(2).run(rank_fn)
    for r in range(2):
        on, off = res["1"][r], res["0"][r]
        assert on[3] and not off[3]
        assert on[0] == off[0]
        assert all(_same(on[1][k], off[1][k]) for k in on[1]) and all(_same(x, y) for x, y in zip(on[2], off[2]))

"""Layer 1 of the one-launch GCNConv step without its gather (csrc/fused.hip: gcnx_gcn_conv_fwd_pre): S = A X carries no
trainable parameter, so it is computed once -- by the first gathering step on a batch, or by the loader for the whole
dataset (DeviceDataset(aggregate_x=True), gcnx_collate2) -- and later steps run the product and the epilogue alone.  The
product is the gathering launch's operation for operation, so every comparison against that launch here is exact (uint32
views); the fp64 comparison uses the fused forward tests' tolerances (test_gpu_kernels.py: 2e-5 for fp32 products, 5e-5
for the split-bf16 ones)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT = 2e-5            # test_gpu_kernels.TIGHT
X3_TOL = 5e-5           # test_gcn_conv_fused_forward's bound for bf16x3
SENT = -777.25


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
            if i + 5 < gp[g + 1]:
                rows += [i, i + 5]; cols += [i + 5, i]
    rows, cols = np.asarray(rows), np.asarray(cols)
    keep = ~np.isin(rows, skip_rows)
    rows, cols = rows[keep], cols[keep]
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=int(gp[-1])))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), gp


def _frame(ctx, n, width, pad_rows=1, pad_cols=4):
    """A sentinel-filled [n + 2 pad_rows, width + 2 pad_cols] array and the [n, width] view in its middle (16-byte aligned,
    ld = width + 2 pad_cols)."""
    from gcnx.device import DeviceArray
    ld = width + 2 * pad_cols
    frame = ctx.to_device(np.full((n + 2 * pad_rows, ld), SENT, np.float32))
    view = DeviceArray(ctx, frame.ptr + (pad_rows * ld + pad_cols) * 4, (n, width), np.float32, ld=ld, base=frame)
    return frame, view


def _frame_untouched(frame, n, width, pad_rows=1, pad_cols=4):
    h = frame.numpy().copy()
    inner = h[pad_rows:pad_rows + n, pad_cols:pad_cols + width].copy()
    h[pad_rows:pad_rows + n, pad_cols:pad_cols + width] = SENT
    return bool((h == SENT).all()), inner


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("fo", [16, 64, 128])
@pytest.mark.parametrize("fi", [32, 64, 128])
def test_pre_equals_the_gathering_forward(ctx, fi, fo, prec):
    """pre(S) == gcn_conv_fwd(A, X).out bit for bit with S that call's own output, for one row, both sides of a tile edge and
    three tiles, weighted and unweighted operators with empty rows, with and without bias / ReLU; S and out are strided
    views inside sentinel frames (padding columns and the rows before and after stay untouched); and against fp64."""
    from gcnx import device as D
    from gcnx.device import DeviceCSR
    rng = np.random.default_rng(1000 * fi + 10 * fo + (prec == "f32"))
    w = (rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32)
    bias = rng.standard_normal(fo).astype(np.float32)
    dw, dbias = ctx.to_device(w), ctx.to_device(bias)
    tol = TIGHT if prec == "f32" else X3_TOL
    for n in (1, 31, 33, 70):
        skip = tuple(r for r in (0, 17, 40) if r < n and n > 1)
        rowptr, colidx, gp = _chains(np.array([n], np.int64), skip_rows=skip)
        x = rng.standard_normal((n, fi), dtype=np.float32)
        dx = ctx.to_device(x)
        for weighted in (False, True):
            vals = (rng.random(len(colidx)) + 0.25).astype(np.float32) if weighted else None
            a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp, symmetric=False)
            for act, b in (("relu", dbias), (None, None), ("relu", None), (None, dbias)):
                s_frame, s = _frame(ctx, n, fi)
                ref_out = ctx.empty((n, fo))
                D.gcn_conv_fwd(ctx, a, dx, dw, b, ref_out, act=act, s=s, prec=prec)
                o_frame, out = _frame(ctx, n, fo)
                D.gcn_conv_fwd_pre(ctx, s, dw, b, out, act=act, prec=prec)
                ok_s, s_h = _frame_untouched(s_frame, n, fi)
                ok_o, out_h = _frame_untouched(o_frame, n, fo)
                what = (n, weighted, act, b is not None)
                assert ok_s and ok_o, what
                assert _same(out_h, ref_out.numpy()), what
                # fp64: S = A X, then the dense product
                dense = np.zeros((n, n))
                for r in range(n):
                    for e in range(rowptr[r], rowptr[r + 1]):
                        dense[r, colidx[e]] += 1.0 if vals is None else float(vals[e])
                s64 = dense @ x.astype(np.float64)
                ref = s64 @ w.astype(np.float64) + (bias.astype(np.float64) if b is not None else 0.0)
                ref = np.maximum(ref, 0) if act == "relu" else ref
                top = max(float(np.abs(ref).max()), 1e-30)
                assert float(np.abs(s_h.astype(np.float64) - s64).max()) / max(float(np.abs(s64).max()), 1e-30) < TIGHT, what
                assert float(np.abs(out_h.astype(np.float64) - ref).max()) / top < tol, what
                if skip:
                    assert not s_h[list(skip)].any()             # rows without entries: S = 0, out = act(bias)


def test_pre_on_the_flagship_shape(ctx):
    """32 E. coli-shaped graphs, F = 128: more tiles (706) than the launch has workgroups, so that workgroups walk several
    tiles with the next tile's rows in flight; contiguous S, a ragged last tile."""
    from gcnx import device as D, synth
    from gcnx.device import DeviceCSR
    hb = synth.ecoli_shard(0, 32, 128, seed=1)
    assert hb.n % 32 != 0 and hb.n > 2 * 256 * 32             # more tiles than two workgroups per CU: some walk two
    vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, vals, hb.graph_ptr)
    rng = np.random.default_rng(5)
    w = ctx.to_device((rng.standard_normal((128, 128)) / 11).astype(np.float32))
    bias = ctx.to_device(rng.standard_normal(128).astype(np.float32))
    x = ctx.to_device(hb.x)
    for prec in ("f32", "bf16x3"):
        s, ref, out = ctx.empty((hb.n, 128)), ctx.empty((hb.n, 128)), ctx.zeros((hb.n, 128))
        D.gcn_conv_fwd(ctx, a, x, w, bias, ref, act="relu", s=s, prec=prec)
        D.gcn_conv_fwd_pre(ctx, s, w, bias, out, act="relu", prec=prec)
        assert _same(out.numpy(), ref.numpy()) and 0.2 < (ref.numpy() > 0).mean() < 0.8, prec


def test_pre_refuses_what_the_fused_forward_refuses(ctx):
    """Shapes without a kernel are GCNX_ERR_UNSUPPORTED, bad arguments GCNX_ERR_INVALID, empty inputs no-ops."""
    from gcnx import _lib
    lib, h = ctx.lib, ctx.h
    n = 40
    s, w, out = ctx.zeros((n, 128)), ctx.zeros((128, 128)), ctx.zeros((n, 256))

    def pre(n_=n, fi=64, fo=64, lds=128, ldo=128, s_=s.ptr, out_=out.ptr, act=1, prec=0, w_=w.ptr):
        return lib.gcnx_gcn_conv_fwd_pre(h, s_, lds, n_, fi, w_, fo, None, act, out_, ldo, prec)
    assert pre() == 0
    assert pre(n_=0) == 0 and pre(fo=0) == 0
    for kw in (dict(fi=96), dict(fi=16), dict(fi=256, lds=256), dict(fo=24), dict(fo=8), dict(fo=144, ldo=144), dict(lds=32),
               dict(lds=66)):
        assert pre(**kw) == _lib.ERR_UNSUPPORTED, kw
    assert "gcnx_gcn_conv_fwd_pre" in _lib.last_error(h)
    assert pre(prec=1) == _lib.ERR_UNSUPPORTED                      # bf16 operands: not a precision of this launch
    assert pre(ldo=32) == 1 and pre(ldo=66) == 1                    # narrower than fo; not a multiple of 4 floats
    assert pre(s_=s.ptr + 4) == 1 and "16-byte aligned" in _lib.last_error(h)
    assert pre(out_=out.ptr + 8) == 1
    assert pre(s_=None) == 1 and "NULL pointer" in _lib.last_error(h)
    assert pre(out_=s.ptr) == 1 and pre(n_=-1) == 1 and pre(act=7) == 1
    assert not out.numpy().any()


# ---- the model -----------------------------------------------------------------------------------------------------------
ORDER = ("w1", "b1", "w2", "b2", "w3", "b3")


def _batch(ctx, f, seed, sizes=(5, 40, 33)):
    """Three graphs of 5, 40 and 33 nodes: the first tile spans two graphs, the second graph spans two tiles."""
    from gcnx import synth
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    rowptr, colidx, gp = _chains(np.array(sizes, np.int64))
    vals = synth.gcn_norm_host(rowptr, colidx)
    rng = np.random.default_rng(seed)
    n, b = int(gp[-1]), len(sizes)
    x = rng.standard_normal((n, f), dtype=np.float32) * np.float32(0.05)      # (unit features saturate the softmax: zero gradients)
    y = np.eye(2, dtype=np.float32)[rng.integers(0, 2, b)]
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, vals, gp)
    return DeviceBatch(ctx, ctx.to_device(x), a, Segments(ctx, gp), ctx.to_device(y)), x


def _model(ctx, monkeypatch, f, prec, reuse, use_graph=False):
    from gcnx.models import GCN2
    monkeypatch.setenv("GCNX_AX_REUSE", "1" if reuse else "0")
    m = GCN2(ctx, 2, hidden=f, prec=prec, seed=11, use_graph=use_graph)
    m.build(f)
    assert m._knob["ax_reuse"] == reuse
    return m


def _state(m, step):
    return step, m.gradients(), m.get_weights()


def _equal_state(a, b):
    return (a[0] == b[0] and all(_same(a[1][k], b[1][k]) for k in ORDER) and all(_same(x, y) for x, y in zip(a[2], b[2])))


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("f", [32, 128])
def test_gcn2_steps_with_and_without_the_kept_aggregate_are_identical(ctx, monkeypatch, f, prec):
    """Four train_steps: loss, the six gradients and the six weights after every step, the kept-S1 route (eager and with
    use_graph=True: warm, capture, replay, replay) and the batch.ax route against GCNX_AX_REUSE=0; evaluate_batch after the
    steps likewise."""
    from gcnx import device as D
    from gcnx.models import DeviceBatch
    batch, _ = _batch(ctx, f, seed=f)
    ref_m = _model(ctx, monkeypatch, f, prec, reuse=False)
    ref = []
    for _ in range(4):
        ref.append(_state(ref_m, ref_m.train_step(batch, None, lr=0.05)))
        assert ref_m._s1_uid is None and ref_m._bufs["_s1"] is ref_m._bufs["s1"]
    assert ref_m._fused(batch) and ref_m._head_late(batch)
    assert all(np.isfinite(r[0][0]) and r[0][0] > 0 and all(np.any(r[1][k] != 0) for k in ORDER) for r in ref)
    ref_eval = ref_m.evaluate_batch(batch, None)
    # the aggregate of this batch as the gathering launch writes it: what a loader would hand over as batch.ax
    s = ctx.empty((batch.n, f))
    D.gcn_conv_fwd(ctx, batch.a, batch.x, ctx.zeros((f, 16)), None, ctx.empty((batch.n, 16)), act=None, s=s)
    with_ax = DeviceBatch(ctx, batch.x, batch.a, batch.seg, batch.y, ax=s)
    for route in ("kept", "graph", "ax"):
        m = _model(ctx, monkeypatch, f, prec, reuse=True, use_graph=route == "graph")
        bt = with_ax if route == "ax" else batch
        for k in range(4):
            got = _state(m, m.train_step(bt, None, lr=0.05))
            assert _equal_state(got, ref[k]), (route, k)
            if route == "ax":
                assert m._bufs["_s1"] is s and m._s1_uid is None
            else:
                assert m._s1_uid == batch.uid
                assert (m._bufs["_s1"] is m._bufs["s1"])
        if route == "graph":
            assert m.use_graph and any(not isinstance(g, str) for g in m._graphs.values())     # a captured step did replay
        ev = m.evaluate_batch(bt, None)
        assert ev[0] == ref_eval[0] and ev[1] == ref_eval[1] and _same(ev[2], ref_eval[2]), route
        assert _same(m(bt), ref_m(batch)), route


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("f", [32, 128])
def test_gcn2_kept_aggregate_is_dropped_when_the_batch_changes(ctx, monkeypatch, f, prec):
    """P, Q, P through one model (Q of P's shape: the buffers are not re-keyed, only the uid tells them apart), then a
    forward-only pass of Q between two steps on P, then x of P overwritten in place + invalidate(): always the bits of
    the model that gathers every step."""
    p, _ = _batch(ctx, f, seed=1)
    q, _ = _batch(ctx, f, seed=2)
    z, xz = _batch(ctx, f, seed=3)                       # the batch P turns into when its x is overwritten
    z.y = p.y
    m, ref_m = _model(ctx, monkeypatch, f, prec, reuse=True), _model(ctx, monkeypatch, f, prec, reuse=False)
    for k, bt in enumerate((p, p, q, p, p)):
        got, ref = _state(m, m.train_step(bt, None, lr=0.05)), _state(ref_m, ref_m.train_step(bt, None, lr=0.05))
        assert _equal_state(got, ref), k
        assert m._s1_uid == bt.uid and np.isfinite(ref[0][0]) and all(np.any(ref[1][j] != 0) for j in ORDER)
    ev, ref_ev = m.evaluate_batch(q, None), ref_m.evaluate_batch(q, None)      # forward only: uses no S1 of P, marks none
    assert ev[:2] == ref_ev[:2] and _same(ev[2], ref_ev[2]) and m._s1_uid is None
    assert _equal_state(_state(m, m.train_step(p, None, lr=0.05)), _state(ref_m, ref_m.train_step(p, None, lr=0.05)))
    assert m._s1_uid == p.uid
    old = p.uid
    p.x.copy_from_host(xz)
    p.invalidate()
    assert p.uid != old and p.ax is None
    for k in range(2):
        got, ref = _state(m, m.train_step(p, None, lr=0.05)), _state(ref_m, ref_m.train_step(z, None, lr=0.05))
        assert _equal_state(got, ref), k
    # a batch of another shape re-keys the buffers: nothing is kept across that
    r, _ = _batch(ctx, f, seed=4, sizes=(33, 5, 40, 9))
    assert _equal_state(_state(m, m.train_step(r, None, lr=0.05)), _state(ref_m, ref_m.train_step(r, None, lr=0.05)))
    m._ensure(p)
    assert m._s1_uid is None


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _dataset(f=32, sizes=(5, 40, 33, 12, 64, 7, 50)):
    import scipy.sparse as sp
    from gcnx import Graph, ListDataset
    rng = np.random.default_rng(9)
    graphs = []
    for g, n in enumerate(sizes):
        rowptr, colidx, _ = _chains(np.array([n], np.int64))
        a = sp.csr_matrix((np.ones(len(colidx), np.float32), colidx, rowptr), shape=(n, n))
        y = np.zeros(2, np.float32); y[g % 2] = 1
        graphs.append(Graph(x=rng.standard_normal((n, f), dtype=np.float32), a=a, y=y))
    return ListDataset(graphs)


def test_loader_hands_every_batch_its_aggregate(ctx):
    """DeviceDataset(aggregate_x=True): batch.ax of every batch of a shuffled epoch (7 graphs, batch size 3) is bit for bit
    the S output of the gathering forward on that batch; aggregate_x=False leaves ax unset; gcnx_collate's old argument
    list still assembles the same batch."""
    from gcnx import device as D, DeviceDataset, DeviceDisjointLoader
    ds = _dataset()
    dd = DeviceDataset(ctx, ds, normalize="spektral", aggregate_x=True)
    plain = DeviceDataset(ctx, ds, normalize="spektral")
    assert dd.ax is not None and dd.ax.shape == dd.x.shape and plain.ax is None
    w0 = ctx.zeros((32, 16))
    seen = 0
    for (batch, _), (pb, _) in zip(DeviceDisjointLoader(dd, batch_size=3, epochs=1, shuffle=True, seed=4),
                                   DeviceDisjointLoader(plain, batch_size=3, epochs=1, shuffle=True, seed=4)):
        s = ctx.zeros((batch.n, 32))
        D.gcn_conv_fwd(ctx, batch.a, batch.x, w0, None, ctx.empty((batch.n, 16)), act=None, s=s)
        assert batch.ax is not None and _same(batch.ax.numpy(), s.numpy()) and s.numpy().any()
        assert pb.ax is None and _same(pb.x.numpy(), batch.x.numpy()) and _same(pb.a.vals.numpy(), batch.a.vals.numpy())
        assert np.array_equal(pb.a.colidx.numpy(), batch.a.colidx.numpy())
        seen += batch.n_graphs
    assert seen == 7


def test_fit_with_and_without_the_loaders_aggregate_is_identical(ctx, monkeypatch):
    """One epoch of fit over the shuffled loader: the same final weights with aggregate_x on and off."""
    from gcnx import DeviceDataset, DeviceDisjointLoader
    from gcnx.train import fit
    ds = _dataset()
    res = {}
    for agg in (False, True):
        m = _model(ctx, monkeypatch, 32, "f32", reuse=True)
        loader = DeviceDisjointLoader(DeviceDataset(ctx, ds, normalize="spektral", aggregate_x=agg), batch_size=3, epochs=1,
                                      shuffle=True, seed=4)
        out = fit(m, loader, epochs=1, verbose=False)
        assert (m._bufs["_s1"] is not m._bufs["s1"]) == agg        # the last step read batch.ax / its own S1
        res[agg] = ([h[:2] for h in out["history"]], m.get_weights())          # (train loss, train accuracy) of the epoch
    assert res[True][0] == res[False][0] and np.isfinite(res[True][0][0][0])
    assert all(_same(x, y) for x, y in zip(res[True][1], res[False][1]))

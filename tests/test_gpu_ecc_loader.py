"""GPU tests of the device loader's edge side: gcnx_collate_edges through the C ABI against the NumPy gather of
tests/ecc_loader_ref.py (pinned on the CPU by tests/test_ecc_loader_host.py), the preset transposed pattern of a device batch
against gcnx_csr_transpose_perm on the batch's own CSR, device batches against DisjointLoader's, and gcnx.ECCNet trained and
evaluated from either loader -- bit for bit: the inputs are the same bits and every launch on this path has a fixed order."""
import numpy as np
import pytest

import ecc_loader_ref as L

pytestmark = pytest.mark.gpu
SENT_I, SENT_F = -77, -3.0          # no valid integer is negative; the edge features lie in (0, 1)


def _dataset(u):
    import gcnx
    return gcnx.ListDataset(L.graphs(u))


# ---- 1. the kernel through the C ABI ---------------------------------------------------------------------------------------------
def _call(ctx, d, s):
    ctx._ck(ctx.lib.gcnx_collate_edges(ctx.h, d["desc"].ptr, d["b"], d["node_ptr"].ptr, d["rowptr"].ptr, d["rowptr_t"].ptr,
                                       d["colidx_t"].ptr, d["perm_t"].ptr, d["e"].ptr, d["e"].ld, s, d["o_rowptr_t"].ptr,
                                       d["o_colidx_t"].ptr, d["o_perm_t"].ptr, d["o_e"].ptr, d["o_e"].ld))


@pytest.mark.parametrize("layout", ["dense", "wide_out", "wide_in"])
@pytest.mark.parametrize("s", [1, 2, 3, 16])
def test_collate_edges_against_the_numpy_gather(ctx, s, layout):
    """Integers equal the reference exactly, o_e equals the host collate's rows bit for bit, everything outside the written
    ranges (the capacity tails, the padding columns of a strided o_e) keeps its sentinel, and a second run gives the same bits.
    dense: lde == s == ldoe (the flat copy); wide_out: ldoe > s; wide_in: lde > s (the row / column form)."""
    from gcnx.loader import collate_disjoint
    u = L.union(s=s, seed=0)
    graphs = L.graphs(u)
    union_t = L.transpose_perm(u["rowptr"], u["colidx"])
    nnz_all = u["e"].shape[0]
    pad_in, pad_out = (3 if layout == "wide_in" else 0), (5 if layout == "wide_out" else 0)
    e_host = np.full((nnz_all, s + pad_in), 9.0, np.float32)
    e_host[:, pad_in // 2:pad_in // 2 + s] = u["e"]
    e_big = ctx.to_device(e_host)
    d = {"node_ptr": ctx.to_device(u["node_ptr"]), "rowptr": ctx.to_device(u["rowptr"]),
         "rowptr_t": ctx.to_device(union_t[0]), "colidx_t": ctx.to_device(union_t[1]), "perm_t": ctx.to_device(union_t[2]),
         "e": e_big.cols(pad_in // 2, pad_in // 2 + s)}
    assert d["e"].ld == s + pad_in
    for sel in L.SELECTIONS:
        desc, n, nnz = L.descriptor(u, sel)
        want = L.gather(u, sel, union_t)
        (_, _, e_collate, _), _ = collate_disjoint([graphs[j] for j in sel])
        assert e_collate.shape == (nnz, s)
        ncap, ecap = n + 5, nnz + 7                                         # capacity-sized outputs: the tails stay untouched
        o_big = ctx.to_device(np.full((ecap, s + pad_out), SENT_F, np.float32))
        d.update(desc=ctx.to_device(desc), b=len(sel), o_rowptr_t=ctx.to_device(np.full(ncap + 1, SENT_I, np.int32)),
                 o_colidx_t=ctx.to_device(np.full(ecap, SENT_I, np.int32)), o_perm_t=ctx.to_device(np.full(ecap, SENT_I, np.int32)),
                 o_e=o_big.cols(2 if pad_out else 0, (2 if pad_out else 0) + s))
        assert d["o_e"].ld == s + pad_out
        _call(ctx, d, s)
        got = {k: d[k].numpy() for k in ("o_rowptr_t", "o_colidx_t", "o_perm_t")}
        full = o_big.numpy()
        c0 = 2 if pad_out else 0
        assert np.array_equal(got["o_rowptr_t"][:n + 1], want["rowptr_t"]), (sel, "rowptr_t")
        assert np.array_equal(got["o_colidx_t"][:nnz], want["colidx_t"]), (sel, "colidx_t")
        assert np.array_equal(got["o_perm_t"][:nnz], want["perm_t"]), (sel, "perm_t")
        assert np.array_equal(full[:nnz, c0:c0 + s], e_collate.astype(np.float32)), (sel, "e")
        assert np.array_equal(full[:nnz, c0:c0 + s], want["e"])
        assert np.all(got["o_rowptr_t"][n + 1:] == SENT_I) and np.all(got["o_colidx_t"][nnz:] == SENT_I)
        assert np.all(got["o_perm_t"][nnz:] == SENT_I)
        assert np.all(full[nnz:] == SENT_F) and np.all(full[:, :c0] == SENT_F) and np.all(full[:, c0 + s:] == SENT_F)
        _call(ctx, d, s)                                                    # again: the same bits everywhere
        assert all(np.array_equal(d[k].numpy(), got[k]) for k in got) and np.array_equal(o_big.numpy(), full)
    assert np.array_equal(e_big.numpy(), e_host)                             # the inputs were only read


def test_collate_edges_validates_its_arguments(ctx):
    from gcnx import _lib
    u = L.union(s=2, seed=0)
    union_t = L.transpose_perm(u["rowptr"], u["colidx"])
    desc, n, nnz = L.descriptor(u, [4, 0, 7])
    names = ("desc", "node_ptr", "rowptr", "rowptr_t", "colidx_t", "perm_t", "e", "o_rowptr_t", "o_colidx_t", "o_perm_t", "o_e")
    o_e = ctx.to_device(np.full((nnz + 1, 2), SENT_F, np.float32))
    o_rp = ctx.to_device(np.full(n + 1, SENT_I, np.int32))
    arr = dict(desc=ctx.to_device(desc), node_ptr=ctx.to_device(u["node_ptr"]), rowptr=ctx.to_device(u["rowptr"]),
               rowptr_t=ctx.to_device(union_t[0]), colidx_t=ctx.to_device(union_t[1]), perm_t=ctx.to_device(union_t[2]),
               e=ctx.to_device(u["e"]), o_rowptr_t=o_rp, o_colidx_t=ctx.empty(nnz + 1, np.int32),
               o_perm_t=ctx.empty(nnz + 1, np.int32), o_e=o_e)
    assert set(arr) == set(names)
    ptr = {k: v.ptr for k, v in arr.items()}

    def call(b=3, s=2, lde=2, ldoe=2, **over):
        p = dict(ptr, **over)
        return ctx.lib.gcnx_collate_edges(ctx.h, p["desc"], b, p["node_ptr"], p["rowptr"], p["rowptr_t"], p["colidx_t"], p["perm_t"],
                                          p["e"], lde, s, p["o_rowptr_t"], p["o_colidx_t"], p["o_perm_t"], p["o_e"], ldoe)
    for k in names:
        assert call(**{k: None}) != _lib.OK, k
    assert call(s=0, lde=0, ldoe=0) != _lib.OK and call(lde=1) != _lib.OK and call(ldoe=1) != _lib.OK and call(b=-1) != _lib.OK
    with pytest.raises(_lib.GcnxError, match="gcnx_collate_edges"):
        ctx._ck(call(ldoe=1))
    assert call(b=0) == _lib.OK                                             # as gcnx_collate2: nothing to do
    assert np.all(o_e.numpy() == SENT_F) and np.all(o_rp.numpy() == SENT_I) # none of the calls above wrote anything
    assert call() == _lib.OK
    assert np.array_equal(o_e.numpy()[:nnz], L.gather(u, [4, 0, 7], union_t)["e"])


# ---- 2. the preset transposed pattern against the library's own transpose --------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
def test_preset_transpose_equals_csr_transpose_perm_of_the_batch(ctx, weighted):
    """Every batch of a shuffled epoch: transpose_perm() of the operator ECCNet uses (``batch.a.unweighted()``: a new view for a
    weighted dataset, which must be handed the preset) returns views of the loader's buffers -- no host sort ran -- holding
    what gcnx_csr_transpose_perm computes on a fresh DeviceCSR of the batch's own rowptr / colidx."""
    import gcnx
    from gcnx import device as D
    dsd = gcnx.DeviceDataset(ctx, _dataset(L.union(f=5, s=2, seed=0)), weighted=weighted, edge_features=True)
    assert (dsd.csr.vals is not None) == weighted and dsd.e.shape == (int(dsd.nnz_sizes.sum()), 2)
    loader = gcnx.DeviceDisjointLoader(dsd, batch_size=3, epochs=1, shuffle=True, seed=5)
    bufs, seen = loader._bufs, 0
    for batch, _ in loader:
        a = batch.a.unweighted()
        assert (a is not batch.a) == weighted
        t = a.transpose_perm()
        assert [v.ptr for v in t] == [bufs.rowptr_t.ptr, bufs.colidx_t.ptr, bufs.perm_t.ptr]
        assert [v.ptr for v in batch.a.transpose_perm()] == [v.ptr for v in t] and batch.e.ptr == bufs.e.ptr
        n, nnz = batch.a.n, batch.a.nnz
        assert t[0].shape == (n + 1,) and t[1].shape == t[2].shape == (max(nnz, 1),) and batch.e.shape == (nnz, 2)
        fresh = D.DeviceCSR(ctx, n, nnz, batch.a.rowptr, batch.a.colidx, None, symmetric=False)
        want = fresh.transpose_perm()
        assert all(w.ptr != v.ptr for w, v in zip(want, t))
        assert np.array_equal(t[0].numpy(), want[0].numpy())
        assert np.array_equal(t[1].numpy()[:nnz], want[1].numpy()[:nnz]) and np.array_equal(t[2].numpy()[:nnz], want[2].numpy()[:nnz])
        seen += 1
    assert seen == 3


# ---- 3. the same batches as the host loader ------------------------------------------------------------------------------------
def test_device_batches_equal_the_host_loaders(ctx):
    import gcnx
    from gcnx.models import DeviceBatch
    ds = _dataset(L.union(sizes=L.SIZES[:7], f=5, s=2, seed=1))
    dsd = gcnx.DeviceDataset(ctx, ds, weighted=False, edge_features=True)
    dev = gcnx.DeviceDisjointLoader(dsd, batch_size=3, epochs=1, shuffle=True, seed=11)
    host = gcnx.DisjointLoader(ds, batch_size=3, epochs=1, shuffle=True, seed=11)
    sizes = []
    for (inputs, target), (db, none) in zip(host, dev):
        assert none is None and len(inputs) == 4
        hb = DeviceBatch.from_host(ctx, inputs, target, weighted=False)
        nnz = hb.a.nnz
        assert (db.n, db.a.nnz, db.n_graphs) == (hb.n, nnz, hb.n_graphs)
        assert np.array_equal(db.x.numpy(), hb.x.numpy()) and np.array_equal(db.y.numpy(), hb.y.numpy())
        assert np.array_equal(db.a.rowptr.numpy(), hb.a.rowptr.numpy())
        assert np.array_equal(db.a.colidx.numpy()[:nnz], hb.a.colidx.numpy()[:nnz])
        assert np.array_equal(db.seg.dev.numpy(), hb.seg.dev.numpy())
        assert db.e.shape == hb.e.shape == (nnz, 2) and np.array_equal(db.e.numpy(), hb.e.numpy())
        assert db.a.vals is None and hb.a.vals is None
        (rp_d, ci_d, pm_d), (rp_h, ci_h, pm_h) = db.a.transpose_perm(), hb.a.transpose_perm()      # preset / sorted on the host
        assert np.array_equal(rp_d.numpy(), rp_h.numpy())
        assert np.array_equal(ci_d.numpy()[:nnz], ci_h.numpy()[:nnz]) and np.array_equal(pm_d.numpy()[:nnz], pm_h.numpy()[:nnz])
        sizes.append(db.n_graphs)
    assert sizes == [3, 3, 1]                                               # the last batch holds one graph


# ---- 4. the model ------------------------------------------------------------------------------------------------------------
def _undirected_union(seed):
    """Graphs of test_gpu_ecc._net_batch's kind: undirected with self loops, 10 .. 39 nodes, density 0.15, F = 16, S = 2."""
    sizes = np.random.default_rng(seed).integers(10, 40, 7).tolist()
    return L.union(sizes=sizes, f=16, s=2, seed=seed, directed=False, density=0.15, self_loops=True)


def _flat_weights(w):
    return [np.asarray(v) for v in w]


@pytest.mark.parametrize("kn", [None, [8]])
@pytest.mark.parametrize("kind", ["undirected", "directed"])
def test_eccnet_trains_and_evaluates_the_same_from_either_loader(ctx, kind, kn):
    """gcnx.fit for two epochs and gcnx.evaluate, fed by DeviceDisjointLoader over DeviceDataset(edge_features=True) and by
    DisjointLoader with the same seed and data: history, weights of every epoch, loss, accuracy and predictions are equal."""
    import gcnx
    u = _undirected_union(6) if kind == "undirected" else L.union(f=16, s=2, seed=0)
    ds = _dataset(u)
    dsd = gcnx.DeviceDataset(ctx, ds, edge_features=True)
    assert dsd.symmetric == (kind == "undirected")

    def run(tr, te, ev):
        m = gcnx.ECCNet(ctx, 2, channels=32, kernel_network=kn, seed=1)
        out = gcnx.fit(m, tr, te, epochs=2, verbose=False)
        return m, out, gcnx.evaluate(m, ev)
    m_d, out_d, ev_d = run(gcnx.DeviceDisjointLoader(dsd, batch_size=3, epochs=2, shuffle=True, seed=4),
                           gcnx.DeviceDisjointLoader(dsd, batch_size=4, shuffle=False),
                           gcnx.DeviceDisjointLoader(dsd, batch_size=4, shuffle=True, seed=9))
    m_h, out_h, ev_h = run(gcnx.DisjointLoader(ds, batch_size=3, epochs=2, shuffle=True, seed=4),
                           gcnx.DisjointLoader(ds, batch_size=4, shuffle=False),
                           gcnx.DisjointLoader(ds, batch_size=4, shuffle=True, seed=9))
    hist_d, hist_h = np.array(out_d["history"]), np.array(out_h["history"])
    assert hist_d.shape == (2, 4) and np.all(np.isfinite(hist_d))
    assert np.array_equal(hist_d, hist_h), (hist_d, hist_h)
    for ep, (wd, wh) in enumerate(zip(out_d["weights"], out_h["weights"])):
        assert len(wd) == len(wh) and all(np.array_equal(p, q) for p, q in zip(wd, wh)), ep
    wd, wh = _flat_weights(m_d.get_weights()), _flat_weights(m_h.get_weights())
    assert len(wd) == len(wh) and all(np.array_equal(p, q) for p, q in zip(wd, wh))
    (loss_d, acc_d), preds_d = ev_d
    (loss_h, acc_h), preds_h = ev_h
    assert loss_d == loss_h and acc_d == acc_h and len(preds_d) == len(preds_h) == -(-len(ds) // 4)
    assert all(np.array_equal(p, q) for p, q in zip(preds_d, preds_h))
    assert out_d["performance"] == out_h["performance"]


# ---- 5. defaults and errors ----------------------------------------------------------------------------------------------------
def test_defaults_are_unchanged_and_edge_features_compose_with_aggregate_x(ctx):
    import gcnx
    from gcnx.device_loader import collate_on_device
    ds = _dataset(L.union(f=32, s=2, seed=0, directed=False, self_loops=True))
    plain = gcnx.DeviceDataset(ctx, ds)
    b0 = collate_on_device(plain, [4, 0, 7])
    assert b0.e is None and plain.e is None and getattr(b0.a, "_tperm", None) is None
    with pytest.raises(ValueError, match="no edge features"):
        gcnx.ECCNet(ctx, 2, channels=32, seed=1).train_step(b0, None, lr=0.02)
    both = gcnx.DeviceDataset(ctx, ds, normalize="spektral", aggregate_x=True, edge_features=True)
    b1 = collate_on_device(both, [4, 0, 7])
    assert b1.ax is not None and b1.ax.shape == b1.x.shape and b1.e.shape == (b1.a.nnz, 2)
    only_ax = collate_on_device(gcnx.DeviceDataset(ctx, ds, normalize="spektral", aggregate_x=True), [4, 0, 7])
    only_e = collate_on_device(gcnx.DeviceDataset(ctx, ds, edge_features=True), [4, 0, 7])
    assert np.array_equal(b1.ax.numpy(), only_ax.ax.numpy()) and np.array_equal(b1.e.numpy(), only_e.e.numpy())
    assert np.array_equal(b1.x.numpy(), b0.x.numpy()) and np.array_equal(b1.a.colidx.numpy(), b0.a.colidx.numpy())
    for v, w in zip(b1.a.transpose_perm(), only_e.a.transpose_perm()):
        assert np.array_equal(v.numpy(), w.numpy())
    # what the constructor refuses, by the graph's index
    graphs = L.graphs(L.union(f=4, s=2, seed=0))
    graphs[5].e = graphs[5].e[:-1]
    with pytest.raises(ValueError, match=r"graph 5\b"):
        gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs), edge_features=True)
    assert collate_on_device(gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs)), [5, 1]).e is None      # ignored by default, as before

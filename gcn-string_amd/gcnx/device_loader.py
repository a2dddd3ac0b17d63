"""Device-resident dataset and loader.

``DisjointLoader`` (gcnx.loader) assembles every batch on the host -- vstack / block_diag / find, as Spektral does
for gcn.py:316-317 -- and ``DeviceBatch.from_host`` uploads it.  Once the kernels are fast that host work and the
PCIe copy dominate an epoch.  Here the whole dataset is uploaded ONCE as one disjoint union (features, CSR with
gcn_filter already applied per graph -- the filter of a block-diagonal matrix is the block-diagonal of the filters --
labels, node offsets); a batch is then one ``gcnx_collate`` launch that gathers the selected graphs' rows and
re-bases their indices, into buffers sized for the largest possible batch and reused for every batch.  Per batch
only 3(B+1) ints cross PCIe.  Iteration order, shuffling and batch boundaries are those of ``DisjointLoader``.

``DeviceDataset(aggregate_x=True)`` also keeps S = A X of the union: the filter being block-diagonal, A X of a batch is the
selected graphs' rows of it, gathered by the same launch (gcnx_collate2) into ``batch.ax`` -- GCN2's first layer then
needs no neighbour gather at all, in any step of any epoch.  It costs a second copy of the features (N_all x F x 4 bytes).

``DeviceDataset(edge_features=True)`` also keeps the graphs' edge features e [nnz_all, S] (one row per stored entry) and the
union's transposed pattern with its entry permutation (one ``transpose_perm()`` at construction).  The union is block-diagonal,
so a batch's rows of e AND its transposed pattern are gathers too: a second launch per batch (gcnx_collate_edges) fills
``batch.e`` and presets what ``batch.a.transpose_perm()`` returns -- gcnx.ECCNet trains from these batches with no host sort,
no download and no synchronisation per batch.
"""
from __future__ import annotations

import math

import numpy as np

from . import device as D
from .loader import collate_disjoint
from .models import DeviceBatch


def union_edge_features(graphs, nnz_sizes):
    """The edge features of a list of graphs as one float32 array [sum(nnz_sizes), S], the graphs' rows in dataset order:
    the e of the disjoint union.  Every graph must carry a 2-D ``e`` with one row per stored entry of its adjacency
    (``nnz_sizes[k]`` rows for graph k: the entries left after the COO build, which drops explicitly stored zeros -- the rule
    of DeviceBatch.from_host), all of one width S >= 1.  Pure NumPy; raises ValueError naming the first graph that does not."""
    parts, width = [], None
    if len(graphs) != len(nnz_sizes):
        raise ValueError(f"{len(graphs)} graphs but {len(nnz_sizes)} entry counts")
    for k, g in enumerate(graphs):
        e = getattr(g, "e", None)
        if e is None:
            raise ValueError(f"graph {k} carries no edge features: DeviceDataset(edge_features=True) needs Graph(e=...) on every "
                             f"graph (from_networkx(use_edge_data='entries'))")
        e = np.asarray(e)
        nnz = int(nnz_sizes[k])
        if e.ndim != 2 or e.shape[0] != nnz:
            raise ValueError(f"graph {k}: edge features e have shape {e.shape}: expected one row per stored entry of the adjacency "
                             f"({nnz} entries, row-major; from_networkx(use_edge_data='entries') builds them so)")
        if e.shape[1] < 1:
            raise ValueError(f"graph {k}: edge features e have shape {e.shape}: at least one column")
        if width is None:
            width = e.shape[1]
        elif e.shape[1] != width:
            raise ValueError(f"graph {k}: edge features e have {e.shape[1]} columns, the graphs before it {width}")
        parts.append(e.astype(np.float32, copy=False))
    if width is None:
        raise ValueError("no graphs: the width of the edge features is unknown")
    return np.ascontiguousarray(np.concatenate(parts, 0), np.float32)


class DeviceDataset:
    """All graphs of a ``Dataset`` resident in HBM.  By default edge features are not carried: graphs built with
    ``Graph(e=...)`` are accepted and their ``e`` is ignored (gcnx_collate gathers x, the adjacency and the labels only), and
    the batches of a DeviceDisjointLoader serve GCN2 / GeneralGNN / GCN.  With ``edge_features=True`` the batches also carry
    ``e`` and their transposed pattern (gcnx_collate_edges), which is what gcnx.ECCNet reads."""

    def __init__(self, ctx, dataset, normalize=None, weighted=True, symmetric=None, aggregate_x=False, edge_features=False):
        """aggregate_x: also compute S_all = A X once, here, and hand every batch its rows as ``batch.ax`` (see the module
        docstring).  Doubles the feature storage: N_all x F x 4 bytes more.  False (default): batches carry no ``ax``.
        edge_features: keep e of every graph (union_edge_features states what they must look like) and the union's
        ``transpose_perm()``; every batch then has ``batch.e`` [nnz, S] and a preset ``batch.a.transpose_perm()``.  False
        (default): ``batch.e`` is None whatever the graphs carry."""
        self.ctx = ctx
        graphs = [dataset[i] for i in range(len(dataset))]
        inputs, y = collate_disjoint(graphs)
        x, a, i = inputs[0], inputs[1], inputs[-1]          # ((x, a, e, i), y) when the graphs carry e: ignored here
        sizes = np.array([g.n_nodes for g in graphs], np.int64)
        self.n_graphs = len(graphs)
        self.node_ptr_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(self.node_ptr_host[-1])
        rows = np.asarray(a.indices)[:, 0]
        rowptr_host = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=rowptr_host[1:])
        self.ent_ptr_host = rowptr_host[self.node_ptr_host]          # entry offset of every graph
        self.sizes = sizes
        self.nnz_sizes = np.diff(self.ent_ptr_host)
        e = union_edge_features(graphs, self.nnz_sizes) if edge_features else None     # (refused before anything is uploaded)
        seg = D.Segments(ctx, self.node_ptr_host)
        csr = D.DeviceCSR.from_coo(ctx, a.indices, a.values, n, graph_ptr=seg.host, symmetric=symmetric, weighted=weighted)
        if normalize:
            csr = csr.gcn_norm(normalize)
        self.csr, self.symmetric = csr, csr.symmetric    # checked once on the union (symmetric=None); batches inherit it
        self.x = ctx.to_device(x, np.float32)
        y = np.asarray(y, np.float32)
        self.y = ctx.to_device(y.reshape(self.n_graphs, -1), np.float32)
        self.node_ptr = seg.dev
        self.n_features, self.n_labels = self.x.shape[1], self.y.shape[1]
        self.e = self.tperm = None
        self.n_edge_features = 0
        self.ax = self._aggregate() if aggregate_x else None
        if edge_features:
            tperm = csr.transpose_perm()                   # of the union: once (a download, a host counting sort, an upload)
            # block-diagonality, as the re-basing of gcnx_collate_edges needs it: every graph's block of the transpose starts
            # where its block of the CSR does (and so, by the next graph's offset, covers the same entry range)
            if not np.array_equal(tperm[0].numpy()[self.node_ptr_host].astype(np.int64), self.ent_ptr_host):
                raise ValueError("DeviceDataset(edge_features=True): the union's adjacency is not block-diagonal with respect to "
                                 "the graphs (an entry leaves its graph): its transpose cannot be gathered per graph")
            self.n_edge_features = int(e.shape[1])
            self.e = ctx.to_device(e) if e.shape[0] else ctx.empty((0, self.n_edge_features))
            self.tperm = tperm

    def _aggregate(self, max_rows=1 << 20):
        """S_all = A X with, in every row, the bits the one-launch GCNConv forward writes as its S output for a batch that
        holds the row's graph: that launch itself, run for its S output alone (a [F, 16] zero weight; the product is
        discarded) over runs of consecutive graphs collated like any batch.  A row is accumulated by one lane group in CSR
        order from zero wherever it lies in a tile, and a graph's rows and entries keep their order in every batch, so the
        bits do not depend on the batch.  (The row-gather SpMM splits a row's entries over lane groups: other bits.)"""
        ctx, f = self.ctx, self.n_features
        n = int(self.node_ptr_host[-1])
        if f not in (32, 64, 128):
            raise ValueError(f"DeviceDataset(aggregate_x=True) needs 32, 64 or 128 features (the one-launch GCNConv's widths), got {f}")
        out = ctx.empty((max(n, 1), f))
        w0 = ctx.zeros((f, 16))
        g = 0
        while g < self.n_graphs:
            h = g + 1
            while h < self.n_graphs and self.node_ptr_host[h + 1] - self.node_ptr_host[g] <= max_rows:
                h += 1
            batch = collate_on_device(self, np.arange(g, h))
            if batch.n:
                if not D.gcn_conv_fused_ok(ctx, batch.n, f, 16):
                    raise ValueError(f"DeviceDataset(aggregate_x=True): a graph of {batch.n} rows is beyond the one-launch GCNConv")
                s = D.DeviceArray._view(out, int(self.node_ptr_host[g]) * f, (batch.n, f))
                D.gcn_conv_fwd(ctx, batch.a, batch.x, w0, None, ctx.empty((batch.n, 16)), act=None, s=s)
            ctx.sync()                                       # the chunk's buffers go with it
            g = h
        return out

    def __len__(self):
        return self.n_graphs

    def capacity(self, batch_size):
        """Rows / entries of the largest batch of `batch_size` graphs."""
        b = min(batch_size, self.n_graphs)
        return int(np.sort(self.sizes)[-b:].sum()), int(np.sort(self.nnz_sizes)[-b:].sum())


class _BatchBuffers:
    def __init__(self, ctx, ds, batch_size):
        ncap, ecap = ds.capacity(batch_size)
        self.x = ctx.empty((ncap, ds.n_features))
        self.ax = ctx.empty((ncap, ds.n_features)) if getattr(ds, "ax", None) is not None else None
        self.rowptr = ctx.empty(ncap + 1, np.int32)
        self.colidx = ctx.empty(max(ecap, 1), np.int32)
        self.vals = ctx.empty(max(ecap, 1), np.float32) if ds.csr.vals is not None else None
        self.y = ctx.empty((batch_size, ds.n_labels))
        self.gp = ctx.empty(batch_size + 1, np.int32)
        self.ids = ctx.empty(max(ncap, 1), np.int32)     # DisjointLoader's id vector i, written by the collate launch
        self.desc = ctx.empty(3 * (batch_size + 1), np.int32)
        self.e = self.rowptr_t = self.colidx_t = self.perm_t = None
        if getattr(ds, "e", None) is not None:           # edge features and the transposed pattern (gcnx_collate_edges)
            self.e = ctx.empty((max(ecap, 1), ds.n_edge_features))
            self.rowptr_t = ctx.empty(ncap + 1, np.int32)
            self.colidx_t = ctx.empty(max(ecap, 1), np.int32)
            self.perm_t = ctx.empty(max(ecap, 1), np.int32)


def collate_on_device(ds, indices, bufs=None):
    """The DeviceBatch of the graphs `indices` (dataset order positions), assembled by one gcnx_collate2 launch (with the
    dataset's A X rows as ``batch.ax`` when it keeps them) and, for a dataset that keeps edge features, one gcnx_collate_edges
    launch behind it: ``batch.e``, and the batch CSR's ``transpose_perm()`` preset to views of the loader's buffers."""
    ctx = ds.ctx
    sel = np.asarray(indices, np.int64)
    b = len(sel)
    bufs = bufs or _BatchBuffers(ctx, ds, b)
    bn = np.concatenate([[0], np.cumsum(ds.sizes[sel])])
    be = np.concatenate([[0], np.cumsum(ds.nnz_sizes[sel])])
    n, nnz = int(bn[-1]), int(be[-1])
    desc = np.concatenate([sel, [0], bn, be]).astype(np.int32)
    V = D.DeviceArray._view                              # (views without flat()'s checks: eight per batch)
    dview = V(bufs.desc, 0, (int(desc.size),))
    dview.copy_from_host(desc, wait=False)               # queued: the host runs ahead of the GPU across batches
    f, c = ds.n_features, ds.n_labels
    csr = ds.csr
    ax = getattr(ds, "ax", None)                         # (None while the dataset is still computing it)
    ctx._ck(ctx.lib.gcnx_collate2(ctx.h, dview.ptr, b, ds.node_ptr.ptr, csr.rowptr.ptr, csr.colidx.ptr,
                                  csr.vals.ptr if csr.vals is not None else None, ds.x.ptr, ds.x.ld, f, ds.y.ptr, c,
                                  bufs.rowptr.ptr, bufs.colidx.ptr, bufs.vals.ptr if bufs.vals is not None else None,
                                  bufs.x.ptr, bufs.x.ld, bufs.y.ptr, bufs.gp.ptr, bufs.ids.ptr,
                                  ax.ptr if ax is not None else None, ax.ld if ax is not None else 0,
                                  bufs.ax.ptr if ax is not None else None, bufs.ax.ld if ax is not None else 0))
    seg = D.Segments.from_device(ctx, V(bufs.gp, 0, (b + 1,)), bn)
    seg._ids = V(bufs.ids, 0, (max(n, 1),))              # (otherwise built on the host on first use and uploaded)
    a = D.DeviceCSR(ctx, n, nnz, V(bufs.rowptr, 0, (n + 1,)), V(bufs.colidx, 0, (max(nnz, 1),)),
                    V(bufs.vals, 0, (max(nnz, 1),)) if bufs.vals is not None else None, seg.dev, b, ds.symmetric,
                    int(ds.sizes[sel].max()) if b else 0)
    e = None
    if getattr(ds, "e", None) is not None:
        s = ds.n_edge_features
        rp_t, ci_t, pm_t = ds.tperm
        ctx._ck(ctx.lib.gcnx_collate_edges(ctx.h, dview.ptr, b, ds.node_ptr.ptr, csr.rowptr.ptr, rp_t.ptr, ci_t.ptr, pm_t.ptr,
                                           ds.e.ptr, ds.e.ld, s, bufs.rowptr_t.ptr, bufs.colidx_t.ptr, bufs.perm_t.ptr,
                                           bufs.e.ptr, bufs.e.ld))
        # what transpose_perm() would compute (download, host sort, upload, synchronise) is already there
        a._tperm = (V(bufs.rowptr_t, 0, (n + 1,)), V(bufs.colidx_t, 0, (max(nnz, 1),)), V(bufs.perm_t, 0, (max(nnz, 1),)))
        e = V(bufs.e, 0, (nnz, s))
    batch = DeviceBatch(ctx, V(bufs.x, 0, (n, f)), a, seg, V(bufs.y, 0, (b, c)), e=e,
                        ax=V(bufs.ax, 0, (n, f)) if ax is not None else None)
    batch._bufs = bufs                                   # keeps the capacity buffers alive with the batch
    return batch


class DeviceDisjointLoader:
    """``DisjointLoader`` over a ``DeviceDataset``: same arguments, same order of graphs (same seed -> same
    batches), but yields ``(DeviceBatch, None)`` -- the labels ride in ``batch.y`` -- assembled on the device.
    Every batch reuses one set of capacity-sized buffers: a batch is valid until the next one is drawn."""

    def __init__(self, dataset, batch_size=1, epochs=None, shuffle=True, seed=None):
        assert isinstance(dataset, DeviceDataset)
        self.dataset, self.batch_size, self.epochs, self.shuffle = dataset, int(batch_size), epochs, shuffle
        self._rng = np.random.default_rng(seed) if seed is not None else np.random
        self._bufs = _BatchBuffers(dataset.ctx, dataset, min(self.batch_size, len(dataset)))
        self._gen = self._generator()

    @property
    def steps_per_epoch(self):
        return int(math.ceil(len(self.dataset) / self.batch_size))

    def _generator(self):
        n = len(self.dataset)
        epoch = 0
        while self.epochs is None or epoch < self.epochs:
            order = np.arange(n)
            if self.shuffle:
                self._rng.shuffle(order)
            for s in range(0, n, self.batch_size):
                yield order[s:s + self.batch_size]
            epoch += 1

    def __iter__(self):
        return self

    def __next__(self):
        return collate_on_device(self.dataset, next(self._gen), self._bufs), None

    def load(self):
        return self

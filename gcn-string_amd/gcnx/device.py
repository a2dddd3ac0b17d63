"""Device context, device arrays and the thin op layer over the C ABI (include/gcnx.h)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L


class _Side:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx._ck(self.ctx.lib.gcnx_side_begin(self.ctx.h))
        return self

    def __exit__(self, *exc):
        self.ctx._ck(self.ctx.lib.gcnx_side_end(self.ctx.h))
        return False


_DEFAULT_CTX = None


def default_context():
    """The process-wide Context the models use when none is passed (``GeneralGNN(n_labels, activation="softmax")`` -- Spektral's
    own signature, gcn.py:320): device LOCAL_RANK (one process per GPU), created on first use; raises without a GPU."""
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None or not _DEFAULT_CTX._live:
        _DEFAULT_CTX = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _DEFAULT_CTX


def with_default_context(init):
    """Constructor decorator: the leading ``ctx`` may be left out (then it is default_context())."""
    import functools

    @functools.wraps(init)
    def wrapper(self, *args, **kw):
        if "ctx" in kw or (args and isinstance(args[0], Context)):
            return init(self, *args, **kw)
        return init(self, default_context(), *args, **kw)
    return wrapper


class Context:
    """One GPU + one HIP stream (gcnx_ctx).  Not thread-safe; one per process per GPU."""

    def __init__(self, device=0):
        self.lib = L.load()
        h = C.c_void_p()
        L.check(self.lib.gcnx_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self._live = True
        self._force_plan = os.environ.get("GCNX_SPMM_KERNEL", "")[:1] in ("t", "p")

    # -- info ------------------------------------------------------------------------------
    def info(self):
        name = C.create_string_buffer(64)
        cus = C.c_int()
        hbm = C.c_size_t()
        self._ck(self.lib.gcnx_device_info(self.h, name, 64, C.byref(cus), C.byref(hbm)))
        return {"arch": name.value.decode(), "cus": cus.value, "hbm_bytes": hbm.value}

    def _ck(self, rc):
        L.check(rc, self.h)

    SPMM_KERNELS = {"auto": 0, "rows": 1, "tile": 2, "pipe": 3}

    def set_lr_source(self, scalar):
        """The update launches read the learning rate from this 1-element fp32 device array instead of their ``lr`` argument
        (None: the argument again); gcnx_set_lr_source.  A captured step then serves every value of a schedule."""
        self._ck(self.lib.gcnx_set_lr_source(self.h, scalar.ptr if scalar is not None else None))

    def set_tuning(self, key, value):
        """Kernel-selection knobs of this context (gcnx_set_tuning; diagnostics: results never depend on them).
        ``set_tuning("spmm_kernel", "auto" | "rows" | "tile" | "pipe")``, ``("gemm_stream", 0 | 1)``, ..."""
        if key == "spmm_kernel":
            self._force_plan = value in ("tile", "pipe")
            value = self.SPMM_KERNELS[value]
        self._ck(self.lib.gcnx_set_tuning(self.h, key.encode(), int(value)))

    # -- memory ----------------------------------------------------------------------------
    def empty(self, shape, dtype=np.float32):
        return DeviceArray.alloc(self, shape, dtype)

    def zeros(self, shape, dtype=np.float32):
        a = DeviceArray.alloc(self, shape, dtype)
        a.fill_zero()
        return a

    def to_device(self, host, dtype=None):
        host = np.ascontiguousarray(host, dtype=dtype)
        a = DeviceArray.alloc(self, host.shape, host.dtype)
        if host.nbytes:
            self._ck(self.lib.gcnx_h2d(self.h, a.ptr, host.ctypes.data, host.nbytes))
        return a

    def sync(self):
        self._ck(self.lib.gcnx_sync(self.h))

    def side(self):
        """``with ctx.side(): ...`` -- the gcnx calls inside run on the side stream, after everything submitted
        so far and concurrently with what follows; ``ctx.join()`` makes the main stream wait for them."""
        return _Side(self)

    def join(self):
        self._ck(self.lib.gcnx_side_join(self.h))

    # -- events / graphs -------------------------------------------------------------------
    def event(self):
        return Event(self)

    def capture(self, fn):
        """Capture the gcnx calls made by fn() into a replayable HIP graph."""
        self._ck(self.lib.gcnx_capture_begin(self.h))
        try:
            fn()
        except Exception:
            g = C.c_void_p()
            self.lib.gcnx_capture_end(self.h, C.byref(g))
            if g:
                self.lib.gcnx_graph_destroy(self.h, g)
            raise
        g = C.c_void_p()
        self._ck(self.lib.gcnx_capture_end(self.h, C.byref(g)))
        return Graph(self, g)

    def close(self):
        if self._live:
            self._live = False
            self.lib.gcnx_ctx_destroy(self.h)

    def __del__(self):
        pass  # explicit close(); device arrays may outlive an implicit destructor order


class Event:
    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx._ck(ctx.lib.gcnx_event_create(ctx.h, C.byref(self.h)))

    def record(self):
        self.ctx._ck(self.ctx.lib.gcnx_event_record(self.ctx.h, self.h))
        return self

    def elapsed_ms_since(self, start):
        ms = C.c_float()
        self.ctx._ck(self.ctx.lib.gcnx_event_elapsed_ms(self.ctx.h, start.h, self.h, C.byref(ms)))
        return ms.value


class Graph:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def launch(self):
        self.ctx._ck(self.ctx.lib.gcnx_graph_launch(self.ctx.h, self.h))

    def destroy(self):
        if self.h:
            self.ctx.lib.gcnx_graph_destroy(self.ctx.h, self.h)
            self.h = None


class DeviceArray:
    """Row-major device buffer (1-D or 2-D) or a column-slice view of one (ld = row stride)."""

    __slots__ = ("ctx", "ptr", "shape", "dtype", "ld", "_base", "_owner", "_spmm_plan")

    def __init__(self, ctx, ptr, shape, dtype, ld=None, base=None, owner=False):
        self.ctx, self.ptr, self.shape, self.dtype = ctx, ptr, tuple(int(s) for s in shape), np.dtype(dtype)
        self.ld = int(ld) if ld is not None else (self.shape[-1] if self.shape else 1)
        self._base, self._owner = base, owner
        self._spmm_plan = None

    @classmethod
    def _view(cls, base, nelem_off, shape):
        """Contiguous view of ``base`` starting at element ``nelem_off`` with a shape of plain ints -- flat() without its
        checks, for callers that build many views per step (the per-batch activation views of a streamed epoch)."""
        self = object.__new__(cls)
        self.ctx, self.ptr, self.shape, self.dtype = base.ctx, base.ptr + nelem_off * base.dtype.itemsize, shape, base.dtype
        self.ld = shape[-1]
        self._base, self._owner, self._spmm_plan = base, False, None
        return self

    @classmethod
    def alloc(cls, ctx, shape, dtype):
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        ctx._ck(ctx.lib.gcnx_malloc(ctx.h, max(nbytes, 16), C.byref(p)))
        return cls(ctx, p.value, shape, dtype, owner=True)

    @property
    def size(self):
        n = 1
        for d in self.shape:
            n *= d
        return n

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def contiguous(self):
        return len(self.shape) < 2 or self.ld == self.shape[1]

    def cols(self, c0, c1):
        """View of columns [c0, c1) -- Spektral's concat-skip is written in place through these."""
        assert len(self.shape) == 2 and 0 <= c0 <= c1 <= self.shape[1]
        return DeviceArray(self.ctx, self.ptr + c0 * self.dtype.itemsize, (self.shape[0], c1 - c0), self.dtype,
                           ld=self.ld, base=self)

    def flat(self, off, n, shape=None):
        """View of n elements starting at element `off` of a contiguous buffer."""
        assert self.contiguous and off + n <= self.size
        return DeviceArray(self.ctx, self.ptr + off * self.dtype.itemsize, shape or (n,), self.dtype, base=self)

    def fill_zero(self):
        assert self.contiguous
        self.ctx._ck(self.ctx.lib.gcnx_memset(self.ctx.h, self.ptr, 0, self.nbytes))

    def copy_from_host(self, host, wait=True):
        """wait=False: small copies are staged and queued in stream order without stalling the host (gcnx_h2d_async)."""
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.size == self.size and self.contiguous
        fn = self.ctx.lib.gcnx_h2d if wait else self.ctx.lib.gcnx_h2d_async
        self.ctx._ck(fn(self.ctx.h, self.ptr, host.ctypes.data, host.nbytes))

    def numpy(self):
        if self.contiguous:
            out = np.empty(self.shape, dtype=self.dtype)
            if out.nbytes:
                self.ctx._ck(self.ctx.lib.gcnx_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
            return out
        # strided view: fetch the enclosing rows and slice on the host
        rows, cols = self.shape
        span = (rows - 1) * self.ld + cols
        buf = np.empty(span, dtype=self.dtype)
        self.ctx._ck(self.ctx.lib.gcnx_d2h(self.ctx.h, buf.ctypes.data, self.ptr, buf.nbytes))
        full = np.zeros(rows * self.ld, dtype=self.dtype)
        full[:span] = buf
        return full.reshape(rows, self.ld)[:, :cols].copy()

    def free(self):
        if self._owner and self.ptr and self.ctx._live:
            self.ctx.lib.gcnx_free(self.ctx.h, self.ptr)
        self.ptr = None
        self._owner = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCSR:
    """Adjacency of a disjoint batch on the device: CSR int32 (+ fp32 values or None = ones).

    ``block_ptr`` (= graph_ptr) marks the diagonal blocks; ``symmetric`` lets the backward pass
    reuse this CSR for A^T (true for the reference's undirected contact graphs and for
    gcn_filter of a symmetric A); otherwise ``transpose()`` builds the transposed CSR once.
    ``symmetric=None`` (the default of the constructors that take host data): checked once on the device
    (gcnx_csr_inspect) -- the reference's loader accepts any scipy matrix, and a directed adjacency run through the
    symmetric shortcut would give silently wrong gradients.  The same pass checks that no entry leaves its
    graph_ptr block (what the tile plan and the folded pool backward assume); a batch that fails it is refused.
    """

    def __init__(self, ctx, n, nnz, rowptr, colidx, vals=None, block_ptr=None, n_blocks=0, symmetric=None, max_block_rows=0):
        self.ctx, self.n, self.nnz = ctx, int(n), int(nnz)
        self.max_block_rows = int(max_block_rows)     # rows of the largest graph, where the constructor knew graph_ptr on the host (0: unknown)
        self.rowptr, self.colidx, self.vals = rowptr, colidx, vals
        self.block_ptr, self.n_blocks = block_ptr, int(n_blocks)
        self._t = None
        self._plan = None
        self.dense_shape = (self.n, self.n)
        if symmetric is None:
            props = self.inspect()
            symmetric = bool(props & L.CSR_SYMMETRIC)
            if block_ptr is not None and self.n_blocks > 0 and not props & L.CSR_BLOCK_DIAGONAL:
                raise ValueError("adjacency is not block-diagonal with respect to graph_ptr (a DisjointLoader batch is: "
                                 "sp.block_diag); graph_ptr must start at 0, end at N and be non-decreasing")
        self.symmetric = bool(symmetric)

    def inspect(self):
        """Device-side structure check (gcnx_csr_inspect): bit set of L.CSR_SYMMETRIC / CSR_BLOCK_DIAGONAL /
        CSR_GRAPH_PTR_OK."""
        props = C.c_int(0)
        has_blocks = self.block_ptr is not None and self.n_blocks > 0
        self.ctx._ck(self.ctx.lib.gcnx_csr_inspect(self.ctx.h, self.rowptr.ptr, self.colidx.ptr,
                                                    self.vals.ptr if self.vals is not None else None, self.n,
                                                    self.block_ptr.ptr if has_blocks else None,
                                                    self.n_blocks if has_blocks else 0, C.byref(props)))
        return props.value

    @property
    def plan(self):
        """gcnx_spmm_plan of this batch's block structure (built on first use, shared by every
        CSR that shares block_ptr: normalised / unweighted / transposed views)."""
        if self.block_ptr is None or self.n_blocks == 0:
            return None
        # The tile kernels need >= 4 (graph, 32-column slab) units per CU (gcnx_spmm_csr); below ~128 graphs no
        # width reaches that, and building a plan (a D2H copy, a host sort, an upload) per streamed batch is wasted.
        # (r3: a large batch of FEW graphs -- config 5: 122 power-law graphs of 8 192 nodes -- gets a plan too: it lists the hub
        # rows, which then run as segments on workgroups of their own)
        # (r4: and a batch that holds a graph of >= 4096 rows, whatever its size -- the plan lists the column-block work of such
        # graphs, whose feature rows do not fit an XCD's L2: spmm_cb_kernel)
        if self.n_blocks < 128 and self.n < 131072 and self.max_block_rows < 4096 and not getattr(self.ctx, "_force_plan", False):
            return None
        holder = self.block_ptr
        p = getattr(holder, "_spmm_plan", None)
        if p is None:
            h = C.c_void_p()
            self.ctx._ck(self.ctx.lib.gcnx_spmm_plan_create(self.ctx.h, holder.ptr, self.n_blocks, C.byref(h)))
            p = _Plan(self.ctx, h)
            holder._spmm_plan = p
        if self._plan is not p:
            # the tile kernels' degree order of THIS operator's rows (gcnx_spmm_plan_bind: synchronises and rebuilds, so it
            # happens here, ONCE per (plan, rowptr) -- the normalised / unweighted / row-mean views share rowptr and with it
            # the order -- and never inside a captured call: a view created inside a captured sequence finds the order bound)
            key = (self.rowptr.ptr, self.n)
            if key not in p.bound:
                self.ctx._ck(self.ctx.lib.gcnx_spmm_plan_bind(self.ctx.h, p.h, self.rowptr.ptr, self.n))
                p.bound.add(key)
            self._plan = p
        return p.h

    def rebind(self):
        """The row pointers behind ``rowptr`` were rewritten in place: rebuild the plan's row order for them
        (gcnx_spmm_plan_bind, case (b) of include/gcnx.h).  Not inside a captured sequence."""
        self._plan = None
        p = getattr(self.block_ptr, "_spmm_plan", None) if self.block_ptr is not None else None
        if p is not None:
            p.bound.discard((self.rowptr.ptr, self.n))
        return self.plan

    @classmethod
    def from_host_csr(cls, ctx, rowptr, colidx, vals=None, graph_ptr=None, symmetric=None):
        n = len(rowptr) - 1
        d_rp = ctx.to_device(rowptr, np.int32)
        d_ci = ctx.to_device(colidx, np.int32)
        d_v = ctx.to_device(vals, np.float32) if vals is not None else None
        d_gp = ctx.to_device(graph_ptr, np.int32) if graph_ptr is not None else None
        return cls(ctx, n, len(colidx), d_rp, d_ci, d_v, d_gp, 0 if graph_ptr is None else len(graph_ptr) - 1, symmetric,
                   _max_block(graph_ptr))

    @classmethod
    def from_coo(cls, ctx, indices, values, n, graph_ptr=None, symmetric=None, weighted=True):
        """DisjointLoader's SparseTensor (indices[nnz,2] int64 row-major sorted) -> device CSR
        via gcnx_coo_to_csr (the COO never becomes a host CSR)."""
        indices = np.asarray(indices)
        nnz = indices.shape[0]
        rows = ctx.to_device(indices[:, 0], np.int64)
        cols = ctx.to_device(indices[:, 1], np.int64)
        d_rp = ctx.empty(n + 1, np.int32)
        d_ci = ctx.empty(max(nnz, 1), np.int32)
        ctx._ck(ctx.lib.gcnx_coo_to_csr(ctx.h, rows.ptr, cols.ptr, nnz, n, d_rp.ptr, d_ci.ptr))
        rows.free(); cols.free()
        d_v = ctx.to_device(values, np.float32) if (weighted and values is not None) else None
        d_gp = ctx.to_device(graph_ptr, np.int32) if graph_ptr is not None else None
        return cls(ctx, n, nnz, d_rp, d_ci, d_v, d_gp, 0 if graph_ptr is None else len(graph_ptr) - 1, symmetric, _max_block(graph_ptr))

    def gcn_norm(self, mode="spektral"):
        """Device gcn_filter: returns a CSR sharing structure with self, values = A^."""
        out = self.ctx.empty(max(self.nnz, 1), np.float32)
        self.ctx._ck(self.ctx.lib.gcnx_gcn_norm(self.ctx.h, self.rowptr.ptr, self.colidx.ptr,
                                                 self.vals.ptr if self.vals is not None else None, self.n,
                                                 L.NORM_SPEKTRAL if mode == "spektral" else L.NORM_PYG, out.ptr))
        return DeviceCSR(self.ctx, self.n, self.nnz, self.rowptr, self.colidx, out, self.block_ptr, self.n_blocks,
                         self.symmetric, self.max_block_rows)

    def cheb_norm(self):
        """ChebConv's operator S (gcnx_cheb_norm): a CSR sharing structure with self, values r_i w_ij r_j off the diagonal and 0
        on it, r = deg^-1/2 of the column sums without the diagonal (PyG's get_laplacian; L^ = c_s S + c_d I is applied by
        cheb_basis / cheb_sum).  Built once per operator; its ``transpose()`` is S^T."""
        if getattr(self, "_cheb", None) is None:
            out = self.ctx.empty(max(self.nnz, 1), np.float32)
            t = self.transpose()
            self.ctx._ck(self.ctx.lib.gcnx_cheb_norm(self.ctx.h, self.rowptr.ptr, self.colidx.ptr, _p(self.vals), t.rowptr.ptr,
                                                      t.colidx.ptr, _p(t.vals), self.n, out.ptr))
            self._cheb = DeviceCSR(self.ctx, self.n, self.nnz, self.rowptr, self.colidx, out, self.block_ptr, self.n_blocks,
                                   self.symmetric, self.max_block_rows)
        return self._cheb

    def rgcn_operator(self, e, rule="nonzero", num_relations=None):
        """RGCNConv's per-entry operands (gcnx_rgcn_operator): (rel, val, rel_t, val_t) -- rel [nnz] uint8, the relation of every
        stored entry read off the edge features e [nnz, edge_dim], val [nnz] = 1 / (entries of the entry's row with its relation),
        and both in the order of the transposed pattern (``transpose_perm``).  rule "nonzero": the first non-zero column of e,
        edge_dim where there is none (num_relations = edge_dim + 1); "index": column 0 holds the relation, and a value outside
        0 .. num_relations - 1 is clamped into that range on the device.  Not cached here: the caller keeps it with the batch."""
        ctx, ne = self.ctx, max(self.nnz, 1)
        edge_dim = e.shape[1]
        r = edge_dim + 1 if num_relations is None and rule == "nonzero" else int(num_relations)
        assert e.shape[0] >= self.nnz and rule in L.RGCN_RULES
        _, _, perm = self.transpose_perm()
        rel, rel_t = ctx.empty(ne, np.uint8), ctx.empty(ne, np.uint8)
        val, val_t = ctx.empty(ne, np.float32), ctx.empty(ne, np.float32)
        ctx._ck(ctx.lib.gcnx_rgcn_operator(ctx.h, self.rowptr.ptr, _p(e), e.ld, edge_dim, L.RGCN_RULES[rule], r, perm.ptr, self.n, self.nnz,
                                           rel.ptr, val.ptr, rel_t.ptr, val_t.ptr))
        return rel, val, rel_t, val_t

    def transpose(self):
        if self.symmetric:
            return self
        if self._t is None:
            ctx = self.ctx
            rp = ctx.empty(self.n + 1, np.int32)
            ci = ctx.empty(max(self.nnz, 1), np.int32)
            v = ctx.empty(max(self.nnz, 1), np.float32) if self.vals is not None else None
            ctx._ck(ctx.lib.gcnx_csr_transpose(ctx.h, self.rowptr.ptr, self.colidx.ptr,
                                               self.vals.ptr if self.vals is not None else None, self.n, self.nnz,
                                               rp.ptr, ci.ptr, v.ptr if v is not None else None))
            self._t = DeviceCSR(ctx, self.n, self.nnz, rp, ci, v, self.block_ptr, self.n_blocks, False, self.max_block_rows)
        return self._t

    def transpose_perm(self):
        """(rowptr_t, colidx_t, perm_t) of the transposed pattern, perm_t[p] = entry of THIS CSR that became entry p of the
        transpose (gcnx_csr_transpose_perm): the destination-side view ECCConv's forward gathers by, with the row of the
        per-entry features that belongs to every entry.  Built once per operator, also for a symmetric one (the two
        directions of an edge are different entries with rows of their own)."""
        if getattr(self, "_tperm", None) is None:
            ctx = self.ctx
            rp, ci, pm = ctx.empty(self.n + 1, np.int32), ctx.empty(max(self.nnz, 1), np.int32), ctx.empty(max(self.nnz, 1), np.int32)
            ctx._ck(ctx.lib.gcnx_csr_transpose_perm(ctx.h, self.rowptr.ptr, self.colidx.ptr, self.n, self.nnz, rp.ptr, ci.ptr, pm.ptr))
            self._tperm = (rp, ci, pm)
        return self._tperm

    def row_mean(self):
        """Same structure with 1 / (entries of the row) on every entry: GeneralConv(aggregate="mean") -- the mean over a row's
        messages (tf.math.unsorted_segment_mean); a row without entries aggregates to 0.  Built once per operator."""
        if getattr(self, "_row_mean", None) is None:
            deg = np.diff(self.rowptr.numpy()).astype(np.int64)
            vals = np.repeat(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0).astype(np.float32), deg)
            self._row_mean = DeviceCSR(self.ctx, self.n, self.nnz, self.rowptr, self.colidx, self.ctx.to_device(vals), self.block_ptr,
                                       self.n_blocks, False, self.max_block_rows)
        return self._row_mean

    def unweighted(self):
        """Same structure, values ignored (GeneralConv aggregation).  One view per operator (as row_mean): the models ask
        for it inside their step sequence, and a view keeps its transposed CSR and its plan binding."""
        if self.vals is None:
            return self
        if getattr(self, "_unweighted", None) is None:
            self._unweighted = DeviceCSR(self.ctx, self.n, self.nnz, self.rowptr, self.colidx, None, self.block_ptr, self.n_blocks,
                                         self.symmetric, self.max_block_rows)
        if getattr(self._unweighted, "_tperm", None) is None:
            # the same pattern: the view takes the transposed pattern this operator already has (a device loader's batch
            # arrives with it: gcnx_collate_edges), instead of sorting for one of its own
            self._unweighted._tperm = getattr(self, "_tperm", None)
        return self._unweighted


def _max_block(graph_ptr):
    gp = np.asarray(graph_ptr) if graph_ptr is not None else None
    return int(np.diff(gp).max()) if gp is not None and gp.size > 1 else 0


class _Plan:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        self.bound = set()          # (rowptr pointer, n) pairs whose row order the plan holds

    def __del__(self):
        try:
            if self.h and self.ctx._live:
                self.ctx.lib.gcnx_spmm_plan_destroy(self.ctx.h, self.h)
        except Exception:
            pass


class Segments:
    """Graph membership of the rows of a disjoint batch: graph_ptr int32[B+1] on the device
    (the sorted id vector ``i`` of DisjointLoader, run-length encoded)."""

    def __init__(self, ctx, graph_ptr_host):
        gp = np.asarray(graph_ptr_host, dtype=np.int32)
        self.ctx, self.n_graphs, self.n = ctx, len(gp) - 1, int(gp[-1])
        self.host = gp
        self.dev = ctx.to_device(gp, np.int32)

    @classmethod
    def from_device(cls, ctx, dev, graph_ptr_host):
        """graph_ptr already on the device (device-side collate); the host copy is kept for shapes."""
        self = cls.__new__(cls)
        gp = np.asarray(graph_ptr_host, dtype=np.int32)
        self.ctx, self.n_graphs, self.n, self.host, self.dev = ctx, len(gp) - 1, int(gp[-1]), gp, dev
        return self

    @property
    def has_empty(self):
        """True if some graph of the batch has no nodes (never out of DisjointLoader; possible through the raw surface)."""
        if getattr(self, "_has_empty", None) is None:
            self._has_empty = bool(self.n_graphs) and bool(np.any(np.diff(self.host) <= 0))
        return self._has_empty

    @property
    def ids(self):
        """The DisjointLoader id vector i[N] (graph of every row) on the device, built on first use."""
        if getattr(self, "_ids", None) is None:
            self._ids = self.ctx.to_device(np.repeat(np.arange(self.n_graphs, dtype=np.int32), np.diff(self.host)), np.int32)
        return self._ids

    @classmethod
    def from_ids(cls, ctx, i, n_graphs=None):
        i = np.asarray(i)
        b = int(i.max()) + 1 if n_graphs is None and i.size else (n_graphs or 0)
        if i.size and np.any(np.diff(i) < 0):
            raise ValueError("segment ids must be sorted (DisjointLoader order)")
        gp = np.zeros(b + 1, dtype=np.int64)
        np.cumsum(np.bincount(i, minlength=b), out=gp[1:])
        return cls(ctx, gp)


# ------------------------------------------------------------------------------------------- #
# ops: one function per C entry point, operating on DeviceArrays
# ------------------------------------------------------------------------------------------- #

def _p(a):
    """Device pointer of an fp32 operand (or None).  A float64 upload would be silently
    reinterpreted by the kernels, so the dtype is checked here, at the boundary."""
    if a is None:
        return None
    if a.dtype != np.float32 and a.dtype != np.int32:
        raise TypeError(f"libgcnx operands are float32/int32, got {a.dtype}")
    return a.ptr


def gemm(ctx, x, w, bias, out, act=None, prec="f32", alpha=None):
    n, fi = x.shape
    fo = w.shape[1]
    assert w.shape[0] == fi and out.shape == (n, fo)
    ctx._ck(ctx.lib.gcnx_gemm(ctx.h, _p(x), x.ld, _p(w), _p(bias), _p(out), out.ld, n, fi, fo, L.PRECS[prec],
                              L.ACTS[act], _p(alpha)))
    return out


def gemm_relu_bits(ctx, x, w, bias, out, bits, prec="bf16"):
    """out = relu(x w + bias) and the bit image of [out > 0] for gemm_dx(mask_bits=...) (gcnx_gemm_relu_bits).  Returns
    False -- nothing launched -- when the streaming bf16 kernel does not serve the shape: call gemm(act="relu") then."""
    n, fi = x.shape
    fo = w.shape[1]
    assert w.shape[0] == fi and out.shape == (n, fo) and bits.nbytes >= n * 64
    rc = ctx.lib.gcnx_gemm_relu_bits(ctx.h, _p(x), x.ld, _p(w), _p(bias), _p(out), out.ld, n, fi, fo, L.PRECS[prec], bits.ptr)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


# ---- bf16 STORAGE between bf16-operand weight GEMMs (include/gcnx.h: "bf16 STORAGE ...").  Arrays of dtype uint16 hold
# bfloat16 bit patterns.  Each wrapper returns False -- nothing launched -- when the library answers GCNX_ERR_UNSUPPORTED.
def _is16(a):
    return a.dtype == np.uint16


def spmm_bf16out(ctx, a, h, bias, out16, act=None):
    """out16 = bf16(act(A h + bias)) (gcnx_spmm_csr_bf16out): the aggregation with its result stored as bfloat16."""
    n, f = h.shape
    assert a.n == n and out16.shape == (n, f) and _is16(out16)
    rc = ctx.lib.gcnx_spmm_csr_bf16out(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(h), h.ld, _p(bias), out16.ptr, out16.ld,
                                       n, f, L.ACTS[act], a.plan)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def spmm_pool_bwd_bf16out(ctx, at, y, seg, dpooled, out16, mode="sum", y_bits=None):
    """out16 = bf16(A^T (pool'(dpooled) * [y > 0])) from the bit image of y (gcnx_spmm_csr_pool_bwd_bf16out)."""
    n, f = y.shape
    assert at.n == n and out16.shape == (n, f) and _is16(out16) and dpooled.shape == (seg.n_graphs, f)
    if y_bits is None or at.n_blocks != seg.n_graphs:
        return False
    rc = ctx.lib.gcnx_spmm_csr_pool_bwd_bf16out(ctx.h, at.rowptr.ptr, at.colidx.ptr, _p(at.vals), _p(y), y.ld, seg.dev.ptr,
                                                seg.n_graphs, _p(dpooled), dpooled.ld, out16.ptr, out16.ld, n, f, L.POOLS[mode],
                                                at.plan, _p(y_bits))
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def stream_images(ctx, jobs, storage):
    """The bf16 images of up to four 256 x 256 weight operands in one launch (gcnx_gemm_stream_images).  jobs: (w, transpose)
    pairs -- transpose = True: the operand of gemm_fwd_bf16 (x w), False: of gemm_dx_bf16 (dh w^T); storage: a uint16 array
    of at least len(jobs) * 65536 elements.  Returns the device pointers, to be passed as ``wimg``."""
    assert storage.dtype == np.uint16 and storage.size >= len(jobs) * (L.STREAM_IMAGE_BYTES // 2) and len(jobs) <= 4
    arr = (L.StreamImageJob * len(jobs))()
    ptrs = []
    for i, (w, tr) in enumerate(jobs):
        assert w.shape == (256, 256) and w.contiguous
        ptrs.append(storage.ptr + i * L.STREAM_IMAGE_BYTES)
        arr[i] = L.StreamImageJob(w.ptr, 256, 256, 1 if tr else 0, ptrs[-1])
    ctx._ck(ctx.lib.gcnx_gemm_stream_images(ctx.h, len(jobs), C.cast(arr, C.c_void_p)))
    return ptrs


def gemm_fwd_bf16(ctx, x16, w, bias, out, act=None, bits=None, wimg=None):
    """out = act(x16 w + bias) with x16 stored as bfloat16; out is stored as bfloat16 when it is a uint16 array
    (gcnx_gemm_fwd_bf16); bits (optional, act = "relu"): the bit image of [out > 0] for gemm_dx_bf16."""
    n, fi = x16.shape
    fo = w.shape[1]
    assert _is16(x16) and w.shape[0] == fi and out.shape == (n, fo) and (bits is None or bits.nbytes >= n * 64)
    rc = ctx.lib.gcnx_gemm_fwd_bf16(ctx.h, x16.ptr, x16.ld, _p(w), _p(bias), out.ptr, out.ld, int(_is16(out)), n, fi, fo, L.ACTS[act],
                                    _p(bits), wimg)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def gemm_dx_bf16(ctx, dh16, w, dx, mask_bits=None, db=None, wimg=None):
    """dx = dh16 w^T (* the ReLU mask in mask_bits), db = column sums of dx; dh16 stored as bfloat16, dx as bfloat16 when it
    is a uint16 array (gcnx_gemm_dx_bf16)."""
    n, fo = dh16.shape
    fi = w.shape[0]
    assert _is16(dh16) and w.shape[1] == fo and dx.shape == (n, fi)
    rc = ctx.lib.gcnx_gemm_dx_bf16(ctx.h, dh16.ptr, dh16.ld, _p(w), dx.ptr, dx.ld, int(_is16(dx)), n, fi, fo, _p(mask_bits), _p(db), wimg)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def gemm_dw_bf16(ctx, x16, dh16, dw):
    """dw = x16^T dh16, both stored as bfloat16 (gcnx_gemm_dw_bf16)."""
    n, fi = x16.shape
    fo = dh16.shape[1]
    assert _is16(x16) and _is16(dh16) and dh16.shape[0] == n and dw.shape == (fi, fo)
    rc = ctx.lib.gcnx_gemm_dw_bf16(ctx.h, x16.ptr, x16.ld, dh16.ptr, dh16.ld, _p(dw), n, fi, fo)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def spmm(ctx, a, h, bias, out, act=None):
    n, f = h.shape
    assert a.n == n and out.shape == (n, f)
    ctx._ck(ctx.lib.gcnx_spmm_csr(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(h), h.ld, _p(bias), _p(out),
                                  out.ld, n, f, L.ACTS[act], a.plan))
    return out


def ecc_expand(ctx, a, u, x, scat, root=False, identity_perm=False):
    """scat[:, :C*F] = the edge-conditioned aggregation of x over the stored entries of ``a`` (messages from an entry's row to
    its column; u [nnz, S'] = the entry's channels, None = no channel but the constant one), C = S' + 1; root: x copied
    into the next F columns (gcnx_ecc_expand).  identity_perm: ``a`` IS the destination-side CSR and u is in its order."""
    n, f = x.shape
    sp = u.shape[1] if u is not None else 0
    assert a.n == n and scat.shape[0] == n and scat.shape[1] >= (sp + 1 + bool(root)) * f and (u is None or u.shape[0] == a.nnz)
    rp, ci, pm = (a.rowptr, a.colidx, None) if identity_perm else a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_ecc_expand(ctx.h, rp.ptr, ci.ptr, pm.ptr if pm is not None else None, _p(u), u.ld if u is not None else 0, sp,
                                    _p(x), x.ld, f, _p(scat), scat.ld, n, a.nnz, 1 if root else 0))
    return scat


def ecc_bwd(ctx, a, u, x, dscat, dx_root=None, dx=None, du=None):
    """dx = dx_root + the gradient of ecc_expand wrt x, du = its gradient wrt u, in one launch (gcnx_ecc_bwd); either may be
    None.  dscat: [N, C*F] (a column view of the GEMM's dX is fine)."""
    n, f = a.n, (x.shape[1] if x is not None else dx.shape[1])
    sp = u.shape[1] if u is not None else 0
    assert dscat.shape == (n, (sp + 1) * f) and (du is None or du.shape == (a.nnz, sp))
    ctx._ck(ctx.lib.gcnx_ecc_bwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(u), u.ld if u is not None else 0, sp, _p(x),
                                 x.ld if x is not None else 0, _p(dscat), dscat.ld, _p(dx_root), dx_root.ld if dx_root is not None else 0,
                                 f, _p(dx), dx.ld if dx is not None else 0, _p(du), du.ld if du is not None else 0, n, a.nnz))
    return dx, du


def segment_pool(ctx, seg, x, pooled, mode="sum", argmax=None):
    ctx._ck(ctx.lib.gcnx_segment_pool(ctx.h, seg.dev.ptr, _p(x), x.ld, _p(pooled), seg.n_graphs, x.shape[1],
                                      L.POOLS[mode], _p(argmax)))
    return pooled


def segment_pool_bwd(ctx, seg, dpooled, dx, mode="sum", argmax=None, y=None, db=None):
    n, f = dx.shape
    ctx._ck(ctx.lib.gcnx_segment_pool_bwd(ctx.h, seg.dev.ptr, _p(dpooled), _p(dx), dx.ld, n, seg.n_graphs, f,
                                          L.POOLS[mode], _p(argmax), _p(y), y.ld if y is not None else 0, _p(db)))
    return dx


def attn_pool_scratch_floats(ctx, n, b, f, slice_rows=0):
    """Floats of scratch that serve attn_pool with this slice_rows and attn_pool_bwd (gcnx_attn_pool_scratch_floats)."""
    return int(ctx.lib.gcnx_attn_pool_scratch_floats(int(n), int(b), int(f), int(slice_rows)))


def attn_pool(ctx, seg, x, a, pooled, alpha=None, scratch=None, slice_rows=0):
    """pooled[g] = sum_i alpha_i x_i, alpha = softmax over the rows of graph g of <x_i, a> (gcnx_attn_pool).  a: [f] or [f, 1];
    alpha [n] is stored if given.  slice_rows = 0: the library's route (one workgroup per graph without scratch); > 0: graphs
    cut into slices of that many rows (needs scratch)."""
    n, f = x.shape
    b = seg.n_graphs
    assert seg.n == n and a.size == f and a.contiguous and pooled.shape == (b, f)
    assert alpha is None or (alpha.size == n and alpha.contiguous)
    assert scratch is None or scratch.size >= attn_pool_scratch_floats(ctx, n, b, f, slice_rows)
    ctx._ck(ctx.lib.gcnx_attn_pool(ctx.h, seg.dev.ptr, _p(x), x.ld, _p(a), n, b, f, int(slice_rows), _p(pooled), pooled.ld,
                                   _p(alpha), _p(scratch)))
    return pooled


def attn_pool_bwd(ctx, seg, x, a, alpha, pooled, dpooled, dx=None, da=None, scratch=None):
    """dx [n, f] (written, not accumulated) and da (the shape of a) from alpha and pooled as attn_pool wrote them
    (gcnx_attn_pool_bwd); either may be None.  scratch: attn_pool_scratch_floats floats, needed for da."""
    n, f = x.shape
    b = seg.n_graphs
    assert seg.n == n and a.size == f and a.contiguous and alpha.size == n and alpha.contiguous
    assert pooled.shape == dpooled.shape == (b, f) and (dx is None or dx.shape == (n, f))
    assert da is None or (da.size == f and da.contiguous and scratch is not None)
    assert scratch is None or scratch.size >= attn_pool_scratch_floats(ctx, n, b, f)
    ctx._ck(ctx.lib.gcnx_attn_pool_bwd(ctx.h, seg.dev.ptr, _p(x), x.ld, _p(a), _p(alpha), _p(pooled), pooled.ld, _p(dpooled),
                                       dpooled.ld, n, b, f, _p(dx), dx.ld if dx is not None else 0, _p(da), _p(scratch)))
    return dx, da


def pool_dense_softmax_cce(ctx, seg, x, pooled, w, bias, y, probs, loss_acc=None, denom=None, dw=None, db=None,
                           dpooled=None, mode="sum", argmax=None, db_relu=None, cce="logits"):
    """segment_pool + dense_softmax_cce as one call (gcnx_pool_dense_softmax_cce): ``pooled`` is written as well;
    ``db_relu`` = column sums of pool'(dpooled) * [x > 0] (the bias gradient of the ReLU layer that produced x)."""
    b, h = pooled.shape
    c = w.shape[1]
    assert x.shape[1] == h and seg.n_graphs == b
    ctx._ck(ctx.lib.gcnx_pool_dense_softmax_cce(ctx.h, seg.dev.ptr, _p(x), x.ld, L.POOLS[mode], _p(argmax), _p(pooled),
                                                pooled.ld, _p(w), _p(bias), _p(y), b, h, c,
                                                float(denom if denom else max(b, 1)), _p(probs), _p(loss_acc), _p(dw),
                                                _p(db), _p(dpooled), dpooled.ld if dpooled is not None else 0,
                                                _p(db_relu), L.CCES[cce]))
    return probs


def pooled_dense_softmax_cce(ctx, seg, pooled, cnt, w, bias, y, probs, loss_acc=None, denom=None, dw=None, db=None, dpooled=None,
                             mode="sum", db_relu=None, cce="logits"):
    """dense_softmax_cce on pooled rows that are already there (spmm_relu_bits_pool), + db_relu from the positive counts
    (gcnx_pooled_dense_softmax_cce)."""
    b, h = pooled.shape
    c = w.shape[1]
    assert seg.n_graphs == b and (cnt is None or cnt.shape == (b, h))
    ctx._ck(ctx.lib.gcnx_pooled_dense_softmax_cce(ctx.h, seg.dev.ptr, L.POOLS[mode], _p(pooled), pooled.ld, _p(cnt), _p(w), _p(bias), _p(y),
                                                  b, h, c, float(denom if denom else max(b, 1)), _p(probs), _p(loss_acc), _p(dw), _p(db),
                                                  _p(dpooled), dpooled.ld if dpooled is not None else 0, _p(db_relu), L.CCES[cce]))
    return probs


def spmm_relu_bits(ctx, a, h, bias, out, bits):
    """out = relu(A h + bias) on the tile kernels, which also write the bit image of [out > 0] (int32 [(f / 32) * n]) that
    spmm_pool_bwd(y_bits=...) folds from.  Returns False -- nothing launched -- if the tile kernels do not serve this
    batch (gcnx_spmm_csr_relu_bits: GCNX_ERR_UNSUPPORTED); the caller then takes spmm()."""
    n, f = h.shape
    assert a.n == n and out.shape == (n, f) and bits.size >= (f // 32) * n
    rc = ctx.lib.gcnx_spmm_csr_relu_bits(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(h), h.ld, _p(bias), _p(out), out.ld,
                                         n, f, a.plan, _p(bits))
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def spmm_pool_bwd(ctx, at, y, seg, dpooled, out, mode="sum", y_bits=None):
    """out = A^T (pool'(dpooled) * [y > 0]) in one gather (gcnx_spmm_csr_pool_bwd); ``at`` is the transposed operator."""
    n, f = y.shape
    assert at.n == n and out.shape == (n, f) and dpooled.shape == (seg.n_graphs, f)
    ctx._ck(ctx.lib.gcnx_spmm_csr_pool_bwd(ctx.h, at.rowptr.ptr, at.colidx.ptr, _p(at.vals), _p(y), y.ld, seg.dev.ptr,
                                           seg.n_graphs, _p(dpooled), dpooled.ld, _p(out), out.ld, n, f, L.POOLS[mode],
                                           at.plan if at.n_blocks == seg.n_graphs else None, _p(y_bits)))
    return out


def spmm_relu_bits_pool(ctx, a, h, bias, out, bits, seg, pooled, cnt, mode="sum"):
    """The pooled GCNConv's forward of a training step without its output (gcnx_spmm_csr_relu_bits_pool): the bit image of
    relu(A h + b), the graphs' pooled rows and positive counts; rows of ``out`` are written for graphs taller than a tile only.
    False -- nothing launched -- when the tile kernels do not serve the batch."""
    n, f = h.shape
    assert a.n == n and out.shape == (n, f) and pooled.shape == (seg.n_graphs, f) and cnt.shape == (seg.n_graphs, f)
    if a.plan is None or a.n_blocks != seg.n_graphs:
        return False
    rc = ctx.lib.gcnx_spmm_csr_relu_bits_pool(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(h), h.ld, _p(bias), _p(out), out.ld, n, f,
                                              a.plan, bits.ptr, seg.dev.ptr, seg.n_graphs, L.POOLS[mode], _p(pooled), pooled.ld, _p(cnt))
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def gcn_conv_fused_ok(ctx, n, fi, fo, ldx=None):
    """True if gcn_conv_fwd / gcn_conv_bwd_pool serve these shapes (gcnx_gcn_conv_fused_ok)."""
    return bool(ctx.lib.gcnx_gcn_conv_fused_ok(int(n), int(fi), int(fo), int(ldx if ldx is not None else fi)))


def gcn_conv_fwd(ctx, a, x, w, bias, out, act="relu", s=None, wt=None, prec="f32", pool=None, mask8=None):
    """out = act((A x) w + bias) in one launch; s (optional) receives A x, wt (optional, [fo, fi]) w^T
    (gcnx_gcn_conv_fwd).  pool = (seg, tile_part, tile_cnt): the launch also leaves the global pool's per-tile partial
    sums / positive counts of ``out`` in the two [pool_tile_rows(n, b), fo] arrays (gcnx_gcn_conv_fwd_pool).
    mask8 ([n, fo] uint8, act "relu"): also receives [out > 0] as bytes; ``out`` may then be None -- the fp32 activation is
    not stored (gcnx_gcn_conv_fwd_mask8)."""
    n, fi = x.shape
    fo = w.shape[1]
    assert a.n == n and w.shape[0] == fi and w.contiguous and (s is None or s.shape == (n, fi))
    assert (out is None and mask8 is not None) or out.shape == (n, fo)
    if mask8 is not None:
        assert mask8.dtype == np.uint8 and mask8.shape == (n, fo)
        seg, tp, tc = pool if pool is not None else (None, None, None)
        assert pool is None or (tp.shape == tc.shape == (pool_tile_rows(n, seg.n_graphs), fo) and tp.contiguous and tc.contiguous)
        ctx._ck(ctx.lib.gcnx_gcn_conv_fwd_mask8(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(x), x.ld, n, fi, _p(w), fo, _p(bias),
                                                L.ACTS[act], _p(s), s.ld if s is not None else 0, _p(out),
                                                out.ld if out is not None else 0, _p(wt), L.PRECS[prec],
                                                seg.ids.ptr if seg is not None else None, seg.n_graphs if seg is not None else 0,
                                                _p(tp), _p(tc), mask8.ptr, mask8.ld))
        return out
    if pool is None:
        ctx._ck(ctx.lib.gcnx_gcn_conv_fwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(x), x.ld, n, fi, _p(w), fo, _p(bias),
                                          L.ACTS[act], _p(s), s.ld if s is not None else 0, _p(out), out.ld, _p(wt), L.PRECS[prec]))
        return out
    seg, tp, tc = pool
    assert tp.shape == tc.shape == (pool_tile_rows(n, seg.n_graphs), fo) and tp.contiguous and tc.contiguous
    ctx._ck(ctx.lib.gcnx_gcn_conv_fwd_pool(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(x), x.ld, n, fi, _p(w), fo, _p(bias),
                                           L.ACTS[act], _p(s), s.ld if s is not None else 0, _p(out), out.ld, _p(wt), L.PRECS[prec],
                                           seg.ids.ptr, seg.n_graphs, _p(tp), _p(tc)))
    return out


def gcn_conv_fwd_pre(ctx, s, w, bias, out, act="relu", prec="f32"):
    """out = act(s w + bias) in one launch, s = A x as gcn_conv_fwd(..., s=s) wrote it (gcnx_gcn_conv_fwd_pre): the product and
    epilogue of that launch without its gather, bit for bit the same ``out``."""
    n, fi = s.shape
    fo = w.shape[1]
    assert w.shape[0] == fi and w.contiguous and out.shape == (n, fo)
    ctx._ck(ctx.lib.gcnx_gcn_conv_fwd_pre(ctx.h, _p(s), s.ld, n, fi, _p(w), fo, _p(bias), L.ACTS[act], _p(out), out.ld,
                                          L.PRECS[prec]))
    return out


def sage_conv_ok(ctx, n, fi, fo, ldx=None):
    """True if sage_conv serves these shapes (gcnx_sage_conv_ok)."""
    return bool(ctx.lib.gcnx_sage_conv_ok(int(n), int(fi), int(fo), int(ldx if ldx is not None else fi)))


def sage_conv(ctx, a, x, w_nb, w_root, bias, out, s=None, w_transposed=False):
    """out = (A x) w_nb + x w_root + bias in one launch; s (optional) receives A x (gcnx_sage_conv).  w_transposed: both
    weights are [fo, fi] -- the backward form dX = (A^T dZ) W_nb^T + dZ W_root^T with the layer's weights as stored."""
    n, fi = x.shape
    fo = w_nb.shape[0] if w_transposed else w_nb.shape[1]
    assert a.n == n and w_nb.shape == w_root.shape == ((fo, fi) if w_transposed else (fi, fo)) and w_nb.contiguous and w_root.contiguous
    assert out.shape == (n, fo) and (s is None or s.shape == (n, fi)) and (bias is None or bias.shape == (fo,))
    ctx._ck(ctx.lib.gcnx_sage_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), _p(x), x.ld, n, fi, _p(w_nb), _p(w_root), fo,
                                   1 if w_transposed else 0, _p(bias), _p(s), s.ld if s is not None else 0, _p(out), out.ld))
    return out


def appnp_resident_ok(ctx, max_graph_rows, f, ldx=None):
    """True if the one-launch route of appnp_propagate serves a batch whose tallest graph has this many rows
    (gcnx_appnp_resident_ok)."""
    return bool(ctx.lib.gcnx_appnp_resident_ok(int(max_graph_rows), int(f), int(ldx if ldx is not None else f)))


def appnp_scratch_floats(ctx, n, f):
    """Floats of ``scratch`` for the streamed route of appnp_propagate with k >= 2 (gcnx_appnp_scratch_floats)."""
    return int(ctx.lib.gcnx_appnp_scratch_floats(int(n), int(f)))


def appnp_propagate(ctx, a, x, out, k, alpha, scratch=None, col_block=0):
    """out = z^k, z^0 = x, z^{j+1} = (1 - alpha) A z^j + alpha x (gcnx_appnp_propagate).  The graphs of ``a`` (block_ptr, n_blocks,
    max_block_rows) let the library keep each graph's rows in LDS across all k hops; without them, or with col_block=-1, k
    launches alternate between out and scratch (appnp_scratch_floats).  col_block > 0 forces the one-launch route with that
    many columns per workgroup.  The backward is the same call on ``a.transpose()`` with x = dz."""
    n, f = x.shape
    assert a.n == n and out.shape == (n, f) and (scratch is None or scratch.size >= appnp_scratch_floats(ctx, n, f))
    has_blocks = a.block_ptr is not None and a.n_blocks > 0
    ctx._ck(ctx.lib.gcnx_appnp_propagate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), a.block_ptr.ptr if has_blocks else None,
                                         a.n_blocks if has_blocks else 0, a.max_block_rows if has_blocks else 0, _p(x), x.ld, n, f,
                                         int(k), float(alpha), int(col_block), _p(out), out.ld, _p(scratch)))
    return out


def cheb_resident_ok(ctx, max_graph_rows, f, ld=None):
    """True if the one-launch route of cheb_basis / cheb_sum serves a batch whose tallest graph has this many rows
    (gcnx_cheb_resident_ok); ld: the leading dimension of the call's input."""
    return bool(ctx.lib.gcnx_cheb_resident_ok(int(max_graph_rows), int(f), int(ld if ld is not None else f)))


def cheb_scratch_floats(ctx, n, f):
    """Floats of ``scratch`` for the streamed route of cheb_sum with k >= 3 (gcnx_cheb_scratch_floats)."""
    return int(ctx.lib.gcnx_cheb_scratch_floats(int(n), int(f)))


def _cheb_graphs(a):
    has_blocks = a.block_ptr is not None and a.n_blocks > 0
    return (a.block_ptr.ptr if has_blocks else None, a.n_blocks if has_blocks else 0, a.max_block_rows if has_blocks else 0)


def cheb_basis(ctx, a, x, out, k, lambda_max=2.0, scratch=None, col_block=0):
    """Block j of out [n, k f] = T_j(L^) x, j = 0 .. k-1, on the operator ``a`` = S (DeviceCSR.cheb_norm) (gcnx_cheb_basis): the
    backward of cheb_sum on ``a.transpose()`` with x = dz.  The graphs of ``a`` let the library keep each graph's rows in LDS
    across all k - 1 gathers; without them, or with col_block=-1, one launch per gather.  col_block > 0 forces the one-launch
    route with that many columns per workgroup."""
    n, f = x.shape
    assert a.n == n and out.shape == (n, k * f)
    ctx._ck(ctx.lib.gcnx_cheb_basis(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), *_cheb_graphs(a), _p(x), x.ld, n, f, int(k),
                                    float(lambda_max), int(col_block), _p(out), out.ld, _p(scratch)))
    return out


def cheb_sum(ctx, a, h, bias, out, k, lambda_max=2.0, scratch=None, col_block=0):
    """out [n, f] = sum_j T_j(L^) H_j + bias by Clenshaw summation, H_j = block j of h [n, k f] (gcnx_cheb_sum).  scratch
    (cheb_scratch_floats) is what the streamed route with k >= 3 alternates with out; routes and col_block as cheb_basis."""
    n, f = out.shape
    assert a.n == n and h.shape == (n, k * f) and (bias is None or bias.shape == (f,))
    assert scratch is None or scratch.size >= cheb_scratch_floats(ctx, n, f)
    ctx._ck(ctx.lib.gcnx_cheb_sum(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), *_cheb_graphs(a), _p(h), h.ld, _p(bias), n, f, int(k),
                                  float(lambda_max), int(col_block), _p(out), out.ld, _p(scratch)))
    return out


def rgcn_conv_ok(ctx, n, fi, fo, num_relations, ldx=None):
    """True if rgcn_conv serves these shapes (gcnx_rgcn_conv_ok)."""
    return bool(ctx.lib.gcnx_rgcn_conv_ok(int(n), int(fi), int(fo), int(num_relations), int(ldx if ldx is not None else fi)))


def rgcn_conv(ctx, rowptr, colidx, rel, val, x, w, bias, out, num_relations, root_weight=True, m=None, w_transposed=False):
    """out = [A_0 x | .. | A_{R-1} x | x] w + bias in one launch (gcnx_rgcn_conv); A_r: the entries of relation ``rel`` == r with
    their ``val`` (DeviceCSR.rgcn_operator).  w: the row-stacked [W_0; ..; W_{R-1}; W_root] ([(R + 1) fi, fo]; R blocks without
    root_weight).  m (optional) receives the panel [A_0 x | .. | A_{R-1} x].  w_transposed: every block is [fo, fi] -- the
    backward form dX = dZ W_root^T + sum_r A_r^T (dZ W_r^T) on the transposed pattern with rel_t / val_t and the layer's
    weights as stored."""
    n, fi = x.shape
    r = int(num_relations)
    nb = r + (1 if root_weight else 0)
    fo = out.shape[1]
    assert w.size == nb * fi * fo and w.contiguous and out.shape == (n, fo) and (bias is None or bias.shape == (fo,))
    assert m is None or m.shape == (n, r * fi)
    ctx._ck(ctx.lib.gcnx_rgcn_conv(ctx.h, rowptr.ptr, colidx.ptr, rel.ptr, val.ptr, _p(x), x.ld, n, fi, _p(w), 1 if root_weight else 0,
                                   fo, r, 1 if w_transposed else 0, _p(bias), _p(m), m.ld if m is not None else 0, _p(out), out.ld))
    return out


def rgcn_aggregate(ctx, rowptr, colidx, rel, val, x, m, num_relations):
    """m [n, R f] = [A_0 x | .. | A_{R-1} x] for any width, stride and alignment (gcnx_rgcn_aggregate), with the bits of
    rgcn_conv's panel.  m must not alias x."""
    n, f = x.shape
    assert m.shape == (n, int(num_relations) * f)
    ctx._ck(ctx.lib.gcnx_rgcn_aggregate(ctx.h, rowptr.ptr, colidx.ptr, rel.ptr, val.ptr, _p(x), x.ld, n, f, int(num_relations), _p(m),
                                        m.ld))
    return m


def gin_conv_ok(ctx, n, k0, k1, k2=0, ldx=None):
    """True if gin_conv serves these shapes (gcnx_gin_conv_ok); k2 = 0: the single-stage form."""
    return bool(ctx.lib.gcnx_gin_conv_ok(int(n), int(k0), int(k1), int(k2), int(ldx if ldx is not None else k0)))


def gin_conv(ctx, a, x, eps, w_a, b_a, w_b, b_b, out, t=None, u=None, w_transposed=False):
    """out = relu(T w_a + b_a) w_b + b_b with T = (1 + eps) x + A x in one launch (gcnx_gin_conv); A = the stored pattern of
    ``a``, its values are not read.  eps: a device array of one float, or None (0).  t / u (optional) receive T and
    relu(T w_a + b_a).  w_b None: the single-stage form out = T w_a (+ b_a), no ReLU (u and b_b must be None).
    w_transposed: the weights are [out, in] -- the backward form dX = ((1 + eps) dU + A^T dU) W_a^T with the layer's weight
    as stored."""
    n, k0 = x.shape
    k1 = w_a.shape[0] if w_transposed else w_a.shape[1]
    k2 = 0 if w_b is None else (w_b.shape[0] if w_transposed else w_b.shape[1])
    assert a.n == n and w_a.shape == ((k1, k0) if w_transposed else (k0, k1)) and w_a.contiguous
    assert w_b is None or (w_b.shape == ((k2, k1) if w_transposed else (k1, k2)) and w_b.contiguous)
    assert out.shape == (n, k2 or k1) and (t is None or t.shape == (n, k0)) and (u is None or u.shape == (n, k1))
    assert (b_a is None or b_a.shape == (k1,)) and (b_b is None or b_b.shape == (k2,)) and (eps is None or eps.size == 1)
    ctx._ck(ctx.lib.gcnx_gin_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, n, k0, _p(eps), _p(w_a), _p(b_a), k1, _p(w_b),
                                  _p(b_b), k2, 1 if w_transposed else 0, _p(t), t.ld if t is not None else 0, _p(u),
                                  u.ld if u is not None else 0, _p(out), out.ld))
    return out


def gin_aggregate(ctx, a, x, eps, out):
    """out = (1 + eps) x + A x for any width (gcnx_gin_aggregate); A = the stored pattern of ``a``; eps: a device array of one
    float, or None (0).  out must not alias x."""
    n, f = x.shape
    assert a.n == n and out.shape == (n, f) and (eps is None or eps.size == 1)
    ctx._ck(ctx.lib.gcnx_gin_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, _p(eps), _p(out), out.ld, n, f))
    return out


def gin_eps_grad_parts(n):
    """Floats of scratch gin_eps_grad needs for n rows (one partial sum per 64 rows)."""
    return max((int(n) + 63) // 64, 1)


def gin_eps_grad(ctx, x, dt, parts, deps):
    """deps[0] = sum_i <x_i, dt_i> in a fixed order (gcnx_gin_eps_grad); parts: gin_eps_grad_parts(n) floats of scratch."""
    n, f = x.shape
    assert dt.shape == (n, f) and parts.size >= gin_eps_grad_parts(n) and deps.size == 1
    ctx._ck(ctx.lib.gcnx_gin_eps_grad(ctx.h, _p(x), x.ld, _p(dt), dt.ld, n, f, _p(parts), _p(deps)))
    return deps


def gine_conv_ok(ctx, n, k0, k1, k2, ldx=None, edge_dim=1):
    """True if gine_conv serves these shapes (gcnx_gine_conv_ok; answers without a context: ctx only carries the library)."""
    return bool(ctx.lib.gcnx_gine_conv_ok(int(n), int(k0), int(k1), int(k2), int(ldx if ldx is not None else k0), int(edge_dim)))


def _gine_edge(a, e, w_e, b_e, f):
    """(e pointer, lde, edge_dim, w_e pointer, b_e pointer) of the edge operands: e [nnz, D] (any ld), w_e [D, f], b_e [f] or None."""
    d = e.shape[1]
    assert e.shape[0] == a.nnz and w_e.shape == (d, f) and w_e.contiguous and (b_e is None or b_e.shape == (f,))
    return _p(e), e.ld, d, _p(w_e), _p(b_e)


def gine_conv(ctx, a, x, eps, e, w_e, b_e, w_a, b_a, w_b, b_b, out, t=None, u=None):
    """out = relu(T w_a + b_a) w_b + b_b with T = (1 + eps) x + sum_j relu(x_j + e_ij w_e + b_e) in one launch (gcnx_gine_conv);
    the sum runs over the stored entries of ``a`` (row = target), its values are not read; e [nnz, D] in the entry order.  eps: a
    device array of one float, or None (0).  t / u (optional) receive T and relu(T w_a + b_a)."""
    n, k0 = x.shape
    k1, k2 = w_a.shape[1], w_b.shape[1]
    assert a.n == n and w_a.shape == (k0, k1) and w_a.contiguous and w_b.shape == (k1, k2) and w_b.contiguous
    assert out.shape == (n, k2) and (t is None or t.shape == (n, k0)) and (u is None or u.shape == (n, k1))
    assert (b_a is None or b_a.shape == (k1,)) and (b_b is None or b_b.shape == (k2,)) and (eps is None or eps.size == 1)
    ep, lde, d, wp, bp = _gine_edge(a, e, w_e, b_e, k0)
    ctx._ck(ctx.lib.gcnx_gine_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, n, k0, _p(eps), ep, lde, d, wp, bp, _p(w_a), _p(b_a),
                                   k1, _p(w_b), _p(b_b), k2, _p(t), t.ld if t is not None else 0, _p(u),
                                   u.ld if u is not None else 0, _p(out), out.ld))
    return out


def gine_aggregate(ctx, a, x, eps, e, w_e, b_e, out):
    """out = (1 + eps) x + sum_j relu(x_j + e_ij w_e + b_e) for any width (gcnx_gine_aggregate).  out must not alias x."""
    n, f = x.shape
    assert a.n == n and out.shape == (n, f) and (eps is None or eps.size == 1)
    ep, lde, d, wp, bp = _gine_edge(a, e, w_e, b_e, f)
    ctx._ck(ctx.lib.gcnx_gine_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, _p(eps), ep, lde, d, wp, bp, _p(out), out.ld, n, f))
    return out


def gine_bwd_scratch_floats(ctx, n, f, edge_dim):
    """Floats of scratch gine_bwd_edges needs (gcnx_gine_bwd_scratch_floats)."""
    return int(ctx.lib.gcnx_gine_bwd_scratch_floats(int(n), int(f), int(edge_dim)))


def gine_bwd_edges(ctx, a, x, e, w_e, b_e, dt, dw_e, db_e, scratch):
    """dw_e [D, f] and db_e [f] (None: not wanted) from dt = dT on the forward pattern of ``a`` (gcnx_gine_bwd_edges): written, not
    accumulated.  scratch: gine_bwd_scratch_floats floats."""
    n, f = x.shape
    ep, lde, d, wp, bp = _gine_edge(a, e, w_e, b_e, f)
    assert a.n == n and dt.shape == (n, f) and dw_e.shape == (d, f) and dw_e.contiguous and (db_e is None or db_e.shape == (f,))
    assert scratch.size >= gine_bwd_scratch_floats(ctx, n, f, d)
    ctx._ck(ctx.lib.gcnx_gine_bwd_edges(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, ep, lde, d, wp, bp, _p(dt), dt.ld, n, f, _p(dw_e),
                                        _p(db_e), _p(scratch)))
    return dw_e


def gine_bwd_nodes(ctx, a, x, eps, e, w_e, b_e, dt, dx):
    """dx = (1 + eps) dT + the masked dT of every target, on the transposed pattern of ``a`` with its entry permutation
    (a.transpose_perm(); gcnx_gine_bwd_nodes).  dx must not alias dt or x."""
    n, f = x.shape
    ep, lde, d, wp, bp = _gine_edge(a, e, w_e, b_e, f)
    assert a.n == n and dt.shape == dx.shape == (n, f) and (eps is None or eps.size == 1)
    rp, ci, pm = a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_gine_bwd_nodes(ctx.h, rp.ptr, ci.ptr, pm.ptr, _p(x), x.ld, _p(eps), ep, lde, d, wp, bp, _p(dt), dt.ld, _p(dx),
                                        dx.ld, n, f))
    return dx


def pna_aggregate(ctx, a, x, pq, avg_deg_log, c, stats=None):
    """c [n, 13f] = [x | A | s_amp A | s_att A], A = [mean | min | max | std] of the messages P_i + Q_j over the stored
    entries of every row of ``a`` (gcnx_pna_aggregate); pq [n, 2f] = P | Q.  stats [n, 6f] (optional) receives
    meanQ | minQ | maxQ | std | cmin | cmax for pna_bwd.  The values of ``a`` are not read."""
    n, f = x.shape
    assert a.n == n and pq.shape == (n, 2 * f) and c.shape == (n, 13 * f) and (stats is None or stats.shape == (n, 6 * f))
    ctx._ck(ctx.lib.gcnx_pna_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(x), x.ld, _p(pq), pq.ld, float(avg_deg_log), _p(c), c.ld,
                                       _p(stats), stats.ld if stats is not None else 0, n, f))
    return c


def pna_bwd_scratch_floats(ctx, n, f):
    """Floats of scratch pna_bwd needs for n rows of width f (gcnx_pna_bwd_scratch_floats)."""
    out = C.c_int64()
    ctx._ck(ctx.lib.gcnx_pna_bwd_scratch_floats(int(n), int(f), C.byref(out)))
    return int(out.value)


def pna_bwd(ctx, a, a_t, pq, stats, dc, avg_deg_log, dpq, scratch):
    """dpq [n, 2f] = dP | dQ from dc [n, 13f] (gcnx_pna_bwd); a_t = a.transpose(); pq and stats as pna_aggregate read and
    wrote them.  Block 0 of dc (the direct dX) is not touched.  scratch: pna_bwd_scratch_floats floats."""
    n, f = pq.shape[0], pq.shape[1] // 2
    assert a.n == n and a_t.n == n and pq.shape == (n, 2 * f) and stats.shape == (n, 6 * f) and dc.shape == (n, 13 * f)
    assert dpq.shape == (n, 2 * f) and scratch.contiguous and scratch.size >= 4 * n * f
    ctx._ck(ctx.lib.gcnx_pna_bwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, a_t.rowptr.ptr, a_t.colidx.ptr, _p(pq), pq.ld, _p(stats), stats.ld,
                                 _p(dc), dc.ld, float(avg_deg_log), _p(dpq), dpq.ld, _p(scratch), n, f))
    return dpq


def gat_conv_ok(ctx, n, heads, c, ldh=None):
    """True if the GATConv kernels serve these shapes (gcnx_gat_conv_ok)."""
    return bool(ctx.lib.gcnx_gat_conv_ok(int(n), int(heads), int(c), int(ldh if ldh is not None else heads * c)))


def gat_bwd_scratch_floats(ctx, n, heads, c):
    return int(ctx.lib.gcnx_gat_bwd_scratch_floats(int(n), int(heads), int(c)))


def gat_scores(ctx, hf, att_src, att_dst, a_src, a_dst):
    """a_src[j, h] = <hf[j, h, :], att_src[h, :]>, a_dst likewise (gcnx_gat_scores).  att_*: [heads, c]; a_*: [n, heads]."""
    n, (heads, c) = hf.shape[0], att_src.shape
    assert hf.shape[1] == heads * c and att_dst.shape == (heads, c) and a_src.shape == a_dst.shape == (n, heads)
    assert att_src.contiguous and att_dst.contiguous and a_src.contiguous and a_dst.contiguous
    ctx._ck(ctx.lib.gcnx_gat_scores(ctx.h, _p(hf), hf.ld, n, heads, c, _p(att_src), _p(att_dst), _p(a_src), _p(a_dst)))
    return a_src, a_dst


def gat_aggregate(ctx, a, hf, a_src, a_dst, bias, out, alpha=None, o_pre=None, slope=0.2):
    """out = softmax-weighted gather of hf over the stored entries of ``a`` (row = target) + bias; alpha [nnz, heads] and
    o_pre (the result before the bias) are stored if given (gcnx_gat_aggregate)."""
    n, heads = a_src.shape
    hc = hf.shape[1]
    assert a.n == n == hf.shape[0] and hc % heads == 0 and a_dst.shape == (n, heads) and out.shape == (n, hc)
    assert (alpha is None or (alpha.shape == (a.nnz, heads) and alpha.contiguous)) and (o_pre is None or o_pre.shape == (n, hc))
    assert (bias is None or bias.shape == (hc,)) and a_src.contiguous and a_dst.contiguous
    ctx._ck(ctx.lib.gcnx_gat_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(hf), hf.ld, n, heads, hc // heads, _p(a_src), _p(a_dst),
                                       _p(bias), float(slope), _p(out), out.ld, _p(alpha), _p(o_pre),
                                       o_pre.ld if o_pre is not None else 0))
    return out


def gat_bwd_edges(ctx, a, hf, a_src, a_dst, alpha, dout, o, dz, da_dst, o_bias=None, slope=0.2):
    """dz [nnz, heads] (the CSR's entry order) and da_dst [n, heads] from dout and O = o (- o_bias) (gcnx_gat_bwd_edges)."""
    n, heads = a_src.shape
    hc = hf.shape[1]
    assert a.n == n and dout.shape == o.shape == (n, hc) and alpha.shape == dz.shape == (a.nnz, heads) and da_dst.shape == (n, heads)
    assert alpha.contiguous and dz.contiguous and da_dst.contiguous and a_src.contiguous and a_dst.contiguous
    ctx._ck(ctx.lib.gcnx_gat_bwd_edges(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(hf), hf.ld, n, heads, hc // heads, _p(a_src), _p(a_dst),
                                       float(slope), _p(alpha), _p(dout), dout.ld, _p(o), o.ld, _p(o_bias), _p(dz), _p(da_dst)))
    return dz, da_dst


def gat_bwd_nodes(ctx, a, alpha, dz, dout, hf, da_dst, att_src, att_dst, dhf, da_src, datt_src, datt_dst, scratch):
    """dhf, da_src, datt_src, datt_dst on the transposed pattern of ``a`` with its entry permutation (a.transpose_perm();
    gcnx_gat_bwd_nodes).  scratch: gat_bwd_scratch_floats floats."""
    n, (heads, c) = a.n, att_src.shape
    assert dout.shape == hf.shape == dhf.shape == (n, heads * c) and alpha.shape == dz.shape == (a.nnz, heads)
    assert da_dst.shape == da_src.shape == (n, heads) and datt_src.shape == datt_dst.shape == att_dst.shape == (heads, c)
    assert scratch.size >= gat_bwd_scratch_floats(ctx, n, heads, c)
    assert all(t.contiguous for t in (alpha, dz, da_dst, da_src, att_src, att_dst, datt_src, datt_dst))
    rp, ci, pm = a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_gat_bwd_nodes(ctx.h, rp.ptr, ci.ptr, pm.ptr, n, heads, c, _p(alpha), _p(dz), _p(dout), dout.ld, _p(hf), hf.ld,
                                       _p(da_dst), _p(att_src), _p(att_dst), _p(dhf), dhf.ld, _p(da_src), _p(datt_src), _p(datt_dst),
                                       _p(scratch)))
    return dhf


def gatv2_conv_ok(ctx, n, heads, c, ldx=None, edge_dim=0):
    """True if the GATv2Conv kernels serve these shapes (gcnx_gatv2_conv_ok); ldx: the leading dimension of Xl | Xr."""
    return bool(ctx.lib.gcnx_gatv2_conv_ok(int(n), int(heads), int(c), int(ldx if ldx is not None else 2 * heads * c), int(edge_dim)))


def gatv2_bwd_scratch_floats(ctx, n, heads, c, edge_dim=0):
    return int(ctx.lib.gcnx_gatv2_bwd_scratch_floats(int(n), int(heads), int(c), int(edge_dim)))


def _edge_operands(a, e, w_e, width):
    """(e pointer, lde, edge_dim, w_e pointer) of the optional edge operands of GATv2Conv, ResGatedGraphConv and TransformerConv:
    e [nnz, D] (any ld), w_e [D, width]."""
    if e is None:
        assert w_e is None
        return None, 0, 0, None
    d = e.shape[1]
    assert e.shape[0] == a.nnz and w_e is not None and w_e.shape == (d, width) and w_e.contiguous
    return _p(e), e.ld, d, _p(w_e)


def gatv2_aggregate(ctx, a, xlr, att, bias, out, e=None, w_e=None, alpha=None, o_pre=None, slope=0.2):
    """out = softmax-weighted sum of Xl over the stored entries of ``a`` (row = target) + bias, the scores from
    LeakyReLU(Xl[j] + Xr[i] + e_ij w_e) . att (gcnx_gatv2_aggregate).  xlr = Xl | Xr [n, 2 heads c]; att [heads, c]; alpha
    [nnz, heads] and o_pre (the result before the bias) are stored if given."""
    heads, c = att.shape
    hc, n = heads * c, xlr.shape[0]
    assert a.n == n and xlr.shape[1] == 2 * hc and out.shape == (n, hc) and att.contiguous and (bias is None or bias.shape == (hc,))
    assert (alpha is None or (alpha.shape == (a.nnz, heads) and alpha.contiguous)) and (o_pre is None or o_pre.shape == (n, hc))
    ep, lde, d, wp = _edge_operands(a, e, w_e, hc)
    ctx._ck(ctx.lib.gcnx_gatv2_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(xlr), xlr.ld, n, heads, c, ep, lde, d, wp, _p(att), _p(bias),
                                         float(slope), _p(out), out.ld, _p(alpha), _p(o_pre), o_pre.ld if o_pre is not None else 0))
    return out


def gatv2_bwd_edges(ctx, a, xlr, att, alpha, dout, o, dscore, dxr, datt, scratch, e=None, w_e=None, dw_e=None, slope=0.2):
    """dscore [nnz, heads] (the CSR's entry order), dxr [n, heads c], datt [heads, c] and dw_e [D, heads c] from dout and O = o
    (gcnx_gatv2_bwd_edges).  scratch: gatv2_bwd_scratch_floats floats."""
    heads, c = att.shape
    hc, n = heads * c, xlr.shape[0]
    assert a.n == n and xlr.shape[1] == 2 * hc and dout.shape == o.shape == dxr.shape == (n, hc)
    assert alpha.shape == dscore.shape == (a.nnz, heads) and datt.shape == (heads, c)
    assert att.contiguous and alpha.contiguous and dscore.contiguous and datt.contiguous
    ep, lde, d, wp = _edge_operands(a, e, w_e, hc)
    assert (dw_e is None) == (d == 0) and (dw_e is None or (dw_e.shape == (d, hc) and dw_e.contiguous))
    assert scratch.size >= gatv2_bwd_scratch_floats(ctx, n, heads, c, d)
    ctx._ck(ctx.lib.gcnx_gatv2_bwd_edges(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(xlr), xlr.ld, n, heads, c, ep, lde, d, wp, _p(att),
                                         float(slope), _p(alpha), _p(dout), dout.ld, _p(o), o.ld, _p(dscore), _p(dxr), dxr.ld, _p(datt),
                                         _p(dw_e), _p(scratch)))
    return dscore, dxr


def gatv2_bwd_nodes(ctx, a, xlr, att, alpha, dscore, dout, dxl, e=None, w_e=None, slope=0.2):
    """dxl [n, heads c] on the transposed pattern of ``a`` with its entry permutation (a.transpose_perm(); gcnx_gatv2_bwd_nodes)."""
    heads, c = att.shape
    hc, n = heads * c, xlr.shape[0]
    assert a.n == n and xlr.shape[1] == 2 * hc and dout.shape == dxl.shape == (n, hc)
    assert alpha.shape == dscore.shape == (a.nnz, heads) and att.contiguous and alpha.contiguous and dscore.contiguous
    ep, lde, d, wp = _edge_operands(a, e, w_e, hc)
    rp, ci, pm = a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_gatv2_bwd_nodes(ctx.h, rp.ptr, ci.ptr, pm.ptr, _p(xlr), xlr.ld, n, heads, c, ep, lde, d, wp, _p(att), float(slope),
                                         _p(alpha), _p(dscore), _p(dout), dout.ld, _p(dxl), dxl.ld))
    return dxl


def resgated_conv_ok(ctx, n, h, ldp=None, edge_dim=0):
    """True if the ResGatedGraphConv kernels serve these shapes (gcnx_resgated_conv_ok); ldp: the leading dimension of K | Q | V."""
    return bool(ctx.lib.gcnx_resgated_conv_ok(int(n), int(h), int(ldp if ldp is not None else 3 * h), int(edge_dim)))


def resgated_bwd_scratch_floats(ctx, n, h, edge_dim=0):
    """Floats of scratch resgated_bwd_targets needs (gcnx_resgated_bwd_scratch_floats)."""
    out = C.c_int64()
    ctx._ck(ctx.lib.gcnx_resgated_bwd_scratch_floats(int(n), int(h), int(edge_dim), C.byref(out)))
    return int(out.value)


def resgated_aggregate(ctx, a, p, out, e=None, w_e=None, skip=None, bias=None):
    """out = skip + bias + sum over the stored entries of ``a`` (row = target) of sigmoid(K[i] + Q[j] + e_ij (W_ke + W_qe)) *
    (V[j] + e_ij W_ve) (gcnx_resgated_aggregate).  p = K | Q | V in its first 3 h columns; w_e [D, 3 h] = W_ke | W_qe | W_ve."""
    n, h = out.shape
    assert a.n == n and p.shape[0] == n and p.shape[1] >= 3 * h and (bias is None or bias.shape == (h,))
    assert skip is None or skip.shape == (n, h)
    ep, lde, d, wp = _edge_operands(a, e, w_e, 3 * h)
    ctx._ck(ctx.lib.gcnx_resgated_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(p), p.ld, n, h, ep, lde, d, wp, _p(skip),
                                            skip.ld if skip is not None else 0, _p(bias), _p(out), out.ld))
    return out


def resgated_bwd_targets(ctx, a, p, dout, dk, scratch=None, ds=None, e=None, w_e=None, dw_e=None):
    """dk [n, h] = dK, ds (if given) = dout, dw_e [D, 3 h] on the forward pattern of ``a`` (gcnx_resgated_bwd_targets).
    scratch: resgated_bwd_scratch_floats floats (None with no edge features)."""
    n, h = dout.shape
    assert a.n == n and p.shape[0] == n and p.shape[1] >= 3 * h and dk.shape == (n, h) and (ds is None or ds.shape == (n, h))
    ep, lde, d, wp = _edge_operands(a, e, w_e, 3 * h)
    assert (dw_e is None) == (d == 0) and (dw_e is None or (dw_e.shape == (d, 3 * h) and dw_e.contiguous))
    assert d == 0 or scratch.size >= resgated_bwd_scratch_floats(ctx, n, h, d)
    ctx._ck(ctx.lib.gcnx_resgated_bwd_targets(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(p), p.ld, n, h, ep, lde, d, wp, _p(dout), dout.ld,
                                              _p(dk), dk.ld, _p(ds), ds.ld if ds is not None else 0, _p(dw_e), _p(scratch)))
    return dk


def resgated_bwd_sources(ctx, a, p, dout, dqv, e=None, w_e=None):
    """dqv [n, 2 h] = dQ | dV on the transposed pattern of ``a`` with its entry permutation (a.transpose_perm();
    gcnx_resgated_bwd_sources)."""
    n, h = dout.shape
    assert a.n == n and p.shape[0] == n and p.shape[1] >= 3 * h and dqv.shape == (n, 2 * h)
    ep, lde, d, wp = _edge_operands(a, e, w_e, 3 * h)
    rp, ci, pm = a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_resgated_bwd_sources(ctx.h, rp.ptr, ci.ptr, pm.ptr, _p(p), p.ld, n, h, ep, lde, d, wp, _p(dout), dout.ld,
                                              _p(dqv), dqv.ld))
    return dqv


def transformer_conv_ok(ctx, n, heads, c, ldp=None, edge_dim=0):
    """True if the TransformerConv kernels serve these shapes (gcnx_transformer_conv_ok); ldp: the leading dimension of Q | K | V."""
    return bool(ctx.lib.gcnx_transformer_conv_ok(int(n), int(heads), int(c), int(ldp if ldp is not None else 3 * heads * c), int(edge_dim)))


def transformer_bwd_scratch_floats(ctx, n, heads, c, edge_dim=0, beta=False):
    """Floats of scratch transformer_bwd_targets and transformer_beta_bwd need (gcnx_transformer_bwd_scratch_floats)."""
    out = C.c_int64()
    ctx._ck(ctx.lib.gcnx_transformer_bwd_scratch_floats(int(n), int(heads), int(c), int(edge_dim), int(bool(beta)), C.byref(out)))
    return int(out.value)


def transformer_aggregate(ctx, a, p, out, heads, e=None, w_e=None, skip=None, w_beta=None, alpha=None, o_pre=None):
    """out = O (+ skip, or the beta-gated mix of skip and O with w_beta [3 heads c]); O = softmax-weighted sum of V[j] + e_ij w_e
    over the stored entries of ``a`` (row = target), the scores <Q[i], K[j] + e_ij w_e> / sqrt(c) per head
    (gcnx_transformer_aggregate).  p = Q | K | V in its first 3 heads c columns; alpha [nnz, heads] and o_pre = O are stored if
    given."""
    n, hc = out.shape
    c = hc // heads
    assert a.n == n and heads * c == hc and p.shape[0] == n and p.shape[1] >= 3 * hc
    assert (skip is None or skip.shape == (n, hc)) and (w_beta is None or (w_beta.shape == (3 * hc,) and w_beta.contiguous))
    assert (alpha is None or (alpha.shape == (a.nnz, heads) and alpha.contiguous)) and (o_pre is None or o_pre.shape == (n, hc))
    ep, lde, d, wp = _edge_operands(a, e, w_e, hc)
    ctx._ck(ctx.lib.gcnx_transformer_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(p), p.ld, n, heads, c, ep, lde, d, wp, _p(skip),
                                               skip.ld if skip is not None else 0, _p(w_beta), _p(out), out.ld, _p(alpha), _p(o_pre),
                                               o_pre.ld if o_pre is not None else 0))
    return out


def transformer_beta_bwd(ctx, dout, o, skip, w_beta, d_o, d_s, dw_beta, scratch):
    """d_o = dO, d_s = dS [n, hc] and dw_beta [3 hc] of the beta gate from dout, O = o and S = skip (gcnx_transformer_beta_bwd).
    scratch: transformer_bwd_scratch_floats(beta=True) floats."""
    n, hc = dout.shape
    assert o.shape == skip.shape == d_o.shape == d_s.shape == (n, hc) and w_beta.shape == dw_beta.shape == (3 * hc,)
    assert w_beta.contiguous and dw_beta.contiguous
    ctx._ck(ctx.lib.gcnx_transformer_beta_bwd(ctx.h, _p(dout), dout.ld, _p(o), o.ld, _p(skip), skip.ld, _p(w_beta), n, hc, _p(d_o),
                                              d_o.ld, _p(d_s), d_s.ld, _p(dw_beta), _p(scratch)))
    return d_o, d_s


def transformer_bwd_targets(ctx, a, p, alpha, d_o, o, dscore, dq, heads, scratch=None, ds=None, e=None, w_e=None, dw_e=None):
    """dscore [nnz, heads] (the CSR's entry order), dq [n, heads c] = dQ, ds (if given) = d_o and dw_e [D, heads c] on the forward
    pattern of ``a`` (gcnx_transformer_bwd_targets).  scratch: transformer_bwd_scratch_floats floats (None with no edge features)."""
    n, hc = d_o.shape
    c = hc // heads
    assert a.n == n and heads * c == hc and p.shape[0] == n and p.shape[1] >= 3 * hc and o.shape == dq.shape == (n, hc)
    assert (ds is None or ds.shape == (n, hc)) and alpha.shape == dscore.shape == (a.nnz, heads) and alpha.contiguous and dscore.contiguous
    ep, lde, d, wp = _edge_operands(a, e, w_e, hc)
    assert (dw_e is None) == (d == 0) and (dw_e is None or (dw_e.shape == (d, hc) and dw_e.contiguous))
    assert d == 0 or scratch.size >= transformer_bwd_scratch_floats(ctx, n, heads, c, d)
    ctx._ck(ctx.lib.gcnx_transformer_bwd_targets(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(p), p.ld, n, heads, c, ep, lde, d, wp, _p(alpha),
                                                 _p(d_o), d_o.ld, _p(o), o.ld, _p(dscore), _p(dq), dq.ld, _p(ds),
                                                 ds.ld if ds is not None else 0, _p(dw_e), _p(scratch)))
    return dscore, dq


def transformer_bwd_sources(ctx, a, p, alpha, dscore, d_o, dkv, heads):
    """dkv [n, 2 heads c] = dK | dV on the transposed pattern of ``a`` with its entry permutation (a.transpose_perm();
    gcnx_transformer_bwd_sources)."""
    n, hc = d_o.shape
    c = hc // heads
    assert a.n == n and heads * c == hc and p.shape[0] == n and p.shape[1] >= 3 * hc and dkv.shape == (n, 2 * hc)
    assert alpha.shape == dscore.shape == (a.nnz, heads) and alpha.contiguous and dscore.contiguous
    rp, ci, pm = a.transpose_perm()
    ctx._ck(ctx.lib.gcnx_transformer_bwd_sources(ctx.h, rp.ptr, ci.ptr, pm.ptr, _p(p), p.ld, n, heads, c, _p(alpha), _p(dscore), _p(d_o),
                                                 d_o.ld, _p(dkv), dkv.ld))
    return dkv


def topk_select_ok(ctx, max_graph_rows, f):
    """True if topk_select serves a batch whose largest graph has this many rows (gcnx_topk_select_ok)."""
    return bool(ctx.lib.gcnx_topk_select_ok(int(max_graph_rows), int(f)))


def topk_kept_ptr(graph_ptr_host, ratio):
    """graph_ptr' of TopKPool(ratio): the prefix sums of k_g = ceil(ratio * n_g), in float64 on the host (an empty graph
    keeps nothing) -- N' = graph_ptr'[-1] is known without reading anything back."""
    n_g = np.diff(np.asarray(graph_ptr_host, np.int64))
    k = np.minimum(np.ceil(np.float64(ratio) * n_g.astype(np.float64)).astype(np.int64), n_g)
    return np.concatenate([[0], np.cumsum(np.maximum(k, 0))]).astype(np.int32)


def topk_select(ctx, seg, kept_ptr, n_kept, x, p, y, idx, pos):
    """y = x p / ||p||; idx = the kept rows (kept_ptr[g + 1] - kept_ptr[g] of graph g with the largest y, in row order),
    pos = their new row numbers, -1 for dropped rows (gcnx_topk_select).  kept_ptr: int32[B + 1] on the device, n_kept its
    last element (what idx has to hold).
    NotImplementedError where the batch is not served (a graph of more than 16384 rows): there is no other route."""
    n, f = x.shape
    big = _max_block(seg.host)
    assert seg.n == n and p.size == f and p.contiguous and y.shape == (n,) and pos.shape == (n,) and kept_ptr.shape == (seg.n_graphs + 1,)
    assert y.dtype == np.float32 and idx.dtype == np.int32 and pos.dtype == np.int32 and kept_ptr.dtype == np.int32
    assert 0 <= n_kept <= n and idx.size >= n_kept
    if not topk_select_ok(ctx, big, f):
        raise NotImplementedError(f"gcnx_topk_select: a graph of {big} rows (f={f}) is not served (one workgroup ranks a graph: up to 16384 rows)")
    ctx._ck(ctx.lib.gcnx_topk_select(ctx.h, seg.dev.ptr, kept_ptr.ptr, seg.n_graphs, big, _p(x), x.ld, f, _p(p), y.ptr, idx.ptr, pos.ptr))
    return y, idx, pos


def topk_gather(ctx, x, y, idx, n_kept, out, sigmoid_gating=False):
    """out[r] = x[idx[r]] * gate(y[idx[r]]) for r < n_kept (gcnx_topk_gather); gate = tanh, or sigmoid."""
    f = x.shape[1]
    assert out.shape == (n_kept, f) and idx.dtype == np.int32 and idx.size >= n_kept and y.shape == (x.shape[0],)
    ctx._ck(ctx.lib.gcnx_topk_gather(ctx.h, _p(x), x.ld, _p(y), idx.ptr, int(n_kept), f, 1 if sigmoid_gating else 0, _p(out), out.ld))
    return out


def topk_bwd(ctx, x, y, pos, p, dxo, dx, dp, sigmoid_gating=False):
    """dx (every row: zeros for dropped rows) and dp from dxo = dLoss / dX' (gcnx_topk_bwd)."""
    n, f = x.shape
    assert dx.shape == (n, f) and dxo.shape[1] == f and pos.shape == (n,) and pos.dtype == np.int32 and p.size == f and dp.size == f
    assert p.contiguous and dp.contiguous
    ctx._ck(ctx.lib.gcnx_topk_bwd(ctx.h, _p(x), x.ld, _p(y), pos.ptr, _p(p), n, f, 1 if sigmoid_gating else 0, _p(dxo), dxo.ld,
                                  _p(dx), dx.ld, _p(dp)))
    return dx, dp


def csr_induce(ctx, a, idx, pos, n_kept, rowptr_out, colidx_out, vals_out=None):
    """A[idx][:, idx] of a DeviceCSR into the given arrays (gcnx_csr_induce): rowptr_out int32[n_kept + 1], colidx_out /
    vals_out with room for a.nnz entries.  Nothing is read back: nnz' is rowptr_out[n_kept]."""
    assert rowptr_out.size >= n_kept + 1 and colidx_out.size >= a.nnz and (a.vals is None) == (vals_out is None)
    assert idx.dtype == np.int32 and pos.dtype == np.int32 and pos.shape == (a.n,) and rowptr_out.dtype == colidx_out.dtype == np.int32
    ctx._ck(ctx.lib.gcnx_csr_induce(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), idx.ptr, pos.ptr, int(n_kept), rowptr_out.ptr,
                                    colidx_out.ptr, _p(vals_out)))


def read_int32(ctx, arr, index):
    """One int32 of a device array on the host: a 4-byte copy, which waits for the stream (gcnx_d2h)."""
    out = np.empty(1, np.int32)
    ctx._ck(ctx.lib.gcnx_d2h(ctx.h, out.ctypes.data, arr.ptr + 4 * int(index), 4))
    return int(out[0])


def to_bf16(ctx, x):
    """bf16 copy (uint16 bit patterns, round to nearest even) of a contiguous fp32 array (gcnx_f32_to_bf16)."""
    assert x.contiguous and x.dtype == np.float32
    y = ctx.empty(x.shape, np.uint16)
    ctx._ck(ctx.lib.gcnx_f32_to_bf16(ctx.h, x.ptr, y.ptr, x.size))
    return y


def to_bf16_into(ctx, x, y16):
    """y16 <- bf16(x), round to nearest even (gcnx_f32_to_bf16), into an existing uint16 array of the same shape."""
    assert x.contiguous and y16.contiguous and x.dtype == np.float32 and y16.dtype == np.uint16 and x.shape == y16.shape
    ctx._ck(ctx.lib.gcnx_f32_to_bf16(ctx.h, x.ptr, y16.ptr, x.size))
    return y16


def from_bf16(ctx, x):
    assert x.contiguous and x.dtype == np.uint16
    y = ctx.empty(x.shape, np.float32)
    ctx._ck(ctx.lib.gcnx_bf16_to_f32(ctx.h, x.ptr, y.ptr, x.size))
    return y


def spmm_bf16(ctx, a, h, bias, out, act=None):
    """out = bf16(act(A h + bias)) with h and out stored as bf16 (uint16 arrays), fp32 accumulation (gcnx_spmm_csr_bf16)."""
    n, f = h.shape
    assert a.n == n and out.shape == (n, f) and h.dtype == np.uint16 and out.dtype == np.uint16
    ctx._ck(ctx.lib.gcnx_spmm_csr_bf16(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(a.vals), h.ptr, h.ld, _p(bias), out.ptr, out.ld, n, f,
                                       L.ACTS[act]))
    return out


def pool_tile_rows(n, b):
    """Rows of the per-tile partial-sum arrays gcn_conv_fwd(pool=...) fills: one per (32-row tile, graph) pair at most."""
    return (int(n) + 31) // 32 + int(b)


def head_args(seg, tile_part, tile_cnt, pool_sum, pool_cnt, w, bias, y, denom, probs, loss_acc, dw, db, db_relu, pooled, dpooled,
              mode="sum", cce="logits"):
    """gcnx_head_args for gcn_conv_bwd_pool(head=...) and gemm_dw2(leaf=...).  The DeviceArrays must outlive the calls."""
    b, h = seg.n_graphs, w.shape[0]
    c = w.shape[1]
    assert w.contiguous and pooled.contiguous and dpooled.contiguous and pooled.shape == (b, h) and dpooled.shape == (b, h)
    assert tile_part.shape[1] == h and tile_cnt.shape == tile_part.shape and tile_part.contiguous and tile_cnt.contiguous
    assert pool_sum.shape == (b, h) and pool_cnt.shape == (b, h) and pool_sum.contiguous and pool_cnt.contiguous
    return L.HeadArgs(_p(tile_part), _p(tile_cnt), tile_part.shape[0], _p(pool_sum), _p(pool_cnt), seg.dev.ptr, b, h, L.POOLS[mode],
                      _p(w), _p(bias), _p(y), c, float(denom), L.CCES[cce], _p(probs), _p(loss_acc), _p(dw), _p(db), _p(db_relu),
                      _p(pooled), _p(dpooled))


def gcn_conv_bwd_pool(ctx, at, y2, seg, dpooled, w2, y1, dz2, dz1, db1=None, mode="sum", scratch=None, w2t=None, prec="f32",
                      head=None, mask8=None):
    """dz2 = pool'(dpooled) * [y2 > 0], dz1 = ((A^T dz2) w2^T) * [y1 > 0], db1 = column sums of dz1 -- one launch
    (gcnx_gcn_conv_bwd_pool).  With ``scratch`` the db1 reduction is left pending: returns the PendingReduce for
    gemm_dw2 (all zeros when nothing is pending).  w2t: w2^T as written by gcn_conv_fwd(wt=...), read instead of w2.
    mask8: [y2 > 0] as bytes (gcn_conv_fwd(mask8=...)), gathered instead of y2, which may then be None
    (gcnx_gcn_conv_bwd_pool_mask8: the same results bit for bit)."""
    if mask8 is not None:
        assert mask8.dtype == np.uint8 and (y2 is None or y2.shape == mask8.shape)
        y2 = mask8
    n, f2 = y2.shape
    f1 = w2.shape[0]
    assert at.n == n and w2.shape == (f1, f2) and w2.contiguous and y1.shape == (n, f1) and dz1.shape == (n, f1)
    assert (head is not None or dpooled.shape == (seg.n_graphs, f2)) and (dz2 is None or dz2.shape == (n, f2))
    pend = L.PendingReduce()
    fn = ctx.lib.gcnx_gcn_conv_bwd_pool_mask8 if mask8 is not None else ctx.lib.gcnx_gcn_conv_bwd_pool
    ctx._ck(fn(ctx.h, at.rowptr.ptr, at.colidx.ptr, _p(at.vals), y2.ptr if mask8 is not None else _p(y2), y2.ld, seg.ids.ptr,
                                           seg.dev.ptr, seg.n_graphs, _p(dpooled), dpooled.ld if dpooled is not None else 0,
                                           L.POOLS[mode], n, f2,
                                           _p(w2t if w2t is not None else w2), f1, 1 if w2t is not None else 0, _p(y1), y1.ld, _p(dz2), dz2.ld if dz2 is not None else 0, _p(dz1), dz1.ld, _p(db1),
                                           _p(scratch), scratch.size if scratch is not None else 0,
                                           C.byref(pend) if scratch is not None else None, L.PRECS[prec],
                                           C.byref(head) if head is not None else None))
    return pend


def gcn_conv_bwd_scratch_floats(ctx, n, f1):
    return int(ctx.lib.gcnx_gcn_conv_bwd_scratch_floats(int(n), int(f1)))


def gemm_dw2(ctx, xa, dha, dwa, xb, dhb, dwb, prec="f32", params=None, grads=None, lr=0.0, pending=None, leaf=None):
    """dwa = xa^T dha and dwb = xb^T dhb in one launch; with params / grads (the flat buffers both gradients are
    views of) the reduction also applies the SGD step and finishes ``pending`` (gcnx_gemm_dw2)."""
    n, fia = xa.shape
    foa = dha.shape[1]
    fib, fob = xb.shape[1], dhb.shape[1]
    assert xb.shape[0] == n and dha.shape[0] == n and dhb.shape[0] == n and dwa.shape == (fia, foa) and dwb.shape == (fib, fob)
    ctx._ck(ctx.lib.gcnx_gemm_dw2(ctx.h, _p(xa), xa.ld, _p(dha), dha.ld, _p(dwa), fia, foa, _p(xb), xb.ld, _p(dhb), dhb.ld,
                                  _p(dwb), fib, fob, n, L.PRECS[prec], _p(params), _p(grads),
                                  params.size if params is not None else (grads.size if grads is not None else 0), float(lr),
                                  C.byref(pending) if pending is not None else None, C.byref(leaf) if leaf is not None else None))


def dw2_slice_plan(graph_ptr_host, kchunk):
    """The row slices of gemm_dw2_graph for one batch, on the host (gcnx_dw2_slice_plan): int32 [nslices, 4] rows of
    {row_begin, row_end, graph, float32 bits of 1 / rows of the graph}; no slice spans two graphs, cuts at multiples of kchunk from a graph's start."""
    gp = np.ascontiguousarray(graph_ptr_host, dtype=np.int32)
    lib = L.load()
    cnt = int(lib.gcnx_dw2_slice_plan(gp.ctypes.data, len(gp) - 1, int(kchunk), None, 0))
    if cnt < 0:
        raise ValueError("dw2_slice_plan: graph_ptr must be non-decreasing and kchunk a positive multiple of 32")
    plan = np.zeros((cnt, 4), np.int32)
    if cnt:
        assert int(lib.gcnx_dw2_slice_plan(gp.ctypes.data, len(gp) - 1, int(kchunk), plan.ctypes.data, cnt)) == cnt
    return plan


def gemm_dw2_graph_plan(ctx, seg, n, fia, foa, fib, fob, mode="sum", prec="f32"):
    """(plan on the device, slice count, kchunk) when gemm_dw2_graph serves these shapes for the graphs of ``seg``, else None
    (gcnx_gemm_dw2_graph_kchunk, gcnx_dw2_slice_plan, gcnx_gemm_dw2_graph_ok).  A constant of the batch: one small upload."""
    if mode not in ("sum", "avg", "mean") or prec not in L.PRECS:
        return None
    kchunk = int(ctx.lib.gcnx_gemm_dw2_graph_kchunk(ctx.h, int(n), fia, foa, fib, fob))
    if kchunk <= 0:
        return None
    plan = dw2_slice_plan(seg.host, kchunk)
    if not ctx.lib.gcnx_gemm_dw2_graph_ok(ctx.h, int(n), fia, foa, fib, fob, kchunk, len(plan), L.POOLS[mode], L.PRECS[prec]):
        return None
    return ctx.to_device(plan, np.int32), len(plan), kchunk


def gemm_dw2_graph(ctx, xa, dha, dwa, xb, mask8, dwb, plan, dpooled, mode="sum", params=None, grads=None, lr=0.0, pending=None,
                   leaf=None):
    """dwa = xa^T dha as gemm_dw2 computes it, and dwb = xb^T (mask8 * pool'(dpooled)[graph]) from per-graph mask products on
    the bf16 MFMA (gcnx_gemm_dw2_graph); ``plan`` is gemm_dw2_graph_plan's triple.  False -- nothing launched -- when the
    library answers GCNX_ERR_UNSUPPORTED."""
    n, fia = xa.shape
    foa = dha.shape[1]
    fib, fob = xb.shape[1], mask8.shape[1]
    table, nslices, kchunk = plan
    assert xb.shape[0] == n and dha.shape[0] == n and mask8.shape[0] == n and mask8.dtype == np.uint8
    assert dwa.shape == (fia, foa) and dwb.shape == (fib, fob) and dpooled.shape[1] == fob
    rc = ctx.lib.gcnx_gemm_dw2_graph(ctx.h, _p(xa), xa.ld, _p(dha), dha.ld, _p(dwa), fia, foa, _p(xb), xb.ld, mask8.ptr, mask8.ld,
                                     _p(dwb), fib, fob, n, table.ptr, nslices, kchunk, _p(dpooled), dpooled.ld, L.POOLS[mode],
                                     _p(params), _p(grads),
                                     params.size if params is not None else (grads.size if grads is not None else 0), float(lr),
                                     C.byref(pending) if pending is not None else None, C.byref(leaf) if leaf is not None else None)
    if rc == L.ERR_UNSUPPORTED:
        return False
    ctx._ck(rc)
    return True


def pool_bwd_colsum(ctx, seg, dpooled, y, db, mode="sum"):
    """db = column sums of pool'(dpooled) * [y > 0] without materialising it (gcnx_pool_bwd_colsum)."""
    ctx._ck(ctx.lib.gcnx_pool_bwd_colsum(ctx.h, seg.dev.ptr, seg.n_graphs, _p(dpooled), dpooled.ld, _p(y), y.ld,
                                         y.shape[1], L.POOLS[mode], _p(db)))
    return db


def softmax_cce(ctx, logits, y, probs, loss_acc, dlogits=None, denom=None, cce="logits"):
    """cce = "logits": the softmax_cross_entropy_with_logits form Keras runs inside tf.function (gcn.py:328-335);
    "probs": the renormalise-and-clip form it runs on eager tensors (evaluate, gcn.py:351-354)."""
    b, c = logits.shape
    ctx._ck(ctx.lib.gcnx_softmax_cce(ctx.h, _p(logits), _p(y), b, c, float(denom if denom else b), _p(probs),
                                     _p(loss_acc), _p(dlogits), L.CCES[cce]))


def dense_softmax_cce(ctx, pooled, w, bias, y, probs, loss_acc=None, denom=None, dw=None, db=None, dpooled=None,
                      cce="logits"):
    """The classifier head in one launch (gcnx_dense_softmax_cce): probs = softmax(pooled W + b); with labels y
    also loss_acc = [CCE sum / denom, #correct] (overwritten); with dw also dw, db, dpooled."""
    b, h = pooled.shape
    c = w.shape[1]
    ctx._ck(ctx.lib.gcnx_dense_softmax_cce(ctx.h, _p(pooled), pooled.ld, _p(w), _p(bias), _p(y), b, h, c,
                                           float(denom if denom else max(b, 1)), _p(probs), _p(loss_acc), _p(dw), _p(db),
                                           _p(dpooled), dpooled.ld if dpooled is not None else 0, L.CCES[cce]))
    return probs


def act_bias_grad(ctx, dy, y, dz, act, db=None, alpha=None, dalpha=None):
    n, f = dy.shape
    ctx._ck(ctx.lib.gcnx_act_bias_grad(ctx.h, _p(dy), dy.ld, _p(y), y.ld if y is not None else 0, _p(dz), dz.ld, n,
                                       f, L.ACTS[act], _p(alpha), _p(db), _p(dalpha)))
    return dz


def gemm_dw(ctx, x, dh, dw, prec="f32"):
    n, fi = x.shape
    fo = dh.shape[1]
    assert dh.shape[0] == n and dw.shape == (fi, fo) and dw.contiguous
    ctx._ck(ctx.lib.gcnx_gemm_dw(ctx.h, _p(x), x.ld, _p(dh), dh.ld, _p(dw), n, fi, fo, L.PRECS[prec]))
    return dw


def gemm_dx(ctx, dh, w, dx, prec="f32", accumulate=False, y_mask=None, db=None, mask_bits=None):
    """dx = dh w^T (* [y_mask > 0], db = column sums).  mask_bits: the bit image gemm_relu_bits wrote for the same
    activation -- read instead of y_mask (gcnx_gemm_dx_bits)."""
    n, fo = dh.shape
    fi = w.shape[0]
    assert w.shape[1] == fo and dx.shape == (n, fi)
    if mask_bits is not None:
        assert not accumulate
        ctx._ck(ctx.lib.gcnx_gemm_dx_bits(ctx.h, _p(dh), dh.ld, _p(w), _p(dx), dx.ld, n, fi, fo, L.PRECS[prec], mask_bits.ptr, _p(db)))
        return dx
    ctx._ck(ctx.lib.gcnx_gemm_dx(ctx.h, _p(dh), dh.ld, _p(w), _p(dx), dx.ld, n, fi, fo, L.PRECS[prec],
                                 1 if accumulate else 0, _p(y_mask), y_mask.ld if y_mask is not None else 0, _p(db)))
    return dx


def gemm_dw_sgd(ctx, x, dh, dw, params, grads, lr, prec="f32", pending=None):
    """dw = X^T dH (a view into the flat ``grads``), then params -= lr * grads over the whole flat buffers
    (gcnx_gemm_dw_sgd: the split-K reduction launch applies the update, and finishes a ``pending`` reduction left
    by dense_bwd_deferred)."""
    n, fi = x.shape
    fo = dh.shape[1]
    assert dh.shape[0] == n and dw.shape == (fi, fo) and dw.contiguous and params.size == grads.size
    ctx._ck(ctx.lib.gcnx_gemm_dw_sgd(ctx.h, _p(x), x.ld, _p(dh), dh.ld, _p(dw), n, fi, fo, L.PRECS[prec], _p(params),
                                     _p(grads), params.size, float(lr), C.byref(pending) if pending is not None else None))


def dense_bwd_scratch_floats(ctx, n, fi, fo):
    return int(ctx.lib.gcnx_dense_bwd_scratch_floats(ctx.h, n, fi, fo))


def dense_bwd_deferred(ctx, x, dh, w, dx, dw, scratch, prec="f32", y_mask=None, db_prev=None):
    """dense_bwd whose reductions (db_prev, dw) are left in ``scratch`` for the step's last launch; returns the
    PendingReduce to hand to gemm_dw_sgd (all zeros if the fused form did not apply: results are then final)."""
    n, fo = dh.shape
    fi = w.shape[0]
    assert w.shape[1] == fo and dx.shape == (n, fi) and x.shape == (n, fi) and dw.shape == (fi, fo) and w.contiguous
    pend = L.PendingReduce()
    ctx._ck(ctx.lib.gcnx_dense_bwd_deferred(ctx.h, _p(x), x.ld, _p(dh), dh.ld, _p(w), n, fi, fo, L.PRECS[prec], _p(dx), dx.ld,
                                            _p(y_mask), y_mask.ld if y_mask is not None else 0, _p(db_prev), _p(dw),
                                            _p(scratch), scratch.size if scratch is not None else 0, C.byref(pend)))
    return pend


def dense_bwd(ctx, x, dh, w, dx, dw, prec="f32", y_mask=None, db_prev=None):
    """Backward of H = X W given dH in one call (gcnx_dense_bwd): dw = X^T dH, dx = dH W^T (* [y_mask > 0]),
    db_prev = column sums of dx."""
    n, fo = dh.shape
    fi = w.shape[0]
    assert w.shape[1] == fo and dx.shape == (n, fi) and x.shape == (n, fi) and dw.shape == (fi, fo) and w.contiguous
    ctx._ck(ctx.lib.gcnx_dense_bwd(ctx.h, _p(x), x.ld, _p(dh), dh.ld, _p(w), n, fi, fo, L.PRECS[prec], _p(dx), dx.ld,
                                   _p(y_mask), y_mask.ld if y_mask is not None else 0, _p(db_prev), _p(dw)))
    return dx


def sgd(ctx, params, grads, lr):
    ctx._ck(ctx.lib.gcnx_sgd(ctx.h, _p(params), _p(grads), params.size, float(lr)))


OPTIM_MAX_PARTIALS = 256             # GCNX_OPTIM_MAX_PARTIALS


def grad_sqnorm_partials(n):
    """Workgroups (= partial sums) gcnx_grad_sqnorm is launched with for n gradients: one per 256, at most 256."""
    return max(1, min(OPTIM_MAX_PARTIALS, -(-int(n) // 256)))


def grad_sqnorm(ctx, grads, partials, n_partials=None):
    """partials[:n_partials] = the workgroups' shares of sum g^2 in a fixed order (gcnx_grad_sqnorm); returns n_partials --
    what the update launch is told.  No host read: adam / sgd_momentum finish the sum."""
    k = grad_sqnorm_partials(grads.size) if n_partials is None else int(n_partials)
    assert partials.size >= min(k, OPTIM_MAX_PARTIALS)
    ctx._ck(ctx.lib.gcnx_grad_sqnorm(ctx.h, _p(grads), grads.size, _p(partials), k))
    return k


def adam(ctx, params, grads, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, partials=None, n_partials=0,
         clipnorm=None, norm_out=None):
    """One Adam / AdamW step over flat buffers (gcnx_adam).  t: the uint32 device step count, already advanced
    (counter_add).  clipnorm needs the partials of grad_sqnorm; norm_out (1 float) receives the gradient norm."""
    assert grads.size == m.size == v.size == params.size
    ctx._ck(ctx.lib.gcnx_adam(ctx.h, _p(params), _p(grads), _p(m), _p(v), params.size, _p(t), float(lr), float(beta1), float(beta2),
                              float(eps), float(weight_decay), _p(partials), int(n_partials), float(clipnorm or 0.0), _p(norm_out)))


def sgd_momentum(ctx, params, grads, vel, lr, momentum=0.0, nesterov=False, partials=None, n_partials=0, clipnorm=None,
                 norm_out=None):
    """One Keras SGD(momentum, nesterov) step over flat buffers (gcnx_sgd_momentum); clipping as in adam."""
    assert grads.size == vel.size == params.size
    ctx._ck(ctx.lib.gcnx_sgd_momentum(ctx.h, _p(params), _p(grads), _p(vel), params.size, float(lr), float(momentum), int(bool(nesterov)),
                                      _p(partials), int(n_partials), float(clipnorm or 0.0), _p(norm_out)))


BN_EPS, BN_MOMENTUM = 1e-3, 0.99     # Keras BatchNormalization defaults


def bn_stats(ctx, z, sums, shift=None):
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_stats(ctx.h, _p(z), z.ld, n, f, _p(shift), _p(sums)))


def bn_finalize(ctx, sums, count, mean, inv, moving_mean=None, moving_var=None, shift=None, momentum=BN_MOMENTUM, eps=BN_EPS):
    ctx._ck(ctx.lib.gcnx_bn_finalize(ctx.h, _p(sums), float(count), mean.size, momentum, eps, _p(shift), _p(mean), _p(inv),
                                     _p(moving_mean), _p(moving_var)))


def bn_moments(ctx, z, sums, mean, inv, moving_mean=None, moving_var=None, momentum=BN_MOMENTUM, eps=BN_EPS):
    """Batch mean / biased variance the way tf.nn.moments takes them (variance of the centred data): a first
    pass for the mean, a second one centred on it (gcnx_bn_moments; `sums` is kept for signature compatibility
    with the bn_stats / bn_finalize pair used for sync-BN)."""
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_moments(ctx.h, _p(z), z.ld, n, f, momentum, eps, _p(mean), _p(inv), _p(moving_mean),
                                    _p(moving_var)))


def wimage_elems(ctx, fi, fo, transpose, prec):
    """bf16 elements of the weight image of W [fi, fo] (or of W^T) for gemm_wimage; 0 for prec "f32"."""
    return int(ctx.lib.gcnx_wimage_elems(int(fi), int(fo), 1 if transpose else 0, L.PRECS[prec]))


def wimage_prepare(ctx, jobs):
    """ONE launch writes the images of several matrices: jobs = [(w, img, transpose, prec), ...] (gcnx_wimage_prepare)."""
    if not jobs:
        return
    arr = (L.WimageJob * len(jobs))()
    for k, (w, img, transpose, prec) in enumerate(jobs):
        fi, fo = w.shape
        arr[k] = L.WimageJob(w.ptr, img.ptr, fi, fo, 1 if transpose else 0, L.PRECS[prec])
    ctx._ck(ctx.lib.gcnx_wimage_prepare(ctx.h, len(jobs), C.cast(arr, C.c_void_p)))


def gemm_wimage(ctx, x, img, fi, fo, out, transpose=False, bias=None, prec="bf16x3", accumulate=False, bn_parts=None):
    """out = x W + bias (transpose False) / out (+)= x W^T (True) with W read from its image (gcnx_gemm_wimage).  Returns
    None when the kernel does not serve the shape (nothing launched), else the number of batch-norm parts written to
    ``bn_parts`` (0 without)."""
    n = x.shape[0]
    nparts = C.c_int32(0)
    rc = ctx.lib.gcnx_gemm_wimage(ctx.h, _p(x), x.ld, img.ptr, int(fi), int(fo), 1 if transpose else 0, _p(bias), _p(out), out.ld, n,
                                  L.PRECS[prec], 1 if accumulate else 0, _p(bn_parts), C.byref(nparts) if bn_parts is not None else None)
    if rc == L.ERR_UNSUPPORTED:
        return None
    ctx._ck(rc)
    return nparts.value


def gemm_wimage_parts(ctx, n):
    return int(ctx.lib.gcnx_gemm_wimage_parts(ctx.h, int(n)))


def bn_finalize_parts(ctx, parts, nparts, mean, inv, moving_mean=None, moving_var=None, momentum=BN_MOMENTUM, eps=BN_EPS):
    """mean / inv (and the moving statistics) from the (rows, mean, M2) parts gemm_wimage left (gcnx_bn_finalize_parts)."""
    ctx._ck(ctx.lib.gcnx_bn_finalize_parts(ctx.h, _p(parts), int(nparts), mean.size, momentum, eps, _p(mean), _p(inv),
                                           _p(moving_mean), _p(moving_var)))


def bn_act(ctx, z, mean, inv, gamma, beta, y, act=None, alpha=None):
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act(ctx.h, _p(z), z.ld, n, f, _p(mean), _p(inv), _p(gamma), _p(beta), L.ACTS[act], _p(alpha),
                                _p(y), y.ld))
    return y


def bn_act_bwd(ctx, dy, z, mean, inv, gamma, beta, dz, scratch, act=None, alpha=None, training=True, dgamma=None, dbeta=None,
               dalpha=None):
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act_bwd(ctx.h, _p(dy), dy.ld, _p(z), z.ld, n, f, _p(mean), _p(inv), _p(gamma), _p(beta),
                                    L.ACTS[act], _p(alpha), 1 if training else 0, _p(dz), dz.ld, _p(dgamma), _p(dbeta),
                                    _p(dalpha), _p(scratch)))
    return dz


def bn_act_bwd_stats(ctx, dy, z, mean, inv, gamma, beta, scratch, act=None, alpha=None, dgamma=None, dbeta=None, dalpha=None):
    """First half of bn_act_bwd (sync-BN): the three local column sums -> scratch[3f] and the parameter gradients."""
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act_bwd_stats(ctx.h, _p(dy), dy.ld, _p(z), z.ld, n, f, _p(mean), _p(inv), _p(gamma), _p(beta),
                                          L.ACTS[act], _p(alpha), _p(scratch), _p(dgamma), _p(dbeta), _p(dalpha)))


def bn_act_bwd_apply(ctx, dy, z, mean, inv, gamma, beta, sums, count, dz, act=None, alpha=None, training=True):
    """Second half: dz from the (all-reduced) sums and the global row count."""
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act_bwd_apply(ctx.h, _p(dy), dy.ld, _p(z), z.ld, n, f, _p(mean), _p(inv), _p(gamma), _p(beta),
                                          L.ACTS[act], _p(alpha), _p(sums), float(count), 1 if training else 0, _p(dz), dz.ld))
    return dz


def dropout(ctx, x, rate, seed, stream_id, step=None, out=None):
    """Keras Dropout(rate), training mode (gcnx_dropout): out = x * keep / (1 - rate); the same call on the incoming gradient
    is the backward pass (the mask is a stateless hash of (seed, stream_id, step, element)).  In place by default."""
    out = x if out is None else out
    n, f = x.shape
    assert out.shape == (n, f)
    ctx._ck(ctx.lib.gcnx_dropout(ctx.h, _p(x), x.ld, n, f, float(rate), int(seed) & 0xFFFFFFFF, int(stream_id) & 0xFFFFFFFF, _p(step),
                                 _p(out), out.ld))
    return out


def counter_add(ctx, counter, inc=1):
    """*counter += inc on the stream (a uint32 device scalar: the optimizer's step count)."""
    ctx._ck(ctx.lib.gcnx_counter_add(ctx.h, _p(counter), int(inc)))


def add(ctx, a, b, out):
    """out = a + b (GeneralGNN(connectivity="sum"))."""
    n, f = a.shape
    assert b.shape == (n, f) and out.shape == (n, f)
    ctx._ck(ctx.lib.gcnx_add(ctx.h, _p(a), a.ld, _p(b), b.ld, _p(out), out.ld, n, f))
    return out


def spmm_minmax(ctx, a, h, out, cnt=None, mode="max"):
    """GeneralConv(aggregate="max" | "min" | "prod") (gcnx_spmm_csr_minmax / gcnx_spmm_csr_prod): out[t] = max / min / product over
    the entries (t, s) of h[s] (values ignored); cnt = what the gradient needs -- the number of entries attaining the extremum, or
    for "prod" the product of the row's non-zero messages (0 where two or more are zero)."""
    n, f = h.shape
    assert a.n == n and out.shape == (n, f) and mode in ("max", "min", "prod")
    if mode == "prod":
        ctx._ck(ctx.lib.gcnx_spmm_csr_prod(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(h), h.ld, _p(out), out.ld, _p(cnt),
                                           cnt.ld if cnt is not None else 0, n, f))
        return out
    ctx._ck(ctx.lib.gcnx_spmm_csr_minmax(ctx.h, a.rowptr.ptr, a.colidx.ptr, _p(h), h.ld, _p(out), out.ld, _p(cnt),
                                         cnt.ld if cnt is not None else 0, n, f, 1 if mode == "min" else 0))
    return out


def spmm_minmax_bwd(ctx, at, h, out, cnt, dy, dh, mode="max"):
    """Gradient of spmm_minmax wrt h (gcnx_spmm_csr_minmax_bwd / gcnx_spmm_csr_prod_bwd); ``at`` is the transposed operator."""
    n, f = h.shape
    assert at.n == n and out.shape == (n, f) and cnt.shape == (n, f) and dy.shape == (n, f) and dh.shape == (n, f)
    if mode == "prod":
        ctx._ck(ctx.lib.gcnx_spmm_csr_prod_bwd(ctx.h, at.rowptr.ptr, at.colidx.ptr, _p(h), h.ld, _p(out), out.ld, _p(cnt), cnt.ld,
                                               _p(dy), dy.ld, _p(dh), dh.ld, n, f))
        return dh
    ctx._ck(ctx.lib.gcnx_spmm_csr_minmax_bwd(ctx.h, at.rowptr.ptr, at.colidx.ptr, _p(h), h.ld, _p(out), out.ld, _p(cnt), cnt.ld,
                                             _p(dy), dy.ld, _p(dh), dh.ld, n, f))
    return dh


# ---- the reference's torch GCN (gcn_utills.py:795-853): BatchNorm1d + PReLU() + global_max_pool, BCE head ----------------
TORCH_BN_EPS = 1e-5                  # torch.nn.BatchNorm1d default


def graph_norm_scratch_floats(ctx, n, b, f, slice_rows=0):
    """Floats of scratch that serve graph_norm_act and graph_norm_act_bwd with this slice_rows (gcnx_graph_norm_scratch_floats)."""
    return int(ctx.lib.gcnx_graph_norm_scratch_floats(int(n), int(b), int(f), int(slice_rows)))


def graph_norm_act(ctx, seg, z, mean_scale, gamma, beta, y, mean, inv, act=None, alpha=None, scratch=None, slice_rows=0,
                   eps=TORCH_BN_EPS):
    """y = act(gamma * (z - mean_scale * mu_g) * inv_g + beta) with the statistics of each graph's own rows, and the per-graph
    mean / inv [b, f] (gcnx_graph_norm_act).  act: None or "prelu_shared" with its slope alpha.  y may be z.  slice_rows = 0:
    the library's route (one workgroup per graph without scratch); > 0: graphs cut into slices of that many rows (needs scratch)."""
    n, f = z.shape
    b = seg.n_graphs
    assert seg.n == n and y.shape == (n, f) and all(t.size == f and t.contiguous for t in (mean_scale, gamma, beta))
    assert mean.shape == inv.shape == (b, f) and mean.contiguous and inv.contiguous
    assert scratch is None or scratch.size >= graph_norm_scratch_floats(ctx, n, b, f, slice_rows)
    ctx._ck(ctx.lib.gcnx_graph_norm_act(ctx.h, seg.dev.ptr, _p(z), z.ld, _p(mean_scale), _p(gamma), _p(beta), float(eps), L.ACTS[act],
                                        _p(alpha), n, b, f, int(slice_rows), _p(y), y.ld, _p(mean), _p(inv), _p(scratch)))
    return y


def graph_norm_act_bwd(ctx, seg, dy, z, mean, inv, mean_scale, gamma, beta, dz, act=None, alpha=None, dgamma=None, dbeta=None,
                       dmean_scale=None, dalpha=None, scratch=None, slice_rows=0):
    """dz [n, f] (written, not accumulated; may be dy) and the parameter gradients, each of which may be None, from z, mean and
    inv as graph_norm_act left them (gcnx_graph_norm_act_bwd)."""
    n, f = z.shape
    b = seg.n_graphs
    assert seg.n == n and dy.shape == dz.shape == (n, f) and all(t.size == f and t.contiguous for t in (mean_scale, gamma, beta))
    assert mean.shape == inv.shape == (b, f) and mean.contiguous and inv.contiguous
    assert all(t is None or (t.size == f and t.contiguous) for t in (dgamma, dbeta, dmean_scale))
    assert scratch is None or scratch.size >= graph_norm_scratch_floats(ctx, n, b, f, slice_rows)
    ctx._ck(ctx.lib.gcnx_graph_norm_act_bwd(ctx.h, seg.dev.ptr, _p(dy), dy.ld, _p(z), z.ld, _p(mean), _p(inv), _p(mean_scale),
                                            _p(gamma), _p(beta), L.ACTS[act], _p(alpha), n, b, f, int(slice_rows), _p(dz), dz.ld,
                                            _p(dgamma), _p(dbeta), _p(dmean_scale), _p(dalpha), _p(scratch)))
    return dz


def sddmm(ctx, a, l, r, out, scale=None, accumulate=False):
    """out[e] (+)= scale[e] * <l[row(e)], r[col(e)]> over the stored entries of ``a`` (gcnx_sddmm_csr): with Z = A H the gradient
    with respect to A's values for l = dZ, r = H.  l, r [n, f] (any leading dimension), scale / out [nnz]."""
    n, f = l.shape
    assert a.n == n and r.shape == (n, f) and out.size >= a.nnz and (scale is None or scale.size >= a.nnz)
    ctx._ck(ctx.lib.gcnx_sddmm_csr(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.n, a.nnz, _p(l), l.ld, _p(r), r.ld, f, _p(scale), _p(out),
                                   1 if accumulate else 0))
    return out


def mask_scratch_floats(ctx, n=0, f=0, per_row=False):
    """Floats of scratch for edge_mask_bwd (f = 0) / feat_mask_bwd (gcnx_mask_scratch_floats)."""
    return int(ctx.lib.gcnx_mask_scratch_floats(int(n), int(f), 1 if per_row else 0))


def edge_mask_fwd(ctx, a, logits, vals_out, perm_t=None, vals_t_out=None):
    """vals_out = a.vals * sigmoid(logits) off the diagonal, a.vals on it; vals_t_out[p] = vals_out[perm_t[p]] (gcnx_edge_mask_fwd)."""
    assert a.vals is not None and logits.size >= a.nnz and vals_out.size >= a.nnz
    assert vals_t_out is None or (perm_t is not None and vals_t_out.size >= a.nnz)
    ctx._ck(ctx.lib.gcnx_edge_mask_fwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.n, a.nnz, _p(a.vals), _p(logits),
                                       perm_t.ptr if perm_t is not None else None, _p(vals_out), _p(vals_t_out)))
    return vals_out


def edge_mask_bwd(ctx, a, logits, dv, dlogits, terms, scratch, c_size=0.0, c_ent=0.0):
    """dlogits from dv = dLoss/d(masked values) plus the regularisers' gradients, terms[0 .. 1] = sum sigmoid, sum entropy over
    the off-diagonal entries (gcnx_edge_mask_bwd).  a: the UNMASKED operator."""
    assert a.vals is not None and min(logits.size, dv.size, dlogits.size) >= a.nnz and terms.size >= 2
    assert scratch.size >= mask_scratch_floats(ctx)
    ctx._ck(ctx.lib.gcnx_edge_mask_bwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.n, a.nnz, _p(a.vals), _p(logits), _p(dv), float(c_size),
                                       float(c_ent), _p(dlogits), _p(terms), _p(scratch)))
    return dlogits


def feat_mask_fwd(ctx, x, logits, out):
    """out = x * sigmoid(logits); logits [1, f] / [f] (one per feature) or [n, f] contiguous (gcnx_feat_mask_fwd)."""
    n, f = x.shape
    assert out.shape == (n, f) and logits.contiguous and logits.size in (f, n * f)
    per_row = logits.size != f                              # (one row: both forms are the same product)
    ctx._ck(ctx.lib.gcnx_feat_mask_fwd(ctx.h, _p(x), x.ld, _p(logits), 1 if per_row else 0, n, f, _p(out), out.ld))
    return out


def feat_mask_bwd(ctx, dxm, x, logits, dlogits, terms, scratch, c_size=0.0, c_ent=0.0):
    """dlogits (the shape of logits) from dxm = dLoss/d(x * sigmoid(logits)) plus the regularisers' gradients; terms[0 .. 1] =
    sum sigmoid, sum entropy over the logits (gcnx_feat_mask_bwd)."""
    n, f = x.shape
    assert dxm.shape == (n, f) and logits.contiguous and logits.size in (f, n * f) and dlogits.size == logits.size and terms.size >= 2
    per_row = logits.size != f
    assert scratch.size >= mask_scratch_floats(ctx, n, f, per_row)
    ctx._ck(ctx.lib.gcnx_feat_mask_bwd(ctx.h, _p(dxm), dxm.ld, _p(x), x.ld, _p(logits), 1 if per_row else 0, n, f, float(c_size),
                                       float(c_ent), _p(dlogits), _p(terms), _p(scratch)))
    return dlogits


def pdn_ok(ctx, edge_dim, edge_hidden):
    """True if the PDN operator kernels serve this MLP: edge_dim 1 .. 8, edge_hidden 1 .. 64 (gcnx_pdn_ok)."""
    return bool(ctx.lib.gcnx_pdn_ok(int(edge_dim), int(edge_hidden)))


def pdn_bwd_scratch_floats(ctx, n, nnz, edge_dim, edge_hidden):
    return int(ctx.lib.gcnx_pdn_bwd_scratch_floats(int(n), int(nnz), int(edge_dim), int(edge_hidden)))


def _pdn_mlp(e, w1, b1, w2, b2):
    d, he = w1.shape
    assert e.shape[1] == d and b1.size == he and w2.size == he and b2.size == 1
    assert w1.contiguous and b1.contiguous and w2.contiguous
    return d, he


def pdn_operator(ctx, a, e, w1, b1, w2, b2, w_out, r_out, vals_out, unit=None, perm_t=None, vals_t_out=None):
    """The PDNConv operator on the pattern of ``a``: w_out [nnz] = the gates sigmoid(MLP(e)) (1 where unit), r_out [n] =
    deg^-1/2 of the weighted degrees, vals_out [nnz] = r_i w_e r_j, vals_t_out[p] = vals_out[perm_t[p]] (gcnx_pdn_operator).
    e [nnz, d] with any leading dimension; w1 [d, he], b1 [he], w2 [he], b2 [1]; unit: uint8 [nnz] or None."""
    d, he = _pdn_mlp(e, w1, b1, w2, b2)
    assert e.shape[0] >= a.nnz and min(w_out.size, vals_out.size) >= a.nnz and r_out.size >= a.n
    assert (perm_t is None) == (vals_t_out is None) and (vals_t_out is None or vals_t_out.size >= a.nnz)
    assert unit is None or (unit.dtype == np.uint8 and unit.size >= a.nnz)
    ctx._ck(ctx.lib.gcnx_pdn_operator(ctx.h, a.rowptr.ptr, a.colidx.ptr, a.n, a.nnz, _p(e), e.ld, d, _p(w1), _p(b1), _p(w2), _p(b2), he,
                                      unit.ptr if unit is not None else None, perm_t.ptr if perm_t is not None else None, _p(w_out),
                                      _p(r_out), _p(vals_out), _p(vals_t_out)))
    return vals_out


def pdn_operator_bwd(ctx, a, e, w1, b1, w2, b2, w, r, g, dw1, db1, dw2, db2, scratch, unit=None):
    """The gradients of the gate MLP from g = dLoss/d(vals_out) [nnz] in forward entry order (gcnx_pdn_operator_bwd); w, r as
    pdn_operator left them.  ``a`` carries its transposed pattern (DeviceCSR.transpose_perm)."""
    d, he = _pdn_mlp(e, w1, b1, w2, b2)
    rp_t, ci_t, pm = a.transpose_perm()
    assert min(w.size, g.size) >= a.nnz and r.size >= a.n
    assert dw1.size == d * he and db1.size == he and dw2.size == he and db2.size == 1 and dw1.contiguous
    assert scratch.size >= pdn_bwd_scratch_floats(ctx, a.n, a.nnz, d, he)
    assert unit is None or (unit.dtype == np.uint8 and unit.size >= a.nnz)
    ctx._ck(ctx.lib.gcnx_pdn_operator_bwd(ctx.h, a.rowptr.ptr, a.colidx.ptr, rp_t.ptr, ci_t.ptr, pm.ptr, a.n, a.nnz, _p(e), e.ld, d,
                                          _p(w1), _p(b1), _p(w2), _p(b2), he, unit.ptr if unit is not None else None, _p(w), _p(r),
                                          _p(g), _p(dw1), _p(db1), _p(dw2), _p(db2), _p(scratch)))


def bn_act_pool(ctx, seg, z, mean, inv, gamma, beta, pooled, argmax, act="prelu_shared", alpha=None, mode="max"):
    """pooled[g] = max over graph g's rows of act(BN(z)) and its argmax rows, in one pass (gcnx_bn_act_pool)."""
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act_pool(ctx.h, seg.dev.ptr, seg.n_graphs, _p(z), z.ld, f, _p(mean), _p(inv), _p(gamma), _p(beta),
                                     L.ACTS[act], _p(alpha), L.POOLS[mode], _p(pooled), pooled.ld, argmax.ptr))
    return pooled


def bn_act_pool_bwd(ctx, seg, dpooled, argmax, z, mean, inv, gamma, beta, dz, act="prelu_shared", alpha=None, dgamma=None,
                    dbeta=None, dalpha=None, mode="max"):
    """dZ and the BN / PReLU parameter gradients from dPooled (gcnx_bn_act_pool_bwd)."""
    n, f = z.shape
    ctx._ck(ctx.lib.gcnx_bn_act_pool_bwd(ctx.h, seg.dev.ptr, seg.n_graphs, _p(dpooled), dpooled.ld, argmax.ptr, _p(z), z.ld, n, f,
                                         _p(mean), _p(inv), _p(gamma), _p(beta), L.ACTS[act], _p(alpha), L.POOLS[mode], _p(dz),
                                         dz.ld, _p(dgamma), _p(dbeta), _p(dalpha)))
    return dz


def bn_act_pool_bwd_stats(ctx, seg, dpooled, argmax, z, mean, inv, gamma, beta, sums, act="prelu_shared", alpha=None, dgamma=None,
                          dbeta=None, dalpha=None, mode="max"):
    """First launch of bn_act_pool_bwd (sync-BN): the three LOCAL column sums -> sums[3f] and the local parameter gradients
    (gcnx_bn_act_pool_bwd_stats)."""
    f = z.shape[1]
    ctx._ck(ctx.lib.gcnx_bn_act_pool_bwd_stats(ctx.h, seg.dev.ptr, seg.n_graphs, _p(dpooled), dpooled.ld, argmax.ptr, _p(z), z.ld, f,
                                               _p(mean), _p(inv), _p(gamma), _p(beta), L.ACTS[act], _p(alpha), L.POOLS[mode],
                                               _p(sums), _p(dgamma), _p(dbeta), _p(dalpha)))


def bn_act_pool_bwd_apply(ctx, seg, dpooled, argmax, z, mean, inv, gamma, beta, sums, count, dz, act="prelu_shared", alpha=None,
                          mode="max"):
    """Second launch: dZ over the local rows from the (all-reduced) sums and the global row count
    (gcnx_bn_act_pool_bwd_apply)."""
    f = z.shape[1]
    ctx._ck(ctx.lib.gcnx_bn_act_pool_bwd_apply(ctx.h, seg.dev.ptr, seg.n_graphs, _p(dpooled), dpooled.ld, argmax.ptr, _p(z), z.ld, f,
                                               _p(mean), _p(inv), _p(gamma), _p(beta), L.ACTS[act], _p(alpha), L.POOLS[mode],
                                               _p(sums), float(count), _p(dz), dz.ld))
    return dz


def bce_head_scratch_floats(ctx, b, h):
    return int(ctx.lib.gcnx_bce_head_scratch_floats(int(b), int(h)))


def bce_head_args(pooled, p, scratch, out, probs, y=None, loss_acc=None, denom=None, g=None, dpooled=None, eps=TORCH_BN_EPS):
    """gcnx_bce_head_args.  p / g: dicts of the head's parameters / gradients ("w3", "b3", "g3", "be3", "a3", "w4", ...;
    w3 [h, h] and w4 [1, h] in torch's [out, in] layout).  y: labels [b, 2] one-hot (t = y[:, 1]), [b, 1] or [b]
    (t = y[:, 0] / y); None for the forward alone.  g (needs y): the gradients are written."""
    b, h = pooled.shape
    if y is not None:
        stride = y.shape[1] if len(y.shape) == 2 else 1
        col = 1 if stride == 2 else 0
        if stride > 2:
            raise ValueError(f"binary labels are [B], [B, 1] or one-hot [B, 2], got {tuple(y.shape)}")
    else:
        stride, col = 1, 0
    gp = (lambda k: _p(g[k])) if g is not None else (lambda k: None)
    return L.BceHeadArgs(
        _p(pooled), pooled.ld, b, h, _p(p["w3"]), _p(p["b3"]), _p(p["g3"]), _p(p["be3"]), _p(p["a3"]),
        _p(p["w4"]), _p(p["b4"]), _p(p["g4"]), _p(p["be4"]), _p(p["a4"]), float(eps), float(denom if denom else b),
        _p(y), stride, col, 1 if g is not None else 0, _p(out), _p(probs), _p(loss_acc),
        _p(dpooled), dpooled.ld if dpooled is not None else 0,
        gp("w3"), gp("b3"), gp("g3"), gp("be3"), gp("a3"), gp("w4"), gp("b4"), gp("g4"), gp("be4"), gp("a4"),
        _p(scratch), scratch.size)


def bn_prelu_bce_head(ctx, args):
    """The post-pool half of the torch GCN in one launch (gcnx_bn_prelu_bce_head); args from bce_head_args."""
    ctx._ck(ctx.lib.gcnx_bn_prelu_bce_head(ctx.h, C.byref(args)))


def bce_head_phase_scratch_floats(ctx, b, h):
    return int(ctx.lib.gcnx_bce_head_phase_scratch_floats(int(b), int(h)))


def bce_head_phase_red_floats(ctx, h):
    return int(ctx.lib.gcnx_bce_head_phase_red_floats(int(h)))


def bce_head_phase_slice(phase, h):
    """(offset, length) of the slice of `red` that phase `phase` of gcnx_bce_head_phase leaves for the all-reduce (include/gcnx.h),
    None after phase 6."""
    return ((0, h), (h, h), (2 * h, 1), (2 * h + 1, 1), (2 * h + 2, 2), (2 * h + 4, 2 * h), None)[phase]


def bce_head_phase(ctx, args, phase, count, red):
    """One phase of the head over a graph shard (gcnx_bce_head_phase): args from bce_head_args with the LOCAL rows, count = the
    global row count, red: device float[bce_head_phase_red_floats(h)] whose phase slice the caller all-reduces before the next
    phase."""
    ctx._ck(ctx.lib.gcnx_bce_head_phase(ctx.h, C.byref(args), int(phase), float(count), _p(red)))

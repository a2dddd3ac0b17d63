"""Models on the hot path.

``GCN2``: GCNConv(F->H, relu) -> GCNConv(H->H, relu) -> GlobalSumPool -> Dense(H->C) softmax,
categorical cross-entropy, SGD -- the "2-layer GCNConv + global pool" topology the reference
defines at gcn_utills.py:805-808,832-842 written with the Spektral layers the live script uses,
driven exactly like the reference's train_step / evaluate (src/scripts/gcn.py:328-340,
342-362): forward, CategoricalCrossentropy, gradients of every trainable variable, SGD apply,
mean categorical accuracy.  BN-free, so an N-GPU step equals the 1-GPU step.

The step is a fixed sequence of libgcnx calls on preallocated buffers; after one eager run it
is captured into a HIP graph (the role tf.function plays at gcn.py:328) and replayed.

``GCN``: the reference's torch class (gcn_utills.py:795-853): GCNConv·BatchNorm1d·PReLU twice, global_max_pool,
Linear·BatchNorm1d·PReLU twice, one logit with BCEWithLogitsLoss (eager launches).

``SAGE``: ``GCN`` with PyG's SAGEConv(aggr="mean") in the place of both GCNConv layers, the step the reference's author notes
above them (gcn_utills.py:804-806); one launch per convolution (csrc/sage.hip).

``GIN``: ``GCN`` with PyG's GINConv(Sequential(Linear, ReLU, Linear), train_eps) in the place of both GCNConv layers: sum
aggregation and a two-layer MLP, one launch per convolution (csrc/gin.hip).
``GINE``: ``GIN`` with PyG's GINEConv(edge_dim): every message is relu(x_j + lin(e_ij)), the cheapest way to read the edge
features (csrc/gine.hip); trains from the same batches as ``ResGated``.

``RGCN``: ``GCN`` with PyG's RGCNConv(num_relations, aggr="mean", root_weight) in the place of both GCNConv layers: the contacts and
the DCA bridges, which the edge features tell apart, get weights of their own; all relations from one gather (csrc/rgcn.hip).

``PNA``: ``GCN`` with PyG's PNAConv(mean / min / max / std, identity / amplification / attenuation) in the place of both
GCNConv layers: four statistics of every neighbourhood from one gather (csrc/pna.hip).

``GAT``: ``GCN`` with PyG's GATConv(heads, concat=True) in the place of both GCNConv layers: a softmax over the stored
entries of every row with learned scores (csrc/gat.hip).

``GATv2``: ``GCN`` with PyG's GATv2Conv(heads, concat=True, edge_dim) in the place of both GCNConv layers: attention whose scores
read the dca / proximity edge features (csrc/gatv2.hip); trains from DeviceDataset(edge_features=True) batches.
``ResGated``: ``GCN`` with PyG's ResGatedGraphConv(edge_dim, root_weight) in the place of both GCNConv layers: per-channel sigmoid
gates that read target, source and edge features (csrc/resgated.hip); trains from the same batches.
``Transformer``: ``GCN`` with PyG's TransformerConv(heads, beta, edge_dim, root_weight) in the place of both GCNConv layers: scaled
dot-product attention whose keys and values carry the edge features (csrc/transformer.hip); trains from the same batches.

``TopKNet``: GCNConv -> TopKPool -> GCNConv -> global pool -> Dense(softmax), with the pooling layer the reference's script imports
(gcn.py:10); selection, gather and the induced adjacency on the device (csrc/topk.hip), eager launches.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

from . import convs
from . import device as D
from .layers import glorot_uniform
from .loader import SparseTensor
from .params import block_views, from_pyg, join_blocks, to_pyg


class DeviceBatch:
    """A DisjointLoader batch resident in HBM: x [N,F] fp32, adjacency CSR, graph segments,
    one-hot labels y [B,C] fp32; optionally edge features e [nnz, S] fp32, row k belonging to stored entry k of the CSR.
    ax (optional, [N,F] fp32): the aggregated features A x of this batch, bit for bit what the one-launch GCNConv forward
    writes as its S output (DeviceDataset(aggregate_x=True) gathers it per batch); GCN2's first layer then runs without a
    gather.

    Contract: ``x`` and ``a`` are not modified in place once a model has seen the batch -- the cached transpose of ``a``
    assumes it, and so does GCN2, which keeps S1 = A x of the batch it is stepping on from one step to the next.  A caller
    that does overwrite ``x`` calls ``invalidate()`` afterwards."""

    _next_uid = 0
    unit = None                          # gcnx.PDN: uint8 [nnz] on the device, 1 on the loops it added to a host adjacency (else None)

    def __init__(self, ctx, x, a, seg, y=None, e=None, ax=None):
        self.ctx, self.x, self.a, self.seg, self.y, self.e, self.ax = ctx, x, a, seg, y, e, ax
        assert ax is None or ax.shape == x.shape
        DeviceBatch._next_uid += 1
        self.uid = DeviceBatch._next_uid  # never reused (unlike id()): keys captured graphs
        self.n, self.f = x.shape
        self.n_graphs = seg.n_graphs

    def invalidate(self):
        """After ``x`` was overwritten in place: the batch takes a fresh uid, so that every model drops the graphs it
        captured for it and whatever it derived from the old ``x`` (GCN2's kept S1); ``ax`` no longer matches and is dropped."""
        DeviceBatch._next_uid += 1
        self.uid = DeviceBatch._next_uid
        self.ax = None

    @classmethod
    def from_host(cls, ctx, inputs, y=None, normalize=None, weighted=True, symmetric=None):
        """inputs = (x, a, i) or (x, a, e, i) as yielded by DisjointLoader.  ``a`` is a SparseTensor (COO) or a
        scipy sparse matrix.  normalize='spektral'|'pyg' applies gcn_filter on the device (the
        CSR must then hold every diagonal entry, as the reference's self-looped graphs do).
        e [nnz, S]: one row per stored entry of ``a`` in row-major order (gcnx_coo_to_csr keeps that order, so CSR entry k
        is COO entry k); kept as ``batch.e``.  Any other row count -- one row per undirected edge, or rows for explicitly
        stored zeros, which the COO build drops -- raises ValueError."""
        e = None
        if len(inputs) == 4:
            x, a, e, i = inputs
        else:
            x, a, i = inputs
        n = x.shape[0]
        seg = i if isinstance(i, D.Segments) else D.Segments.from_ids(ctx, i)
        dx = ctx.to_device(x, np.float32)
        if isinstance(a, D.DeviceCSR):
            csr = a
        else:
            if not isinstance(a, SparseTensor):
                from .loader import sp_matrix_to_sp_tensor
                a = sp_matrix_to_sp_tensor(a)
            csr = D.DeviceCSR.from_coo(ctx, a.indices, a.values, n, graph_ptr=seg.host, symmetric=symmetric,
                                       weighted=weighted)
        if normalize:
            csr = csr.gcn_norm(normalize)
        dy = ctx.to_device(y, np.float32) if y is not None else None
        de = None
        if e is not None:
            e = np.asarray(e)
            if e.ndim != 2 or e.shape[0] != csr.nnz:
                raise ValueError(f"edge features e have shape {e.shape}: expected one row per stored entry of the adjacency "
                                 f"({csr.nnz} entries, row-major; from_networkx(use_edge_data='entries') builds them so)")
            de = ctx.to_device(e, np.float32) if e.shape[0] else ctx.empty((0, e.shape[1]))
        return cls(ctx, dx, csr, seg, dy, de)


def _without_e(inputs):
    """(x, a, e, i) -> (x, a, i): the models that do not read edge features take the loader's output as it is, as
    spektral.models.GeneralGNN does, whatever rows e has (the reference's use_edge_data=True gives one per undirected edge)."""
    return (inputs[0], inputs[1], inputs[-1]) if len(inputs) == 4 else inputs


class _Capacity:
    """Grow-only device storage behind per-batch views.  A streamed epoch brings a new (N, B) with every batch;
    re-allocating the activations per step (tens of MB) cost more than the step itself."""

    def __init__(self, ctx):
        self.ctx, self.store = ctx, {}

    def view(self, name, rows, width, dtype=np.float32, zero=False):
        need = int(rows) * int(width)
        cur = self.store.get(name)
        if cur is None or cur.size < need or cur.dtype != np.dtype(dtype):
            size = max(need, int(1.25 * cur.size) if cur is not None else 0, 1)
            cur = (self.ctx.zeros if zero else self.ctx.empty)(size, dtype)
            self.store[name] = cur
        return D.DeviceArray._view(cur, 0, (int(rows), int(width)))


_CAPTURE_FAILED_GCN2 = ("gcnx: RCCL all-reduce could not be captured into the step graph ({}); falling back to an eager "
                        "collective between two graphs")
_CAPTURE_FAILED_SYNC_BN = "gcnx: the sync-BN step could not be captured with its collectives ({}); running it eagerly"


class _GraphRunner:
    """The training-step protocol of the four models (GCN2, GeneralGNN, GCN, ECCNet), and the graph replay under it.

    A model provides:
      __init__          ctx, comm (or None), use_graph, prec, cce_train / cce_eval, built = False, _bufs = None, _graphs = {}
      build             its parameters: _alloc_flat(entries, align), or its own placement in flat_p / flat_g (+ 2 floats)
      _as_batch         its own lines around _adopt (what it passes to DeviceBatch.from_host, what it checks)
      _ensure           the buffer list of one batch shape, as views from _views()
      _forward, _backward                       the launches
      __call__, loss_and_grads, train_step, evaluate_batch     the sequence of the above; public signatures are the model's
      get_weights, set_weights, gradients, trainable_variables
      uses_edge_features = True                 if it reads DeviceBatch.e
    and inherits:
      _adopt            a DeviceBatch as it is (labels attached late), host inputs through DeviceBatch.from_host
      _views            the grow-only capacity behind the per-batch views (self._cap)
      _alloc_flat       n_params, flat_p, flat_g, p, g, loss_acc: packed, or every tensor on a 4-float boundary
      _bind, _run, _drop_graphs                 eager once, then capture, then replay; graphs die with their batch
      _lr_key           the learning rate as a device scalar
      _multi, _comm_in_graph                    more than one rank; the collectives recorded into the step graph
      _run_with_comm_fallback                   _run; a capture that fails with the collectives inside falls back for good
      _global_counts_cached, _global_graphs     sync-BN: the global (N, B, ...) of a batch, one host all-reduce per batch
      set_optimizer, _apply_sgd                 the update: one gcnx_sgd launch, or the launches of a gcnx.optim optimizer
      _finish_step, fetch_metrics, _loss_acc_host, stash_metrics, collect_metrics     what a step and an evaluation return
      losses            [] (no regularisers: gcn.py:335 adds sum(model.losses))"""

    use_graph = True
    uses_edge_features = False           # ECCNet: True.  Everyone else takes (x, a, e, i) and drops e (_adopt, gcnx.fit / gcnx.evaluate)
    comm = None
    _cap = None
    _counts_uid = None
    _comm_capture_failed = False

    # ---- batches, storage, parameters ---------------------------------------------------------------------------------
    def _adopt(self, inputs, target=None, **from_host_kw):
        """A DeviceBatch as it is (``target`` uploaded if it carries no labels yet); host inputs through DeviceBatch.from_host."""
        if isinstance(inputs, DeviceBatch):
            if target is not None and inputs.y is None:
                inputs.y = self.ctx.to_device(target, np.float32)
            return inputs
        if not self.uses_edge_features:
            inputs = _without_e(inputs)
        return DeviceBatch.from_host(self.ctx, inputs, target, **from_host_kw)

    def _views(self):
        """``view(name, rows, width, dtype, zero)`` of this model's grow-only storage (created on first use)."""
        if self._cap is None:
            self._cap = _Capacity(self.ctx)
        return self._cap.view

    def _alloc_flat(self, entries, align=1):
        """One flat parameter and one flat gradient buffer (single all-reduce, single SGD launch); the tensors of ``entries``
        -- ordered (key, shape) -- are views p[key] / g[key], each on a multiple of ``align`` floats (padding has zero gradients:
        the update leaves it at zero).  The gradients end in two extra floats, ``loss_acc`` = (loss sum, correct count), which
        so ride in the same all-reduce.  Returns {key: offset}."""
        offs, off = {}, 0
        for k, shape in entries:
            offs[k] = off
            off += -(-int(np.prod(shape)) // align) * align
        self.n_params = off
        self.flat_p = self.ctx.zeros(off)
        self.flat_g = self.ctx.zeros(off + 2)
        self.p, self.g = {}, {}
        for k, shape in entries:
            n = int(np.prod(shape))
            self.p[k] = self.flat_p.flat(offs[k], n, shape)
            self.g[k] = self.flat_g.flat(offs[k], n, shape)
        self.loss_acc = self.flat_g.flat(off, 2)
        return offs

    @property
    def losses(self):
        return []  # no regularisers (gcn.py:335 adds sum(model.losses))

    # ---- more than one rank --------------------------------------------------------------------------------------------
    def _multi(self):
        return self.comm is not None and self.comm.world_size > 1

    def _comm_in_graph(self):
        """Multi-GPU: the step's collectives are recorded INTO the step graph (RCCL enqueues on the ctx stream and
        supports stream capture), so a sharded step is one graph launch -- gradient kernels, ncclAllReduce, SGD --
        instead of graph | eager collective | graph (two graph boundaries around a 0.14 ms step).  Falls back to
        that form if the communicator cannot be captured (the thread-rank test transport) or a capture
        with a collective inside ever fails."""
        return (self.use_graph and self._multi() and getattr(self.comm, "capturable", False)
                and not self._comm_capture_failed)

    def _run_with_comm_fallback(self, tag, seq, fused_comm, message, retry):
        """_run(tag, seq).  If it raises with the collectives inside (``fused_comm``): from now on they stay outside the
        graphs (every rank runs the same software, so every rank lands here together) -- returns ``retry()``, the step
        entered again; None if the step ran."""
        try:
            self._run(tag, seq)
        except Exception as e:
            if not fused_comm:
                raise
            print(message.format(e), file=sys.stderr)
            self._comm_capture_failed = True
            self._drop_graphs()
            return retry()
        return None

    def _global_counts_cached(self, batch, values):
        """Sync-BN: [n, b(, ranks without a graph)] of this rank's shard summed over the ranks, as {"n", "b"(, "empty")}:
        one host round trip per BATCH (cached by its uid), not per step."""
        if self._counts_uid != batch.uid:
            tot = self.comm.allreduce_host(values, "sum")
            self._counts = {k: float(t) for k, t in zip(("n", "b", "empty"), tot)}
            self._counts_uid = batch.uid
        return self._counts

    def _global_graphs(self, batch):
        """Graphs of the whole batch: what the cached global counts say where the batch is a rank's shard."""
        return self._counts["b"] if self._multi() else batch.n_graphs

    # ---- the end of a step ---------------------------------------------------------------------------------------------
    _opt = None                          # a gcnx.optim optimizer (set_optimizer), or None: plain SGD

    def set_optimizer(self, opt):
        """Put a gcnx.Adam / gcnx.SGD behind this model's update (None: plain SGD again, the launches of a model that never
        had one).  Before or after build(); the optimizer's state is allocated once the model is built.  Captured graphs
        hold the state pointers and the update's launches: they are dropped."""
        self._opt = opt
        self._drop_graphs()
        if opt is not None and self.built:
            opt.bind(self)

    def _apply_sgd(self, lr):
        """The update of a step.  Without an optimizer the one gcnx_sgd launch; with one its step count, the norm launch if it
        clips, and its update launch (gcnx.optim), on the gradients every rank holds after the all-reduce."""
        if self._opt is None:
            D.sgd(self.ctx, self.flat_p, self.flat_g.flat(0, self.n_params), lr)
        else:
            self._opt.step(self, lr)

    def _finish_step(self, fetch, n_graphs):
        """What train_step returns.  fetch: True -> (loss, acc); False -> None; "stash" -> None, the metrics kept on the
        device for collect_metrics()."""
        if fetch == "stash":
            self.stash_metrics(n_graphs)
            return None
        if not fetch:
            return None
        return self.fetch_metrics(n_graphs)

    def fetch_metrics(self, n_graphs):
        """(loss, accuracy over ``n_graphs``) of the last step or evaluation: one device -> host copy, which waits for it."""
        la = self.loss_acc.numpy()
        return float(la[0]), float(la[1]) / float(n_graphs)

    _loss_acc_host = fetch_metrics                           # (evaluate_batch's name for the same read)

    def _bind(self, batch):
        """Captured graphs hold the pointers of one batch: drop them when the batch changes."""
        if getattr(self, "_bound_uid", None) != batch.uid:
            for tag in [t for t in self._graphs if t[0] != "sgd"]:
                g = self._graphs.pop(tag)
                if not isinstance(g, str):
                    g.destroy()
            self._bound_uid = batch.uid

    def _run(self, tag, fn):
        """Run fn eagerly the first time (sizes the workspace), then capture + replay."""
        if not self.use_graph:
            fn()
            return
        st = self._graphs.get(tag)
        if st is None:
            fn()
            self._graphs[tag] = "warm"
        elif st == "warm":
            self._graphs[tag] = self.ctx.capture(fn)
            self._graphs[tag].launch()
        else:
            st.launch()

    # ---- metrics without a host round trip per step ---------------------------------------------------------------
    _MRING = 1024

    def stash_metrics(self, n_graphs):
        """After train_step(..., fetch=False): keep this step's (loss, hit count) on the device -- an 8-byte copy in
        stream order -- instead of reading it back; collect_metrics() returns the stashed steps.  A loop that reads
        loss and accuracy after every step waits for the GPU every step, and the GPU then waits for the host to queue
        the next one: the reference's loop only uses them at the end of the epoch (gcn.py:375-377)."""
        if getattr(self, "_mring", None) is None:
            self._mring, self._mcount, self._mdone = self.ctx.zeros(2 * self._MRING), [], []
        if len(self._mcount) == self._MRING:
            self._mdone.extend(self._read_ring())
        k = len(self._mcount)
        self.ctx._ck(self.ctx.lib.gcnx_d2d(self.ctx.h, self._mring.ptr + 8 * k, self.loss_acc.ptr, 8))
        self._mcount.append(float(n_graphs))

    def _read_ring(self):
        la = self._mring.numpy().reshape(-1, 2)[:len(self._mcount)]
        out = [(float(l), float(h) / n) for (l, h), n in zip(la, self._mcount)]
        self._mcount = []
        return out

    def collect_metrics(self):
        """[(loss, accuracy)] of the steps stashed since the last call (one device -> host copy)."""
        if getattr(self, "_mring", None) is None:
            return []
        out = self._mdone + self._read_ring()
        self._mdone = []
        return out

    # ---- the learning rate as a device scalar --------------------------------------------------------------------------
    # A rate passed by value is an argument of the captured update launch: one graph per VALUE (the reference's
    # PiecewiseConstantDecay has three, gcn.py:321-325; a schedule that moves every step would capture every step).  With the
    # rate in a device scalar (gcnx_set_lr_source) one captured step serves them all and a new value costs a 4-byte queued copy.
    lr_on_device = os.environ.get("GCNX_LR_DEVICE", "1") != "0"

    def _lr_key(self, lr):
        """Announce this step's rate; returns what the captured graphs are keyed on ("dev", or the value itself)."""
        if not self.lr_on_device or lr is None:
            self.ctx.set_lr_source(None)
            return lr
        if getattr(self, "_lr_buf", None) is None:
            self._lr_buf, self._lr_val = self.ctx.zeros(1), None
        self.ctx.set_lr_source(self._lr_buf)                # (a ctx can serve several models: each step names its own source)
        if self._lr_val != float(lr):
            self._lr_buf.copy_from_host(np.asarray([lr], np.float32), wait=False)
            self._lr_val = float(lr)
        return "dev"

    def _drop_graphs(self):
        for g in getattr(self, "_graphs", {}).values():
            if not isinstance(g, str):
                g.destroy()
        self._graphs = {}


class GCN2(_GraphRunner):
    PARAM_ORDER = ("w1", "b1", "w2", "b2", "w3", "b3")

    @D.with_default_context
    def __init__(self, ctx, n_labels=2, hidden=None, pool="sum", prec="f32", seed=0, comm=None, use_graph="auto",
                 cce_train="logits", cce_eval="probs"):
        """cce_train / cce_eval: which branch of keras.backend.categorical_crossentropy the loss follows (see
        gcnx_cce_mode in include/gcnx.h).  train_step runs under tf.function (gcn.py:328-335), where Keras swaps the
        Softmax op's output for its input and calls softmax_cross_entropy_with_logits ("logits": no clip, gradient
        (p - y)/B everywhere); evaluate() is eager (gcn.py:351-354) and, on TF < 2.6, takes the renormalise-and-clip
        branch ("probs").  cce_eval="logits" is the TF >= 2.6 behaviour (the output carries _keras_logits).  The
        reference pins neither TensorFlow nor Spektral, so both stay selectable: PARITY UNPINNED."""
        self.ctx, self.n_labels, self.hidden, self.pool, self.prec = ctx, int(n_labels), hidden, pool, prec
        self.cce_train, self.cce_eval = cce_train, cce_eval
        self.comm = comm                     # gcnx.comm.Communicator or None
        # use_graph: True -- every step replays ONE captured HIP graph (the tf.function of gcn.py:328); False -- eager launches;
        # "auto" (default, r4): eager where the step is the five launches of the one-launch layers (E. coli-sized batches, F <= 128,
        # binary labels, one process), captured everywhere else.  Back-to-back replays of a graph leave ~10 us between the last
        # kernel of one and the first of the next on this runtime; five eager launches per step keep the queue full from Python
        # and have no such boundary: config 2 0.1020 -> 0.0948 ms per step on the same box (the 12-to-88-launch steps of large
        # batches and of GeneralGNN are host-bound when issued eagerly: there the graph wins).
        self._graph_opt = use_graph
        self.use_graph = use_graph is not False
        # tuning knobs (diagnostics; DESIGN section 7: the knob list), read ONCE here -- the sequence a model runs never changes under it
        self._knob = {"fold": os.environ.get("GCNX_FOLD", "1") != "0", "duo": os.environ.get("GCNX_DUO", "1") != "0",
                      "fused": os.environ.get("GCNX_FUSED", "1") != "0", "side": int(os.environ.get("GCNX_SIDE", "1")),
                      "head_late": os.environ.get("GCNX_HEAD_LATE", "1") != "0",
                      "s_order": os.environ.get("GCNX_S_ORDER", "1") != "0",
                      "buckets": os.environ.get("GCNX_COMM_BUCKETS", "1") != "0",
                      "act16": os.environ.get("GCNX_ACT16", "1") != "0",
                      "pool_in_spmm": os.environ.get("GCNX_POOL_IN_SPMM", "1") != "0",
                      "mask8": os.environ.get("GCNX_MASK8", "1") != "0",
                      "ax_reuse": os.environ.get("GCNX_AX_REUSE", "1") != "0"}
        self._s1_uid = None                  # uid of the batch whose S1 = A X bufs["s1"] holds (one-launch route), or None
        self.dw2_plans_built = 0             # slice plans of gemm_dw2_graph built so far (_dw2_graph_plan): tests read it
        self._rng = np.random.default_rng(seed)
        self.built = False
        self._bufs = None
        self._graphs = {}

    # ---- parameters: one flat buffer (single all-reduce, single SGD launch) -----------------
    def build(self, f_in):
        h = self.hidden or f_in
        c = self.n_labels
        self.f_in, self.hidden = f_in, h
        shapes = {"w1": (f_in, h), "b1": (h,), "w2": (h, h), "b2": (h,), "w3": (h, c), "b3": (c,)}
        self._alloc_flat([(k, shapes[k]) for k in self.PARAM_ORDER])       # packed: _bucket_split() counts on it
        init = {"w1": glorot_uniform(self._rng, f_in, h), "w2": glorot_uniform(self._rng, h, h),
                "w3": glorot_uniform(self._rng, h, c)}
        for k, v in init.items():
            self.p[k].copy_from_host(v)
        self.built = True

    def get_weights(self):
        return [self.p[k].numpy() for k in self.PARAM_ORDER]

    def set_weights(self, weights):
        for k, w in zip(self.PARAM_ORDER, weights):
            self.p[k].copy_from_host(np.asarray(w, np.float32).reshape(self.p[k].shape))

    @property
    def trainable_variables(self):
        return [self.p[k] for k in self.PARAM_ORDER]

    # ---- buffers for one batch shape ---------------------------------------------------------
    def _ensure(self, batch):
        """Activation buffers for this batch shape.  Storage is grow-only capacity (a streamed epoch brings a new
        (N, B) with every batch: re-allocating ~60 MB per step cost more than the step); the returned arrays are
        views of exactly the batch's shape."""
        if not self.built:
            self.build(batch.f)
        key = (batch.n, batch.n_graphs)
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        n, b, h, c = batch.n, batch.n_graphs, self.hidden, self.n_labels
        self._drop_graphs()
        self._s1_uid = None                                     # new views, possibly new storage: no S1 is kept across this
        v = self._views()
        self._bufs = {"key": key}
        for k in ("h", "y1", "y2", "dz", "h2", "dz2"):          # h2 / dz2: the side section still reads h / dz
            self._bufs[k] = v(k, n, h)
        if self._fused(batch):                                  # one-launch layers: S1 = A X, S2 = A Y1 (operands of dW)
            self._bufs["s1"], self._bufs["s2"] = v("s1", n, self.f_in), v("s2", n, h)
            self._bufs["w2t"] = v("w2t", h, h)                  # W2^T, a by-product of layer 2's forward launch
            # [Y2 > 0] as bytes: what the backward launch gathers.  NOTE: a train_step on the head-late route then does not
            # store the fp32 "y2" at all -- the buffer keeps whatever an earlier loss_and_grads / forward call left in it
            # (GCNX_MASK8=0 only turns that gather back to fp32 rows: the image is still what dW2's mask products read)
            self._bufs["y2m8"] = v("y2m8", n, h, np.uint8)
            # head inside the backward: the pool's per-tile partial sums / positive counts (layer 2's launch writes them)
            # and the per-graph totals (the backward launch does)
            tr = D.pool_tile_rows(n, b)
            self._bufs["tp_part"], self._bufs["tp_cnt"] = v("tp_part", tr, h), v("tp_cnt", tr, h)
            self._bufs["pool_sum"], self._bufs["pool_cnt"] = v("pool_sum", b, h), v("pool_cnt", b, h)
        elif self._s_order():
            self._bufs["s1"] = v("s1", n, self.f_in)            # S1 = A X: layer 1 evaluated as (A X) W1, dW1 = S1^T dZ1
        for k, w in (("pooled", h), ("probs", c), ("dpooled", h)):
            self._bufs[k] = v(k, b, w)
        self._bufs["arg"] = v("arg", b, h, np.int32) if self.pool == "max" else None
        return self._bufs

    # ---- the call sequences --------------------------------------------------------------------
    def _forward(self, batch, bufs, with_loss, denom, train=False):
        ctx, p, prec = self.ctx, self.p, self.prec
        bufs["_mask8"] = bufs["_dw2_mask8"] = None
        if self._fused(batch):
            # small-feature regime: each GCNConv is one launch, evaluated as (A X) W (gcnx_gcn_conv_fwd); A X is kept
            # for the weight gradient when a backward pass follows
            keep = with_loss == "grads"
            late = keep and self._head_late(batch)
            # S1 = A X holds no trainable parameter: a constant of the batch.  Given with the batch (batch.ax, gathered by the
            # loader) or still in bufs["s1"] from the last gradient step on this very batch, layer 1 is the product and the
            # epilogue alone (gcnx_gcn_conv_fwd_pre: same bits, no gather); otherwise the gathering launch, which writes S1 --
            # and only a pass that writes it marks it valid (GCNX_AX_REUSE=0: the gather every step)
            if self._s1_uid != batch.uid:
                self._s1_uid = None                             # another batch runs through the model
            s1 = None
            if self._knob["ax_reuse"]:
                s1 = batch.ax if batch.ax is not None else (bufs["s1"] if self._s1_uid is not None else None)
            if s1 is not None:
                D.gcn_conv_fwd_pre(ctx, s1, p["w1"], p["b1"], bufs["y1"], act="relu", prec=prec)
            else:
                D.gcn_conv_fwd(ctx, batch.a, batch.x, p["w1"], p["b1"], bufs["y1"], act="relu", s=bufs["s1"] if keep else None,
                               prec=prec)
                if keep and self._knob["ax_reuse"]:
                    self._s1_uid = batch.uid
            bufs["_s1"] = s1 if s1 is not None else bufs["s1"]  # the S operand of dW1
            # with a backward pass to follow, layer 2's launch also writes [Y2 > 0] as bytes: the backward launch only tests
            # Y2 for > 0 and gathers the byte image instead (a quarter of the bytes and of the loads; GCNX_MASK8=0: fp32 rows).
            # In a training step with the head folded in nothing else reads Y2: its fp32 store is dropped (loss_and_grads
            # keeps it, and so does every route whose pool or head is a launch of its own).
            m8 = bufs["y2m8"] if keep and self._knob["mask8"] else None
            bufs["_mask8"] = m8
            # The same image is the 0/1 operand of dW2's mask products (gcnx_gemm_dw2_graph), whatever the backward launch
            # gathers: where that route serves the batch the launch writes it with GCNX_MASK8=0 too (beside the fp32 Y2), so
            # the knob changes the gather and not one bit of the step.
            img = m8
            if keep and self._dw2_graph_plan(batch) is not None:
                img = bufs["_dw2_mask8"] = bufs["y2m8"]
            D.gcn_conv_fwd(ctx, batch.a, bufs["y1"], p["w2"], p["b2"], None if (m8 is not None and train and late) else bufs["y2"],
                           act="relu", s=bufs["s2"] if keep else None, wt=bufs["w2t"] if keep else None, prec=prec,
                           pool=(batch.seg, bufs["tp_part"], bufs["tp_cnt"]) if late else None, mask8=img)
        else:
            bufs["act16"] = False
            if self._s_order() and self._act16_try(batch, with_loss):
                # bf16 STORAGE of what only bf16-operand weight GEMMs read (r3): with prec = "bf16" every weight GEMM rounds its
                # operands to bfloat16 as it loads them, so S1 = A X and Y1 (read by the two products of layer 2's kernel and
                # by the two weight-gradient products) are stored rounded -- the same bits in every result, half the bytes in
                # the aggregation's output, in both operands of dW1 / dW2 and in the input of three of the five GEMMs.
                s16 = self._cap.view("s1_16", batch.n, self.f_in, np.uint16)
                if D.spmm_bf16out(ctx, batch.a, batch.x, None, s16):          # (False: the tile kernels do not serve this batch)
                    y16 = self._cap.view("y1_16", batch.n, self.hidden, np.uint16)
                    bufs["y1bits"] = self._cap.view("y1bits", batch.n, 16, np.int32) if with_loss == "grads" else None
                    # the bf16 images of the step's three weight operands (W1 and W2 forward, W2 for dX) in one launch
                    bufs["wimg"] = D.stream_images(ctx, [(p["w1"], True), (p["w2"], True), (p["w2"], False)],
                                                   self._cap.view("wimg", 3, 65536, np.uint16))
                    if not (D.gemm_fwd_bf16(ctx, s16, p["w1"], p["b1"], y16, act="relu", bits=bufs["y1bits"], wimg=bufs["wimg"][0])
                            and D.gemm_fwd_bf16(ctx, y16, p["w2"], None, bufs["h"], wimg=bufs["wimg"][1])):
                        raise RuntimeError("gcnx: the streaming bf16 GEMM refused a shape the bf16-storage path was chosen for")
                    bufs["act16"], bufs["y1bits_ok"], bufs["s1_16"], bufs["y1_16"] = True, with_loss == "grads", s16, y16
            if bufs["act16"]:
                pass
            elif self._s_order():
                # layer 1 as (A X) W1: the same product as GCNConv's A (X W1), two launches either way -- but the layer's
                # input needs no gradient, so with S1 = A X kept dW1 = S1^T dZ1 and the backward pass has no aggregation
                # for this layer (one of the step's four, 575 us of 4.7 ms at config 3)
                D.spmm(ctx, batch.a, batch.x, None, bufs["s1"])
                # with a backward pass to follow and the streaming bf16 kernel serving the product: [Y1 > 0] also as a bit
                # image, which the dX launch of the backward pass reads instead of Y1 (1 GB -> 32 MB at config 3)
                bufs["y1bits_ok"] = False
                if (with_loss == "grads" and prec in ("bf16", "bf16x3") and self.hidden == 256 and self.f_in == 256
                        and batch.n >= 32768):            # (the streaming kernel's shape: K = 256 too)
                    bufs["y1bits"] = self._cap.view("y1bits", batch.n, 16, np.int32)     # grow-only storage, stable pointers
                    bufs["y1bits_ok"] = D.gemm_relu_bits(ctx, bufs["s1"], p["w1"], p["b1"], bufs["y1"], bufs["y1bits"], prec=prec)
                if not bufs["y1bits_ok"]:
                    D.gemm(ctx, bufs["s1"], p["w1"], p["b1"], bufs["y1"], act="relu", prec=prec)
            else:
                D.gemm(ctx, batch.x, p["w1"], None, bufs["h"], prec=prec)
                D.spmm(ctx, batch.a, bufs["h"], p["b1"], bufs["y1"], act="relu")
            if not bufs["act16"]:
                D.gemm(ctx, bufs["y1"], p["w2"], None, bufs["h"], prec=prec)
            # pooled layer on the tile kernels with a backward pass to follow: its launch also writes [Y2 > 0] as a bit
            # image, which the folded backward aggregation expands instead of reading Y2 again (1 GB -> 32 MB at config 3)
            bufs["y2bits_ok"] = bufs["pool_done"] = False
            if (self._fold(batch) and batch.a.plan is not None and self.hidden % 32 == 0
                    and (with_loss == "grads" or self._knob["pool_in_spmm"])):                 # (forward-only passes too: evaluate())
                bufs["y2bits"] = self._cap.view("y2bits", batch.n, self.hidden // 32, np.int32)
                # ... and on tile graphs the launch leaves the pooled rows and positive counts too: Y2 is neither written
                # nor read back by a pool launch there (r3; rows of the graphs taller than a tile are, as before)
                if self._knob["pool_in_spmm"] and not self._head_late(batch):
                    bufs["pool_cnt2"] = self._cap.view("pool_cnt2", batch.n_graphs, self.hidden)
                    bufs["pool_done"] = D.spmm_relu_bits_pool(ctx, batch.a, bufs["h"], p["b2"], bufs["y2"], bufs["y2bits"], batch.seg,
                                                              bufs["pooled"], bufs["pool_cnt2"], self.pool)
                bufs["y2bits_ok"] = bufs["pool_done"] or (with_loss == "grads" and
                                                          D.spmm_relu_bits(ctx, batch.a, bufs["h"], p["b2"], bufs["y2"], bufs["y2bits"]))
            if not bufs["y2bits_ok"]:
                D.spmm(ctx, batch.a, bufs["h"], p["b2"], bufs["y2"], act="relu")
        # Global pool, then Dense(softmax) + CCE + accuracy + the head gradients in one launch; with few graphs the
        # head also combines the pool's row-slice partial sums (gcnx_pool_dense_softmax_cce)
        head = dict(mode=self.pool, argmax=bufs["arg"])
        bufs["_head_late"] = None
        if with_loss == "grads" and self._head_late(batch):
            # one-launch layers with a backward pass to follow: neither a pool nor a head launch here.  Layer 2's launch
            # left the pool's per-tile partial sums; the backward aggregation adds them up and evaluates dPooled per graph
            # itself, and the rest of the head (probabilities, loss, accuracy, dW3, db3, db2 -- leaves) rides in the
            # weight-gradient launch: the pool's 7 us and the head's 10 are off the critical path.
            bufs["_head_late"] = D.head_args(batch.seg, bufs["tp_part"], bufs["tp_cnt"], bufs["pool_sum"], bufs["pool_cnt"], p["w3"],
                                             p["b3"], batch.y, denom, bufs["probs"], self.loss_acc, self.g["w3"], self.g["b3"],
                                             self.g["b2"], bufs["pooled"], bufs["dpooled"], mode=self.pool, cce=self.cce_train)
        elif with_loss == "grads" and bufs.get("pool_done"):
            D.pooled_dense_softmax_cce(ctx, batch.seg, bufs["pooled"], bufs["pool_cnt2"], p["w3"], p["b3"], batch.y, bufs["probs"],
                                       self.loss_acc, denom, dw=self.g["w3"], db=self.g["b3"], dpooled=bufs["dpooled"], mode=self.pool,
                                       db_relu=self.g["b2"], cce=self.cce_train)
        elif with_loss == "grads":
            # db2 rides along when the backward folds pool' into the aggregation (dZ2 is never materialised there)
            D.pool_dense_softmax_cce(ctx, batch.seg, bufs["y2"], bufs["pooled"], p["w3"], p["b3"], batch.y, bufs["probs"],
                                     self.loss_acc, denom, dw=self.g["w3"], db=self.g["b3"], dpooled=bufs["dpooled"],
                                     db_relu=self.g["b2"] if self._fold(batch) else None, cce=self.cce_train, **head)
        elif bufs.get("pool_done"):       # evaluate() / a plain forward: the head on the pooled rows the aggregation left
            D.pooled_dense_softmax_cce(ctx, batch.seg, bufs["pooled"], None, p["w3"], p["b3"], batch.y if with_loss else None, bufs["probs"],
                                       self.loss_acc if with_loss else None, denom, mode=self.pool, cce=self.cce_eval)
        elif with_loss:
            D.pool_dense_softmax_cce(ctx, batch.seg, bufs["y2"], bufs["pooled"], p["w3"], p["b3"], batch.y, bufs["probs"],
                                     self.loss_acc, denom, cce=self.cce_eval, **head)
        else:
            D.pool_dense_softmax_cce(ctx, batch.seg, bufs["y2"], bufs["pooled"], p["w3"], p["b3"], None, bufs["probs"], **head)

    def _backward(self, batch, bufs, lr=None, buckets=False):
        """All gradients; with ``lr`` (single process) the SGD step too -- returns True if it was applied here.
        buckets (multi-GPU): the gradient all-reduce is issued from here in two buckets where the sequence allows it
        (the two-launch layers of large batches); ``self._reduced_in_backward`` tells the caller."""
        ctx, p, g, prec = self.ctx, self.p, self.g, self.prec
        self._reduced_in_backward = False
        at = batch.a.transpose()
        # The gradient leaves of layer 2 (db2, dW2: nothing later in the backward pass reads them) run in ONE side
        # section, concurrently with the main chain dX -> db1 -> A^T -> dW1.  One fork and one join per step: each
        # costs ~10 us of cross-queue signalling, which is why there are not three sections.  The buffers the side
        # section reads (dz, h) stay unmodified until the join: the main chain continues in dz2 / h2.
        side = self._knob["side"]                      # tuning knob GCNX_SIDE: 0 = serial, 1 = one section, 7 = three sections
        if side != 1:
            return self._backward_knob(batch, bufs, 0 if side == 0 else 7)
        # SUM / AVG pooling: dZ2 = pool'(dPooled) * [Y2 > 0] is never materialised -- the aggregation gathers the mask
        # from Y2 (row gather in the latency regime, masked LDS tiles with a plan) and scales by the graph's dPooled
        # vector; db2 counts the mask (in the head with few graphs, gcnx_pool_bwd_colsum on the side stream otherwise).
        fold = self._fold(batch)
        if self._fused(batch):
            # pool' + ReLU' + A^T + W2^T + ReLU' in one launch (dZ2 and dZ1 out, db1 partials pending; db2 came out of
            # the head), then both weight gradients -- dW1 = S1^T dZ1, dW2 = S2^T dZ2 -- and the update in the last two
            ha = bufs.get("_head_late")
            # dZ2 = [Y2 > 0] * pool'(dPooled)[graph] is a 0/1 image scaled per graph and column: dW2 = sum_g dP_g * (S2_g^T mask_g) comes
            # from the byte image on the bf16 MFMA with exact products (gcnx_gemm_dw2_graph), the backward launch then does not
            # store dZ2 at all.  Decided BEFORE that launch; what the route does not serve runs the sequence below it.
            plan = self._dw2_graph_plan(batch) if bufs.get("_dw2_mask8") is not None else None
            pend = D.gcn_conv_bwd_pool(ctx, at, bufs["y2"], batch.seg, None if ha is not None else bufs["dpooled"], p["w2"], bufs["y1"],
                                       None if plan is not None else bufs["dz"], bufs["dz2"], db1=g["b1"], mode=self.pool,
                                       scratch=self._defer_scratch(batch), w2t=bufs["w2t"], prec=prec, head=ha, mask8=bufs.get("_mask8"))
            if plan is not None:
                upd = lr is not None
                if not D.gemm_dw2_graph(ctx, bufs["_s1"], bufs["dz2"], g["w1"], bufs["s2"], bufs["_dw2_mask8"], g["w2"], plan, bufs["dpooled"],
                                        mode=self.pool, params=self.flat_p if upd else None, grads=self.flat_g.flat(0, self.n_params),
                                        lr=lr if upd else 0.0, pending=pend, leaf=ha):
                    raise RuntimeError("gcnx: gcnx_gemm_dw2_graph refused a call gcnx_gemm_dw2_graph_ok had accepted")
                return upd
            if lr is None:
                D.gemm_dw2(ctx, bufs["_s1"], bufs["dz2"], g["w1"], bufs["s2"], bufs["dz"], g["w2"], prec="f32",
                           grads=self.flat_g.flat(0, self.n_params), pending=pend, leaf=ha)
                return False
            D.gemm_dw2(ctx, bufs["_s1"], bufs["dz2"], g["w1"], bufs["s2"], bufs["dz"], g["w2"], prec="f32", params=self.flat_p,
                       grads=self.flat_g.flat(0, self.n_params), lr=lr, pending=pend, leaf=ha)
            return True
        act16 = bool(bufs.get("act16"))
        dh16 = self._cap.view("dh2_16", batch.n, self.hidden, np.uint16) if act16 else None
        dh16_done = False
        if fold and act16 and bufs.get("y2bits_ok"):
            dh16_done = D.spmm_pool_bwd_bf16out(ctx, at, bufs["y2"], batch.seg, bufs["dpooled"], dh16, self.pool, y_bits=bufs["y2bits"])
        if dh16_done:
            pass                                                                # dH2 = A^T dZ2, stored as bf16
        elif fold:
            D.spmm_pool_bwd(ctx, at, bufs["y2"], batch.seg, bufs["dpooled"], bufs["h"], self.pool,
                            y_bits=bufs["y2bits"] if bufs.get("y2bits_ok") else None)                # dH2 = A^T dZ2
        else:
            D.segment_pool_bwd(ctx, batch.seg, bufs["dpooled"], bufs["dz"], self.pool, bufs["arg"], y=bufs["y2"])  # dZ2 (ReLU mask fused)
            D.spmm(ctx, at, bufs["dz"], None, bufs["h"])                       # dH2 = A^T dZ2
        if fold and batch.a.plan is None and self._knob["duo"]:
            # db2 came out of the head, and dW2 shares dX's launch (gcnx_dense_bwd): one stream, no fork / join --
            # the second stream's signalling cost 25 us of a 194 us step
            if lr is None:
                D.dense_bwd(ctx, bufs["y1"], bufs["h"], p["w2"], bufs["dz2"], g["w2"], prec=prec, y_mask=bufs["y1"],
                            db_prev=g["b1"])                                   # dW2, dZ1, db1
                if buckets:
                    self._allreduce_tail_bucket()                              # beside layer 1's dW (and its aggregation)
                xs, dh1 = self._layer1_dw_operands(batch, bufs, at)
                D.gemm_dw(ctx, xs, dh1, g["w1"], prec=prec)                    # dW1 = X^T (A^T dZ1) or S1^T dZ1
                if buckets:
                    self._allreduce_head_bucket()
                return False
            # With the update in the same step, the reductions that finish the leaves dW2 / db1 wait for the last
            # launch: the split-K reduction of dW1 folds them in and applies the SGD step to every parameter.
            pend = D.dense_bwd_deferred(ctx, bufs["y1"], bufs["h"], p["w2"], bufs["dz2"], g["w2"], self._defer_scratch(batch),
                                        prec=prec, y_mask=bufs["y1"], db_prev=g["b1"])
            xs, dh1 = self._layer1_dw_operands(batch, bufs, at)
            D.gemm_dw_sgd(ctx, xs, dh1, g["w1"], self.flat_p, self.flat_g.flat(0, self.n_params), lr, prec=prec,
                          pending=pend)
            return True
        # The side section pays only while the main chain still has layer 1's backward aggregation to run beside the
        # leaves.  With layer 1 in (A X) W1 order the chain is dX -> dW1, streaming GEMMs that share one bound (HBM, or
        # the fp32 MFMA) with dW2: on one stream the step measured 1-3 % faster at config 3 in every precision (4.12
        # against 4.21-4.25 ms in bf16), the same at config 5.
        if act16 and not dh16_done:
            D.to_bf16_into(ctx, bufs["h"], dh16)                                # (dH2 came from an fp32 path: the same rounding)
        with (contextlib.nullcontext() if "s1" in bufs else ctx.side()):
            if not fold:
                D.act_bias_grad(ctx, bufs["dz"], None, bufs["dz"], None, db=g["b2"])     # db2 = colsum(dZ2)
            # (folded: db2 came out of the head -- from the pool's own count of positive entries)
            if act16:
                self._must(D.gemm_dw_bf16(ctx, bufs["y1_16"], dh16, g["w2"]))   # dW2 = Y1^T dH2
            else:
                D.gemm_dw(ctx, bufs["y1"], bufs["h"], g["w2"], prec=prec)      # dW2 = Y1^T dH2
        if buckets:
            # Multi-GPU ("enqueue behind the layer-1 dW GEMM"): the gradients of layers 2 and 3
            # and the metric tail -- {dW2, db2, dW3, db3, loss, #correct}, the contiguous tail of the flat buffer -- are
            # final here, so their all-reduce runs on the side stream while layer 1's backward (dX, dW1: two of the step's
            # five weight GEMMs) runs on the main one; {dW1, db1} follows as a second bucket behind the join (collectives of
            # one communicator never overlap each other).  A transport that cannot be captured (the thread-rank test
            # communicator reduces through the host) issues the same two buckets in line.
            ctx.join()
            self._allreduce_tail_bucket()
        if act16:
            dz16 = self._cap.view("dz1_16", batch.n, self.hidden, np.uint16)
            self._must(D.gemm_dx_bf16(ctx, dh16, p["w2"], dz16, mask_bits=bufs["y1bits"], db=g["b1"], wimg=bufs["wimg"][2]))   # dZ1 (bf16), db1
            self._must(D.gemm_dw_bf16(ctx, bufs["s1_16"], dz16, g["w1"]))      # dW1 = S1^T dZ1
        else:
            D.gemm_dx(ctx, bufs["h"], p["w2"], bufs["dz2"], prec=prec, y_mask=bufs["y1"], db=g["b1"],
                      mask_bits=bufs["y1bits"] if bufs.get("y1bits_ok") else None)                   # dZ1, db1
            xs, dh1 = self._layer1_dw_operands(batch, bufs, at)
            D.gemm_dw(ctx, xs, dh1, g["w1"], prec=prec)                        # dW1 = X^T (A^T dZ1) or S1^T dZ1
        ctx.join()
        if buckets:
            self._allreduce_head_bucket()

    @staticmethod
    def _must(ok):
        if not ok:
            raise RuntimeError("gcnx: a bf16-storage kernel refused a shape its producer had accepted")

    def _act16_try(self, batch, with_loss):
        """bf16 storage of S1, Y1, dH2, dZ1 (the tensors only weight GEMMs read): a step -- training, or the forward pass of
        evaluate() -- with plain bf16 GEMM operands at the streaming kernels' shape, the aggregation on a tile plan.  The first producer (gcnx_spmm_csr_bf16out) has the
        last word.  GCNX_ACT16=0 keeps fp32 storage (same results, bit for bit: tested)."""
        return (self.prec == "bf16" and self._knob["act16"] and self.hidden == 256 and self.f_in == 256
                and batch.n >= 32768 and batch.a.plan is not None and batch.a.vals is not None and self._knob["side"] == 1)

    def _allreduce_tail_bucket(self):
        """{dW2, db2, dW3, db3, loss, #correct}: on the side stream (a second branch of a captured step) when the transport
        enqueues on a stream; in line otherwise."""
        off = self._bucket_split()
        tail = self.flat_g.flat(off, self.n_params + 2 - off)
        with (self.ctx.side() if getattr(self.comm, "capturable", False) else contextlib.nullcontext()):
            self.comm.allreduce_sum(tail)

    def _allreduce_head_bucket(self):
        """{dW1, db1}, behind the join: collectives of one communicator never overlap each other."""
        self.ctx.join()
        self.comm.allreduce_sum(self.flat_g.flat(0, self._bucket_split()))
        self._reduced_in_backward = True

    def _bucket_split(self):
        """First element of the all-reduce's second-layer bucket in the flat gradient buffer: [w1, b1 | w2, b2, w3, b3, loss, acc]."""
        return int(np.prod(self.p["w1"].shape)) + int(np.prod(self.p["b1"].shape))

    def _s_order(self):
        """Layer 1 as (A X) W1 in the two-launch (non-fused) paths: when the aggregation is not wider that way (F <= H)."""
        return self._knob["s_order"] and self.built and self.f_in <= self.hidden

    def _layer1_dw_operands(self, batch, bufs, at):
        """The two operands of dW1 with dZ1 in bufs["dz2"]: (S1, dZ1) when the forward kept S1 = A X, otherwise
        (X, A^T dZ1) -- after the backward aggregation of layer 1."""
        if "s1" in bufs and not self._fused(batch):
            return bufs["s1"], bufs["dz2"]
        D.spmm(self.ctx, at, bufs["dz2"], None, bufs["h2"])                    # dH1 = A^T dZ1
        return batch.x, bufs["h2"]

    def _defer_scratch(self, batch):
        """Device buffer that holds the deferred partial results of layer 2's dense backward (grow-only)."""
        need = max(D.dense_bwd_scratch_floats(self.ctx, batch.n, self.hidden, self.hidden),
                   D.gcn_conv_bwd_scratch_floats(self.ctx, batch.n, self.hidden))
        cur = getattr(self, "_defer_buf", None)
        if cur is None or cur.size < need:
            self._defer_buf = self.ctx.empty(max(need, 4))
        return self._defer_buf

    def _fold(self, batch):
        """SUM / AVG pooling: pool' and the ReLU mask fold into the backward aggregation (dZ2 is never materialised) and
        db2 = sum_g dPooled[g] * #[Y2_g > 0] comes out of the head (few graphs) or of gcnx_pool_bwd_colsum."""
        return (self.pool in ("sum", "avg") and self.hidden % 4 == 0 and (batch.a.plan is None or self.hidden % 32 == 0)
                and self._knob["fold"] and self._knob["side"] == 1)

    def _fused(self, batch):
        """The small-feature regime (config 2): every GCNConv and the backward from the pool down to dZ1 are single
        launches (csrc/fused.hip).  Needs the folded backward's conditions and F, H in {32, 64, 128}; prec "f32" (exact
        fp32 products) or "bf16x3" (split-bf16 products in the conv launches; the two weight gradients stay on the fp32
        MFMA -- sums over N rows, at least as accurate)."""
        route = batch.__dict__.setdefault("_route", {})      # asked several times per step: once per (batch, model)
        key = ("fused", id(self), self.prec, self.built, batch.a.plan is None)
        if key not in route:
            route[key] = bool(self.built and self._fold(batch) and self.prec in ("f32", "bf16x3") and self._knob["fused"]
                              and self._knob["duo"] and self.f_in in (32, 64, 128) and self.hidden in (32, 64, 128)
                              and D.gcn_conv_fused_ok(self.ctx, batch.n, self.f_in, self.hidden)
                              and D.gcn_conv_fused_ok(self.ctx, batch.n, self.hidden, self.hidden))
        return route[key]

    def _dw2_graph_plan(self, batch):
        """The slice plan of gcnx_gemm_dw2_graph for this batch, or None where the route does not serve the step (shapes, too
        many tiny graphs, the knob dw2_graph).  A constant of the batch, built on the host and uploaded once per
        batch uid -- before the step's launches, never inside a capture -- and kept WITH the batch (a captured step holds the
        table's address for as long as the batch lives); DeviceBatch.invalidate() gives the batch a new uid and so a new plan."""
        if not self._fused(batch):
            return None
        route = batch.__dict__.setdefault("_route", {})
        key = ("dw2_graph", id(self), batch.uid)
        if key not in route:
            route[key] = D.gemm_dw2_graph_plan(self.ctx, batch.seg, batch.n, self.f_in, self.hidden, self.hidden, self.hidden,
                                               mode=self.pool)
            self.dw2_plans_built += 1
        return route[key]

    def _head_late(self, batch):
        """One-launch layers (see _fused; SUM / AVG pooling), at most 2 classes (the reference's binary labels) and no graph
        without nodes: pool and classifier head are evaluated inside the forward / backward launches (gcnx_gcn_conv_fwd_pool,
        gcnx_head_args) instead of as launches between them."""
        return (self._knob["head_late"] and self._fused(batch) and self.n_labels <= 2 and batch.y is not None
                and not batch.seg.has_empty)

    def _backward_knob(self, batch, bufs, side):
        """The same backward with individual side sections switched off (GCNX_SIDE bits; measurement only)."""
        ctx, p, g, prec = self.ctx, self.p, self.g, self.prec
        at = batch.a.transpose()
        sec = lambda on: ctx.side() if on else contextlib.nullcontext()
        D.segment_pool_bwd(ctx, batch.seg, bufs["dpooled"], bufs["dz"], self.pool, bufs["arg"], y=bufs["y2"])
        with sec(side & 1):
            D.act_bias_grad(ctx, bufs["dz"], None, bufs["dz"], None, db=g["b2"])
        D.spmm(ctx, at, bufs["dz"], None, bufs["h"])
        ctx.join()
        with sec(side & 2):
            D.gemm_dw(ctx, bufs["y1"], bufs["h"], g["w2"], prec=prec)
        D.gemm_dx(ctx, bufs["h"], p["w2"], bufs["dz"], prec=prec, y_mask=bufs["y1"])
        ctx.join()
        with sec(side & 4):
            D.act_bias_grad(ctx, bufs["dz"], None, bufs["dz"], None, db=g["b1"])
        D.spmm(ctx, at, bufs["dz"], None, bufs["h"])
        D.gemm_dw(ctx, batch.x, bufs["h"], g["w1"], prec=prec)
        ctx.join()

    # ---- public surface: model(inputs, training=...) and train_step ------------------------
    def _as_batch(self, inputs, target=None):
        return self._adopt(inputs, target)                       # (the adjacency's values are read: weighted)

    def __call__(self, inputs, training=False):
        """model([x, a, i], training=False) -> probabilities [B, C] (gcn.py:351)."""
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._bind(batch)
        self._run(("fwd", batch.uid), lambda: self._forward(batch, bufs, False, None))
        return bufs["probs"].numpy()

    def loss_and_grads(self, inputs, target, global_batch=None, _lr=None):
        """Forward + loss + every gradient (no update unless ``_lr``).  Returns the device batch."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        denom = float(global_batch or batch.n_graphs)
        multi = self._multi()
        if self._graph_opt == "auto":
            self.use_graph = bool(multi or not (self._fused(batch) and self._head_late(batch)))
        fused_comm = multi and _lr is not None and self._comm_in_graph()

        # (the bucketed form needs the side stream inside the step: with a capturable communicator only when the collective
        # is recorded into the step graph anyway, or the step runs eagerly)
        buckets = multi and self._knob["buckets"] and (fused_comm or not self.use_graph)
        self._dw2_graph_plan(batch)                             # (an upload the first time a batch is seen: not inside a capture)

        def seq():
            self._forward(batch, bufs, "grads", denom, train=_lr is not None)
            # (an optimizer with state: the gradients-only route, then its own launches -- as the multi-rank step does)
            if self._backward(batch, bufs, None if (multi or self._opt is not None) else _lr, buckets=buckets):
                return
            if fused_comm and not self._reduced_in_backward:
                self.comm.allreduce_sum(self.flat_g)
            if _lr is not None and (fused_comm or not multi):
                # the update rides in the same captured graph (one graph launch per step)
                self._apply_sgd(_lr)
        self._bind(batch)
        self._step_applied = fused_comm or not multi
        lr_key = self._lr_key(_lr)
        # (a failed capture with the collective inside: from now on graph | all-reduce | graph)
        again = self._run_with_comm_fallback(
            ("grad", batch.uid, denom, lr_key if self._step_applied else None), seq, fused_comm, _CAPTURE_FAILED_GCN2,
            fused_comm and (lambda: self.loss_and_grads(batch, None, global_batch=global_batch, _lr=_lr)))
        if again is not None:
            return again
        if multi and not fused_comm and not self._reduced_in_backward:
            self.comm.allreduce_sum(self.flat_g)
        self._last_batch = batch
        self.ctx.set_lr_source(None)                      # (eager gcnx_sgd calls of other users of this ctx take their argument)
        return batch

    def train_step(self, inputs, target=None, lr=0.02, global_batch=None, fetch=True):
        """One optimisation step (gcn.py:330-340).  With a communicator the batch given here is
        this rank's shard and ``global_batch`` the number of graphs over all ranks."""
        batch = self.loss_and_grads(inputs, target, global_batch, _lr=float(lr))
        if not self._step_applied:
            self._run(("sgd", self._lr_key(float(lr))), lambda: self._apply_sgd(lr))
            self.ctx.set_lr_source(None)
        return self._finish_step(fetch, global_batch or batch.n_graphs)

    def evaluate_batch(self, inputs, target):
        """Forward + loss/acc only (the body of evaluate(), gcn.py:350-357)."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, True, float(batch.n_graphs))
        return (*self._loss_acc_host(batch.n_graphs), bufs["probs"].numpy())

    def gradients(self):
        return {k: self.g[k].numpy() for k in self.PARAM_ORDER}


def evaluate(model, loader, normalize=None):
    """The reference's evaluate(loader) (src/scripts/gcn.py:342-362).  One implementation: gcnx.train.evaluate."""
    from .train import evaluate as _evaluate
    return _evaluate(model, loader, normalize)


class GeneralGNN(_GraphRunner):
    """spektral.models.GeneralGNN -- the model the reference trains (src/scripts/gcn.py:320:
    ``GeneralGNN(dataset.n_labels, activation="softmax")``), SURVEY 8.A.3:

        pre-MLP(2) -> 4 x [z = GeneralConv(out); out = concat([z, out])] -> GlobalSumPool -> post-MLP(2)

    MLP layer = Dense -> BatchNormalization -> Dropout(0) -> PReLU (last post layer: softmax);
    GeneralConv = Dense -> BN -> PReLU -> sum-aggregation over a.indices (values ignored).
    Same constructor signature (activation "softmax" as gcn.py:320 passes it, or Spektral's default None = linear head); of
    the other options those listed in __init__ are built, anything else raises.  The skip concatenation is never materialised: every layer reads / writes a
    column slice of one [N, hidden*(message_passing+1)] buffer through leading-dimension views.
    Weights are exposed in Keras order per layer: kernel, bias, gamma, beta, moving_mean,
    moving_variance, alpha.  With a communicator (one process per GPU, a graph shard each) BatchNormalization is
    synchronised: the column sums of both moment passes and of the backward pass are all-reduced, so every rank
    normalises with the statistics of the GLOBAL batch, and the step equals the single-GPU step on the whole batch.
    """

    @D.with_default_context
    def __init__(self, ctx, output, activation=None, hidden=256, message_passing=4, pre_process=2, post_process=2,
                 connectivity="cat", batch_norm=True, dropout=0.0, aggregate="sum", hidden_activation="prelu", pool="sum",
                 prec="f32", seed=0, use_graph=True, comm=None, cce_train="logits", cce_eval="probs"):
        self.use_graph, self._graphs = use_graph, {}
        self.cce_train, self.cce_eval = cce_train, cce_eval     # see GCN2.__init__
        self.comm = comm                                  # gcnx.comm.Communicator: sync-BN + gradient all-reduce
        # activation: "softmax" (gcn.py:320) or None / "linear" (Spektral's own default: the last post layer ends with its
        # BatchNormalization, model(inputs) returns those logits).  A linear head is trained on the from-logits cross-entropy
        # -- CategoricalCrossentropy(from_logits=True), the only form defined on unnormalised outputs -- which is also what
        # tf.function makes of the softmax head (see GCN2.__init__), so the training step is the same launch sequence and
        # only what the model RETURNS differs.
        if activation == "linear":
            activation = None
        if activation not in ("softmax", None):
            raise NotImplementedError(f"GeneralGNN(activation={activation!r}): 'softmax' (gcn.py:320) and None are built")
        self.activation = activation
        if activation is None:
            self.cce_train = self.cce_eval = "logits"
        # Spektral's other options that map onto kernels that exist (r3; PARITY UNPINNED like the rest, the
        # oracle's restatement of them is checked against torch autograd): connectivity "sum" (out = z + out), batch_norm False
        # (no BatchNormalization layers), hidden_activation "relu" / None, dropout > 0 (the Dropout layer between
        # BatchNormalization and the activation of every MLP / GeneralConv layer; training only; this library's own generator)
        if connectivity not in ("cat", "sum"):
            raise NotImplementedError(f"GeneralGNN(connectivity={connectivity!r}): 'cat' (gcn.py:320) and 'sum' are built")
        if hidden_activation == "linear":
            hidden_activation = None
        if hidden_activation not in ("prelu", "relu", None):
            raise NotImplementedError(f"GeneralGNN(hidden_activation={hidden_activation!r}): 'prelu' (gcn.py:320), 'relu' and None are built")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"GeneralGNN(dropout={dropout!r}): a rate in [0, 1)")
        self.connectivity, self.batch_norm, self.dropout = connectivity, bool(batch_norm), float(dropout)
        self.hidden_activation, self.seed = hidden_activation, int(seed)
        # Spektral's other aggregations / pools that map onto kernels that exist (r3): aggregate "mean" is the same gather with
        # the weight 1 / (entries of the row) per entry, pool "avg" / "max" are modes of the segment pool and its backward
        # ("prod", r4: tf.math.unsorted_segment_prod and its zero-aware gradient -- every aggregation Spektral names is built)
        if aggregate not in ("sum", "mean", "max", "min", "prod"):
            raise ValueError(f"GeneralGNN(aggregate={aggregate!r}): Spektral's aggregations are 'sum' (gcn.py:320), 'mean', 'max', 'min', 'prod'")
        if pool not in ("sum", "avg", "max"):
            raise NotImplementedError(f"GeneralGNN(pool={pool!r}): 'sum' (gcn.py:320), 'avg' and 'max' are built")
        self.aggregate, self.pool = aggregate, pool
        self.ctx, self.output, self.hidden, self.mp = ctx, int(output), int(hidden), int(message_passing)
        self.n_pre, self.n_post, self.prec = int(pre_process), int(post_process), prec
        self._rng = np.random.default_rng(seed)
        self.built = False
        self._bufs = None
        self._images_fresh, self._img_jobs = False, []

    # ---- parameters ------------------------------------------------------------------------------
    def build(self, f_in):
        h, mp = self.hidden, self.mp
        dims = []                                         # (group, fan_in, fan_out, has_prelu)
        w = f_in
        for _ in range(self.n_pre):
            dims.append(("pre", w, h, True)); w = h
        cat, bn, prelu = self.connectivity == "cat", self.batch_norm, self.hidden_activation == "prelu"
        for k in range(mp):
            dims.append(("gnn", h * (k + 1) if cat else h, h, True))
        w = self._wpool = h * (mp + 1) if cat else h
        for k in range(self.n_post):
            last = k == self.n_post - 1
            dims.append(("post", w, self.output if last else h, not last)); w = h
        n_train = sum(fi * fo + fo + (2 * fo if bn else 0) + (fo if pr and prelu else 0) for _, fi, fo, pr in dims)
        n_state = sum(2 * fo for _, _, fo, _ in dims) if bn else 0
        self.n_params = n_train
        ctx = self.ctx
        self.flat_p, self.flat_g = ctx.zeros(n_train), ctx.zeros(n_train + 2)
        self.flat_s = ctx.zeros(max(n_state, 1))          # moving_mean | moving_var per layer
        self.loss_acc = self.flat_g.flat(n_train, 2)
        self.layers = []
        self._step_dev = ctx.zeros(1, np.int32)           # the optimizer's step count on the device (Dropout streams)
        off = soff = 0
        for grp, fi, fo, pr in dims:
            L = {"group": grp, "fi": fi, "fo": fo, "act": self.hidden_activation if pr else None, "index": len(self.layers)}
            for name, shape in (("kernel", (fi, fo)), ("bias", (fo,))) + ((("gamma", (fo,)), ("beta", (fo,))) if bn else ()) + \
                    ((("alpha", (fo,)),) if pr and prelu else ()):
                n = int(np.prod(shape))
                L[name] = self.flat_p.flat(off, n, shape)
                L["g_" + name] = self.flat_g.flat(off, n, shape)
                off += n
            L["sums"], L["scratch"] = ctx.zeros(2 * fo), ctx.zeros(3 * fo)
            L["kernel"].copy_from_host(glorot_uniform(self._rng, fi, fo))
            if bn:
                L["moving_mean"] = self.flat_s.flat(soff, fo); L["moving_var"] = self.flat_s.flat(soff + fo, fo); soff += 2 * fo
                L["mean"], L["inv"] = ctx.zeros(fo), ctx.zeros(fo)
                L["gamma"].copy_from_host(np.ones(fo, np.float32))
                L["moving_var"].copy_from_host(np.ones(fo, np.float32))
                L["bn_gamma"], L["bn_beta"], L["bn_g_gamma"], L["bn_g_beta"] = L["gamma"], L["beta"], L["g_gamma"], L["g_beta"]
            else:
                # batch_norm=False: the fused batch-norm + activation passes run with the identity transform (mean 0, 1 / sigma 1,
                # gamma 1, beta 0, inference-mode backward): exactly act(z) and dy * act'(z); nothing of it is a parameter
                L["mean"], L["inv"] = ctx.zeros(fo), ctx.to_device(np.ones(fo, np.float32))
                L["bn_gamma"], L["bn_beta"] = L["inv"], L["mean"]
                L["bn_g_gamma"], L["bn_g_beta"] = ctx.zeros(fo), ctx.zeros(fo)
            self.layers.append(L)
        self.f_in, self.built = f_in, True
        self._alloc_images()

    def _alloc_images(self):
        """bf16 / bf16x3: weight images (MFMA-fragment order, csrc/gemm_panel.hip) of every Dense layer that runs on node
        rows -- the operand of X W and, where the layer's input needs a gradient, of dH W^T.  One launch per step rewrites
        them all (the weights change with every update)."""
        self._img_jobs = []
        self._img_prec = self.prec
        if self.prec == "f32":
            return
        ctx = self.ctx
        for i, L in enumerate(self.layers):
            L.pop("img_fwd", None); L.pop("img_bwd", None)
            if L["group"] == "post" or L["fo"] % 16 or L["fi"] % 4:
                continue
            ef = D.wimage_elems(ctx, L["fi"], L["fo"], False, self.prec)
            L["img_fwd"] = ctx.empty(ef, np.uint16)
            self._img_jobs.append((L["kernel"], L["img_fwd"], False, self.prec))
            if i > 0 and L["fi"] % 16 == 0:
                L["img_bwd"] = ctx.empty(D.wimage_elems(ctx, L["fi"], L["fo"], True, self.prec), np.uint16)
                self._img_jobs.append((L["kernel"], L["img_bwd"], True, self.prec))

    WEIGHT_ORDER = ("kernel", "bias", "gamma", "beta", "moving_mean", "moving_var", "alpha")
    # Order of one layer's arrays in get_weights() / set_weights() (model.get_weights() at gcn.py:383 feeds the .npz dump;
    # PARITY UNPINNED: neither Keras nor Spektral is importable here, these restate their published code):
    #  "layer"  every layer as Dense -> BatchNormalization -> PReLU would list it: kernel, bias, gamma, beta, moving_mean,
    #           moving_variance, alpha.  That IS the Keras order for the pre / post MLPs (a Sequential of separate
    #           Dense / BN / Dropout / PReLU layers, each contributing layer.weights in turn).
    #  "keras"  (default) the same, except that GeneralConv is ONE Keras Layer with child layers: Layer.weights =
    #           trainable_weights + non_trainable_weights, and trainable_weights = the layer's own add_weight variables
    #           (kernel, bias) followed by its children's in attribute order (PReLU is created in __init__, Dropout and
    #           BatchNormalization in build): kernel, bias, alpha, gamma, beta | moving_mean, moving_variance.
    #  "keras_children_first"  the reading the round-1 review proposed (children's trainables before the layer's own):
    #           alpha, gamma, beta, kernel, bias | moving_mean, moving_variance.
    GNN_ORDERS = {"layer": WEIGHT_ORDER,
                  "keras": ("kernel", "bias", "alpha", "gamma", "beta", "moving_mean", "moving_var"),
                  "keras_children_first": ("alpha", "gamma", "beta", "kernel", "bias", "moving_mean", "moving_var")}

    def _weight_keys(self, L, order):
        keys = self.GNN_ORDERS[order] if L["group"] == "gnn" else self.WEIGHT_ORDER
        return [k for k in keys if k in L]

    def get_weights(self, order="keras"):
        return [L[k].numpy() for L in self.layers for k in self._weight_keys(L, order)]

    def set_weights(self, weights, order="keras"):
        it = iter(weights)
        for L in self.layers:
            for k in self._weight_keys(L, order):
                L[k].copy_from_host(np.asarray(next(it), np.float32).reshape(L[k].shape))

    @property
    def trainable_variables(self):
        return [L[k] for L in self.layers for k in ("kernel", "bias", "gamma", "beta", "alpha") if k in L]

    # ---- buffers ---------------------------------------------------------------------------------
    def _ensure(self, batch):
        if not self.built:
            self.build(batch.f)
        key = (batch.n, batch.n_graphs)
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        ctx, n, b, h = self.ctx, batch.n, batch.n_graphs, self.hidden
        self._drop_graphs()
        wcat = h * (self.mp + 1)
        v = self._views()
        wp = self._wpool
        bufs = {"key": key, "cat": v("cat", n, wcat), "dcat": v("dcat", n, wcat), "h": v("h", n, h), "dh": v("dh", n, h),
                "pooled": v("pooled", b, wp), "dpooled": v("dpooled", b, wp), "probs": v("probs", b, self.output),
                "dlogits": v("dlogits", b, self.output), "zy": v("zy", b, self.output, zero=True)}
        for i, L in enumerate(self.layers):
            rows = b if L["group"] == "post" else n
            bufs[f"z{i}"] = v(f"z{i}", rows, L["fo"])             # Dense output (pre-BN), kept for the backward pass
            bufs[f"y{i}"] = v(f"y{i}", rows, L["fo"])             # layer output where it is not a slice of `cat`
        self._bufs = bufs
        return bufs

    def _drop(self, L, t):
        """The layer's Dropout factor applied to t in place (forward: the activation's output -- act(s u) = s act(u) for the
        activations built; backward: the incoming gradient).  Stream = the layer's index, step = the device step count."""
        seed = self.seed + (0x9E37 * self.comm.rank if self._multi() else 0)
        D.dropout(self.ctx, t, self.dropout, seed, L["index"], self._step_dev)

    def _dense_bn(self, L, x, z, y, training):
        self._dense_bn_core(L, x, z, y, training)
        if training and self.dropout > 0.0:
            self._drop(L, y)

    def _dense_bn_core(self, L, x, z, y, training):
        ctx = self.ctx
        if not self.batch_norm:
            if not ("img_fwd" in L and self._images_fresh and
                    D.gemm_wimage(ctx, x, L["img_fwd"], L["fi"], L["fo"], z, bias=L["bias"], prec=self.prec) is not None):
                D.gemm(ctx, x, L["kernel"], L["bias"], z, prec=self._prec_of(L))
            D.bn_act(ctx, z, L["mean"], L["inv"], L["bn_gamma"], L["bn_beta"], y, act=L["act"], alpha=L.get("alpha"))
            return
        if "img_fwd" in L and self._images_fresh:
            # split-bf16 panel GEMM (csrc/gemm_panel.hip); in single-device training its epilogue also leaves the batch-norm
            # statistics of what it writes, as (rows, mean, M2) per workgroup: no pass over z for the moments
            fused_bn = training and not self._multi() and L["fo"] <= 256
            parts = self._bn_parts(x.shape[0], L["fo"]) if fused_bn else None
            nparts = D.gemm_wimage(ctx, x, L["img_fwd"], L["fi"], L["fo"], z, bias=L["bias"], prec=self.prec, bn_parts=parts)
            if nparts is not None:
                if fused_bn:
                    D.bn_finalize_parts(ctx, parts, nparts, L["mean"], L["inv"], L["moving_mean"], L["moving_var"])
                    D.bn_act(ctx, z, L["mean"], L["inv"], L["gamma"], L["beta"], y, act=L["act"], alpha=L.get("alpha"))
                    return
            else:
                D.gemm(ctx, x, L["kernel"], L["bias"], z, prec=self._prec_of(L))
        else:
            D.gemm(ctx, x, L["kernel"], L["bias"], z, prec=self._prec_of(L))
        if training and self._multi():
            # sync-BN: the two moment passes with their column sums all-reduced and the GLOBAL row count
            count = self._counts["b" if L["group"] == "post" else "n"]
            D.bn_stats(ctx, z, L["sums"])
            self.comm.allreduce_sum(L["sums"])
            D.bn_finalize(ctx, L["sums"], count, L["mean"], L["inv"])
            D.bn_stats(ctx, z, L["sums"], shift=L["mean"])
            self.comm.allreduce_sum(L["sums"])
            D.bn_finalize(ctx, L["sums"], count, L["mean"], L["inv"], L["moving_mean"], L["moving_var"], shift=L["mean"])
        elif training:
            D.bn_moments(ctx, z, L["sums"], L["mean"], L["inv"], L["moving_mean"], L["moving_var"])
        else:
            D.bn_finalize(ctx, None, 1, L["mean"], L["inv"], L["moving_mean"], L["moving_var"])
        D.bn_act(ctx, z, L["mean"], L["inv"], L["gamma"], L["beta"], y, act=L["act"], alpha=L.get("alpha"))

    def _agg_operator(self, batch):
        """The aggregation's operator: the 0 / 1 pattern of a (aggregate = "sum"), or the same pattern with 1 / (entries of
        the row) on every entry ("mean": tf.math.unsorted_segment_mean over a row's messages), built once per batch."""
        return batch.a.row_mean() if self.aggregate == "mean" else batch.a.unweighted()     # ("max" / "min": the pattern only)

    def _forward(self, batch, bufs, training):
        h, mp = self.hidden, self.mp
        cat = bufs["cat"]
        a = self._agg_operator(batch)                     # GeneralConv ignores adjacency values (8.A.4)
        x = batch.x
        li = 0
        for k in range(self.n_pre):
            L = self.layers[li]
            y = cat.cols(mp * h, (mp + 1) * h) if k == self.n_pre - 1 else bufs[f"y{li}"]
            self._dense_bn(L, x, bufs[f"z{li}"], y, training)
            x = y; li += 1
        sumc = self.connectivity == "sum"          # "sum": slice (mp - k) of `cat` holds out_k = z_k + out_(k-1) instead of z_k
        for k in range(mp):
            L = self.layers[li]
            inp = cat.cols((mp - k) * h, (mp - k + 1) * h if sumc else (mp + 1) * h)
            minmax = self.aggregate in ("max", "min", "prod")
            # ("max" / "min": the layer's messages, its aggregate and the tie counts are kept for the gradient in per-layer
            # buffers -- `h` is reused by the next layer, the `cat` slice summed over with connectivity "sum")
            hk = self._tmp(bufs, f"msg{li}", (batch.n, h)) if minmax else bufs["h"]
            self._dense_bn(L, inp, bufs[f"z{li}"], hk, training)
            new = cat.cols((mp - k - 1) * h, (mp - k) * h)
            if minmax:                                    # tf.math.unsorted_segment_max / _min over a row's messages
                ck = self._tmp(bufs, f"aggcnt{li}", (batch.n, h))
                zk = self._tmp(bufs, f"agg{li}", (batch.n, h)) if sumc else new
                D.spmm_minmax(self.ctx, a, hk, zk, ck, self.aggregate)
                if sumc:
                    D.add(self.ctx, zk, inp, new)
            else:
                D.spmm(self.ctx, a, bufs["h"], None, new)
                if sumc:
                    D.add(self.ctx, new, inp, new)
            li += 1
        if self.pool == "max":
            bufs["pool_arg"] = self._views()("pool_arg", bufs["pooled"].shape[0], bufs["pooled"].shape[1], np.int32)
        D.segment_pool(self.ctx, batch.seg, cat.cols(0, h) if sumc else cat, bufs["pooled"], self.pool,
                       bufs.get("pool_arg") if self.pool == "max" else None)
        x = bufs["pooled"]
        for k in range(self.n_post):
            L = self.layers[li]
            self._dense_bn(L, x, bufs[f"z{li}"], bufs[f"y{li}"], training)
            x = bufs[f"y{li}"]; li += 1
        return x                                          # [B, output]: BN output = the softmax logits

    def _bwd_dense_bn(self, L, dy, x, z, dx, training, accumulate=False):
        ctx = self.ctx
        dz = dy                                            # in place
        if training and self.dropout > 0.0:
            self._drop(L, dy)                              # Dropout backward: the forward's factor on the incoming gradient
        bn = self.batch_norm
        if not bn:
            D.bn_act_bwd(ctx, dy, z, L["mean"], L["inv"], L["bn_gamma"], L["bn_beta"], dz, L["scratch"], act=L["act"],
                         alpha=L.get("alpha"), training=False, dgamma=L["bn_g_gamma"], dbeta=L["bn_g_beta"],
                         dalpha=L.get("g_alpha"))
        elif training and self._multi():
            # local column sums -> parameter gradients (summed over ranks by the final all-reduce with the rest);
            # the same sums, all-reduced, and the global row count give dz
            count = self._counts["b" if L["group"] == "post" else "n"]
            D.bn_act_bwd_stats(ctx, dy, z, L["mean"], L["inv"], L["gamma"], L["beta"], L["scratch"], act=L["act"],
                               alpha=L.get("alpha"), dgamma=L["g_gamma"], dbeta=L["g_beta"], dalpha=L.get("g_alpha"))
            self.comm.allreduce_sum(L["scratch"])
            D.bn_act_bwd_apply(ctx, dy, z, L["mean"], L["inv"], L["gamma"], L["beta"], L["scratch"], count, dz,
                               act=L["act"], alpha=L.get("alpha"), training=True)
        else:
            D.bn_act_bwd(ctx, dy, z, L["mean"], L["inv"], L["gamma"], L["beta"], dz, L["scratch"], act=L["act"],
                         alpha=L.get("alpha"), training=training, dgamma=L["g_gamma"], dbeta=L["g_beta"],
                         dalpha=L.get("g_alpha"))
        if training and bn:
            # The Dense bias under a training-mode BatchNorm has the gradient sum_rows dz = gamma inv (sum g - n mean(g) -
            # mean(g xhat) sum xhat) = 0 identically (sum xhat = 0; with sync-BN the sums are the global ones): TensorFlow
            # evaluates that sum and returns rounding noise of order 1e-8; every training path here writes the exact value
            # instead of passing over dz once more (14 column-sum launches per step in the fp32 configuration).
            pass                                           # (loss_and_grads zeroes the whole flat gradient buffer once per step)
        else:
            D.act_bias_grad(ctx, dz, None, dz, None, db=L["g_bias"])
        if "img_fwd" in L and self._images_fresh and (dx is None or "img_bwd" in L):
            D.gemm_dw(ctx, x, dz, L["g_kernel"], prec=self.prec)           # (fi = 256 p: panels of the streaming kernel)
            if dx is None:
                return
            if D.gemm_wimage(ctx, dz, L["img_bwd"], L["fi"], L["fo"], dx, transpose=True, prec=self.prec, accumulate=accumulate) is not None:
                return
            D.gemm_dx(ctx, dz, L["kernel"], dx, prec=self.prec, accumulate=accumulate)
            return
        prec = self._prec_of(L)
        if dx is not None and not accumulate:
            # both products of the layer in one launch pair (gcnx_dense_bwd; falls back inside for ragged widths)
            D.dense_bwd(ctx, x, dz, L["kernel"], dx, L["g_kernel"], prec=prec)
        else:
            D.gemm_dw(ctx, x, dz, L["g_kernel"], prec=prec)
            if dx is not None:
                D.gemm_dx(ctx, dz, L["kernel"], dx, prec=prec, accumulate=accumulate)

    def _backward(self, batch, bufs, training=True):
        h, mp = self.hidden, self.mp
        cat, dcat = bufs["cat"], bufs["dcat"]
        at = self._agg_operator(batch).transpose()
        n_layers = len(self.layers)
        li = n_layers - 1
        d = bufs["dlogits"]                               # d(BN output of the last layer) from softmax+CCE
        for k in reversed(range(self.n_post)):
            L = self.layers[li]
            x = bufs["pooled"] if k == 0 else bufs[f"y{li - 1}"]
            dx = bufs["dpooled"] if k == 0 else bufs[f"y{li - 1}"]     # y of the previous layer is dead: reuse as its dY
            if k > 0:
                dx = self._tmp(bufs, f"dy{li - 1}", x.shape)
            self._bwd_dense_bn(L, d, x, bufs[f"z{li}"], dx, training)
            d = dx; li -= 1
        sumc = self.connectivity == "sum"
        D.segment_pool_bwd(self.ctx, batch.seg, bufs["dpooled"], dcat.cols(0, h) if sumc else dcat, self.pool,
                           bufs.get("pool_arg") if self.pool == "max" else None)
        for k in reversed(range(mp)):
            L = self.layers[li]
            dout = dcat.cols((mp - k - 1) * h, (mp - k) * h)
            if self.aggregate in ("max", "min", "prod"):
                zk = bufs[f"agg{li}"] if sumc else cat.cols((mp - k - 1) * h, (mp - k) * h)
                D.spmm_minmax_bwd(self.ctx, at, bufs[f"msg{li}"], zk, bufs[f"aggcnt{li}"], dout, bufs["dh"], self.aggregate)
            else:
                D.spmm(self.ctx, at, dout, None, bufs["dh"])
            if sumc:                                       # d out_(k-1) = d out_k (the skip) + dz W^T
                inp, din = cat.cols((mp - k) * h, (mp - k + 1) * h), dcat.cols((mp - k) * h, (mp - k + 1) * h)
                self._bwd_dense_bn(L, bufs["dh"], inp, bufs[f"z{li}"], din, training)
                D.add(self.ctx, din, dout, din)
            else:
                inp = cat.cols((mp - k) * h, (mp + 1) * h)
                self._bwd_dense_bn(L, bufs["dh"], inp, bufs[f"z{li}"], dcat.cols((mp - k) * h, (mp + 1) * h), training,
                                   accumulate=True)
            li -= 1
        d = dcat.cols(mp * h, (mp + 1) * h)
        for k in reversed(range(self.n_pre)):
            L = self.layers[li]
            x = batch.x if k == 0 else bufs[f"y{li - 1}"]
            dx = None if k == 0 else self._tmp(bufs, f"dy{li - 1}", x.shape)
            self._bwd_dense_bn(L, d, x, bufs[f"z{li}"], dx, training)
            d = dx; li -= 1

    def _prec_of(self, L):
        """Arithmetic of a layer's products outside the panel kernels: the post-MLP runs on B rows (32 graphs): a few MFLOP
        for which the bf16 tile kernels' operand images cost more than the products (28 us per launch against the fp32
        tiles' few) -- exact fp32 there."""
        return "f32" if L["group"] == "post" else self.prec

    def _bn_parts(self, rows, fo):
        """Scratch for one layer's batch-norm parts [(rows, mean, M2) x workgroups x fo] (consumed before the next layer runs)."""
        need = 3 * max(D.gemm_wimage_parts(self.ctx, rows), 1) * fo
        cur = getattr(self, "_bn_parts_buf", None)
        if cur is None or cur.size < need:
            self._bn_parts_buf = self.ctx.empty(need)
        return self._bn_parts_buf

    def _prepare_images(self):
        """The weight images of this step's forward and backward products, all in one launch."""
        if getattr(self, "_img_prec", None) != self.prec:       # (the precision was switched after build)
            self._alloc_images()
        self._images_fresh = bool(self._img_jobs)
        if self._img_jobs:
            D.wimage_prepare(self.ctx, self._img_jobs)

    def _tmp(self, bufs, key, shape):
        if key not in bufs or bufs[key].shape != tuple(shape):
            shape = tuple(shape) if len(shape) == 2 else (1, int(np.prod(shape)))
            bufs[key] = self._views()("tmp_" + key, shape[0], shape[1])
            if len(shape) != 2:
                bufs[key] = bufs[key].flat(0, shape[1])
        return bufs[key]

    # ---- public surface ----------------------------------------------------------------------------
    def _as_batch(self, inputs, target=None):
        return self._adopt(inputs, target, weighted=False)       # (GeneralConv ignores the adjacency's values)

    def __call__(self, inputs, training=False):
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._prepare_images()
        logits = self._forward(batch, bufs, training)
        if self.activation is None:                        # linear head: the last BatchNormalization's output
            return logits.numpy()
        la = self._tmp(bufs, "la_scratch", (2,))
        la.fill_zero()
        D.softmax_cce(self.ctx, logits, bufs["zy"], bufs["probs"], la, None, None)
        return bufs["probs"].numpy()

    def loss_and_grads(self, inputs, target=None, _lr=None, global_batch=None):
        """Forward (training=True) + loss + every gradient.  With a communicator the batch is this rank's shard:
        the loss is normalised by ``global_batch`` graphs, BatchNorm runs on the global statistics, and one
        all-reduce sums the flat gradient buffer (+ loss / accuracy tail) over the ranks."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        multi = self._multi()
        denom = float(global_batch or batch.n_graphs)
        if multi:
            counts = self._global_counts_cached(batch, [batch.n, batch.n_graphs])      # sync-BN reads them (self._counts)
            denom = float(global_batch or counts["b"])
        # with a capturable communicator (RCCL) the whole sync-BN step -- 2 small all-reduces per layer forward, 1 per
        # layer backward, the gradient all-reduce and SGD -- is recorded into ONE HIP graph
        fused_comm = multi and _lr is not None and self._comm_in_graph()

        def seq():
            self._prepare_images()
            logits = self._forward(batch, bufs, True)
            self.flat_g.fill_zero()                        # loss / accuracy tail and the analytically zero bias gradients: one memset
            D.softmax_cce(self.ctx, logits, batch.y, bufs["probs"], self.loss_acc, bufs["dlogits"], denom, cce=self.cce_train)
            self._backward(batch, bufs, True)
            if fused_comm:
                self.comm.allreduce_sum(self.flat_g)
            if _lr is not None and (fused_comm or not multi):   # the update rides in the same captured graph
                self._apply_sgd(_lr)
            if self.dropout > 0.0:
                D.counter_add(self.ctx, self._step_dev, 1)     # the next step draws new Dropout masks (also from a replayed graph)
        self._bind(batch)
        self._step_applied = fused_comm or not multi
        lr_key = self._lr_key(_lr)
        if multi and not fused_comm:
            seq()                                          # host-mediated collectives inside: not captured
            self.comm.allreduce_sum(self.flat_g)
        else:
            again = self._run_with_comm_fallback(
                ("grad", batch.uid, lr_key, denom), seq, fused_comm, _CAPTURE_FAILED_SYNC_BN,
                fused_comm and (lambda: self.loss_and_grads(batch, None, _lr=_lr, global_batch=global_batch)))
            if again is not None:
                return again
        self.ctx.set_lr_source(None)
        return batch

    def train_step(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None):
        """gcn.py:330-340 for the live model: forward(training=True), CCE, gradients, SGD, accuracy."""
        batch = self.loss_and_grads(inputs, target, _lr=float(lr), global_batch=global_batch)
        if not self._step_applied:
            self._apply_sgd(lr)
        return self._finish_step(fetch, global_batch or self._global_graphs(batch))

    def evaluate_batch(self, inputs, target):
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._prepare_images()
        logits = self._forward(batch, bufs, False)
        self.loss_acc.fill_zero()
        D.softmax_cce(self.ctx, logits, batch.y, bufs["probs"], self.loss_acc, None, batch.n_graphs, cce=self.cce_eval)
        return (*self._loss_acc_host(batch.n_graphs), (logits if self.activation is None else bufs["probs"]).numpy())

    def gradients(self):
        return [{k[2:]: L[k].numpy() for k in L if k.startswith("g_")} for L in self.layers]


def _with_remaining_self_loops(a, n):
    """PyG's add_remaining_self_loops on the batch adjacency (host, COO or scipy): a weight-1 loop where a row stores no
    diagonal entry, existing loops kept.  The device normalisation (gcnx_gcn_norm, PYG mode) needs every diagonal
    stored; values are ignored afterwards (the torch GCN passes no edge_weight)."""
    from .loader import sp_matrix_to_sp_tensor
    if not isinstance(a, SparseTensor):
        a = sp_matrix_to_sp_tensor(a)
    idx = np.asarray(a.indices, np.int64).reshape(-1, 2)
    has = np.zeros(n, bool)
    d = idx[:, 0] == idx[:, 1]
    has[idx[d, 0]] = True
    if has.all():
        return a
    miss = np.nonzero(~has)[0].astype(np.int64)
    idx = np.concatenate([idx, np.stack([miss, miss], 1)])
    vals = np.concatenate([np.asarray(a.values, np.float64).ravel(), np.ones(miss.size)])
    order = np.lexsort((idx[:, 1], idx[:, 0]))
    return SparseTensor(idx[order], vals[order], (n, n))


def _with_mean_self_loops(a, e, n):
    """PyG's add_self_loops=True of GATv2Conv on the batch adjacency (host, COO or scipy; row = target): the stored loops
    are removed, one loop per node is added, and with edge features e [nnz, S] (one row per stored entry, row-major) the
    loop of node i carries the mean of the feature rows of row i's remaining entries -- zeros if it has none
    (fill_value="mean").  Returns (SparseTensor with unit values, e' in its entry order or None)."""
    from .loader import sp_matrix_to_sp_tensor
    if not isinstance(a, SparseTensor):
        a = sp_matrix_to_sp_tensor(a)
    idx = np.asarray(a.indices, np.int64).reshape(-1, 2)
    keep = idx[:, 0] != idx[:, 1]
    rows = idx[keep, 0]
    loops = np.arange(n, dtype=np.int64)
    idx = np.concatenate([idx[keep], np.stack([loops, loops], 1)])
    order = np.lexsort((idx[:, 1], idx[:, 0]))
    if e is not None:
        e = np.asarray(e)
        if e.ndim != 2 or e.shape[0] != keep.size:
            raise ValueError(f"edge features e have shape {e.shape}: expected one row per stored entry of the adjacency ({keep.size})")
        e = e.astype(np.float64)
        fill = np.zeros((n, e.shape[1]))
        np.add.at(fill, rows, e[keep])
        fill /= np.maximum(np.bincount(rows, minlength=n), 1)[:, None]
        e = np.concatenate([e[keep], fill])[order].astype(np.float32)
    return SparseTensor(idx[order], np.ones(order.size), (n, n)), e


def _with_unit_self_loops(a, e, n):
    """PyG's add_remaining_self_loops(fill_value=1) of PDNConv on the batch adjacency (host, COO or scipy; row = target) with
    edge features e [nnz, S] (one row per stored entry, row-major): every stored entry, a stored loop included, keeps its
    place among its row's entries and its feature row; a row that stores no loop gets one in sorted position with a zero
    feature row.  Returns (SparseTensor with unit values, e' in its entry order, unit [nnz'] uint8: 1 on the added loops --
    the entries whose weight is exactly 1 and not learned -- or None where no loop was missing)."""
    from .loader import sp_matrix_to_sp_tensor
    if not isinstance(a, SparseTensor):
        a = sp_matrix_to_sp_tensor(a)
    idx = np.asarray(a.indices, np.int64).reshape(-1, 2)
    e = np.asarray(e)
    if e.ndim != 2 or e.shape[0] != idx.shape[0]:
        raise ValueError(f"edge features e have shape {e.shape}: expected one row per stored entry of the adjacency ({idx.shape[0]})")
    has = np.zeros(n, bool)
    d = idx[:, 0] == idx[:, 1]
    has[idx[d, 0]] = True
    miss = np.nonzero(~has)[0].astype(np.int64)
    if miss.size == 0:
        return SparseTensor(idx, np.ones(idx.shape[0]), (n, n)), e.astype(np.float32), None
    idx = np.concatenate([idx, np.stack([miss, miss], 1)])
    order = np.lexsort((idx[:, 1], idx[:, 0]))
    unit = np.concatenate([np.zeros(e.shape[0], np.uint8), np.ones(miss.size, np.uint8)])[order]
    e = np.concatenate([e.astype(np.float32), np.zeros((miss.size, e.shape[1]), np.float32)])[order]
    return SparseTensor(idx[order], np.ones(order.size), (n, n)), e, unit


def _conv_keys(*names):
    """{k: the names with the convolution's number k appended} -- formatted once per class: the conv hooks run every step."""
    return {k: tuple(f"{name}{k}" for name in names) for k in (1, 2)}


class GCN(_GraphRunner):
    """The reference's torch class ``GCN`` (src/utilities/gcn_utills.py:795-853), BASELINE config 1's topology:

        GCNConv(F->H)·BN·PReLU -> GCNConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    with BCEWithLogitsLoss on the single logit and plain SGD.  Semantics ("torch GCN"): PyG GCNConv on the
    UNWEIGHTED adjacency with add_remaining_self_loops and symmetric normalisation; BatchNorm1d(track_running_stats=False):
    batch statistics (biased variance, eps 1e-5) in training AND evaluation, so a batch of one graph raises ValueError as
    torch does; PReLU(): one slope per layer.  fp32, eager launches.

    Hot path: gcnx_gemm / gcnx_gcn_conv_fwd + gcnx_spmm_csr for the convolutions, gcnx_bn_moments and gcnx_bn_act
    (GCNX_ACT_PRELU_SHARED) for BN1·PReLU1, gcnx_bn_act_pool (BN2·PReLU2·max-pool in one pass, and its two-launch backward)
    and gcnx_bn_prelu_bce_head (Linear·BN·PReLU twice, the loss and all their gradients in one launch).  GCNX_BN_POOL=0
    (read at construction) replaces the fused pool pair by gcnx_bn_act + gcnx_segment_pool and their backward.

    Weights: ``state_dict()`` / ``load_state_dict()`` use torch's key names and layouts; ``get_weights()`` lists the same
    tensors in ``named_parameters()`` order (modules in the reference's __init__ order; inside PyG 2.x GCNConv the bias
    is registered before ``lin.weight``).  That order follows PyG 2.x's source; neither torch_geometric nor the
    reference's checkpoint was available to confirm it against a live module, so prefer the named dicts.

    ``readout="attention"`` (every model of the family takes it; default ``"max"``) replaces global_max_pool by the learned
    readout PyG builds as ``self.pool = AttentionalAggregation(gate_nn=Linear(hidden_channels, 1, bias=False))`` and calls as
    ``self.pool(x, batch)`` -- Spektral's GlobalAttnSumPool: alpha = softmax over each graph's rows of <y2_i, a>, pooled[g] =
    sum_i alpha_i y2_i.  It adds one tensor, ``pool.gate_nn.weight`` [1, hidden], LAST in ``state_dict()`` /
    ``get_weights()`` / ``gradients()`` (after the modules above, as a module registered last), initialised as torch's Linear
    and drawn after every other tensor, so a seed gives all the others the bits it gives without the readout.  Launches:
    gcnx_bn_act + gcnx_attn_pool, backward gcnx_attn_pool_bwd + the BN·PReLU backward (csrc/attn_pool.hip).

    ``norm="graph"`` (every model of the family takes it; default ``"batch"``) replaces the two node-level norms
    ``batch_norm_1`` / ``batch_norm_2`` by PyG's ``GraphNorm(hidden_channels)``: statistics per graph and per channel, with a
    learned share ``mean_scale`` of the mean removed ("GraphNorm"), so the node-level part of a graph's forward no
    longer depends on which graphs share its batch.  ``batch_norm_3`` / ``batch_norm_4`` run on pooled rows and stay
    BatchNorm1d, so a batch of one graph still raises.  It adds two tensors, ``batch_norm_{1,2}.mean_scale`` [hidden], each
    directly behind its ``.bias`` in ``state_dict()`` / ``get_weights()`` / ``gradients()`` and behind the class's list (before
    the attention gate) in the flat buffer; they start at 1 without a draw, so a seed gives every other tensor the bits it
    gives with ``norm="batch"``.  Launches: gcnx_graph_norm_act (GraphNorm·PReLU) per norm and gcnx_graph_norm_act_bwd
    (csrc/graph_norm.hip), the readout as its own launch (gcnx_segment_pool(max) or gcnx_attn_pool).  With ``comm=`` the
    node norms run on the shard's own rows without an all-reduce: 6 of the 13 all-reduces of a sync-BN step are gone."""

    PARAM_ORDER = ("w1", "b1", "g1", "be1", "a1", "w2", "b2", "g2", "be2", "a2",
                   "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4")
    # (torch key, internal key, transposed): named_parameters() order; the conv kernels are stored [in, out] (gcnx_gemm)
    TORCH_KEYS = (("conv1.bias", "b1", False), ("conv1.lin.weight", "w1", True),
                  ("conv2.bias", "b2", False), ("conv2.lin.weight", "w2", True),
                  ("linear_1.weight", "w3", False), ("linear_1.bias", "b3", False),
                  ("linear_2.weight", "w4", False), ("linear_2.bias", "b4", False),
                  ("prelu_1.weight", "a1", False), ("prelu_2.weight", "a2", False),
                  ("prelu_3.weight", "a3", False), ("prelu_4.weight", "a4", False),
                  ("batch_norm_1.weight", "g1", False), ("batch_norm_1.bias", "be1", False),
                  ("batch_norm_2.weight", "g2", False), ("batch_norm_2.bias", "be2", False),
                  ("batch_norm_3.weight", "g3", False), ("batch_norm_3.bias", "be3", False),
                  ("batch_norm_4.weight", "g4", False), ("batch_norm_4.bias", "be4", False))
    PROBE_KEY = "conv1.lin.weight"       # the state_dict tensor whose second dimension is the input width
    EPS = D.TORCH_BN_EPS
    # ---- what a subclass with another convolution sets (and the hooks _initial, _conv_fwd, _conv_bwd) -------------------------
    OPERATOR = "gcn"                     # _op: "gcn" | "mean" | "cheb" | "pattern" | "perm"
    SELF_LOOPS = True                    # a host adjacency gets PyG's add_remaining_self_loops (False: used as stored)
    LEADING_AXIS = ()                    # state_dict keys that carry a leading axis of 1 in PyG ([1, heads, C], [1, 3H])
    STACKS = {}                          # {key of a stacked tensor: the keys of its column blocks, each ``hidden`` wide, in storage
    #                                      order}: the only statement of a model's block order (a subclass sets it in _init)
    EDGE_BLOCKS = {}                     # {state_dict key: the key of its edge block}: ResGated's [node block ‖ edge block] weights
    KERNELS = "GCNConv"                  # the kernel family, as the constructor's messages name it
    HEAD_NOTE = "the one-workgroup head"
    edge_dim = None
    _KEYS = _conv_keys("w", "b", "z")
    READOUTS = ("max", "attention")
    READOUT_KEY = ("pool.gate_nn.weight", "ar", False)      # readout="attention": the gate's weight, [1, hidden] in torch's layout
    NORMS = ("batch", "graph")

    def __init__(self, *args, **kw):
        """GCN([ctx,] hidden_channels=64, num_classes=1, seed=0): the reference's constructor behind an optional ctx."""
        if args and isinstance(args[0], D.Context):
            ctx, args = args[0], args[1:]
        else:
            ctx = kw.pop("ctx", None)
        readout = kw.pop("readout", "max")
        if readout not in self.READOUTS:
            raise NotImplementedError(f"{self._name}: readout={readout!r} must be \"max\" or \"attention\"")
        self.readout = readout
        norm = kw.pop("norm", "batch")
        if norm not in self.NORMS:
            raise NotImplementedError(f"{self._name}: norm={norm!r} must be \"batch\" or \"graph\"")
        self.norm = norm
        self._init(ctx, *args, **kw)
        if norm == "graph":             # batch_norm_{1,2}.mean_scale: behind the class's list, and behind its .bias as torch names them
            self.PARAM_ORDER = tuple(self.PARAM_ORDER) + ("ms1", "ms2")
            keys = []
            for entry in self.TORCH_KEYS:
                keys.append(entry)
                if entry[1] in ("be1", "be2"):
                    keys.append((f"batch_norm_{entry[1][2]}.mean_scale", "ms" + entry[1][2], False))
            self.TORCH_KEYS = tuple(keys)
        if readout == "attention":      # one more tensor behind everything the class lists: every existing view keeps its offset
            self.PARAM_ORDER = tuple(self.PARAM_ORDER) + (self.READOUT_KEY[1],)
            self.TORCH_KEYS = tuple(self.TORCH_KEYS) + (self.READOUT_KEY,)
            self.LEADING_AXIS = tuple(self.LEADING_AXIS) + (self.READOUT_KEY[0],)

    @property
    def _name(self):
        return "gcnx." + type(self).__name__

    def _check_heads(self, h, heads):
        """The heads / hidden_channels pairs the attention kernels serve."""
        if heads not in (1, 2, 4, 8) or h % heads != 0:
            raise NotImplementedError(f"{self._name}: heads={heads} must be 1, 2, 4 or 8 and divide hidden_channels={h}")
        if h not in (16, 32, 64, 128) or h // heads < 4:
            raise NotImplementedError(f"{self._name}: hidden_channels={h} must be 16, 32, 64 or 128 with at least 4 channels per head "
                                      f"(the widths the {self.KERNELS} kernels serve; there is no composed route)")

    def _check_edge_dim(self, edge_dim):
        """edge_dim as the model keeps it: None or an int in 1 .. 8."""
        if edge_dim is not None and not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"{self._name}: edge_dim={edge_dim} must be None or 1 .. 8 (what the {self.KERNELS} kernels serve)")
        return None if edge_dim is None else int(edge_dim)

    def _one_device(self, comm):
        if comm is not None:
            raise NotImplementedError(f"{self._name} runs on one device (comm is not supported)")

    def _init(self, ctx, hidden_channels=64, num_classes=1, seed=0, comm=None):
        if int(num_classes) != 1:
            raise NotImplementedError("gcnx.GCN: num_classes must be 1 (one logit + BCEWithLogitsLoss, as the reference)")
        if comm is not None and not all(hasattr(comm, k) for k in ("rank", "world_size", "allreduce_sum", "allreduce_host")):
            raise NotImplementedError("gcnx.GCN: comm must have the gcnx.comm.Communicator interface (rank, world_size, "
                                      "allreduce_sum, allreduce_host)")
        self.ctx = ctx if ctx is not None else D.default_context()
        self.comm = comm                     # gcnx.comm.Communicator (sync-BN training over graph shards) or None
        self.hidden, self.num_classes = int(hidden_channels), 1
        self.use_graph = False               # eager launches (~20 per step)
        self._bn_pool = os.environ.get("GCNX_BN_POOL", "1") != "0"    # knob, read once
        self._rng = np.random.default_rng(seed)
        self.built = False
        self._bufs = None
        self._graphs = {}
        self._op_cache = None

    # ---- parameters: one flat buffer (one SGD launch) ------------------------------------------------------------------
    def _shapes(self, f_in):
        h = self.hidden
        s = {"w1": (f_in, h), "w2": (h, h), "w3": (h, h), "w4": (1, h), "b4": (1,), "g4": (1,), "be4": (1,), "a4": (1,)}
        for k in ("b1", "g1", "be1", "b2", "g2", "be2", "b3", "g3", "be3"):
            s[k] = (h,)
        for k in ("a1", "a2", "a3"):
            s[k] = (1,)
        return s

    def build(self, f_in):
        if self.hidden > 256:
            raise NotImplementedError(f"{self._name}: hidden_channels <= 256 ({self.HEAD_NOTE})")
        shapes = self._shapes(f_in)
        attention = self.readout == "attention"
        if attention:
            shapes["ar"] = (self.hidden,)
        graph_norm = self.norm == "graph"
        if graph_norm:
            shapes["ms1"] = shapes["ms2"] = (self.hidden,)
        self.f_in = int(f_in)
        # every parameter starts on a 16-byte boundary (the kernels read the weights, biases and attention vectors as float4);
        # the padding floats have zero gradients, so the single update launch over the whole buffer leaves them at zero
        offs = self._alloc_flat([(k, shapes[k]) for k in self.PARAM_ORDER], align=4)
        self._name_blocks()
        initial = self._initial(f_in, shapes, offs)
        if attention:                       # drawn last: every other tensor keeps the bits its seed gives it
            initial["ar"] = self._uniform(self.hidden, self.hidden)
        if graph_norm:                      # no draw from the RNG
            initial["ms1"] = initial["ms2"] = np.ones(self.hidden)
        for k, v in initial.items():
            self.p[k].copy_from_host(np.asarray(v, np.float32))
        self.built = True

    def _initial(self, f_in, shapes, offs):
        """{key: initial value}, drawn from self._rng in the model's own fixed order (what ``seed`` means)."""
        h, rng = self.hidden, self._rng
        return {"w1": glorot_uniform(rng, f_in, h), "w2": glorot_uniform(rng, h, h), **self._head_initial(shapes)}

    def _uniform(self, fan_in, *shape):
        """torch's Linear initialisation: U(+-1 / sqrt(fan_in))."""
        lim = 1.0 / np.sqrt(fan_in)
        return self._rng.uniform(-lim, lim, shape)

    def _head_initial(self, shapes):
        """What every model has behind its convolutions: the head's two Linears, drawn w3, b3, w4, b4 at the point of the model's
        draw order where it calls this; every BatchNorm weight 1, every PReLU slope 0.25."""
        h, u = self.hidden, self._uniform
        init = {"w3": u(h, h, h), "b3": u(h, h), "w4": u(h, 1, h), "b4": u(h, 1)}
        init.update({k: np.ones(shapes[k]) for k in ("g1", "g2", "g3", "g4")})
        init.update({k: np.full(1, 0.25) for k in ("a1", "a2", "a3", "a4")})
        return init

    def _name_blocks(self):
        """The views behind the keys of STACKS' blocks, in ``p`` and ``g`` alike."""
        for t in (self.p, self.g):
            for key, names in self.STACKS.items():
                t.update(block_views(t[key], [(n, self.hidden) for n in names]))

    def _named(self, t):
        return to_pyg(t, self.TORCH_KEYS, self.LEADING_AXIS, self.EDGE_BLOCKS)

    def state_dict(self):
        """{torch key: array in torch's layout}: conv*.lin.weight [out, in], linear_*.weight [out, in], prelu_*.weight [1]."""
        return self._named(self.p)

    def _probe_f_in(self, d):
        return int(np.asarray(d[self.PROBE_KEY]).shape[1])

    def _host_state(self, d):
        """The checked {internal key: array in the stored layout} of a state dict (builds the model if needed): every key
        present, weights transposed, the leading axis of LEADING_AXIS keys dropped, every shape that of its view."""
        if not self.built:
            self.build(self._probe_f_in(d))
        return from_pyg(d, self.TORCH_KEYS, {k: self.p[k].shape for _, k, _ in self.TORCH_KEYS}, self._name, self.LEADING_AXIS,
                        self.EDGE_BLOCKS, self.edge_dim or 0)

    def _stack(self, host):
        """The named blocks of ``host`` into the stacked tensors of STACKS."""
        host.update({key: join_blocks(host, names) for key, names in self.STACKS.items()})
        return host

    def load_state_dict(self, d):
        """Inverse of state_dict (a converted torch checkpoint: tensors as NumPy arrays).  Builds the model if needed."""
        for k, v in self._stack(self._host_state(d)).items():
            self.p[k].copy_from_host(np.ascontiguousarray(v))

    def get_weights(self):
        """The state_dict tensors in named_parameters() order (see the class docstring)."""
        sd = self.state_dict()
        return [sd[tk] for tk, _, _ in self.TORCH_KEYS]

    def set_weights(self, weights):
        self.load_state_dict({tk: w for (tk, _, _), w in zip(self.TORCH_KEYS, weights)})

    def gradients(self):
        """{torch key: gradient of the last loss_and_grads / train_step} in torch's layouts."""
        return self._named(self.g)

    @property
    def trainable_variables(self):
        return [self.p[k] for _, k, _ in self.TORCH_KEYS]

    # ---- batches ------------------------------------------------------------------------------------------------------
    def _as_batch(self, inputs, target=None):
        if not isinstance(inputs, DeviceBatch):
            if self.uses_edge_features and len(inputs) != 4:
                raise ValueError(f"{self._name}(edge_dim={self.edge_dim}) takes (x, a, e, i): build the graphs with edge features "
                                 "(Graph(e=...), from_networkx(use_edge_data='entries'))")
            inputs = self._host_inputs(inputs)
        batch = self._adopt(inputs, target, weighted=False)
        if self.uses_edge_features and batch.e is None:
            raise ValueError(f"{self._name}: the batch carries no edge features (DeviceBatch.e)")
        return batch

    def _host_inputs(self, inputs):
        """Host inputs as from_host takes them.  SELF_LOOPS: a host matrix gets PyG's add_remaining_self_loops; otherwise the
        adjacency (and e) go in as stored, no loop added or removed."""
        if self.SELF_LOOPS:
            x, a, i = _without_e(inputs)
            if not isinstance(a, D.DeviceCSR):
                inputs = (x, _with_remaining_self_loops(a, np.asarray(x).shape[0]), i)
        return inputs

    def _check_e(self, batch):
        d = self.edge_dim or 0
        if d and (batch.e is None or batch.e.shape != (batch.a.nnz, d)):
            raise ValueError(f"{self._name}(edge_dim={d}): the batch's edge features must be [{batch.a.nnz}, {d}], got "
                             f"{None if batch.e is None else list(batch.e.shape)}")

    def _op(self, batch):
        """The operator of the batch's unweighted pattern and what the backward walks, built once per batch object.  OPERATOR:
        "gcn": A^ = D^-1/2 (A + I_missing) D^-1/2 and its transpose; "mean": the row-mean operator and its transpose; "cheb":
        ChebConv's S = D^-1/2 A D^-1/2 without the loops (DeviceCSR.cheb_norm) and its transpose; "pattern":
        the pattern and its transpose; "perm": the pattern twice -- the backward walks its transposed pattern through the entry
        permutation (DeviceCSR.transpose_perm: the one a device loader's batch arrives with, or built here)."""
        if self._op_cache is None or self._op_cache[0] != batch.uid:
            a, kind = batch.a.unweighted(), self.OPERATOR
            if kind == "perm":
                a.transpose_perm()
                a_t = a
            else:
                a = a.gcn_norm("pyg") if kind == "gcn" else a.row_mean() if kind == "mean" else a.cheb_norm() if kind == "cheb" else a
                a_t = a.transpose()
            self._op_cache = (batch.uid, a, a_t)
        return self._op_cache[1], self._op_cache[2]

    def _global_counts(self, batch):
        """(N, B) of the whole sharded batch: one host all-reduce per batch (cached by its uid).  Every rank raises the same
        ValueError when a rank holds no graph or the whole batch holds fewer than 2 graphs (or rows)."""
        tot = self._global_counts_cached(batch, [batch.n, batch.n_graphs, 1.0 if batch.n_graphs == 0 else 0.0])
        n, b, empty_ranks = tot["n"], tot["b"], int(tot["empty"])
        if b < 2 or n < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{int(b)}, {self.hidden}]: "
                             "BatchNorm1d(track_running_stats=False) needs at least 2 graphs per batch")
        if empty_ranks:
            raise ValueError(f"gcnx.GCN: {empty_ranks} rank(s) hold no graph; every rank needs at least one graph of the batch")
        return n, b

    def _ensure(self, batch, sharded=False):
        """sharded: a sync-BN training step, where the batch is one rank's shard (the global sizes are checked by
        _global_counts; the shard may hold a single graph)."""
        if not sharded and (batch.n_graphs < 2 or batch.n < 2):
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{batch.n_graphs}, "
                             f"{self.hidden}]: BatchNorm1d(track_running_stats=False) needs at least 2 graphs per batch")
        if not self.built:
            self.build(batch.f)
        if batch.f != self.f_in:
            raise ValueError(f"gcnx.GCN was built for {self.f_in} node features, got {batch.f}")
        key = (batch.n, batch.n_graphs) + (("sync-BN",) if sharded else ())
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        v, n, b, h = self._views(), batch.n, batch.n_graphs, self.hidden
        bufs = {"key": key}
        for k in ("h1", "z1", "y1", "z2", "y2", "dz2", "t", "dy1", "dz1", "s2"):
            bufs[k] = v(k, n, h)
        for k in ("m1", "i1", "m2", "i2"):
            bufs[k] = v(k, 1, h).flat(0, h)
        bufs["sums"] = v("sums", 1, 3 * h).flat(0, 3 * h)
        bufs["pooled"], bufs["dpooled"] = v("pooled", b, h), v("dpooled", b, h)
        bufs["arg"] = v("arg", b, h, np.int32)
        bufs["out"], bufs["probs"] = v("out", b, 1), v("probs", b, 1)
        nh = D.bce_head_scratch_floats(self.ctx, b, h)
        bufs["head"] = v("head", 1, nh).flat(0, nh)
        if sharded:
            nh, nr = D.bce_head_phase_scratch_floats(self.ctx, b, h), D.bce_head_phase_red_floats(self.ctx, h)
            bufs["phase"], bufs["red"] = v("phase", 1, nh).flat(0, nh), v("red", 1, nr).flat(0, nr)
        if self.readout == "attention":
            ns = max(D.attn_pool_scratch_floats(self.ctx, n, b, h), 4)
            bufs["dy2"], bufs["alpha"] = v("dy2", n, h), v("alpha", 1, n).flat(0, n)
            bufs["attn"] = v("attn", 1, ns).flat(0, ns)
        if self.norm == "graph":            # the per-graph statistics of both node norms, and one scratch for their launches
            ns = max(D.graph_norm_scratch_floats(self.ctx, n, b, h), 4)
            for k in ("gm1", "gi1", "gm2", "gi2"):
                bufs[k] = v(k, b, h)
            bufs["gn"] = v("gn", 1, ns).flat(0, ns)
        self._bufs = bufs
        return bufs

    # ---- the call sequences --------------------------------------------------------------------------------------------
    def _conv(self, a_hat, x, w, bias, out, h_tmp, s=None):
        """A^ (x W) + b.  Returns True if it ran as the one-launch (A^ x) W (then ``s`` receives S = A^ x, the operand of
        dW = S^T dZ, as GCNConv.backward uses it)."""
        return convs.gcn_forward(self.ctx, a_hat, x, w, bias, out, h_tmp, s)

    # the two convolutions of the forward and their backward segments, in terms of the two hooks a subclass with another
    # convolution replaces: conv k reads x and writes bufs["z{k}"]; its backward reads dzk = bufs["dz{k}"] and writes dx if given
    def _conv1(self, a, batch, bufs, mode):
        bufs["e"] = batch.e if self.uses_edge_features else None                    # (conv2 and the backward read the same rows)
        self._conv_fwd(a, batch.x, 1, bufs, mode == "grads")

    def _conv2(self, a, bufs, mode):
        self._conv_fwd(a, bufs["y1"], 2, bufs, mode == "grads")

    def _conv2_bwd(self, a_t, bufs):
        """dZ2 -> conv2's gradients and dY1."""
        self._conv_bwd(a_t, bufs["y1"], 2, bufs["dz2"], bufs, bufs["dy1"])

    def _conv1_bwd(self, a_t, batch, bufs):
        """dZ1 -> conv1's gradients (the input carries no gradient)."""
        self._conv_bwd(a_t, batch.x, 1, bufs["dz1"], bufs, None)

    def _conv_fwd(self, a_hat, x, k, bufs, keep):
        p = self.p
        w, b, z = self._KEYS[k]
        ok = self._conv(a_hat, x, p[w], p[b], bufs[z], bufs["h1"], s=bufs["s2"] if keep and k == 2 else None)
        if k == 2:
            bufs["s2_ok"] = ok

    def _conv_bwd(self, a_t, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, b, _ = self._KEYS[k]
        # conv2 after a one-launch forward (A^ Y1) W2: the association of GCNConv.backward, dW2 = S2^T dZ2
        s = bufs["s2"] if dx is not None and bufs["s2_ok"] else None
        convs.gcn_backward(self.ctx, a_t, x, dzk, p[w], g[w], g[b], bufs["t"], dx, s)

    def _moments(self, z, mean, inv, bufs, counts):
        """Training-mode BatchNorm statistics over the rows of z; with counts (sync-BN) over every rank's rows: the two moment
        passes with their column sums all-reduced and the global row count."""
        ctx, e = self.ctx, self.EPS
        if counts is None:
            D.bn_moments(ctx, z, None, mean, inv, eps=e)
            return
        sums, f = bufs["sums"], z.shape[1]
        D.bn_stats(ctx, z, sums)
        self.comm.allreduce_sum(sums, 2 * f)
        D.bn_finalize(ctx, sums, counts[0], mean, inv, eps=e)
        D.bn_stats(ctx, z, sums, shift=mean)
        self.comm.allreduce_sum(sums, 2 * f)
        D.bn_finalize(ctx, sums, counts[0], mean, inv, shift=mean, eps=e)

    def _forward(self, batch, bufs, mode, denom=None, counts=None):
        """mode: "fwd" (logits only), "loss" (+ loss and hits), "grads" (+ dPooled and the head's gradients).  counts: the
        global (N, B) of a sync-BN training step over graph shards (None: this batch's own statistics)."""
        ctx, p, e = self.ctx, self.p, self.EPS
        a_hat, _ = self._op(batch)
        graph_norm = self.norm == "graph"
        self._conv1(a_hat, batch, bufs, mode)
        if graph_norm:                       # each graph's own statistics: nothing to all-reduce, sharded or not
            self._graph_norm(batch, bufs, 1)
        else:
            self._moments(bufs["z1"], bufs["m1"], bufs["i1"], bufs, counts)
            D.bn_act(ctx, bufs["z1"], bufs["m1"], bufs["i1"], p["g1"], p["be1"], bufs["y1"], act="prelu_shared", alpha=p["a1"])
        self._conv2(a_hat, bufs, mode)
        if graph_norm:
            self._graph_norm(batch, bufs, 2)
            if self.readout == "attention":
                D.attn_pool(ctx, batch.seg, bufs["y2"], p["ar"], bufs["pooled"], bufs["alpha"], bufs["attn"])
            else:
                D.segment_pool(ctx, batch.seg, bufs["y2"], bufs["pooled"], "max", bufs["arg"])
        else:
            self._moments(bufs["z2"], bufs["m2"], bufs["i2"], bufs, counts)
            if self.readout == "attention":
                D.bn_act(ctx, bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"], bufs["y2"], act="prelu_shared", alpha=p["a2"])
                D.attn_pool(ctx, batch.seg, bufs["y2"], p["ar"], bufs["pooled"], bufs["alpha"], bufs["attn"])
            elif self._bn_pool:
                D.bn_act_pool(ctx, batch.seg, bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"], bufs["pooled"], bufs["arg"],
                              alpha=p["a2"])
            else:
                D.bn_act(ctx, bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"], bufs["y2"], act="prelu_shared", alpha=p["a2"])
                D.segment_pool(ctx, batch.seg, bufs["y2"], bufs["pooled"], "max", bufs["arg"])
        y = batch.y if mode != "fwd" else None
        if y is None and mode != "fwd":
            raise ValueError("gcnx.GCN: labels are needed for the loss")
        grads = mode == "grads"
        args = D.bce_head_args(bufs["pooled"], p, bufs["head" if counts is None else "phase"], bufs["out"], bufs["probs"], y=y,
                               loss_acc=self.loss_acc if y is not None else None, denom=denom or batch.n_graphs,
                               g=self.g if grads else None, dpooled=bufs["dpooled"] if grads else None, eps=e)
        if counts is None:
            D.bn_prelu_bce_head(ctx, args)
            return
        # sync-BN (a training step): the head in seven phases, each phase's partial sums all-reduced before the next reads
        # them; the loss, the hits and the gradients stay local parts until the step's gradient all-reduce
        for k in range(7):
            D.bce_head_phase(ctx, args, k, counts[1], bufs["red"])
            if k < 6:
                self.comm.allreduce_sum(bufs["red"].flat(*D.bce_head_phase_slice(k, self.hidden)))

    def _graph_norm(self, batch, bufs, k):
        """GraphNorm_k·PReLU_k: z_k -> y_k, the per-graph mean and inv kept for the backward."""
        p = self.p
        D.graph_norm_act(self.ctx, batch.seg, bufs[f"z{k}"], p[f"ms{k}"], p[f"g{k}"], p[f"be{k}"], bufs[f"y{k}"], bufs[f"gm{k}"],
                         bufs[f"gi{k}"], act="prelu_shared", alpha=p[f"a{k}"], scratch=bufs["gn"], eps=self.EPS)

    def _graph_norm_bwd(self, batch, bufs, k, dy):
        """dY_k -> dZ_k and the gradients of GraphNorm_k (weight, bias, mean_scale) and PReLU_k."""
        p, g = self.p, self.g
        D.graph_norm_act_bwd(self.ctx, batch.seg, dy, bufs[f"z{k}"], bufs[f"gm{k}"], bufs[f"gi{k}"], p[f"ms{k}"], p[f"g{k}"],
                             p[f"be{k}"], bufs[f"dz{k}"], act="prelu_shared", alpha=p[f"a{k}"], dgamma=g[f"g{k}"], dbeta=g[f"be{k}"],
                             dmean_scale=g[f"ms{k}"], dalpha=g[f"a{k}"], scratch=bufs["gn"])

    def _bn_bwd(self, dy, z, mean, inv, gamma, beta, alpha, dz, g_gamma, g_beta, g_alpha, bufs, counts):
        """BN·PReLU backward over the rows of z; with counts (sync-BN) the column sums all-reduced between the two halves."""
        ctx = self.ctx
        if counts is None:
            D.bn_act_bwd(ctx, dy, z, mean, inv, gamma, beta, dz, bufs["sums"], act="prelu_shared", alpha=alpha, dgamma=g_gamma,
                         dbeta=g_beta, dalpha=g_alpha)
            return
        D.bn_act_bwd_stats(ctx, dy, z, mean, inv, gamma, beta, bufs["sums"], act="prelu_shared", alpha=alpha, dgamma=g_gamma,
                           dbeta=g_beta, dalpha=g_alpha)
        self.comm.allreduce_sum(bufs["sums"], 3 * z.shape[1])
        D.bn_act_bwd_apply(ctx, dy, z, mean, inv, gamma, beta, bufs["sums"], counts[0], dz, act="prelu_shared", alpha=alpha)

    def _backward(self, batch, bufs, counts=None):
        ctx, p, g = self.ctx, self.p, self.g
        _, a_t = self._op(batch)
        if self.norm == "graph":
            if self.readout == "attention":
                D.attn_pool_bwd(ctx, batch.seg, bufs["y2"], p["ar"], bufs["alpha"], bufs["pooled"], bufs["dpooled"], bufs["dy2"],
                                g["ar"], bufs["attn"])
                self._graph_norm_bwd(batch, bufs, 2, bufs["dy2"])
            else:
                D.segment_pool_bwd(ctx, batch.seg, bufs["dpooled"], bufs["y2"], "max", bufs["arg"])
                self._graph_norm_bwd(batch, bufs, 2, bufs["y2"])
            self._conv2_bwd(a_t, bufs)
            self._graph_norm_bwd(batch, bufs, 1, bufs["dy1"])
            self._conv1_bwd(a_t, batch, bufs)
            return
        if self.readout == "attention":
            D.attn_pool_bwd(ctx, batch.seg, bufs["y2"], p["ar"], bufs["alpha"], bufs["pooled"], bufs["dpooled"], bufs["dy2"], g["ar"],
                            bufs["attn"])
            self._bn_bwd(bufs["dy2"], bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"], p["a2"], bufs["dz2"], g["g2"], g["be2"],
                         g["a2"], bufs, counts)
        elif self._bn_pool and counts is not None:
            D.bn_act_pool_bwd_stats(ctx, batch.seg, bufs["dpooled"], bufs["arg"], bufs["z2"], bufs["m2"], bufs["i2"], p["g2"],
                                    p["be2"], bufs["sums"], alpha=p["a2"], dgamma=g["g2"], dbeta=g["be2"], dalpha=g["a2"])
            self.comm.allreduce_sum(bufs["sums"], 3 * self.hidden)
            D.bn_act_pool_bwd_apply(ctx, batch.seg, bufs["dpooled"], bufs["arg"], bufs["z2"], bufs["m2"], bufs["i2"], p["g2"],
                                    p["be2"], bufs["sums"], counts[0], bufs["dz2"], alpha=p["a2"])
        elif self._bn_pool:
            D.bn_act_pool_bwd(ctx, batch.seg, bufs["dpooled"], bufs["arg"], bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"],
                              bufs["dz2"], alpha=p["a2"], dgamma=g["g2"], dbeta=g["be2"], dalpha=g["a2"])
        else:
            D.segment_pool_bwd(ctx, batch.seg, bufs["dpooled"], bufs["y2"], "max", bufs["arg"])
            self._bn_bwd(bufs["y2"], bufs["z2"], bufs["m2"], bufs["i2"], p["g2"], p["be2"], p["a2"], bufs["dz2"], g["g2"], g["be2"],
                         g["a2"], bufs, counts)
        self._conv2_bwd(a_t, bufs)
        self._bn_bwd(bufs["dy1"], bufs["z1"], bufs["m1"], bufs["i1"], p["g1"], p["be1"], p["a1"], bufs["dz1"], g["g1"], g["be1"],
                     g["a1"], bufs, counts)
        self._conv1_bwd(a_t, batch, bufs)

    # ---- public surface ---------------------------------------------------------------------------------------------
    def __call__(self, inputs, training=False):
        """model((x, a, i), training=False) -> the logits [B, 1] (torch's forward output; BatchNorm uses batch statistics
        either way)."""
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "fwd")
        return bufs["out"].numpy()

    def forward(self, x, edge_index, batch):
        """The torch-style call: x [N, F], edge_index [2, E] (PyG's source -> target flow: row = edge_index[1], column =
        edge_index[0]; duplicate edges count once), batch [N] graph ids.  Returns the logits [B, 1]."""
        import scipy.sparse as sp
        x = np.asarray(x, np.float32)
        ei = np.asarray(edge_index, np.int64).reshape(2, -1)
        n = x.shape[0]
        a = sp.coo_matrix((np.ones(ei.shape[1]), (ei[1], ei[0])), shape=(n, n)).tocsr()
        a.data[:] = 1.0
        return self((x, a, np.asarray(batch, np.int64)))

    def loss_and_grads(self, inputs, target=None, global_batch=None, _lr=None):
        """Forward + BCE + every gradient (+ the SGD update with ``_lr``).  Returns the device batch.

        With a communicator of world_size > 1 the batch is this rank's shard of whole graphs (gcnx.shard) and the step is
        torch's SyncBatchNorm step on the whole batch: every BatchNorm uses the statistics of all ranks' rows (BN1 / BN2:
        the global node count N; BN3 / BN4: the global graph count B), the loss is normalised by ``global_batch`` (default:
        B), and one all-reduce sums the flat gradient buffer (+ loss / hits) over the ranks before SGD."""
        batch = self._as_batch(inputs, target)
        counts = self._global_counts(batch) if self._multi() else None
        bufs = self._ensure(batch, sharded=counts is not None)
        denom = float(global_batch or (counts[1] if counts else batch.n_graphs))
        self._forward(batch, bufs, "grads", denom, counts)
        self._backward(batch, bufs, counts)
        if counts is not None:
            self.comm.allreduce_sum(self.flat_g)
        if _lr is not None:
            self._apply_sgd(_lr)
        self._last_batch = batch
        return batch

    def train_step(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None):
        """One optimisation step: loss, gradients, p -= lr * g.  fetch: True -> (loss, acc); False -> None; "stash" ->
        None, metrics kept on the device for collect_metrics()."""
        batch = self.loss_and_grads(inputs, target, global_batch, _lr=float(lr))
        return self._finish_step(fetch, global_batch or self._global_graphs(batch))

    def evaluate_batch(self, inputs, target):
        """(loss, accuracy, probabilities [B, 1]) without gradients (BatchNorm on batch statistics, as torch's eval here)."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "loss", float(batch.n_graphs))
        return (*self._loss_acc_host(batch.n_graphs), bufs["probs"].numpy())


class SAGE(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's SAGEConv(aggr="mean"), the step the reference's author notes above
    them ("consider using class SAGEConv instead", gcn_utills.py:804-806):

        SAGEConv(F->H)·BN·PReLU -> SAGEConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    out_i = mean_{j in N(i)} x_j W_l + b + x_i W_r on the adjacency exactly as stored: no self-loop is added or removed, values
    are ignored, a node without stored entries aggregates to 0.  ``forward(x, edge_index, batch)`` counts duplicate edges
    once, as ``GCN`` does (PyG would count them twice in the mean: a deviation).  Everything behind the convolutions is
    ``GCN``'s: BN·PReLU, the fused max-pool pair, the one-launch BCE head, sync-BN over shards (``comm=``), ``fit``.

    Hot path: gcnx_sage_conv, one launch per convolution and one for conv2's dX (csrc/sage.hip), gcnx_gemm_dw2 for each
    layer's two weight gradients.  GCNX_SAGE_FUSED=0 (read at construction), and any shape gcnx_sage_conv refuses (hidden >
    128), takes the composed route instead: gcnx_spmm_csr, gcnx_gemm twice, gcnx_add; gcnx_gemm_dx, gcnx_spmm_csr,
    gcnx_gemm_dx(accumulate) backward.

    Weights: torch key names ``conv{1,2}.lin_l.weight``, ``conv{1,2}.lin_l.bias``, ``conv{1,2}.lin_r.weight`` in
    ``state_dict()`` ([out, in], as torch; stored [in, out] here), listed by ``get_weights()`` in PyG 2.x's
    named_parameters() order (lin_l before lin_r).  Initialisation U(+-1/sqrt(fan_in)) as torch's Linear.  Neither the
    order nor the initialisation was confirmed against a live torch_geometric: prefer the named dicts."""

    PARAM_ORDER = ("wl1", "b1", "wr1", "g1", "be1", "a1", "wl2", "b2", "wr2", "g2", "be2", "a2",
                   "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4")
    TORCH_KEYS = (("conv1.lin_l.weight", "wl1", True), ("conv1.lin_l.bias", "b1", False), ("conv1.lin_r.weight", "wr1", True),
                  ("conv2.lin_l.weight", "wl2", True), ("conv2.lin_l.bias", "b2", False), ("conv2.lin_r.weight", "wr2", True)) + \
        GCN.TORCH_KEYS[4:]
    PROBE_KEY = "conv1.lin_l.weight"
    OPERATOR, SELF_LOOPS, KERNELS = "mean", False, "SAGEConv"
    _KEYS = _conv_keys("wl", "wr", "b", "z", "s")

    def _init(self, ctx, hidden_channels=64, num_classes=1, seed=0, comm=None):
        super()._init(ctx, hidden_channels, num_classes, seed, comm)
        self._fused = os.environ.get("GCNX_SAGE_FUSED", "1") != "0"    # knob, read once

    def _shapes(self, f_in):
        h = self.hidden
        s = super()._shapes(f_in)
        del s["w1"], s["w2"]
        s.update(wl1=(f_in, h), wr1=(f_in, h), wl2=(h, h), wr2=(h, h))
        return s

    def _initial(self, f_in, shapes, offs):
        h, u = self.hidden, self._uniform
        return {"wl1": u(f_in, f_in, h), "b1": u(f_in, h), "wr1": u(f_in, f_in, h),
                "wl2": u(h, h, h), "b2": u(h, h), "wr2": u(h, h, h), **self._head_initial(shapes)}

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        if "s1" not in bufs:
            bufs["s1"] = self._views()("s1", batch.n, batch.f)
        return bufs

    def _one_launch(self, x, fo, *others):
        return (self._fused and D.sage_conv_ok(self.ctx, x.shape[0], x.shape[1], fo, x.ld)
                and all(a.ptr % 16 == 0 for a in (x,) + others))

    def _conv_fwd(self, a_mean, x, k, bufs, keep):
        """z_k = (A x) W_l + x W_r + b, s_k = A x (the operand of dW_l): one launch, or the composed route."""
        ctx, p = self.ctx, self.p
        wl, wr, b, z, s = self._KEYS[k]
        w_nb, w_root, bias, out, s = p[wl], p[wr], p[b], bufs[z], bufs[s]
        if self._one_launch(x, w_nb.shape[1], out, s):
            D.sage_conv(ctx, a_mean, x, w_nb, w_root, bias, out, s=s)
            return
        D.spmm(ctx, a_mean, x, None, s)
        D.gemm(ctx, s, w_nb, bias, out)
        D.gemm(ctx, x, w_root, None, bufs["h1"])
        D.add(ctx, out, bufs["h1"], out)

    def _conv_bwd(self, a_t, x, k, dzk, bufs, dx):
        """dZ_k -> conv k's gradients and, with dx, dx = (A^T dZ_k) W_l^T + dZ_k W_r^T."""
        ctx, p, g = self.ctx, self.p, self.g
        wl, wr, b, _, s = self._KEYS[k]
        D.act_bias_grad(ctx, dzk, None, dzk, None, db=g[b])                          # conv_k.lin_l.bias: column sums of dZ_k
        D.gemm_dw2(ctx, bufs[s], dzk, g[wl], x, dzk, g[wr])                          # dW_l = S_k^T dZ_k, dW_r = x^T dZ_k
        if dx is None:
            return
        if self._one_launch(dzk, self.hidden, dx):
            D.sage_conv(ctx, a_t, dzk, p[wl], p[wr], None, dx, w_transposed=True)
            return
        D.gemm_dx(ctx, dzk, p[wl], bufs["t"])
        D.spmm(ctx, a_t, bufs["t"], None, dx)
        D.gemm_dx(ctx, dzk, p[wr], dx, accumulate=True)


class GIN(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's GINConv(Sequential(Linear, ReLU, Linear), train_eps), the Graph
    Isomorphism Network convolution, in the slot the reference's author left open (gcn_utills.py:804-806):

        GINConv(F->H)·BN·PReLU -> GINConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    ``GIN([ctx,] hidden_channels=64, train_eps=False, num_classes=1, seed=0, comm=None)``; both MLP layers of both
    convolutions are H wide.  out_i = MLP((1 + eps) x_i + sum_{j in N(i)} x_j) on the adjacency exactly as stored: no
    self-loop is added or removed (a stored one counts as one more neighbour), values are ignored.
    ``forward(x, edge_index, batch)`` counts duplicate edges once, as ``GCN`` does (PyG's sum would count them twice: a
    deviation).  Everything behind the convolutions is ``GCN``'s: BN·PReLU, the fused max-pool pair, the one-launch BCE head,
    sync-BN over shards (``comm=``), ``set_optimizer``, ``fit``.

    Hot path: gcnx_gin_conv, one launch per convolution (csrc/gin.hip), which keeps T = (1 + eps) x + A x and
    U = relu(T W_a + b_a); backward gcnx_act_bias_grad, gcnx_gemm_dx(y_mask=U, db) and gcnx_gemm_dw2 per convolution, and for
    conv2's dX the single-stage gcnx_gin_conv on the transposed pattern.  With train_eps, dT = dU W_a^T is formed for
    d eps = sum <x, dT> (gcnx_gin_eps_grad) and conv2's dX is gcnx_gin_aggregate(A^T, dT) instead.  GCNX_GIN_FUSED=0 (read at
    construction), and any shape gcnx_gin_conv refuses (hidden > 128; a width outside {16, 32, 64, 128} on the gathered side),
    takes the composed route per launch: gcnx_gin_aggregate, gcnx_gemm(relu), gcnx_gemm; gcnx_gemm_dx, gcnx_gin_aggregate.

    Weights: torch key names ``conv{1,2}.eps`` [1], ``conv{1,2}.nn.0.weight``, ``.nn.0.bias``, ``.nn.2.weight``, ``.nn.2.bias``
    in ``state_dict()`` ([out, in], as torch; stored [in, out] here).  ``conv{1,2}.eps`` is always in ``state_dict()`` /
    ``load_state_dict()`` -- PyG registers it as a parameter or as a buffer -- and in ``get_weights()`` / ``gradients()`` /
    the flat buffer only with train_eps (one float padded to four, like every tensor).  Initialisation U(+-1/sqrt(fan_in)) as
    torch's Linear, eps 0.  The key order follows PyG 2.x's source (eps before nn.*); it was not confirmed against a live
    torch_geometric: prefer the named dicts."""

    PROBE_KEY = "conv1.nn.0.weight"
    OPERATOR, SELF_LOOPS, KERNELS = "pattern", False, "GINConv"
    _KEYS = _conv_keys("wa", "ba", "wb", "bb", "z", "t", "u", "dt", "e")

    def _init(self, ctx, hidden_channels=64, train_eps=False, num_classes=1, seed=0, comm=None):
        super()._init(ctx, hidden_channels, num_classes, seed, comm)
        self.train_eps = bool(train_eps)
        self._fused = os.environ.get("GCNX_GIN_FUSED", "1") != "0"     # knob, read once
        conv = lambda k: ((f"e{k}",) if self.train_eps else ()) + (f"wa{k}", f"ba{k}", f"wb{k}", f"bb{k}", f"g{k}", f"be{k}", f"a{k}")
        self.PARAM_ORDER = conv(1) + conv(2) + GCN.PARAM_ORDER[10:]
        self.EPS_KEYS = (("conv1.eps", "e1", False), ("conv2.eps", "e2", False))
        keys = lambda k: (self.EPS_KEYS[k - 1:k] if self.train_eps else ()) + (
            (f"conv{k}.nn.0.weight", f"wa{k}", True), (f"conv{k}.nn.0.bias", f"ba{k}", False),
            (f"conv{k}.nn.2.weight", f"wb{k}", True), (f"conv{k}.nn.2.bias", f"bb{k}", False))
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]      # the trainable tensors, named_parameters() order
        self._eps_fixed = None

    def _shapes(self, f_in):
        h = self.hidden
        s = super()._shapes(f_in)
        for k in ("w1", "b1", "w2", "b2"):
            del s[k]
        s.update(e1=(1,), e2=(1,), wa1=(f_in, h), wb1=(h, h), wa2=(h, h), wb2=(h, h), ba1=(h,), bb1=(h,), ba2=(h,), bb2=(h,))
        return s

    def _initial(self, f_in, shapes, offs):
        if not self.train_eps:                  # eps stays a device scalar (a loaded checkpoint may carry a value), outside the
            self._eps_fixed = self.ctx.zeros(8)                       # flat buffers: no gradient, no update
        h, u = self.hidden, self._uniform
        return {"wa1": u(f_in, f_in, h), "ba1": u(f_in, h), "wb1": u(h, h, h), "bb1": u(h, h),
                "wa2": u(h, h, h), "ba2": u(h, h), "wb2": u(h, h, h), "bb2": u(h, h), **self._head_initial(shapes)}

    def _eps(self, k):
        """conv k's eps as a device array of one float: a parameter with train_eps, a constant otherwise."""
        return self.p[f"e{k}"] if self.train_eps else self._eps_fixed.flat(4 * (k - 1), 1)

    def state_dict(self):
        d = super().state_dict()
        if self.train_eps:
            return d
        fixed = self._eps_fixed.numpy()          # both constants in one copy: conv k's at float 4 (k - 1)
        out = {}
        for tk, v in d.items():                 # conv{k}.eps in front of conv{k}.nn.0.weight, as PyG lists its buffer
            for k, (ek, _, _) in enumerate(self.EPS_KEYS):
                if tk == f"conv{k + 1}.nn.0.weight":
                    out[ek] = fixed[4 * k:4 * k + 1].copy()
            out[tk] = v
        return out

    def load_state_dict(self, d):
        super().load_state_dict(d)
        if not self.train_eps:
            missing = [tk for tk, _, _ in self.EPS_KEYS if tk not in d]
            if missing:
                raise KeyError(f"{self._name}.load_state_dict: missing {missing}")
            for tk, k, _ in self.EPS_KEYS:
                self._eps(int(k[1])).copy_from_host(np.asarray(d[tk], np.float32).reshape(1))

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        if "t1" not in bufs:
            v, n, h = self._views(), batch.n, self.hidden
            bufs["t1"], bufs["u1"], bufs["u2"] = v("t1", n, batch.f), v("u1", n, h), v("u2", n, h)
            bufs["t2"], bufs["dt2"] = bufs["s2"], bufs["t"]             # (conv2's T and dT in the base class's buffers)
            if self.train_eps:
                bufs["dt1"] = v("dt1", n, batch.f)
                np_ = D.gin_eps_grad_parts(n)
                bufs["eps_parts"] = v("eps_parts", 1, np_).flat(0, np_)
        return bufs

    def _one_launch(self, x, k1, k2, *others):
        return (self._fused and D.gin_conv_ok(self.ctx, x.shape[0], x.shape[1], k1, k2, x.ld)
                and all(a.ptr % 16 == 0 and a.ld % 4 == 0 for a in (x,) + others))

    def _conv_fwd(self, a, x, k, bufs, keep):
        """z_k = relu(T W_a + b_a) W_b + b_b, T = (1 + eps) x + A x: one launch, or the composed route.  t_k and u_k: room for T
        and the ReLU output (the operands of the weight gradients, and the mask), which the one launch stores only with ``keep``
        (a step that goes on to the gradients); the composed route passes through them either way."""
        ctx, p = self.ctx, self.p
        wa, ba, wb, bb, z, t, u, _, _ = self._KEYS[k]
        wa, ba, wb, bb, out, t, u = p[wa], p[ba], p[wb], p[bb], bufs[z], bufs[t], bufs[u]
        if self._one_launch(x, wa.shape[1], wb.shape[1], out, t, u):
            D.gin_conv(ctx, a, x, self._eps(k), wa, ba, wb, bb, out, t=t if keep else None, u=u if keep else None)
            return
        D.gin_aggregate(ctx, a, x, self._eps(k), t)
        D.gemm(ctx, t, wa, ba, u, act="relu")
        D.gemm(ctx, u, wb, bb, out)

    def _conv_bwd(self, a_t, x, k, dz, bufs, dx):
        """dZ_k -> conv k's gradients and, with dx, the gradient of its input.  dt_k: room for dT = dU W_a^T (train_eps, or the
        composed dX)."""
        ctx, p, g = self.ctx, self.p, self.g
        wa, ba, wb, bb, _, t, u, dt, e = self._KEYS[k]
        t, u, dt = bufs[t], bufs[u], bufs.get(dt)
        du = bufs["h1"]                                                             # (forward scratch of the base class: free here)
        D.act_bias_grad(ctx, dz, None, dz, None, db=g[bb])                           # db_b: column sums of dZ
        D.gemm_dx(ctx, dz, p[wb], du, y_mask=u, db=g[ba])                            # dU = (dZ W_b^T) * [U > 0], db_a
        D.gemm_dw2(ctx, u, dz, g[wb], t, du, g[wa])                                  # dW_b = U^T dZ, dW_a = T^T dU
        if self.train_eps:
            D.gemm_dx(ctx, du, p[wa], dt)                                           # dT = dU W_a^T
            D.gin_eps_grad(ctx, x, dt, bufs["eps_parts"], g[e])                      # d eps = sum <x, dT>
            if dx is not None:
                D.gin_aggregate(ctx, a_t, dt, self._eps(k), dx)                     # dX = (1 + eps) dT + A^T dT
        elif dx is not None:
            if self._one_launch(du, x.shape[1], 0, dx):
                D.gin_conv(ctx, a_t, du, self._eps(k), p[wa], None, None, None, dx, w_transposed=True)
                return
            D.gemm_dx(ctx, du, p[wa], dt)
            D.gin_aggregate(ctx, a_t, dt, self._eps(k), dx)


class GINE(GIN):
    """``GIN`` whose neighbour sum reads the edge features: both convolutions are PyG's GINEConv(Sequential(Linear, ReLU, Linear),
    train_eps, edge_dim=D) (Hu et al.) -- the cheapest way to use the dca / proximity values the reference computes on every
    contact and bridge and its model drops (gcn_utills.py:319-443; gcn.py:71): one add and one ReLU per gathered element,

        out_i = MLP((1 + eps) x_i + sum_{j in N(i)} relu(x_j + lin(e_ij))),   lin = Linear(D, in)

        GINEConv(F->H)·BN·PReLU -> GINEConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    ``GINE([ctx,] hidden_channels=64, edge_dim=2, train_eps=False, num_classes=1, seed=0)``; edge_dim 1 .. 8 (None, PyG's "e is
    already as wide as x", has no kernel).  The model reads ``batch.e`` (``uses_edge_features``): inputs are (x, a, e, i), a
    DeviceBatch that carries e, or the batches of DeviceDisjointLoader(DeviceDataset(..., edge_features=True)), which arrive
    with e and the transposed pattern gathered on the device.  The pattern and e are used as stored on every route: no
    self-loop is added or removed, a stored one is one more neighbour with its own features.  Everything behind the
    convolutions is ``GCN``'s (readout="attention" and norm="graph" included); eps, its place in ``state_dict()`` and the flat
    buffer are ``GIN``'s.  One device: ``comm`` is refused.

    Hot path per convolution (gine_forward / gine_backward of gcnx/convs.py, the one place the sequence is written;
    gcnx.GINEConv runs the same two functions): gcnx_gine_conv, one launch (csrc/gine.hip), which keeps T and U; backward
    gcnx_act_bias_grad, gcnx_gemm_dx(y_mask=U, db), gcnx_gemm_dw2, gcnx_gemm_dx -> dT, gcnx_gine_bwd_edges (forward CSR: dW_e,
    db_e), gcnx_gin_eps_grad (train_eps) and, for conv2 only, gcnx_gine_bwd_nodes (transposed pattern + entry permutation).
    GCNX_GINE_FUSED=0 (read at construction), and any shape gcnx_gine_conv refuses (hidden > 128; a gathered width outside
    {16, 32, 64, 128}), takes the composed route per launch: gcnx_gine_aggregate, gcnx_gemm(relu), gcnx_gemm.

    Weights: ``GIN``'s keys and, behind each convolution's ``nn.*``, ``conv{1,2}.lin.weight`` ([in, D] as torch; stored [D, in])
    and ``conv{1,2}.lin.bias``.  The key order follows PyG's source (eps, nn.*, lin.*); it was not confirmed against a live
    torch_geometric: prefer the named dicts.  Initialisation U(+-1/sqrt(fan_in)) as torch's Linear (lin: fan_in = D), eps 0."""

    OPERATOR, SELF_LOOPS, KERNELS = "perm", False, "GINEConv"
    _KEYS = _conv_keys("wa", "ba", "wb", "bb", "z", "t", "u", "dt", "e", "we", "bl")
    uses_edge_features = True

    def _init(self, ctx, hidden_channels=64, edge_dim=2, train_eps=False, num_classes=1, seed=0, comm=None):
        self._one_device(comm)
        if edge_dim is None:
            raise NotImplementedError(f"{self._name}: edge_dim=None (edge features already as wide as the input) has no kernel; "
                                      "edge_dim must be 1 .. 8")
        self.edge_dim = self._check_edge_dim(edge_dim)
        super()._init(ctx, hidden_channels, train_eps, num_classes, seed, None)
        self._fused = os.environ.get("GCNX_GINE_FUSED", "1") != "0"    # knob, read once
        conv = lambda k: ((f"e{k}",) if self.train_eps else ()) + (f"wa{k}", f"ba{k}", f"wb{k}", f"bb{k}", f"we{k}", f"bl{k}",
                                                                   f"g{k}", f"be{k}", f"a{k}")
        self.PARAM_ORDER = conv(1) + conv(2) + GCN.PARAM_ORDER[10:]
        keys = lambda k: (self.EPS_KEYS[k - 1:k] if self.train_eps else ()) + (
            (f"conv{k}.nn.0.weight", f"wa{k}", True), (f"conv{k}.nn.0.bias", f"ba{k}", False),
            (f"conv{k}.nn.2.weight", f"wb{k}", True), (f"conv{k}.nn.2.bias", f"bb{k}", False),
            (f"conv{k}.lin.weight", f"we{k}", True), (f"conv{k}.lin.bias", f"bl{k}", False))
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        h, d = self.hidden, self.edge_dim
        s.update(we1=(d, f_in), we2=(d, h), bl1=(f_in,), bl2=(h,))
        return s

    def _initial(self, f_in, shapes, offs):
        if not self.train_eps:                  # (as GIN: the two constants outside the flat buffers)
            self._eps_fixed = self.ctx.zeros(8)
        h, d, u = self.hidden, self.edge_dim, self._uniform
        init = {}
        for k, f in ((1, f_in), (2, h)):        # drawn in PyG's order per convolution: nn.0, nn.2, lin
            init[f"wa{k}"], init[f"ba{k}"] = u(f, f, h), u(f, h)
            init[f"wb{k}"], init[f"bb{k}"] = u(h, h, h), u(h, h)
            init[f"we{k}"], init[f"bl{k}"] = u(d, d, f), u(d, f)
        init.update(self._head_initial(shapes))
        return init

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        if "gine_scratch" not in bufs:
            v, n = self._views(), batch.n
            if "dt1" not in bufs:                # (GIN forms dT of conv1 with train_eps only; here dW_e needs it always)
                bufs["dt1"] = v("dt1", n, batch.f)
            ns = max(D.gine_bwd_scratch_floats(self.ctx, n, max(batch.f, self.hidden), self.edge_dim), 4)
            bufs["gine_scratch"] = v("gine_scratch", 1, ns).flat(0, ns)
        return bufs

    def _one_launch(self, x, k1, k2, *others):
        return (self._fused and D.gine_conv_ok(self.ctx, x.shape[0], x.shape[1], k1, k2, x.ld, self.edge_dim)
                and all(a.ptr % 16 == 0 and a.ld % 4 == 0 for a in (x,) + others))

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        wa, ba, wb, bb, z, t, u, _, _, we, bl = self._KEYS[k]
        out, t, u = bufs[z], bufs[t], bufs[u]
        convs.gine_forward(self.ctx, a, x, bufs["e"], self._eps(k), p[we], p[bl], p[wa], p[ba], p[wb], p[bb], t, u, out,
                           self._one_launch(x, p[wa].shape[1], p[wb].shape[1], out, t, u), keep)

    def _conv_bwd(self, a, x, k, dz, bufs, dx):
        p, g = self.p, self.g
        wa, ba, wb, bb, _, t, u, dt, e, we, bl = self._KEYS[k]
        convs.gine_backward(self.ctx, a, x, bufs["e"], self._eps(k), bufs[t], bufs[u], dz, p[we], p[bl], p[wa], p[wb],
                            g[e] if self.train_eps else None, g[we], g[bl], g[wa], g[ba], g[wb], g[bb], bufs["h1"], bufs[dt],
                            bufs["gine_scratch"], bufs.get("eps_parts"), dx)


class PDN(GCN):
    """``GCN`` whose two GCNConv layers take an ``edge_weight`` learned from the edge features: both convolutions are PyG's
    PDNConv(in, out, edge_dim=D, hidden_channels=He) (Pathfinder Discovery Networks, Rozemberczki et al. 2021) -- the smallest
    way to use the dca / proximity values the reference computes on every contact and bridge and its model drops
    (gcn_utills.py:319-443; gcn.py:71): the convolution stays GCNConv, only its operator is learned,

        w_e = sigmoid(Linear(He, 1)(relu(Linear(D, He)(e_ij))))      A^_v[i, j] = deg_i^-1/2 w_e deg_j^-1/2,  deg_i = sum_row w_e

        PDNConv(F->H)·BN·PReLU -> PDNConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    ``PDN([ctx,] hidden_channels=64, edge_dim=2, edge_hidden=16, num_classes=1, seed=0)``; edge_dim 1 .. 8 (None raises: the
    model is nothing without it), edge_hidden 1 .. 64 (what csrc/pdn.hip serves).  The model reads ``batch.e``
    (``uses_edge_features``): inputs are (x, a, e, i), a DeviceBatch that carries e, or the batches of
    DeviceDisjointLoader(DeviceDataset(..., edge_features=True)).  Self-loops are PyG's add_remaining_self_loops(fill_value=1):
    a DeviceCSR / a DeviceBatch is used as stored, a stored loop being an entry like any other that goes through the MLP (the
    reference's graphs carry every loop); a host adjacency gets the missing loops with weight exactly 1, outside the MLP and
    without a gradient (_with_unit_self_loops; the flags ride on the batch as ``DeviceBatch.unit``).  Everything behind the
    convolutions is ``GCN``'s (readout="attention" and norm="graph" included).  One device: ``comm`` is refused.

    Each convolution has its own gate MLP and so its own operator pair (A^_v and, for the backward, a CSR of the transposed
    pattern with the same values: A^_v is not symmetric even on a symmetric pattern), rebuilt every step.  Hot path per
    convolution (pdn_forward / pdn_backward of gcnx/convs.py, the one place the sequence is written; gcnx.PDNConv runs the same
    two functions): gcnx_pdn_operator (csrc/pdn.hip), then GCNConv's launches; backward GCNConv's launches on the transposed
    operator, gcnx_gemm_dx -> dZ W^T where they did not leave it, gcnx_sddmm_csr -> dLoss/dv, gcnx_pdn_operator_bwd.  No
    gradient flows to the edge features.

    ``edge_weights(inputs)`` -> (w_1, w_2): the gates of both convolutions before normalisation, host arrays [nnz] in the
    batch's CSR order (1 on added loops), from a forward in evaluation mode: a trained-in answer to "which contacts matter"
    (``gcnx.explain.edge_layout`` gives the entries' (source, target) and graphs).

    Weights: per ``conv{1,2}``, PyG's names ``.bias`` [H], ``.lin.weight`` [H, in], ``.mlp.0.weight`` [He, D], ``.mlp.0.bias``
    [He], ``.mlp.2.weight`` [1, He], ``.mlp.2.bias`` [1] in that order (a module's own parameters before its children's), then
    ``GCN``'s.  The order follows PyG's source, not a live module: prefer the named dicts.  Initialisation as PyG's
    reset_parameters: glorot-uniform weights drawn lin, mlp.0, mlp.2 per convolution, zero biases, then the head."""

    OPERATOR, KERNELS = "perm", "PDNConv"
    MAX_EDGE_HIDDEN = 64
    _KEYS = _conv_keys("w", "b", "z", "pa", "pb", "pc", "pd", "pw", "pr", "pt")
    uses_edge_features = True
    _pending_unit = None

    def _init(self, ctx, hidden_channels=64, edge_dim=2, edge_hidden=16, num_classes=1, seed=0, comm=None):
        self._one_device(comm)
        if edge_dim is None:
            raise NotImplementedError(f"{self._name}: edge_dim=None: the model learns its edge weights from the edge features; "
                                      "edge_dim must be 1 .. 8")
        self.edge_dim = self._check_edge_dim(edge_dim)
        if not 1 <= int(edge_hidden) <= self.MAX_EDGE_HIDDEN:
            raise NotImplementedError(f"{self._name}: edge_hidden={edge_hidden} must be 1 .. {self.MAX_EDGE_HIDDEN} (what the "
                                      f"{self.KERNELS} kernels serve)")
        self.edge_hidden = int(edge_hidden)
        super()._init(ctx, hidden_channels, num_classes, seed, None)
        conv = lambda k: (f"w{k}", f"b{k}", f"pa{k}", f"pb{k}", f"pc{k}", f"pd{k}", f"g{k}", f"be{k}", f"a{k}")
        self.PARAM_ORDER = conv(1) + conv(2) + GCN.PARAM_ORDER[10:]
        keys = lambda k: ((f"conv{k}.bias", f"b{k}", False), (f"conv{k}.lin.weight", f"w{k}", True),
                          (f"conv{k}.mlp.0.weight", f"pa{k}", True), (f"conv{k}.mlp.0.bias", f"pb{k}", False),
                          (f"conv{k}.mlp.2.weight", f"pc{k}", True), (f"conv{k}.mlp.2.bias", f"pd{k}", False))
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        d, he = self.edge_dim, self.edge_hidden
        for k in (1, 2):                        # stored [in, out]: mlp.0.weight [D, He], mlp.2.weight [He, 1]
            s.update({f"pa{k}": (d, he), f"pb{k}": (he,), f"pc{k}": (he, 1), f"pd{k}": (1,)})
        return s

    def _initial(self, f_in, shapes, offs):
        h, d, he, rng = self.hidden, self.edge_dim, self.edge_hidden, self._rng
        init = {}
        for k, f in ((1, f_in), (2, h)):        # PyG's reset_parameters per convolution: lin, mlp.0, mlp.2; every bias zero
            init[f"w{k}"] = glorot_uniform(rng, f, h)
            init[f"pa{k}"] = glorot_uniform(rng, d, he)
            init[f"pc{k}"] = glorot_uniform(rng, he, 1)
        init.update(self._head_initial(shapes))
        return init

    def _host_inputs(self, inputs):
        """A host matrix gets the missing loops as unit entries; their flags wait in ``_pending_unit`` for ``_ensure``, which sees
        the batch built from these inputs next.  A DeviceCSR goes in as stored."""
        x, a, e, i = inputs
        self._pending_unit = None
        if not isinstance(a, D.DeviceCSR):
            a, e, self._pending_unit = _with_unit_self_loops(a, e, np.asarray(x).shape[0])
        return (x, a, e, i)

    def _ensure(self, batch, sharded=False):
        unit, self._pending_unit = self._pending_unit, None
        if unit is not None and batch.unit is None and unit.size == batch.a.nnz:
            batch.unit = self.ctx.to_device(unit, np.uint8)
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        nnz = batch.a.nnz
        if bufs.get("pdn_key") != (batch.n, batch.n_graphs, nnz):          # the entry buffers follow nnz as well as (n, b)
            v, n, ne = self._views(), batch.n, max(nnz, 1)
            for k in (1, 2):
                for name in ("pw", "pv", "pvt"):
                    bufs[f"{name}{k}"] = v(f"{name}{k}", 1, ne).flat(0, ne)
                bufs[f"pr{k}"] = v(f"pr{k}", 1, n).flat(0, n)
            bufs["pt1"], bufs["pt2"] = v("pt1", n, batch.f), v("pt2", n, self.hidden)
            bufs["pg"] = v("pg", 1, ne).flat(0, ne)
            ns = max(D.pdn_bwd_scratch_floats(self.ctx, n, nnz, self.edge_dim, self.edge_hidden), 4)
            bufs["pdn_scratch"] = v("pdn_scratch", 1, ns).flat(0, ns)
            bufs["pdn_key"], bufs["pdn_ops"] = (batch.n, batch.n_graphs, nnz), None
        bufs["unit"] = batch.unit
        return bufs

    def _pair(self, a, bufs, k):
        """Conv k's operator pair on the pattern ``a``: CSRs of the pattern and of its transposed pattern over the value
        buffers gcnx_pdn_operator fills every step.  Built once per (batch, buffers); never the symmetric shortcut."""
        ops = bufs["pdn_ops"]
        if ops is None or ops[0] is not a:
            rp_t, ci_t, _ = a.transpose_perm()
            mk = lambda rp, ci, vals: D.DeviceCSR(self.ctx, a.n, a.nnz, rp, ci, vals, a.block_ptr, a.n_blocks, False, a.max_block_rows)
            ops = bufs["pdn_ops"] = (a, {j: (mk(a.rowptr, a.colidx, bufs[f"pv{j}"]), mk(rp_t, ci_t, bufs[f"pvt{j}"])) for j in (1, 2)})
        return ops[1][k]

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        w, b, z, pa, pb, pc, pd, pw, pr, _ = self._KEYS[k]
        a_v, a_vt = self._pair(a, bufs, k)
        ok = convs.pdn_forward(self.ctx, a, a_v, a_vt, x, bufs["e"], bufs["unit"], p[pa], p[pb], p[pc], p[pd], p[w], p[b], bufs[pw],
                               bufs[pr], bufs[z], bufs["h1"], s=bufs["s2"] if keep and k == 2 else None)
        if k == 2:
            bufs["s2_ok"] = ok

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, b, _, pa, pb, pc, pd, pw, pr, pt = self._KEYS[k]
        s = bufs["s2"] if dx is not None and bufs["s2_ok"] else None
        convs.pdn_backward(self.ctx, a, self._pair(a, bufs, k)[1], x, bufs["e"], bufs["unit"], p[pa], p[pb], p[pc], p[pd], bufs[pw],
                           bufs[pr], dzk, p[w], g[w], g[b], g[pa], g[pb], g[pc], g[pd], bufs["t"], bufs[pt], bufs["pg"],
                           bufs["pdn_scratch"], dx, s)

    def edge_weights(self, inputs):
        """(w_1, w_2): the gates of conv1 and conv2 before normalisation, host arrays [nnz] in the batch's CSR order, from a
        forward in evaluation mode.  An added unit loop reads 1."""
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "fwd")
        nnz = batch.a.nnz
        return bufs["pw1"].numpy()[:nnz].copy(), bufs["pw2"].numpy()[:nnz].copy()


class APPNP(GCN):
    """``GCN`` with each GCNConv replaced by ``Linear`` + PyG's ``APPNP(K, alpha)`` (Gasteiger et al. 2019, "Predict then
    propagate"; Spektral's APPNPConv), the long-range layer for the slot the reference's author left open
    (gcn_utills.py:804-806): two one-hop convolutions see a residue's 2-hop neighbourhood, K hops of personalised PageRank
    reach the inter-chain bridges from most of a chain.

        Linear(F->H)·APPNP(K, alpha)·BN·PReLU -> Linear(H->H)·APPNP(K, alpha)·BN·PReLU -> global_max_pool -> the head of ``GCN``

        APPNP(K, alpha):  z^0 = h      z^{k+1} = (1 - alpha) A^ z^k + alpha h      A^ = GCNConv's operator (gcn_norm, self-loops)

    ``APPNP([ctx,] hidden_channels=64, K=10, alpha=0.1, num_classes=1, seed=0, comm=None, readout=, norm=)``: K an int in
    0 .. 64 (0: a node MLP), alpha in [0, 1].  The propagation has no parameters and keeps nothing for the backward, which is
    the same propagation on A^^T.  Everything else is ``GCN``'s: the operator, BN·PReLU, the pool pair, the head,
    readout="attention", norm="graph", ``fit``, and sync-BN over shards (``comm=``): the propagation never crosses a graph, so
    a shard's rows are all it needs.

    Hot path per layer (appnp_forward / appnp_backward of gcnx/convs.py; gcnx.APPNPConv runs the same two functions): gcnx_gemm,
    then gcnx_appnp_propagate (csrc/appnp.hip) -- one launch that keeps each graph's rows in LDS across all K hops, or K launches
    where the library streams (K below 3 -- below 2 on graphs of up to 256 rows --, hidden_channels not a multiple of 4, a graph too
    tall for LDS, a batch that does not know its tallest graph); backward gcnx_appnp_propagate on
    the transposed operator, then the Linear's gradients.  GCNX_APPNP_RESIDENT=0 (read at construction) streams always.

    Weights: torch key names ``lin{1,2}.weight`` ([out, in], as torch; stored [in, out] here), ``lin{1,2}.bias``, then
    ``GCN``'s.  Initialisation as torch's Linear, U(+-1/sqrt(fan_in)), drawn lin1.weight, lin1.bias, lin2.weight, lin2.bias,
    then the head.  The key names are this model's own (PyG's APPNP has no parameters; the Linears are named as a module that
    declares them would): prefer the named dicts."""

    TORCH_KEYS = (("lin1.weight", "w1", True), ("lin1.bias", "b1", False),
                  ("lin2.weight", "w2", True), ("lin2.bias", "b2", False)) + GCN.TORCH_KEYS[4:]
    PROBE_KEY = "lin1.weight"
    OPERATOR, SELF_LOOPS, KERNELS = "gcn", True, "APPNP"
    MAX_K = 64

    def _init(self, ctx, hidden_channels=64, K=10, alpha=0.1, num_classes=1, seed=0, comm=None):
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 0 <= int(K) <= self.MAX_K:
            raise NotImplementedError(f"{self._name}: K={K!r} must be an int in 0 .. {self.MAX_K} (what the {self.KERNELS} kernels serve)")
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"{self._name}: alpha={alpha!r} must be in [0, 1]")
        self.K, self.alpha = int(K), float(alpha)
        super()._init(ctx, hidden_channels, num_classes, seed, comm)
        self._col_block = 0 if os.environ.get("GCNX_APPNP_RESIDENT", "1") != "0" else -1    # knob, read once

    def _initial(self, f_in, shapes, offs):
        h, u = self.hidden, self._uniform
        return {"w1": u(f_in, f_in, h), "b1": u(f_in, h), "w2": u(h, h, h), "b2": u(h, h), **self._head_initial(shapes)}

    def _conv_fwd(self, a_hat, x, k, bufs, keep):
        """z_k = P (x W_k + b_k): the Linear into bufs["h1"], then the K hops."""
        p = self.p
        w, b, z = self._KEYS[k]
        convs.appnp_forward(self.ctx, a_hat, x, p[w], p[b], bufs["h1"], bufs[z], self.K, self.alpha, bufs["s2"],
                            col_block=self._col_block)

    def _conv_bwd(self, a_t, x, k, dzk, bufs, dx):
        """dZ_k -> dH = P^T dZ_k in bufs["t"], the Linear's gradients and, with dx, dx = dH W^T."""
        p, g = self.p, self.g
        w, b, _ = self._KEYS[k]
        convs.appnp_backward(self.ctx, a_t, x, dzk, p[w], g[w], g[b], bufs["t"], self.K, self.alpha, bufs["s2"], dx,
                             col_block=self._col_block)


class Cheb(GCN):
    """``GCN`` with each GCNConv replaced by PyG's ``ChebConv(in, hidden, K, normalization="sym", lambda_max)`` (Defferrard et al.
    2016; Spektral's ChebConv with K one less), the K-hop layer with one weight matrix per hop distance, for the slot the
    reference's author left open (gcn_utills.py:804-806): with K = 3 .. 5 a residue's filter weighs "itself", "contacts" and
    "contacts of contacts" separately, and because T_1 = L^ = -S at lambda_max = 2 it can learn differences between a residue and
    its neighbourhood (a high-pass filter), which GCNConv's low-pass operator cannot.

        ChebConv(F->H, K)·BN·PReLU -> ChebConv(H->H, K)·BN·PReLU -> global_max_pool -> the head of ``GCN``

        ChebConv:  out = sum_{k < K} T_k(L^) x W_k + b     T_0 = I  T_1 = L^  T_k = 2 L^ T_{k-1} - T_{k-2}
                   L^ = -(2 / lambda_max) S + (2 / lambda_max - 1) I      S = D^-1/2 A D^-1/2 without the loops (get_laplacian)

    ``Cheb([ctx,] hidden_channels=64, K=3, lambda_max=2.0, num_classes=1, seed=0, comm=None, readout=, norm=)``: K the number of
    terms, an int in 1 .. 16 (1: a node MLP); lambda_max a number > 0 -- nothing is estimated, and a value below the operator's
    largest eigenvalue makes the terms grow with k.  The adjacency is used as stored, unweighted: a stored loop is ignored, an
    isolated node gets L^ z = (2 / lambda_max - 1) z.  Everything else is ``GCN``'s: BN·PReLU, the pool pair, the head,
    readout="attention", norm="graph", ``fit``, and sync-BN over shards (``comm=``): no term crosses a graph.

    Hot path per layer (cheb_forward / cheb_backward of gcnx/convs.py; gcnx.ChebConv runs the same two functions): gcnx_gemm
    (H = x [W_0 | .. | W_{K-1}]), then gcnx_cheb_sum (csrc/cheb.hip) -- Clenshaw summation, K - 1 gathers in one launch that keeps
    each graph's rows in LDS, or K - 1 launches where the library streams (fewer than 3 gathers -- 2 on graphs of up to 256 rows
    --, hidden_channels not a multiple of 4, a graph too tall for LDS, a batch that does not know its tallest graph); backward
    gcnx_cheb_basis on the transposed operator (G = [T_k(L^^T) dZ], K - 1 gathers), one gcnx_gemm_dw and one gcnx_gemm_dx over
    the K H wide panel.  Nothing is kept for the backward.  GCNX_CHEB_RESIDENT=0 (read at construction) streams always.

    Weights: PyG's key names ``conv{1,2}.lins.{k}.weight`` ([out, in], as torch; the column blocks of one stacked [in, K out]
    tensor here), ``conv{1,2}.bias``, then ``GCN``'s.  Initialisation as PyG's: glorot-uniform weights drawn conv1.lins.0 ..
    conv2.lins.{K-1}, zero biases, then the head.  The order follows PyG's source, not a live module: prefer the named dicts."""

    PROBE_KEY = "conv1.lins.0.weight"
    OPERATOR, SELF_LOOPS, KERNELS = "cheb", False, "Chebyshev"
    MAX_K = 16

    def _init(self, ctx, hidden_channels=64, K=3, lambda_max=2.0, num_classes=1, seed=0, comm=None):
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= self.MAX_K:
            raise NotImplementedError(f"{self._name}: K={K!r} must be an int in 1 .. {self.MAX_K} (what the {self.KERNELS} kernels serve)")
        if not float(lambda_max) > 0.0 or not np.isfinite(float(lambda_max)):
            raise ValueError(f"{self._name}: lambda_max={lambda_max!r} must be a finite number > 0")
        self.K, self.lambda_max = int(K), float(lambda_max)
        super()._init(ctx, hidden_channels, num_classes, seed, comm)
        self._col_block = 0 if os.environ.get("GCNX_CHEB_RESIDENT", "1") != "0" else -1     # knob, read once
        blocks = lambda c: tuple(f"w{c}_{k}" for k in range(self.K))
        self.STACKS = {"w1": blocks(1), "w2": blocks(2)}        # lins.k.weight^T: the column blocks of the stacked weights
        keys = lambda c: tuple((f"conv{c}.lins.{k}.weight", f"w{c}_{k}", True) for k in range(self.K)) + ((f"conv{c}.bias", f"b{c}", False),)
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        s.update(w1=(f_in, self.K * self.hidden), w2=(self.hidden, self.K * self.hidden))
        return s

    def _initial(self, f_in, shapes, offs):
        h, rng = self.hidden, self._rng
        stack = lambda f: np.concatenate([glorot_uniform(rng, f, h) for _ in range(self.K)], axis=1)
        return {"w1": stack(f_in), "w2": stack(h), **self._head_initial(shapes)}

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        if "ch" not in bufs:                # H = x W and G = [T_k(L^^T) dZ]: one [n, K hidden] panel serves both directions
            bufs["ch"] = self._views()("cheb_panel", batch.n, self.K * self.hidden)
        return bufs

    def _conv_fwd(self, s_op, x, k, bufs, keep):
        """z_k = sum_j T_j(L^) (x W_k)_j + b_k: the product into bufs["ch"], then the Clenshaw sum."""
        p = self.p
        w, b, z = self._KEYS[k]
        convs.cheb_forward(self.ctx, s_op, x, p[w], p[b], bufs["ch"], bufs[z], self.K, self.lambda_max, bufs["s2"],
                           col_block=self._col_block)

    def _conv_bwd(self, s_t, x, k, dzk, bufs, dx):
        """dZ_k -> the bias gradient, G = [T_j(L^^T) dZ_k] in bufs["ch"], dW = x^T G and, with dx, dx = G W^T."""
        p, g = self.p, self.g
        w, b, _ = self._KEYS[k]
        convs.cheb_backward(self.ctx, s_t, x, dzk, p[w], g[w], g[b], bufs["ch"], self.K, self.lambda_max, bufs["s2"], dx,
                            col_block=self._col_block)


class RGCN(GCN):
    """``GCN`` with each GCNConv replaced by PyG's ``RGCNConv(in, hidden, num_relations, aggr="mean", root_weight, bias=True)``
    (Schlichtkrull et al. 2018) without a decomposition: every stored entry has a type, and every type its own weights.  The
    reference's graphs hold two kinds of edge -- the intra-chain contacts of each protein and the inter-chain DCA bridges that
    link_graphs adds between them (gcn_utills.py:319) -- and mark them in the edge features: dca is set on the bridges only,
    proximity on the contacts only (gcn_utills.py:379-443).  Every other model here sums both kinds through one weight matrix
    or reads the two numbers as continuous features.

        RGCNConv(F->H)·BN·PReLU -> RGCNConv(H->H)·BN·PReLU -> global_max_pool -> the head of ``GCN``

        RGCNConv:  out_i = x_i W_root + b + sum_{r < R} mean_{k in N_r(i)} x_col(k) W_r      N_r(i): row i's entries of relation r

    ``RGCN([ctx,] hidden_channels=64, num_relations=None, relations="nonzero", edge_dim=2, root_weight=True, num_classes=1,
    seed=0, comm=None, readout=, norm=)``; R = num_relations is 1 .. 4.  The adjacency is used as stored, unweighted: no loop is
    added or removed, a stored loop is an entry like any other, the mean over no entry is 0.  The relation of an entry is read
    off ``batch.e`` on the device, once per batch (gcnx_rgcn_operator, kept with the batch's operator):

      relations="nonzero"   the first column d with e[k, d] != 0; edge_dim where there is none; R = edge_dim + 1.  With the
                            reference's features (dca, proximity): bridges 0, contacts 1, and 2 for an entry that carries
                            neither (a stored loop, a proximity that processed to exactly 0).
      relations="index"     e has one column holding the relation as an integer-valued float; num_relations must be given.
                            Host inputs are checked in NumPy before the upload (ValueError for a value that is not an integer
                            in 0 .. R - 1); a DeviceBatch is not read back: the kernel clamps a value outside the range into it.

    The model reads ``batch.e`` (``uses_edge_features``): inputs are (x, a, e, i), a DeviceBatch that carries e, or the batches
    of DeviceDisjointLoader(DeviceDataset(..., edge_features=True)).  Everything behind the convolutions is ``GCN``'s
    (readout="attention", norm="graph" and ``fit`` included).  One device: ``comm`` is refused.

    Hot path per convolution (rgcn_forward / rgcn_backward of gcnx/convs.py; gcnx.RGCNConv runs the same two functions):
    gcnx_rgcn_conv, one launch that gathers a row's entries once into R accumulators and multiplies [means | own rows] with the
    row-stacked weight (csrc/rgcn.hip), keeping the panel M = [mean_0 x | .. | mean_{R-1} x]; backward gcnx_act_bias_grad,
    gcnx_gemm_dw2 (dW = M^T dZ, dW_root = x^T dZ) and, for conv2, the same launch on the transposed pattern.
    GCNX_RGCN_FUSED=0 (read at construction), hidden_channels=256 and unaligned widths take the composed route per launch:
    gcnx_rgcn_aggregate, gcnx_gemm (+ gcnx_gemm, gcnx_add for the root); gcnx_rgcn_aggregate and R + 1 gcnx_gemm_dx backward.

    Weights: PyG's key names and layouts ``conv{1,2}.weight`` [R, in, out], ``conv{1,2}.root`` [in, out] (with root_weight),
    ``conv{1,2}.bias`` [out], then ``GCN``'s.  Stored as one row-stacked [(R + 1) in, out] tensor per convolution, which the
    kernel reads and whose gradient the weight-gradient launch writes.  Initialisation as PyG's: glorot-uniform weights, then
    root, drawn conv1 before conv2, zero biases, then the head.  The order follows PyG's source, not a live module: prefer the
    named dicts."""

    OPERATOR, SELF_LOOPS, KERNELS = "perm", False, "RGCNConv"
    MAX_RELATIONS = 4
    RULES = ("nonzero", "index")
    uses_edge_features = True
    _KEYS = _conv_keys("w", "b", "z", "pm")
    _rel_ops = None

    def _init(self, ctx, hidden_channels=64, num_relations=None, relations="nonzero", edge_dim=2, root_weight=True, num_classes=1,
              seed=0, comm=None):
        self._one_device(comm)
        if relations not in self.RULES:
            raise ValueError(f"{self._name}: relations={relations!r} must be \"nonzero\" or \"index\"")
        if relations == "index":
            if num_relations is None:
                raise ValueError(f"{self._name}: relations=\"index\" needs num_relations")
            edge_dim = 1
        else:
            edge_dim = self._check_edge_dim(edge_dim)
            if edge_dim is None:
                raise ValueError(f"{self._name}: relations=\"nonzero\" reads the relation off the edge features; edge_dim must be 1 .. 3")
            if num_relations is not None and int(num_relations) != edge_dim + 1:
                raise ValueError(f"{self._name}: relations=\"nonzero\" has num_relations = edge_dim + 1 = {edge_dim + 1}, got "
                                 f"num_relations={num_relations}")
            num_relations = edge_dim + 1
        if isinstance(num_relations, bool) or not isinstance(num_relations, (int, np.integer)) or \
                not 1 <= int(num_relations) <= self.MAX_RELATIONS:
            raise NotImplementedError(f"{self._name}: num_relations={num_relations!r} must be an int in 1 .. {self.MAX_RELATIONS} "
                                      f"(what the {self.KERNELS} kernels serve)")
        self.R, self.relations, self.edge_dim, self.root_weight = int(num_relations), relations, int(edge_dim), bool(root_weight)
        super()._init(ctx, hidden_channels, num_classes, seed, None)
        self._fused = os.environ.get("GCNX_RGCN_FUSED", "1") != "0"    # knob, read once
        keys = lambda c: ((f"conv{c}.weight", f"wr{c}", False),) + (((f"conv{c}.root", f"wo{c}", False),) if self.root_weight else ()) + \
            ((f"conv{c}.bias", f"b{c}", False),)
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]

    @property
    def _nb(self):
        return self.R + (1 if self.root_weight else 0)

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        s.update(w1=(self._nb * f_in, self.hidden), w2=(self._nb * self.hidden, self.hidden))
        return s

    def _initial(self, f_in, shapes, offs):
        h, rng = self.hidden, self._rng
        stack = lambda f: np.concatenate([glorot_uniform(rng, f, h) for _ in range(self._nb)], axis=0)    # weight[0 .. R-1], root
        return {"w1": stack(f_in), "w2": stack(h), **self._head_initial(shapes)}

    def _name_blocks(self):
        """conv{c}.weight and conv{c}.root: the two row blocks of the stacked tensor, in ``p`` and ``g`` alike."""
        super()._name_blocks()
        h, r = self.hidden, self.R
        for t in (self.p, self.g):
            for c, f in ((1, self.f_in), (2, h)):
                t[f"wr{c}"] = t[f"w{c}"].flat(0, r * f * h, (r * f, h))
                if self.root_weight:
                    t[f"wo{c}"] = t[f"w{c}"].flat(r * f * h, f * h, (f, h))

    def _named(self, t):
        d = super()._named(t)
        for c in (1, 2):                        # PyG's [R, in, out]
            d[f"conv{c}.weight"] = d[f"conv{c}.weight"].reshape(self.R, -1, self.hidden)
        return d

    def _probe_f_in(self, d):
        return int(np.asarray(d["conv1.weight"]).shape[-2])

    def _host_state(self, d):
        if not self.built and "conv1.weight" in d:
            self.build(self._probe_f_in(d))
        d = dict(d)
        for c in (1, 2):                        # PyG's [R, in, out] into the stored [R in, out]
            w = np.asarray(d.get(f"conv{c}.weight", ()))
            if w.ndim == 3 and w.shape[0] == self.R:
                d[f"conv{c}.weight"] = w.reshape(-1, w.shape[2])
        return super()._host_state(d)

    def _host_inputs(self, inputs):
        """relations="index": the relation column of a host batch is checked here, before the upload."""
        if self.relations == "index":
            e = np.asarray(inputs[2])
            if e.ndim == 2 and e.shape[1] == 1 and e.size and not (np.all(e == np.floor(e)) and e.min() >= 0 and e.max() <= self.R - 1):
                raise ValueError(f"{self._name}(relations=\"index\"): e must hold integers in 0 .. {self.R - 1}")
        return super()._host_inputs(inputs)

    def _op(self, batch):
        """The pattern with its transposed pattern, and (rel, val, rel_t, val_t) of the batch's edge features: built once per
        batch object."""
        fresh = self._op_cache is None or self._op_cache[0] != batch.uid
        a, a_t = super()._op(batch)
        if fresh or self._rel_ops is None:
            self._rel_ops = a.rgcn_operator(batch.e, self.relations, self.R)
        return a, a_t

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        if "pm1" not in bufs:               # the panels M of both convolutions, and A^T dZ2's for the composed backward
            v, n, r = self._views(), batch.n, self.R
            bufs["pm1"], bufs["pm2"], bufs["pmt"] = v("pm1", n, r * batch.f), v("pm2", n, r * self.hidden), v("pmt", n, r * self.hidden)
        return bufs

    def _one_launch(self, x, fo, *others):
        return (self._fused and D.rgcn_conv_ok(self.ctx, x.shape[0], x.shape[1], fo, self.R, x.ld)
                and all(a.ptr % 16 == 0 and a.ld % 4 == 0 for a in (x,) + others))

    def _conv_fwd(self, a, x, k, bufs, keep):
        """z_k = [M | x] W_k + b_k, M = [mean_0 x | .. | mean_{R-1} x] kept in bufs["pm{k}"]: one launch, or the composed route."""
        p = self.p
        w, b, z, pm = self._KEYS[k]
        convs.rgcn_forward(self.ctx, a, self._rel_ops, x, p[w], p[b], bufs[pm], bufs[z], bufs["h1"], self.R, self.root_weight,
                           self._one_launch(x, self.hidden, bufs[z], bufs[pm]), keep)

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        """dZ_k -> conv k's gradients and, with dx, dx = dZ_k W_root^T + sum_r A_r^T (dZ_k W_r^T)."""
        p, g = self.p, self.g
        w, b, _, pm = self._KEYS[k]
        convs.rgcn_backward(self.ctx, a, self._rel_ops, x, bufs[pm], dzk, p[w], g[w], g[b], bufs["pmt"], self.R, self.root_weight,
                            dx is not None and self._one_launch(dzk, x.shape[1], dx), dx)


class PNA(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's PNAConv(aggregators=['mean', 'min', 'max', 'std'],
    scalers=['identity', 'amplification', 'attenuation'], deg, towers=1, pre_layers=1, post_layers=1, divide_input=False),
    Principal Neighbourhood Aggregation -- four statistics of every neighbourhood, each scaled by the node's degree:

        PNAConv(F->H)·BN·PReLU -> PNAConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    ``PNA([ctx,] hidden_channels=64, deg=None, avg_deg_log=None, num_classes=1, seed=0, comm=None)``: exactly one of ``deg``
    (PyG's in-degree histogram, ``PNA.degree_histogram(graphs)``) and ``avg_deg_log`` (delta, the mean of log(d + 1) over the
    training set's nodes) is required.  The adjacency is used exactly as stored (row = target): no self-loop is added or
    removed, values are ignored; a row without entries aggregates to [0 | 0 | 0 | sqrt(1e-5)] (gcnx.layers.PNAConv has the
    formulas).  ``forward(x, edge_index, batch)`` counts duplicate edges once, as ``GCN`` does (a deviation from PyG).
    Everything behind the convolutions is ``GCN``'s: BN·PReLU, the fused max-pool pair, the one-launch BCE head, sync-BN over
    shards (``comm=``), ``set_optimizer``, ``fit``.

    Hot path per convolution (pna_forward / pna_backward of gcnx/convs.py, the one place the sequence is written; gcnx.PNAConv
    runs the same two functions): gcnx_gemm twice (P | Q), gcnx_pna_aggregate (csrc/pna.hip: one gather for the four statistics
    and all 13 blocks of C; the statistics are stored only in a step that computes gradients), gcnx_gemm twice; backward
    gcnx_act_bias_grad, gcnx_gemm_dx, gcnx_gemm_dw2, gcnx_gemm_dx, gcnx_pna_bwd, gcnx_act_bias_grad, gcnx_gemm_dw2, and for
    conv2's dY1 = dC[:, :H] + [dP | dQ] W_pre^T two gcnx_gemm_dx and a gcnx_add.  The 13 H wide products go through the
    general GEMM kernels, which take any width; hidden_channels > 256 is refused (the one-workgroup head).

    Weights: torch key names ``conv{1,2}.pre_nns.0.0.weight`` [F, 2F], ``.pre_nns.0.0.bias``, ``.post_nns.0.0.weight``
    [H, 13F], ``.post_nns.0.0.bias``, ``.lin.weight``, ``.lin.bias`` in ``state_dict()`` ([out, in], as torch; stored [in, out]
    here); initialisation U(+-1/sqrt(fan_in)) as torch's Linear.  ``conv{1,2}.aggr_module.avg_deg_log`` [1] is in
    ``state_dict()`` too and ``load_state_dict()`` takes it when present: a constant -- not in ``get_weights()`` /
    ``gradients()`` / the flat buffers, no gradient.  That key name and the key order follow PyG 2.3's source
    (DegreeScalerAggregation registers the buffer; aggr_module comes before pre_nns); neither was confirmed against a live
    torch_geometric: prefer the named dicts."""

    PROBE_KEY = None                      # no tensor has the input width second: load_state_dict reads pre_nns.0.0.weight [F, 2F]
    OPERATOR, SELF_LOOPS, KERNELS = "pattern", False, "PNAConv"
    HEAD_NOTE = "the one-workgroup head; the 13 H wide products themselves go through the general GEMM kernels"
    _KEYS = _conv_keys("wpre", "bpre", "wpost", "bpost", "wlin", "blin", "pq", "c", "st", "tc", "z", "dc", "dpq", "coef")

    def _init(self, ctx, hidden_channels=64, deg=None, avg_deg_log=None, num_classes=1, seed=0, comm=None, **pna_options):
        from .layers import pna_delta, pna_refuse
        pna_refuse("gcnx.PNA", **pna_options)
        super()._init(ctx, hidden_channels, num_classes, seed, comm)
        delta = pna_delta("gcnx.PNA", deg, avg_deg_log)
        self.avg_deg_log = [delta, delta]                             # conv1's, conv2's (a loaded checkpoint may carry two)
        conv = lambda k: (f"wpre{k}", f"bpre{k}", f"wpost{k}", f"bpost{k}", f"wlin{k}", f"blin{k}", f"g{k}", f"be{k}", f"a{k}")
        self.PARAM_ORDER = conv(1) + conv(2) + GCN.PARAM_ORDER[10:]
        keys = lambda k: ((f"conv{k}.pre_nns.0.0.weight", f"wpre{k}", True), (f"conv{k}.pre_nns.0.0.bias", f"bpre{k}", False),
                          (f"conv{k}.post_nns.0.0.weight", f"wpost{k}", True), (f"conv{k}.post_nns.0.0.bias", f"bpost{k}", False),
                          (f"conv{k}.lin.weight", f"wlin{k}", True), (f"conv{k}.lin.bias", f"blin{k}", False))
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]      # the trainable tensors, named_parameters() order
        self.DELTA_KEYS = ("conv1.aggr_module.avg_deg_log", "conv2.aggr_module.avg_deg_log")

    @staticmethod
    def degree_histogram(graphs):
        """PyG's ``deg`` argument from a dataset: hist[d] = the number of rows (target nodes) with d stored entries, over every
        graph of ``graphs`` (objects with an adjacency ``.a``, or the adjacencies themselves: scipy sparse or dense)."""
        import scipy.sparse as sp
        hist = np.zeros(1, np.int64)
        for g in graphs:
            a = sp.csr_matrix(getattr(g, "a", g))
            d = np.bincount(np.diff(a.indptr))
            if d.size > hist.size:
                hist = np.concatenate([hist, np.zeros(d.size - hist.size, np.int64)])
            hist[:d.size] += d
        return hist

    def _shapes(self, f_in):
        h = self.hidden
        s = super()._shapes(f_in)
        for k in ("w1", "b1", "w2", "b2"):
            del s[k]
        s.update(wpre1=(2 * f_in, f_in), bpre1=(f_in,), wpost1=(13 * f_in, h), bpost1=(h,), wlin1=(h, h), blin1=(h,),
                 wpre2=(2 * h, h), bpre2=(h,), wpost2=(13 * h, h), bpost2=(h,), wlin2=(h, h), blin2=(h,))
        return s

    def _initial(self, f_in, shapes, offs):
        h, u = self.hidden, self._uniform
        init = self._head_initial(shapes)
        for k, f in ((1, f_in), (2, h)):
            init[f"wpre{k}"], init[f"bpre{k}"] = u(2 * f, 2 * f, f), u(2 * f, f)
            init[f"wpost{k}"], init[f"bpost{k}"] = u(13 * f, 13 * f, h), u(13 * f, h)
            init[f"wlin{k}"], init[f"blin{k}"] = u(h, h, h), u(h, h)
        return init

    def state_dict(self):
        d = super().state_dict()
        out = {}
        for tk, v in d.items():                 # conv{k}.aggr_module.avg_deg_log in front of conv{k}.pre_nns.0.0.weight
            for k, dk in enumerate(self.DELTA_KEYS):
                if tk == f"conv{k + 1}.pre_nns.0.0.weight":
                    out[dk] = np.full(1, self.avg_deg_log[k], np.float32)
            out[tk] = v
        return out

    def _probe_f_in(self, d):
        return int(np.asarray(d["conv1.pre_nns.0.0.weight"]).shape[0])       # [F, 2F]

    def load_state_dict(self, d):
        super().load_state_dict(d)
        for k, dk in enumerate(self.DELTA_KEYS):
            if dk in d:
                delta = float(np.asarray(d[dk], np.float64).reshape(-1)[0])
                if not (delta > 0.0 and np.isfinite(delta)):
                    raise ValueError(f"{dk}: must be positive and finite, got {delta}")
                self.avg_deg_log[k] = delta

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        if "pq1" not in bufs:
            v, n, h, f = self._views(), batch.n, self.hidden, batch.f
            for k, w in ((1, f), (2, h)):
                bufs[f"pq{k}"], bufs[f"c{k}"], bufs[f"st{k}"] = v(f"pq{k}", n, 2 * w), v(f"c{k}", n, 13 * w), v(f"st{k}", n, 6 * w)
                bufs[f"tc{k}"] = v(f"tc{k}", n, h)
            # backward scratch, shared by the two convolutions (conv2's runs first): sized for the wider one, viewed per width
            wmax = max(f, h)
            v("pna_dc", n, 13 * wmax), v("pna_dpq", n, 2 * wmax), v("pna_coef", n, 4 * wmax)
            for k, w in ((1, f), (2, h)):
                bufs[f"dc{k}"], bufs[f"dpq{k}"] = v("pna_dc", n, 13 * w), v("pna_dpq", n, 2 * w)
                bufs[f"coef{k}"] = v("pna_coef", n, 4 * w).flat(0, 4 * n * w)
        return bufs

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        wpre, bpre, wpost, bpost, wlin, blin, pq, c, st, tc, z, _, _, _ = self._KEYS[k]
        bufs["a"] = a                           # the forward pattern: gcnx_pna_bwd reads its degrees
        convs.pna_forward(self.ctx, a, x, p[wpre], p[bpre], p[wpost], p[bpost], p[wlin], p[blin], self.avg_deg_log[k - 1], bufs[pq],
                          bufs[c], bufs[st] if keep else None, bufs[tc], bufs[z])

    def _conv_bwd(self, a_t, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        wpre, bpre, wpost, bpost, wlin, blin, pq, c, st, tc, _, dc, dpq, coef = self._KEYS[k]
        convs.pna_backward(self.ctx, bufs["a"], a_t, x, bufs[pq], bufs[c], bufs[st], bufs[tc], dzk, p[wpre], p[wpost], p[wlin], g[wpre],
                           g[bpre], g[wpost], g[bpost], g[wlin], g[blin], self.avg_deg_log[k - 1], bufs["t"], bufs[dc], bufs[dpq],
                           bufs[coef], dx)


class GAT(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's GATConv(heads=H, concat=True, negative_slope=0.2, dropout=0), the
    attention layer for the slot the reference's author marked as open (gcn_utills.py:804-806):

        GATConv(F->H/heads, heads)·BN·PReLU -> GATConv(H->H/heads, heads)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU
        -> Linear(H->1)·BN·PReLU

    ``GAT([ctx,] hidden_channels=64, heads=1, num_classes=1, seed=0, comm=None)``; hidden_channels in {16, 32, 64, 128}, a
    multiple of heads in {1, 2, 4, 8} with at least 4 channels per head (what csrc/gat.hip serves; there is no composed route).
    A host adjacency gets PyG's remaining self-loops, as ``GCN`` (GATConv's remove-then-add gives the same pattern once values
    are ignored); a DeviceCSR is used as stored.  ``forward(x, edge_index, batch)`` counts duplicate edges once, as ``GCN``
    does -- PyG would give a duplicated edge two softmax terms: a deviation.  Everything behind the convolutions is ``GCN``'s:
    BN·PReLU, the fused max-pool pair, the one-launch BCE head, sync-BN over shards (``comm=``; attention never leaves a
    graph), ``fit``.

    Hot path per convolution (gat_forward / gat_backward of gcnx/convs.py, the one place the sequence is written; gcnx.GATConv
    runs the same two functions): gcnx_gemm (Hf = x W), gcnx_gat_scores, gcnx_gat_aggregate; backward gcnx_act_bias_grad,
    gcnx_gat_bwd_edges (forward CSR), gcnx_gat_bwd_nodes (transposed pattern + entry permutation, built once per batch),
    gcnx_gemm_dw, gcnx_gemm_dx.

    Weights: PyG's key names ``conv{1,2}.att_src``, ``.att_dst`` ([1, heads, C]), ``.bias``, ``.lin.weight`` ([out, in], as
    torch; stored [in, out] here) in ``state_dict()``, listed by ``get_weights()`` in named_parameters() order.  That order
    follows PyG 2.x's source; neither torch_geometric nor a checkpoint was available to confirm it against a live module, so
    prefer the named dicts.  Initialisation: glorot-uniform for the attention vectors and the weights, zero bias, as PyG."""

    PARAM_ORDER = ("as1", "ad1", "b1", "w1", "as2", "ad2", "b2", "w2", "g1", "be1", "a1", "g2", "be2", "a2",
                   "w3", "b3", "g3", "be3", "a3", "w4", "b4", "g4", "be4", "a4")
    TORCH_KEYS = (("conv1.att_src", "as1", False), ("conv1.att_dst", "ad1", False), ("conv1.bias", "b1", False),
                  ("conv1.lin.weight", "w1", True),
                  ("conv2.att_src", "as2", False), ("conv2.att_dst", "ad2", False), ("conv2.bias", "b2", False),
                  ("conv2.lin.weight", "w2", True)) + GCN.TORCH_KEYS[4:]
    PROBE_KEY = "conv1.lin.weight"
    LEADING_AXIS = ("conv1.att_src", "conv1.att_dst", "conv2.att_src", "conv2.att_dst")      # [1, heads, C] in PyG, [heads, C] here
    OPERATOR, KERNELS = "perm", "GATConv"
    _KEYS = _conv_keys("w", "as", "ad", "b", "hf", "asrc", "adst", "alpha", "o", "z")
    SLOPE = 0.2

    def _init(self, ctx, hidden_channels=64, heads=1, num_classes=1, seed=0, comm=None):
        h, heads = int(hidden_channels), int(heads)
        self._check_heads(h, heads)
        super()._init(ctx, h, num_classes, seed, comm)
        self.heads = heads

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        hc = (self.heads, self.hidden // self.heads)
        s.update(as1=hc, ad1=hc, as2=hc, ad2=hc)
        return s

    def _initial(self, f_in, shapes, offs):
        h, heads, rng = self.hidden, self.heads, self._rng
        alim = np.sqrt(6.0 / (heads + h // heads))
        att = lambda: rng.uniform(-alim, alim, shapes["as1"])
        return {"as1": att(), "ad1": att(), "w1": glorot_uniform(rng, f_in, h), "as2": att(), "ad2": att(), "w2": glorot_uniform(rng, h, h),
                **self._head_initial(shapes)}

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        nnz = batch.a.nnz
        if bufs.get("gat_key") != (batch.n, batch.n_graphs, nnz):          # the edge buffers follow nnz as well as (n, b)
            v, n, h, heads = self._views(), batch.n, self.hidden, self.heads
            if not D.gat_conv_ok(self.ctx, n, heads, h // heads):
                raise NotImplementedError(f"gcnx.GAT: a batch of {n} rows at hidden_channels={h} is beyond the GATConv kernels")
            for k in ("hf1", "hf2", "o1", "o2", "dhf"):
                bufs[k] = v(k, n, h)
            for k in ("asrc1", "adst1", "asrc2", "adst2", "dadst", "dasrc"):
                bufs[k] = v(k, n, heads)
            for k in ("alpha1", "alpha2", "dz"):
                bufs[k] = v(k, nnz, heads)
            ns = max(D.gat_bwd_scratch_floats(self.ctx, n, heads, h // heads), 1)
            bufs["scratch"] = v("gat_scratch", 1, ns).flat(0, ns)
            bufs["gat_key"] = (batch.n, batch.n_graphs, nnz)
        return bufs

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        w, as_, ad, b, hf, asrc, adst, alpha, o, z = self._KEYS[k]
        convs.gat_forward(self.ctx, a, x, p[w], p[as_], p[ad], p[b], bufs[hf], bufs[asrc], bufs[adst], bufs[alpha] if keep else None,
                          bufs[o] if keep else None, bufs[z], self.SLOPE)

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, as_, ad, b, hf, asrc, adst, alpha, o, _ = self._KEYS[k]
        convs.gat_backward(self.ctx, a, x, bufs[hf], bufs[asrc], bufs[adst], bufs[alpha], bufs[o], dzk, p[w], p[as_], p[ad], g[w], g[as_],
                           g[ad], g[b], bufs["dz"], bufs["dadst"], bufs["dasrc"], bufs["dhf"], bufs["scratch"], dx, self.SLOPE)


class GATv2(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's GATv2Conv(heads=H, concat=True, negative_slope=0.2, dropout=0,
    edge_dim=D, share_weights=False): attention whose scores read the edge features -- the dca / proximity values the
    reference computes on every contact and bridge and its model drops (gcn_utills.py:319-443; gcn.py:71):

        GATv2Conv(F->H/heads, heads)·BN·PReLU -> GATv2Conv(H->H/heads, heads)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU
        -> Linear(H->1)·BN·PReLU

    ``GATv2([ctx,] hidden_channels=64, heads=1, edge_dim=None, num_classes=1, seed=0)``; hidden_channels in {16, 32, 64, 128}, a
    multiple of heads in {1, 2, 4, 8} with at least 4 channels per head, edge_dim None or 1 .. 8 (what csrc/gatv2.hip serves;
    there is no composed route).  With edge_dim the model reads ``batch.e`` (``uses_edge_features``): inputs are (x, a, e, i),
    a DeviceBatch that carries e, or the batches of DeviceDisjointLoader(DeviceDataset(..., edge_features=True)), which arrive
    with e and the transposed pattern gathered on the device (nothing is downloaded or sorted per batch).  A DeviceCSR / a
    DeviceBatch is used as stored, pattern and e (PyG's add_self_loops=False; the reference's graphs carry every loop).  A host
    adjacency gets PyG's add_self_loops=True: stored loops removed, one loop per node added, its features the mean over the
    row's remaining entries (fill_value="mean"; _with_mean_self_loops).  Everything behind the convolutions is ``GCN``'s:
    BN·PReLU, the fused max-pool pair, the one-launch BCE head, ``fit``, the optimizers of gcnx.optim.  One device: ``comm`` is
    refused.

    Hot path per convolution (gatv2_forward / gatv2_backward of gcnx/convs.py, the one place the sequence is written;
    gcnx.GATv2Conv runs the same two functions): gcnx_gemm (Xl | Xr = x [W_l | W_r] + [b_l | b_r], one launch), gcnx_gatv2_aggregate; backward
    gcnx_act_bias_grad, gcnx_gatv2_bwd_edges (forward CSR), gcnx_gatv2_bwd_nodes (transposed pattern + entry permutation),
    gcnx_gemm_dw, gcnx_act_bias_grad, gcnx_gemm_dx.

    Weights: PyG's key names ``conv{1,2}.att`` ([1, heads, C]), ``.bias``, ``.lin_l.weight`` / ``.lin_r.weight`` ([out, in], as
    torch), ``.lin_l.bias`` / ``.lin_r.bias``, ``.lin_edge.weight`` ([out, edge_dim]; with edge_dim) in ``state_dict()``; stored
    as one stacked [in, 2 out] weight and one stacked bias per convolution, the named tensors are views.  The order follows
    PyG 2.x's source, not a live module: prefer the named dicts.  Initialisation: glorot-uniform, zero biases, as PyG."""

    PROBE_KEY = "conv1.lin_l.weight"
    OPERATOR, KERNELS = "perm", "GATv2Conv"
    _KEYS = _conv_keys("w", "lb", "att", "b", "we", "xlr", "alpha", "o", "z")
    SLOPE = 0.2

    def _init(self, ctx, hidden_channels=64, heads=1, edge_dim=None, num_classes=1, seed=0, comm=None):
        h, heads = int(hidden_channels), int(heads)
        self._one_device(comm)
        self._check_heads(h, heads)
        self.edge_dim = self._check_edge_dim(edge_dim)
        super()._init(ctx, h, num_classes, seed, None)
        self.heads, self.uses_edge_features = heads, edge_dim is not None
        conv = lambda k: (f"att{k}", f"b{k}", f"w{k}", f"lb{k}") + ((f"we{k}",) if self.edge_dim else ())
        self.PARAM_ORDER = conv(1) + conv(2) + ("g1", "be1", "a1", "g2", "be2", "a2") + GCN.PARAM_ORDER[10:]
        keys = lambda k: ((f"conv{k}.att", f"att{k}", False), (f"conv{k}.bias", f"b{k}", False),
                          (f"conv{k}.lin_l.weight", f"wl{k}", True), (f"conv{k}.lin_l.bias", f"bl{k}", False),
                          (f"conv{k}.lin_r.weight", f"wr{k}", True), (f"conv{k}.lin_r.bias", f"br{k}", False)) + \
            (((f"conv{k}.lin_edge.weight", f"we{k}", True),) if self.edge_dim else ())
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]
        self.LEADING_AXIS = ("conv1.att", "conv2.att")                 # [1, heads, C] in PyG, [heads, C] here
        # PyG's names: the column halves of the stacked weight, the halves of the stacked bias
        self.STACKS = {"w1": ("wl1", "wr1"), "lb1": ("bl1", "br1"), "w2": ("wl2", "wr2"), "lb2": ("bl2", "br2")}

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        h, d = self.hidden, self.edge_dim or 0
        hc = (self.heads, h // self.heads)
        s.update(att1=hc, att2=hc, w1=(f_in, 2 * h), w2=(h, 2 * h), lb1=(2 * h,), lb2=(2 * h,), we1=(d, h), we2=(d, h))
        return s

    def _initial(self, f_in, shapes, offs):
        h, heads, d, rng = self.hidden, self.heads, self.edge_dim or 0, self._rng
        alim = np.sqrt(6.0 / (heads + h // heads))
        att = lambda: rng.uniform(-alim, alim, shapes["att1"])
        lin = lambda fi: np.concatenate([glorot_uniform(rng, fi, h), glorot_uniform(rng, fi, h)], axis=1)
        init = {"att1": att(), "w1": lin(f_in), "att2": att(), "w2": lin(h), **self._head_initial(shapes)}
        if d:
            init.update(we1=glorot_uniform(rng, d, h), we2=glorot_uniform(rng, d, h))
        return init

    def _host_inputs(self, inputs):
        x, a, i = _without_e(inputs)
        e = inputs[2] if self.uses_edge_features else None
        if not isinstance(a, D.DeviceCSR):                       # a host matrix: PyG's add_self_loops=True, fill_value="mean"
            a, e = _with_mean_self_loops(a, e, np.asarray(x).shape[0])
        return (x, a, e, i) if e is not None else (x, a, i)

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        nnz, d = batch.a.nnz, self.edge_dim or 0
        if bufs.get("gatv2_key") != (batch.n, batch.n_graphs, nnz):        # the edge buffers follow nnz as well as (n, b)
            v, n, h, heads = self._views(), batch.n, self.hidden, self.heads
            if not D.gatv2_conv_ok(self.ctx, n, heads, h // heads, edge_dim=d):
                raise NotImplementedError(f"gcnx.GATv2: a batch of {n} rows at hidden_channels={h} is beyond the GATv2Conv kernels")
            for k in ("xlr1", "xlr2", "dxlr"):
                bufs[k] = v(k, n, 2 * h)
            for k in ("o1", "o2"):
                bufs[k] = v(k, n, h)
            for k in ("alpha1", "alpha2", "dscore"):
                bufs[k] = v(k, nnz, heads)
            ns = max(D.gatv2_bwd_scratch_floats(self.ctx, n, heads, h // heads, d), 1)
            bufs["scratch"] = v("gatv2_scratch", 1, ns).flat(0, ns)
            bufs["gatv2_key"] = (batch.n, batch.n_graphs, nnz)
        return bufs

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        w, lb, att, b, we, xlr, alpha, o, z = self._KEYS[k]
        convs.gatv2_forward(self.ctx, a, x, bufs["e"], p[w], p[lb], p[att], p[b], p.get(we), bufs[xlr], bufs[alpha] if keep else None,
                            bufs[o] if keep else None, bufs[z], self.SLOPE)

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, lb, att, b, we, xlr, alpha, o, _ = self._KEYS[k]
        convs.gatv2_backward(self.ctx, a, x, bufs["e"], bufs[xlr], bufs[alpha], bufs[o], dzk, p[w], p[att], p.get(we), g[w], g[lb], g[att],
                             g[b], g.get(we), bufs["dscore"], bufs["dxlr"], bufs["scratch"], dx, self.SLOPE)


class ResGated(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's ResGatedGraphConv(act=Sigmoid(), edge_dim=D, root_weight, bias=True)
    (Bresson & Laurent's GatedGCN), aggr = add: every message is multiplied channel by channel by a sigmoid gate that reads
    target, source and the edge features -- the dca / proximity values the reference computes on every contact and bridge and
    its model drops (gcn_utills.py:319-443; gcn.py:71).  No softmax: a row's messages do not compete.

        ResGatedGraphConv(F->H)·BN·PReLU -> ResGatedGraphConv(H->H)·BN·PReLU -> global_max_pool -> Linear(H->H)·BN·PReLU
        -> Linear(H->1)·BN·PReLU

    ``ResGated([ctx,] hidden_channels=64, edge_dim=None, root_weight=True, num_classes=1, seed=0)``; hidden_channels in {16, 32,
    64, 128}, edge_dim None or 1 .. 8 (what csrc/resgated.hip serves; there is no composed route).  With edge_dim the model
    reads ``batch.e`` (``uses_edge_features``): inputs are (x, a, e, i), a DeviceBatch that carries e, or the batches of
    DeviceDisjointLoader(DeviceDataset(..., edge_features=True)), which arrive with e and the transposed pattern gathered on the
    device.  The pattern and e are used as stored on every route -- host, device or loader: no self-loop is added or removed
    (the reference's graphs carry every loop).  Everything behind the convolutions is ``GCN``'s: BN·PReLU, the fused max-pool
    pair, the one-launch BCE head, ``fit``, the optimizers of gcnx.optim.  One device: ``comm`` is refused.

    Hot path per convolution (resgated_forward / resgated_backward of gcnx/convs.py, the one place the sequence is written;
    gcnx.ResGatedGraphConv runs the same two functions): gcnx_gemm (P = K | Q | V | S = x [W_k | W_q | W_v | W_s] +
    [b_k | b_q | b_v | 0], one launch), gcnx_resgated_aggregate; backward gcnx_act_bias_grad, gcnx_resgated_bwd_targets (forward CSR), gcnx_resgated_bwd_sources
    (transposed pattern + entry permutation), gcnx_gemm_dw, gcnx_act_bias_grad over the 3 H biased columns, gcnx_gemm_dx.

    Weights: PyG's key names ``conv{1,2}.bias``, ``.lin_key.weight`` / ``.lin_query.weight`` / ``.lin_value.weight`` ([out, in + D] =
    [node block ‖ edge block], as torch), their ``.bias``, ``.lin_skip.weight`` ([out, in], with root_weight) in ``state_dict()``;
    stored as one stacked [in, 4 out] weight (3 out without root_weight), one stacked [3 out] bias and one [D, 3 out] edge weight
    per convolution -- ``load_state_dict`` splits PyG's tensors, ``state_dict`` joins them, ``gradients()`` returns dW_ke and
    dW_qe as the same numbers.  The names and the order follow PyG 2.3+'s source, not a live module (neither torch_geometric
    nor a checkpoint was available): prefer the named dicts.  Initialisation as torch's Linear: U(+-1 / sqrt(fan_in)) for every
    weight and bias, the conv ``bias`` zero."""

    PROBE_KEY = None                      # conv1.lin_key.weight is [H, F + D]: load_state_dict subtracts D itself
    LINS = (("lin_key", "k"), ("lin_query", "q"), ("lin_value", "v"))
    OPERATOR, SELF_LOOPS, KERNELS = "perm", False, "ResGatedGraphConv"
    _KEYS = _conv_keys("w", "lb", "b", "we", "p", "z")

    def _init(self, ctx, hidden_channels=64, edge_dim=None, root_weight=True, num_classes=1, seed=0, comm=None):
        h = int(hidden_channels)
        self._one_device(comm)
        if h not in (16, 32, 64, 128):
            raise NotImplementedError(f"gcnx.ResGated: hidden_channels={h} must be 16, 32, 64 or 128 (the widths the ResGatedGraphConv "
                                      "kernels serve; there is no composed route)")
        self.edge_dim = self._check_edge_dim(edge_dim)
        super()._init(ctx, h, num_classes, seed, None)
        self.root_weight, self.uses_edge_features = bool(root_weight), edge_dim is not None
        self.width = (4 if self.root_weight else 3) * h
        # lz: the zero bias of the S block, directly behind the stacked bias (the product's bias is the two together)
        conv = lambda k: (f"b{k}", f"w{k}", f"lb{k}") + ((f"lz{k}",) if self.root_weight else ()) + ((f"we{k}",) if self.edge_dim else ())
        self.PARAM_ORDER = conv(1) + conv(2) + ("g1", "be1", "a1", "g2", "be2", "a2") + GCN.PARAM_ORDER[10:]
        # the views behind PyG's names: the node blocks wk / wq / wv / ws [in, H]; with edge_dim the state_dict joins the
        # edge blocks wke / wqe / wve [D, H] to the first three
        keys = lambda k: ((f"conv{k}.bias", f"b{k}", False),) + \
            tuple(t for n, s in self.LINS for t in ((f"conv{k}.{n}.weight", f"w{s}{k}", True), (f"conv{k}.{n}.bias", f"b{s}{k}", False))) + \
            (((f"conv{k}.lin_skip.weight", f"ws{k}", True),) if self.root_weight else ())
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]
        self.STACKS, self.EDGE_BLOCKS = {}, {}
        for k in (1, 2):                                # PyG's names: the column blocks of the stacked tensors
            self.STACKS[f"w{k}"] = tuple(f"w{s}{k}" for _, s in self.LINS) + ((f"ws{k}",) if self.root_weight else ())
            self.STACKS[f"lb{k}"] = tuple(f"b{s}{k}" for _, s in self.LINS)
            if self.edge_dim:
                self.STACKS[f"we{k}"] = tuple(f"w{s}e{k}" for _, s in self.LINS)
                self.EDGE_BLOCKS.update({f"conv{k}.{n}.weight": f"w{s}e{k}" for n, s in self.LINS})

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        h, d, w = self.hidden, self.edge_dim or 0, self.width
        s.update(w1=(f_in, w), w2=(h, w), lb1=(3 * h,), lb2=(3 * h,), lz1=(h,), lz2=(h,), we1=(d, 3 * h), we2=(d, 3 * h))
        return s

    def _initial(self, f_in, shapes, offs):
        h, d, w, u = self.hidden, self.edge_dim or 0, self.width, self._uniform
        self._gemm_bias = {}                            # (lz, like the padding, has zero gradients: the update leaves it at zero)
        for k in (1, 2):
            assert not self.root_weight or offs[f"lz{k}"] == offs[f"lb{k}"] + 3 * h
            self._gemm_bias[k] = self.flat_p.flat(offs[f"lb{k}"], w)
        init = self._head_initial(shapes)
        for k, f in ((1, f_in), (2, h)):                # torch's Linear on [x ‖ e]: fan_in = in + D for key / query / value
            blocks = [u(f + d, f, 3 * h)] + ([u(f, f, h)] if self.root_weight else [])
            init[f"w{k}"], init[f"lb{k}"] = np.concatenate(blocks, axis=1), u(f + d, 3 * h)
            if d:
                init[f"we{k}"] = u(f + d, d, 3 * h)
        return init

    def _probe_f_in(self, d):
        return int(np.asarray(d["conv1.lin_key.weight"]).shape[1]) - (self.edge_dim or 0)       # [H, F + D]

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        if "p1" not in bufs:
            v, n, h, w, d = self._views(), batch.n, self.hidden, self.width, self.edge_dim or 0
            if not D.resgated_conv_ok(self.ctx, n, h, ldp=w, edge_dim=d):
                raise NotImplementedError(f"gcnx.ResGated: a batch of {n} rows at hidden_channels={h} is beyond the ResGatedGraphConv kernels")
            for k in ("p1", "p2", "dp"):
                bufs[k] = v("rg_" + k, n, w)
            ns = max(D.resgated_bwd_scratch_floats(self.ctx, n, h, d), 1)
            bufs["scratch"] = v("rg_scratch", 1, ns).flat(0, ns)
        return bufs

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        w, _, b, we, pk, z = self._KEYS[k]
        convs.resgated_forward(self.ctx, a, x, bufs["e"], p[w], self._gemm_bias[k], p[b], p.get(we), bufs[pk], bufs[z])

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, lb, b, we, pk, _ = self._KEYS[k]
        convs.resgated_backward(self.ctx, a, x, bufs["e"], bufs[pk], dzk, p[w], p.get(we), g[w], g[lb], g[b], g.get(we), bufs["dp"],
                                bufs["scratch"], dx)


class Transformer(GCN):
    """``GCN`` with its two GCNConv layers replaced by PyG's TransformerConv(heads=H, concat=True, beta, dropout=0, edge_dim=D,
    bias=True, root_weight) (Shi et al., UniMP): scaled dot-product attention whose keys and values carry the edge features --
    the dca / proximity values the reference computes on every contact and bridge and its model drops (gcn_utills.py:319-443;
    gcn.py:71):

        TransformerConv(F->H/heads, heads)·BN·PReLU -> TransformerConv(H->H/heads, heads)·BN·PReLU -> global_max_pool
        -> Linear(H->H)·BN·PReLU -> Linear(H->1)·BN·PReLU

    ``Transformer([ctx,] hidden_channels=64, heads=1, edge_dim=None, beta=False, root_weight=True, num_classes=1, seed=0)``;
    hidden_channels in {16, 32, 64, 128}, a multiple of heads in {1, 2, 4, 8} with at least 4 channels per head, edge_dim None
    or 1 .. 8 (what csrc/transformer.hip serves; there is no composed route); beta needs root_weight.  With edge_dim the model
    reads ``batch.e`` (``uses_edge_features``): inputs are (x, a, e, i), a DeviceBatch that carries e, or the batches of
    DeviceDisjointLoader(DeviceDataset(..., edge_features=True)), which arrive with e and the transposed pattern gathered on the
    device.  The pattern and e are used as stored on every route -- host, device or loader: no self-loop is added or removed
    (TransformerConv has no add_self_loops; the reference's graphs carry every loop).  Everything behind the convolutions is
    ``GCN``'s: BN·PReLU, the fused max-pool pair, the one-launch BCE head, ``fit``, the optimizers of gcnx.optim.  One device:
    ``comm`` is refused.

    Hot path per convolution (transformer_forward / transformer_backward of gcnx/convs.py, the one place the sequence is written;
    gcnx.TransformerConv runs the same two functions): gcnx_gemm (P = Q | K | V | S = x [W_q | W_k | W_v | W_s] +
    [b_q | b_k | b_v | b_s], one launch), gcnx_transformer_aggregate; backward gcnx_transformer_beta_bwd (beta only),
    gcnx_transformer_bwd_targets (forward CSR), gcnx_transformer_bwd_sources (transposed pattern + entry permutation),
    gcnx_gemm_dw, gcnx_act_bias_grad, gcnx_gemm_dx.

    Weights: PyG's key names ``conv{1,2}.lin_key.weight`` / ``.bias``, ``.lin_query.*``, ``.lin_value.*``, ``.lin_edge.weight``
    ([out, edge_dim]; with edge_dim), ``.lin_skip.*`` (with root_weight), ``.lin_beta.weight`` ([1, 3 out]; with beta) in
    ``state_dict()``, weights [out, in] as torch; stored as one stacked [in, 4 out] weight (3 out without root_weight) and one
    stacked bias per convolution, the named tensors are views.  The gradient of lin_key.bias is analytically zero (a common
    shift of all keys cancels in the softmax).  The order follows PyG 2.x's source, not a live module: prefer the named dicts.
    Initialisation as torch's Linear: U(+-1 / sqrt(fan_in)) for every weight and bias."""

    PROBE_KEY = "conv1.lin_key.weight"
    BLOCKS = (("lin_query", "q"), ("lin_key", "k"), ("lin_value", "v"), ("lin_skip", "s"))       # storage order of the column blocks
    OPERATOR, SELF_LOOPS, KERNELS = "perm", False, "TransformerConv"
    _KEYS = _conv_keys("w", "lb", "we", "wb", "p", "alpha", "o", "z")

    def _init(self, ctx, hidden_channels=64, heads=1, edge_dim=None, beta=False, root_weight=True, num_classes=1, seed=0, comm=None):
        h, heads = int(hidden_channels), int(heads)
        self._one_device(comm)
        self._check_heads(h, heads)
        self.edge_dim = self._check_edge_dim(edge_dim)
        if beta and not root_weight:
            raise NotImplementedError("gcnx.Transformer: beta=True gates the root connection and needs root_weight=True")
        super()._init(ctx, h, num_classes, seed, None)
        self.heads, self.beta, self.root_weight = heads, bool(beta), bool(root_weight)
        self.uses_edge_features = edge_dim is not None
        self.blocks = self.BLOCKS if self.root_weight else self.BLOCKS[:3]
        self.width = len(self.blocks) * h
        conv = lambda k: (f"w{k}", f"lb{k}") + ((f"we{k}",) if self.edge_dim else ()) + ((f"wb{k}",) if self.beta else ())
        self.PARAM_ORDER = conv(1) + conv(2) + ("g1", "be1", "a1", "g2", "be2", "a2") + GCN.PARAM_ORDER[10:]
        lin = lambda k, n, s: ((f"conv{k}.{n}.weight", f"w{s}{k}", True), (f"conv{k}.{n}.bias", f"b{s}{k}", False))
        keys = lambda k: lin(k, "lin_key", "k") + lin(k, "lin_query", "q") + lin(k, "lin_value", "v") + \
            (((f"conv{k}.lin_edge.weight", f"we{k}", True),) if self.edge_dim else ()) + \
            (lin(k, "lin_skip", "s") if self.root_weight else ()) + (((f"conv{k}.lin_beta.weight", f"wb{k}", False),) if self.beta else ())
        self.TORCH_KEYS = keys(1) + keys(2) + GCN.TORCH_KEYS[4:]
        self.LEADING_AXIS = ("conv1.lin_beta.weight", "conv2.lin_beta.weight") if self.beta else ()     # [1, 3 H] in PyG, [3 H] here
        # PyG's names: the column blocks of the stacked weight and bias
        self.STACKS = {}
        for k in (1, 2):
            self.STACKS[f"w{k}"], self.STACKS[f"lb{k}"] = tuple(f"w{s}{k}" for _, s in self.blocks), tuple(f"b{s}{k}" for _, s in self.blocks)

    def _shapes(self, f_in):
        s = super()._shapes(f_in)
        h, d, w = self.hidden, self.edge_dim or 0, self.width
        s.update(w1=(f_in, w), w2=(h, w), lb1=(w,), lb2=(w,), we1=(d, h), we2=(d, h), wb1=(3 * h,), wb2=(3 * h,))
        return s

    def _initial(self, f_in, shapes, offs):
        h, d, w, u = self.hidden, self.edge_dim or 0, self.width, self._uniform
        init = self._head_initial(shapes)
        for k, f in ((1, f_in), (2, h)):
            init[f"w{k}"], init[f"lb{k}"] = u(f, f, w), u(f, w)
            if d:
                init[f"we{k}"] = u(d, d, h)
            if self.beta:
                init[f"wb{k}"] = u(3 * h, 3 * h)
        return init

    def _ensure(self, batch, sharded=False):
        bufs = super()._ensure(batch, sharded)
        self._check_e(batch)
        nnz, d = batch.a.nnz, self.edge_dim or 0
        if bufs.get("tf_key") != (batch.n, batch.n_graphs, nnz):           # the edge buffers follow nnz as well as (n, b)
            v, n, h, heads, w = self._views(), batch.n, self.hidden, self.heads, self.width
            if not D.transformer_conv_ok(self.ctx, n, heads, h // heads, ldp=w, edge_dim=d):
                raise NotImplementedError(f"gcnx.Transformer: a batch of {n} rows at hidden_channels={h} is beyond the TransformerConv kernels")
            for k in ("p1", "p2", "dp"):
                bufs[k] = v("tf_" + k, n, w)
            for k in ("o1", "o2", "d_o"):
                bufs[k] = v("tf_" + k, n, h)
            for k in ("alpha1", "alpha2", "dscore"):
                bufs[k] = v("tf_" + k, nnz, heads)
            ns = max(D.transformer_bwd_scratch_floats(self.ctx, n, heads, h // heads, d, self.beta), 1)
            bufs["scratch"] = v("tf_scratch", 1, ns).flat(0, ns)
            bufs["tf_key"] = (batch.n, batch.n_graphs, nnz)
        return bufs

    def _conv_fwd(self, a, x, k, bufs, keep):
        p = self.p
        w, lb, we, wb, pk, alpha, o, z = self._KEYS[k]
        convs.transformer_forward(self.ctx, a, x, bufs["e"], p[w], p[lb], p.get(we), p.get(wb), bufs[pk], bufs[alpha] if keep else None,
                                  bufs[o] if keep else None, bufs[z], self.heads)

    def _conv_bwd(self, a, x, k, dzk, bufs, dx):
        p, g = self.p, self.g
        w, lb, we, wb, pk, alpha, o, _ = self._KEYS[k]
        convs.transformer_backward(self.ctx, a, x, bufs["e"], bufs[pk], bufs[alpha], bufs[o], dzk, p[w], p.get(we), p.get(wb), g[w], g[lb],
                                   g.get(we), g.get(wb), bufs["dp"], bufs["dscore"], bufs["d_o"], bufs["scratch"], dx, self.heads)


class ECCNet(_GraphRunner):
    """Graph classification on the edge features the reference's pipeline computes and its training script drops
    (``dca`` on the bridges, ``proximity`` on the contacts: gcn_utills.py:379-443; gcn.py:71):

        ECCConv(channels, relu) -> ECCConv(channels, relu) -> GlobalSumPool -> Dense(n_labels, softmax)

    -- the shape of Spektral's ECC graph-classification example and of GCN2 -- with the categorical cross-entropy and one-hot
    labels of gcn.py:259-262,326 and plain SGD.  ``ECCNet([ctx,] n_labels=2, channels=32, kernel_network=None, pool="sum",
    seed=0)``; inputs are ``(x, a, e, i)`` as DisjointLoader yields them for ``Graph(e=...)`` (e: one row per stored entry of a,
    from_networkx(use_edge_data="entries")) or a DeviceBatch that carries ``e`` -- from_host's, or the batches of a
    DeviceDisjointLoader over ``DeviceDataset(edge_features=True)``, which arrive with e and the transposed pattern gathered on
    the device (no host sort per batch).  The values of ``a`` are ignored.

    Follows the GCN2 protocol (model(inputs, training=), loss_and_grads, train_step(fetch=True | False | "stash"),
    evaluate_batch, collect_metrics; one flat parameter buffer, one SGD launch), so gcnx.fit / gcnx.evaluate drive it.
    fp32, eager launches, one device.  Hot path: gcnx_ecc_expand + gcnx_gemm per layer, gcnx_segment_pool,
    gcnx_dense_softmax_cce, gcnx_act_bias_grad / gcnx_gemm_dw / gcnx_gemm_dx / gcnx_ecc_bwd backwards, gcnx_sgd (DESIGN.md,
    "ECCConv", lists one step's launches).

    Weights: ``get_weights(as_dict=True)`` / ``set_weights(dict)`` use {"conv1": {Keras names}, "conv2": {...},
    "dense_kernel", "dense_bias"}; the list form is conv1's, conv2's (layers.ecc_weight_names order), then the Dense pair --
    Keras' own order was not confirmed against a live model (PARITY UNPINNED): prefer the dict."""

    uses_edge_features = True            # gcnx.fit / gcnx.evaluate keep e in the batches they upload for this model

    @D.with_default_context
    def __init__(self, ctx, n_labels=2, channels=32, kernel_network=None, pool="sum", seed=0, comm=None, prec="f32",
                 cce_train="logits", cce_eval="probs"):
        from .layers import ECCConv
        if comm is not None:
            raise NotImplementedError("gcnx.ECCNet runs on one device (comm is not supported)")
        if prec not in ("f32", "fp32"):
            raise NotImplementedError(f"gcnx.ECCNet: prec={prec!r}; fp32 only")
        if pool not in ("sum", "avg", "mean"):
            raise NotImplementedError(f"gcnx.ECCNet: pool={pool!r}; 'sum' (the default) or 'avg'")
        if int(n_labels) < 1:
            raise ValueError(f"gcnx.ECCNet(n_labels={n_labels!r})")
        self.ctx, self.n_labels, self.channels, self.pool = ctx, int(n_labels), int(channels), pool
        self.cce_train, self.cce_eval = cce_train, cce_eval
        self.comm, self.prec = None, "f32"
        self.use_graph = False                                  # eager: 14 library calls per step without a kernel network
        rng = np.random.default_rng(seed)
        s1, s2, self._head_seed = (int(v) for v in rng.integers(0, 2 ** 31, 3))
        self.conv1 = ECCConv(channels, kernel_network, activation="relu", seed=s1)     # (validates channels / kernel_network)
        self.conv2 = ECCConv(channels, kernel_network, activation="relu", seed=s2)
        self.kernel_network = self.conv1.kernel_network
        self.built = False
        self._bufs = None
        self._graphs = {}

    # ---- parameters: one flat buffer (one SGD launch) ------------------------------------------------------------------
    def build(self, f_in, edge_dim):
        h, c = self.channels, self.n_labels
        self.f_in, self.edge_dim = int(f_in), int(edge_dim)
        self.conv1.edge_dim = self.conv2.edge_dim = self.edge_dim
        n1, n2 = self.conv1.n_params(self.f_in), self.conv2.n_params(h)
        self.n_params = n1 + n2 + -(-h * c // 4) * 4 + -(-c // 4) * 4
        self.flat_p = self.ctx.zeros(self.n_params)
        self.flat_g = self.ctx.zeros(self.n_params + 2)          # + (loss sum, correct count)
        off = self.conv1.build(self.ctx, self.f_in, self.flat_p, self.flat_g, 0)
        off = self.conv2.build(self.ctx, h, self.flat_p, self.flat_g, off)
        self.p, self.g = {}, {}
        for k, shape in (("dense_kernel", (h, c)), ("dense_bias", (c,))):
            n = int(np.prod(shape))
            self.p[k], self.g[k] = self.flat_p.flat(off, n, shape), self.flat_g.flat(off, n, shape)
            off += -(-n // 4) * 4
        assert off == self.n_params
        self.loss_acc = self.flat_g.flat(self.n_params, 2)
        self.p["dense_kernel"].copy_from_host(glorot_uniform(np.random.default_rng(self._head_seed), h, c))
        self.built = True

    def get_weights(self, as_dict=False):
        d = {"conv1": self.conv1.get_weights(as_dict=True), "conv2": self.conv2.get_weights(as_dict=True),
             "dense_kernel": self.p["dense_kernel"].numpy(), "dense_bias": self.p["dense_bias"].numpy()}
        if as_dict:
            return d
        return self.conv1.get_weights() + self.conv2.get_weights() + [d["dense_kernel"], d["dense_bias"]]

    def set_weights(self, weights):
        if not self.built:
            raise ValueError("gcnx.ECCNet.set_weights: build(f_in, edge_dim) first (or run a batch)")
        if not isinstance(weights, dict):
            weights = list(weights)
            k = len(weights) - 2
            weights = {"conv1": weights[:k // 2], "conv2": weights[k // 2:k], "dense_kernel": weights[-2], "dense_bias": weights[-1]}
        self.conv1.set_weights(weights["conv1"])
        self.conv2.set_weights(weights["conv2"])
        for k in ("dense_kernel", "dense_bias"):
            self.p[k].copy_from_host(np.asarray(weights[k], np.float32).reshape(self.p[k].shape))

    def gradients(self):
        """Gradients of the last loss_and_grads / train_step, nested and shaped as get_weights(as_dict=True)."""
        return {"conv1": self.conv1.gradients(), "conv2": self.conv2.gradients(),
                "dense_kernel": self.g["dense_kernel"].numpy(), "dense_bias": self.g["dense_bias"].numpy()}

    @property
    def trainable_variables(self):
        return self.conv1.trainable_variables + self.conv2.trainable_variables + [self.p["dense_kernel"], self.p["dense_bias"]]

    # ---- batches -------------------------------------------------------------------------------------------------------
    def _as_batch(self, inputs, target=None):
        if not isinstance(inputs, DeviceBatch) and len(inputs) != 4:
            raise ValueError("gcnx.ECCNet takes (x, a, e, i): build the graphs with edge features (Graph(e=...), "
                             "from_networkx(use_edge_data='entries'))")
        batch = self._adopt(inputs, target, weighted=False)
        if batch.e is None:
            raise ValueError("gcnx.ECCNet: the batch carries no edge features (DeviceBatch.e)")
        return batch

    def _ensure(self, batch):
        if not self.built:
            self.build(batch.f, batch.e.shape[1])
        if batch.f != self.f_in or batch.e.shape[1] != self.edge_dim:
            raise ValueError(f"gcnx.ECCNet was built for {self.f_in} node / {self.edge_dim} edge features, got {batch.f} / {batch.e.shape[1]}")
        key = (batch.n, batch.n_graphs)
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        v, n, b, h, c = self._views(), batch.n, batch.n_graphs, self.channels, self.n_labels
        self._bufs = {"key": key, "y1": v("y1", n, h), "y2": v("y2", n, h), "dy2": v("dy2", n, h),
                      "pooled": v("pooled", b, h), "dpooled": v("dpooled", b, h), "probs": v("probs", b, c)}
        return self._bufs

    # ---- the call sequences ------------------------------------------------------------------------------------------------
    def _forward(self, batch, bufs, mode, denom=None):
        """mode: "fwd" (probabilities), "loss" (+ loss and hits, cce_eval), "grads" (+ dPooled and the head's gradients, cce_train)."""
        ctx, p, g = self.ctx, self.p, self.g
        a = batch.a.unweighted()
        self.conv1([batch.x, a, batch.e], out=bufs["y1"])
        self.conv2([bufs["y1"], a, batch.e], out=bufs["y2"])
        D.segment_pool(ctx, batch.seg, bufs["y2"], bufs["pooled"], self.pool)
        if mode != "fwd" and batch.y is None:
            raise ValueError("gcnx.ECCNet: labels are needed for the loss")
        if mode == "grads":
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], batch.y, bufs["probs"], self.loss_acc, denom,
                                dw=g["dense_kernel"], db=g["dense_bias"], dpooled=bufs["dpooled"], cce=self.cce_train)
        elif mode == "loss":
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], batch.y, bufs["probs"], self.loss_acc, denom,
                                cce=self.cce_eval)
        else:
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], None, bufs["probs"])

    def _backward(self, batch, bufs):
        D.segment_pool_bwd(self.ctx, batch.seg, bufs["dpooled"], bufs["dy2"], self.pool)
        dy1 = self.conv2.backward(bufs["dy2"])
        self.conv1.backward(dy1, need_dx=False)

    # ---- public surface ----------------------------------------------------------------------------------------------------
    def __call__(self, inputs, training=False):
        """model((x, a, e, i), training=False) -> probabilities [B, n_labels]."""
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "fwd")
        return bufs["probs"].numpy()

    def loss_and_grads(self, inputs, target=None, global_batch=None, _lr=None):
        """Forward + loss + every gradient (+ the SGD update with ``_lr``).  Returns the device batch."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "grads", float(global_batch or batch.n_graphs))
        self._backward(batch, bufs)
        if _lr is not None:
            self._apply_sgd(_lr)
        self._last_batch = batch
        return batch

    def train_step(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None):
        """One optimisation step (gcn.py:330-340): loss, gradients, p -= lr * g.  fetch: True -> (loss, acc); False -> None;
        "stash" -> None, metrics kept on the device for collect_metrics()."""
        batch = self.loss_and_grads(inputs, target, global_batch, _lr=float(lr))
        return self._finish_step(fetch, global_batch or batch.n_graphs)

    def evaluate_batch(self, inputs, target):
        """(loss, accuracy, probabilities) without gradients (the body of evaluate(), gcn.py:350-357; loss by cce_eval)."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "loss", float(batch.n_graphs))
        return (*self._loss_acc_host(batch.n_graphs), bufs["probs"].numpy())


class TopKNet(_GraphRunner):
    """Hierarchical pooling between two convolutions, with the one Spektral layer the reference's script imports and the flat
    models cannot express (``from spektral.layers.pooling import TopKPool``, gcn.py:10):

        GCNConv(hidden, relu) -> TopKPool(ratio) -> GCNConv(hidden, relu) -> GlobalSumPool | GlobalAvgPool -> Dense(n_labels, softmax)

    with the categorical cross-entropy and one-hot labels of gcn.py:259-262,326 and plain SGD.  ``TopKNet([ctx,] n_labels=2,
    hidden=64, ratio=0.5, pool="sum", sigmoid_gating=False, seed=0)``; inputs are ``(x, a, i)`` as DisjointLoader yields them
    (an ``e`` is dropped) or a DeviceBatch; the adjacency is used with its values (pass normalize= / GCNConv.preprocess for
    gcn_filter), and the pooled operator A[idx][:, idx] keeps them without renormalising, as Spektral does.

    Follows the ECCNet protocol (model(inputs, training=), loss_and_grads, train_step(fetch=True | False | "stash"),
    evaluate_batch, collect_metrics; one flat parameter buffer with every tensor on a multiple of 4 floats, one SGD launch),
    so gcnx.fit / gcnx.evaluate drive it.  fp32, one device, eager launches: TopKPool reads nnz' back (4 bytes) in the middle
    of the forward pass, so the step cannot be captured (DESIGN.md §4.9 lists one step's launches).

    Weights: ``get_weights()`` lists PARAM_ORDER (conv1 kernel, bias; the pool's kernel [hidden, 1]; conv2 kernel, bias; the
    Dense pair); ``get_weights(as_dict=True)``, ``set_weights(dict)`` and ``gradients()`` use those names."""

    PARAM_ORDER = ("conv1_kernel", "conv1_bias", "pool_kernel", "conv2_kernel", "conv2_bias", "dense_kernel", "dense_bias")

    @D.with_default_context
    def __init__(self, ctx, n_labels=2, hidden=64, ratio=0.5, pool="sum", sigmoid_gating=False, seed=0, comm=None, prec="f32",
                 cce_train="logits", cce_eval="probs"):
        from .layers import GCNConv, TopKPool
        if comm is not None:
            raise NotImplementedError("gcnx.TopKNet runs on one device (comm is not supported)")
        if prec not in ("f32", "fp32"):
            raise NotImplementedError(f"gcnx.TopKNet: prec={prec!r}; fp32 only")
        if pool not in ("sum", "avg", "mean"):
            raise NotImplementedError(f"gcnx.TopKNet: pool={pool!r}; 'sum' (the default) or 'avg'")
        if int(n_labels) < 1 or int(hidden) < 1:
            raise ValueError(f"gcnx.TopKNet(n_labels={n_labels!r}, hidden={hidden!r})")
        self.ctx, self.n_labels, self.hidden, self.pool = ctx, int(n_labels), int(hidden), "avg" if pool == "mean" else pool
        self.cce_train, self.cce_eval = cce_train, cce_eval
        self.comm, self.prec = None, "f32"
        self.use_graph = False                                  # eager: the pool's read-back sits inside the forward pass
        rng = np.random.default_rng(seed)
        s1, sp, s2, self._head_seed = (int(v) for v in rng.integers(0, 2 ** 31, 4))
        self.conv1 = GCNConv(self.hidden, activation="relu", seed=s1)
        self.topk = TopKPool(ratio, sigmoid_gating=sigmoid_gating, seed=sp)          # (validates ratio)
        self.conv2 = GCNConv(self.hidden, activation="relu", seed=s2)
        self.ratio, self.sigmoid_gating = self.topk.ratio, self.topk.sigmoid_gating
        self.built = False
        self._bufs = None
        self._graphs = {}

    # ---- parameters: one flat buffer (one SGD launch), every tensor on a 4-float boundary ----------------------------------
    def build(self, f_in):
        h, c = self.hidden, self.n_labels
        self.f_in = int(f_in)
        head = np.random.default_rng(self._head_seed)
        inits = {}
        for tag, layer, fi in (("conv1", self.conv1, self.f_in), ("pool", self.topk, h), ("conv2", self.conv2, h)):
            layer.ctx, layer.in_dim, layer.built = self.ctx, fi, True
            for name, _, init in layer._param_spec(fi):
                inits[f"{tag}_{name}"] = (layer, name, init)
        inits["dense_kernel"] = (None, None, glorot_uniform(head, h, c))
        inits["dense_bias"] = (None, None, np.zeros(c, np.float32))
        self._alloc_flat([(k, inits[k][2].shape) for k in self.PARAM_ORDER], align=4)
        for k in self.PARAM_ORDER:
            layer, name, init = inits[k]
            self.p[k].copy_from_host(init)
            if layer is not None:
                layer.params[name], layer.grads[name] = self.p[k], self.g[k]
        self.built = True

    def get_weights(self, as_dict=False):
        d = {k: self.p[k].numpy() for k in self.PARAM_ORDER}
        return d if as_dict else [d[k] for k in self.PARAM_ORDER]

    def set_weights(self, weights):
        if not self.built:
            raise ValueError("gcnx.TopKNet.set_weights: build(f_in) first (or run a batch)")
        if not isinstance(weights, dict):
            weights = dict(zip(self.PARAM_ORDER, weights))
        for k in self.PARAM_ORDER:
            self.p[k].copy_from_host(np.asarray(weights[k], np.float32).reshape(self.p[k].shape))

    def gradients(self):
        """Gradients of the last loss_and_grads / train_step, named as get_weights(as_dict=True)."""
        return {k: self.g[k].numpy() for k in self.PARAM_ORDER}

    @property
    def trainable_variables(self):
        return [self.p[k] for k in self.PARAM_ORDER]

    # ---- batches -------------------------------------------------------------------------------------------------------
    def _as_batch(self, inputs, target=None):
        return self._adopt(inputs, target)                       # (the adjacency's values are read: weighted)

    def _ensure(self, batch):
        if not self.built:
            self.build(batch.f)
        if batch.f != self.f_in:
            raise ValueError(f"gcnx.TopKNet was built for {self.f_in} node features, got {batch.f}")
        key = (batch.n, batch.n_graphs, batch.seg)              # (the Segments object: N' depends on every graph's size)
        if self._bufs is not None and self._bufs["key"] == key:
            return self._bufs
        v, n, b, h, c = self._views(), batch.n, batch.n_graphs, self.hidden, self.n_labels
        nk = int(D.topk_kept_ptr(batch.seg.host, self.ratio)[-1])
        self._bufs = {"key": key, "y1": v("y1", n, h), "x2": v("x2", nk, h), "y2": v("y2", nk, h), "dy2": v("dy2", nk, h),
                      "pooled": v("pooled", b, h), "dpooled": v("dpooled", b, h), "probs": v("probs", b, c)}
        return self._bufs

    # ---- the call sequences ------------------------------------------------------------------------------------------------
    def _forward(self, batch, bufs, mode, denom=None):
        """mode: "fwd" (probabilities), "loss" (+ loss and hits, cce_eval), "grads" (+ dPooled and the head's gradients, cce_train)."""
        ctx, p, g = self.ctx, self.p, self.g
        self.conv1([batch.x, batch.a], out=bufs["y1"])
        x2, a2, seg2 = self.topk([bufs["y1"], batch.a, batch.seg], out=bufs["x2"])
        self.conv2([x2, a2], out=bufs["y2"])
        self._seg2 = seg2
        D.segment_pool(ctx, seg2, bufs["y2"], bufs["pooled"], self.pool)
        if mode != "fwd" and batch.y is None:
            raise ValueError("gcnx.TopKNet: labels are needed for the loss")
        if mode == "grads":
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], batch.y, bufs["probs"], self.loss_acc, denom,
                                dw=g["dense_kernel"], db=g["dense_bias"], dpooled=bufs["dpooled"], cce=self.cce_train)
        elif mode == "loss":
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], batch.y, bufs["probs"], self.loss_acc, denom,
                                cce=self.cce_eval)
        else:
            D.dense_softmax_cce(ctx, bufs["pooled"], p["dense_kernel"], p["dense_bias"], None, bufs["probs"])

    def _backward(self, batch, bufs):
        D.segment_pool_bwd(self.ctx, self._seg2, bufs["dpooled"], bufs["dy2"], self.pool)
        dx2 = self.conv2.backward(bufs["dy2"])
        dy1 = self.topk.backward(dx2)
        self.conv1.backward(dy1, need_dx=False)

    # ---- public surface ----------------------------------------------------------------------------------------------------
    def __call__(self, inputs, training=False):
        """model((x, a, i), training=False) -> probabilities [B, n_labels]."""
        batch = self._as_batch(inputs)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "fwd")
        return bufs["probs"].numpy()

    def loss_and_grads(self, inputs, target=None, global_batch=None, _lr=None):
        """Forward + loss + every gradient (+ the SGD update with ``_lr``).  Returns the device batch."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "grads", float(global_batch or batch.n_graphs))
        self._backward(batch, bufs)
        if _lr is not None:
            self._apply_sgd(_lr)
        self._last_batch = batch
        return batch

    def train_step(self, inputs, target=None, lr=0.02, fetch=True, global_batch=None):
        """One optimisation step (gcn.py:330-340): loss, gradients, p -= lr * g.  fetch: True -> (loss, acc); False -> None;
        "stash" -> None, metrics kept on the device for collect_metrics()."""
        batch = self.loss_and_grads(inputs, target, global_batch, _lr=float(lr))
        return self._finish_step(fetch, global_batch or batch.n_graphs)

    def evaluate_batch(self, inputs, target):
        """(loss, accuracy, probabilities) without gradients (the body of evaluate(), gcn.py:350-357; loss by cce_eval)."""
        batch = self._as_batch(inputs, target)
        bufs = self._ensure(batch)
        self._forward(batch, bufs, "loss", float(batch.n_graphs))
        return (*self._loss_acc_host(batch.n_graphs), bufs["probs"].numpy())

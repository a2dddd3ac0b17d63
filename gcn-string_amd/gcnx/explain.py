"""``Explainer``: GNNExplainer (Ying et al. 2019; torch_geometric.explain's GNNExplainer with its default coefficients) for a built
``gcnx.GCN`` -- which stored entries of the batch's operator and which of the node features carried the model's decision.

The model's weights are frozen.  A soft mask on the off-diagonal entries of A^ (one logit per stored entry i <- j, so the two
directions of an edge are masked independently; the diagonal entries -- the loops GCNConv adds itself -- keep the factor 1) and,
optionally, on the input features (``node_mask="common_attributes"``: one logit per feature, ``"attributes"``: one per node and
feature) is learned by Adam on

    L = BCEWithLogits(masked logits, t) / B + 0.005 sum sigma(m) + 1.0 mean ent(sigma(m)) + 1.0 mean sigma(f) + 0.1 mean ent(sigma(f))
    ent(p) = -p log(p + 1e-15) - (1 - p) log(1 - p + 1e-15)

with t the model's own decision on the unmasked batch (``explanation_type="model"``) or the batch's labels (``"phenomenon"``).
Both convolutions read the masked operator A^_m = A^ * sigma(m) (the normalisation is not recomputed: PyG masks the messages
after gcn_norm), the first one X * sigma(f).  DESIGN.md 4.21 is the spec of record.

BatchNorm runs on batch statistics in this model, in training and in evaluation, so THE UNIT OF AN EXPLANATION IS THE BATCH: the
masks of all its graphs are learned jointly against the batch's statistics, and a batch of one graph raises as training does.

How it reaches the model: not through a hook -- the model is driven through the two seams it already has.  ``GCN._op`` serves the
operator pair of a batch from a cache keyed by the batch's uid; the explainer wraps the batch in a DeviceBatch of its own (a
fresh uid, the masked features as ``x``, the target as ``y``) and primes that cache with the masked operator and a CSR of the
TRANSPOSED pattern that carries the masked values through ``transpose_perm()`` (A^_m is not symmetric even where A^ is).  The
model's own ``_forward`` / ``_backward`` then run unchanged, on whichever conv route they pick, and leave dZ1, dZ2 and Y1 in the
model's buffers; from those: T_k = dZ_k W_k^T (gcnx_gemm_dx), dL/dv_e = <T_1[i], X'[j]> + <T_2[i], Y1[j]> (two gcnx_sddmm_csr),
dL/dX' = A^_m^T T_1 (gcnx_spmm_csr), the mask launches (csrc/explain.hip) and gcnx_adam on the explainer's own flat buffers.  The
model's update is never called; ``end()`` puts the cache back."""
from __future__ import annotations

import numpy as np

TERMS = ("loss", "edge_size", "edge_ent", "node_feat_size", "node_feat_ent")
COEFFS = {"edge_size": 0.005, "edge_ent": 1.0, "node_feat_size": 1.0, "node_feat_ent": 0.1}
NODE_MASKS = (None, "common_attributes", "attributes")
EXPLANATION_TYPES = ("model", "phenomenon")


class Explanation:
    """What ``Explainer(...)(inputs)`` returns.  Entries are the E_off off-diagonal stored entries of the batch's operator in CSR
    order: ``edge_mask`` [E_off] = sigma of the final logits, ``edge_index`` [2, E_off] in PyG's flow (row 0 the source = the
    entry's column, row 1 the target = its row), ``graph_of_edge`` [E_off]; ``node_mask`` None, [1, F] or [N, F]; ``history``
    [epochs, 5]: the terms of L per epoch in the order of ``explain.TERMS``; ``target`` [B]."""

    def __init__(self, edge_mask, edge_index, node_mask, history, target, graph_of_edge):
        self.edge_mask, self.edge_index, self.node_mask = edge_mask, edge_index, node_mask
        self.history, self.target, self.graph_of_edge = history, target, graph_of_edge

    def top_edges(self, k, graph=None):
        """(edge_index [2, k'], edge_mask [k']) of the k entries with the largest mask, largest first (ties: CSR order), over the
        whole batch or inside graph ``graph``; k' = min(k, entries there)."""
        if self.edge_mask is None:
            raise ValueError("this explanation carries no edge mask (edge_mask=False)")
        idx = np.arange(self.edge_mask.size) if graph is None else np.flatnonzero(self.graph_of_edge == int(graph))
        idx = idx[np.argsort(-self.edge_mask[idx], kind="stable")[:max(int(k), 0)]]
        return self.edge_index[:, idx], self.edge_mask[idx]


def edge_layout(rowptr, colidx, graph_ptr):
    """(off [nnz] bool: the off-diagonal entries, edge_index [2, E_off], graph_of_edge [E_off]) of a CSR pattern on the host."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    off = rows != colidx
    graph = np.searchsorted(np.asarray(graph_ptr, np.int64), rows[off], side="right") - 1
    return off, np.stack([colidx[off], rows[off]]), graph


def _sigmoid(a):
    return (1.0 / (1.0 + np.exp(-np.asarray(a, np.float32)))).astype(np.float32)


class Explainer:
    """``Explainer(model, epochs=100, lr=0.01, edge_mask=True, node_mask=None, explanation_type="model", coeffs=None, seed=0)``;
    ``explainer(inputs, target=None)`` -> ``Explanation``.  inputs: an (x, a, i) host batch or a DeviceBatch.

    model: a ``gcnx.GCN`` (exactly that class; any ``readout=`` and ``norm=``) on one device.  The unit of an explanation is the
    BATCH: BatchNorm uses batch statistics, so the masks of all graphs of the batch are learned jointly, and a batch of one
    graph raises ValueError as training does.  coeffs: {"edge_size", "edge_ent", "node_feat_size", "node_feat_ent"} over PyG's
    defaults.  Initial logits: ``np.random.default_rng(seed)``, entries N(0, (sqrt(2) sqrt(2 / (2 N)))^2), features N(0, 0.1^2).

    The stepwise surface ``__call__`` is built from: ``begin`` -> (``set_logits`` / ``logits`` / ``forward`` / ``step`` /
    ``objective`` / ``gradients`` / ``history``)* -> ``end``.  ``step`` is one forward, backward and Adam update without a host
    synchronisation; ``forward`` the masked logits alone.  The model is
    left as it was: parameters, optimizer state and the operator cache (its gradient buffer is overwritten)."""

    def __init__(self, model, epochs=100, lr=0.01, edge_mask=True, node_mask=None, explanation_type="model", coeffs=None, seed=0):
        from .models import GCN
        if type(model) is not GCN:
            raise NotImplementedError(f"gcnx.Explainer explains gcnx.GCN, not gcnx.{type(model).__name__}: the masked operator is "
                                      "GCNConv's (subclass convolutions, GCN2, GeneralGNN, ECCNet and TopKNet are not served)")
        if getattr(model, "comm", None) is not None:
            raise NotImplementedError("gcnx.Explainer: gcnx.GCN with comm= (a sharded batch) is not served: one device")
        if node_mask not in NODE_MASKS:
            raise ValueError(f"node_mask={node_mask!r} must be None, \"common_attributes\" or \"attributes\"")
        if explanation_type not in EXPLANATION_TYPES:
            raise ValueError(f"explanation_type={explanation_type!r} must be \"model\" or \"phenomenon\"")
        if not edge_mask and node_mask is None:
            raise ValueError("nothing to learn: edge_mask=False and node_mask=None")
        unknown = sorted(set(coeffs or {}) - set(COEFFS))
        if unknown:
            raise ValueError(f"coeffs: unknown keys {unknown}; known: {sorted(COEFFS)}")
        if int(epochs) < 1:
            raise ValueError(f"epochs={epochs!r} must be at least 1")
        self.model, self.epochs, self.lr = model, int(epochs), float(lr)
        self.edge_mask, self.node_mask, self.explanation_type, self.seed = bool(edge_mask), node_mask, explanation_type, seed
        self.coeffs = {**COEFFS, **{k: float(v) for k, v in (coeffs or {}).items()}}
        self._s = None

    # ---- begin / end ---------------------------------------------------------------------------------------------------------
    def begin(self, inputs, target=None):
        """Adopt the batch, fix the target, draw the initial logits, build the masked operator pair.  Ends a run still open."""
        from . import device as D
        from .models import DeviceBatch
        if self._s is not None:
            self.end()
        m = self.model
        if self.explanation_type == "phenomenon":
            has = inputs.y is not None if isinstance(inputs, DeviceBatch) else False
            if target is None and not has:
                raise ValueError("explanation_type=\"phenomenon\" explains the labels: pass target= (or a DeviceBatch that carries y)")
        saved = m._op_cache
        batch = m._as_batch(inputs, target if self.explanation_type == "phenomenon" else None)
        m._ensure(batch)                                     # (a batch of one graph, a wrong width: raises as training does)
        ctx = m.ctx
        try:
            a_hat, a_t = m._op(batch)
            n, nnz, f, b = batch.n, a_hat.nnz, batch.f, batch.n_graphs
            if self.explanation_type == "model":
                bufs = m._ensure(batch)
                m._forward(batch, bufs, "fwd")
                t = (bufs["out"].numpy().reshape(-1) > 0).astype(np.float32)
            else:
                y = batch.y.numpy()
                t = (y[:, 1] if y.ndim == 2 and y.shape[1] == 2 else y.reshape(-1)).astype(np.float32)
            off, edge_index, graph_of_edge = edge_layout(a_hat.rowptr.numpy(), a_hat.colidx.numpy()[:nnz], batch.seg.host)
            e_off = int(off.sum())
            rng = np.random.default_rng(self.seed)
            ne = -(-nnz // 4) * 4 if self.edge_mask else 0   # (the node logits start on a 16-byte boundary)
            node_shape = None if self.node_mask is None else (1, f) if self.node_mask == "common_attributes" else (n, f)
            nn = int(np.prod(node_shape)) if node_shape else 0
            host = np.zeros(ne + nn, np.float32)
            if self.edge_mask:
                host[:nnz] = rng.normal(0.0, np.sqrt(2.0) * np.sqrt(2.0 / (2.0 * n)), nnz)
            if nn:
                host[ne:] = rng.normal(0.0, 0.1, nn)
            s = {"batch": batch, "saved": saved, "a_hat": a_hat, "n": n, "nnz": nnz, "f": f, "b": b, "off": off, "e_off": e_off,
                 "edge_index": edge_index, "graph_of_edge": graph_of_edge, "target": t, "ne": ne, "nn": nn, "node_shape": node_shape,
                 "steps": 0}
            for k in ("p", "g", "m", "v"):
                s[k] = ctx.to_device(host) if k == "p" else ctx.zeros(ne + nn)
            s["t"] = ctx.zeros(1, np.int32)
            s["y"] = ctx.to_device(t)
            s["last"] = ctx.zeros(6)                         # loss sum / B, hits, sum sigma(m), sum ent(m), sum sigma(f), sum ent(f)
            s["ring"] = ctx.zeros(6 * self.epochs)
            view = lambda buf, o, k, shape=None: buf.flat(o, k, shape) if k else None
            s["pe"], s["ge"] = view(s["p"], 0, nnz if ne else 0), view(s["g"], 0, nnz if ne else 0)
            s["pn"], s["gn"] = view(s["p"], ne, nn, node_shape), view(s["g"], ne, nn, node_shape)
            s["t1"], s["t2"] = ctx.empty((n, f)), ctx.empty((n, m.hidden))
            x_in = batch.x
            if nn:
                s["xm"], s["dxm"] = ctx.empty((n, f)), ctx.empty((n, f))
                s["fscratch"] = ctx.empty(max(D.mask_scratch_floats(ctx, n, f, self.node_mask == "attributes"), 4))
                x_in = s["xm"]
            if ne:
                rp_t, ci_t, pm = batch.a.unweighted().transpose_perm()
                s["perm"], s["vals"], s["vals_t"], s["dv"] = pm, ctx.empty(max(nnz, 1)), ctx.empty(max(nnz, 1)), ctx.empty(max(nnz, 1))
                s["escratch"] = ctx.empty(D.mask_scratch_floats(ctx))
                # A^_m and, for the backward, a CSR of the transposed pattern with the masked values: never the symmetric shortcut
                a_m = D.DeviceCSR(ctx, n, nnz, a_hat.rowptr, a_hat.colidx, s["vals"], a_hat.block_ptr, a_hat.n_blocks, False,
                                  a_hat.max_block_rows)
                a_mt = D.DeviceCSR(ctx, n, nnz, rp_t, ci_t, s["vals_t"], a_hat.block_ptr, a_hat.n_blocks, False, a_hat.max_block_rows)
                s["op"] = (a_m, a_mt)
            else:
                s["op"] = (a_hat, a_t)
            s["mbatch"] = DeviceBatch(ctx, x_in, batch.a, batch.seg, s["y"])
        except Exception:
            m._op_cache = saved
            raise
        self._s = s
        return self

    def end(self):
        """Put the model's operator cache back and drop the run's buffers.  Safe to call twice, and after a step that raised."""
        s, self._s = self._s, None
        if s is not None:
            self.model._op_cache = s["saved"]

    def _state(self):
        if self._s is None:
            raise RuntimeError("gcnx.Explainer: begin(inputs) first")
        return self._s

    # ---- logits --------------------------------------------------------------------------------------------------------------
    def logits(self):
        """{"edge": [nnz] in CSR order (diagonal entries: never read) or None, "node": [1, F] / [N, F] or None}: one read."""
        s = self._state()
        host = s["p"].numpy()
        return {"edge": host[:s["nnz"]].copy() if s["ne"] else None,
                "node": host[s["ne"]:].reshape(s["node_shape"]).copy() if s["nn"] else None}

    def set_logits(self, edge=None, node=None):
        s = self._state()
        if edge is not None:
            if not s["ne"]:
                raise ValueError("edge_mask=False: there are no edge logits")
            s["pe"].copy_from_host(np.asarray(edge, np.float32).reshape(s["nnz"]))
        if node is not None:
            if not s["nn"]:
                raise ValueError("node_mask=None: there are no node logits")
            s["pn"].copy_from_host(np.asarray(node, np.float32).reshape(s["node_shape"]))

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def _scales(self, s):
        c = self.coeffs
        cnt = max(s["nn"], 1)
        return (c["edge_size"], c["edge_ent"] / max(s["e_off"], 1), c["node_feat_size"] / cnt, c["node_feat_ent"] / cnt)

    def _masked(self, s):
        """The mask launches at the current logits and the model's cache primed with their operator pair; the model's buffers."""
        from . import device as D
        m, mb = self.model, s["mbatch"]
        if s["ne"]:
            D.edge_mask_fwd(m.ctx, s["a_hat"], s["pe"], s["vals"], s["perm"], s["vals_t"])
        if s["nn"]:
            D.feat_mask_fwd(m.ctx, s["batch"].x, s["pn"], s["xm"])
        m._op_cache = (mb.uid,) + s["op"]                    # (every time: a call of the model in between re-primed it)
        return m._ensure(mb)

    def forward(self):
        """The masked model's logits [B, 1] at the current logits (a forward alone; reads them back)."""
        s = self._state()
        bufs = self._masked(s)
        self.model._forward(s["mbatch"], bufs, "fwd")
        return bufs["out"].numpy()

    def step(self):
        """One forward, backward and Adam update of the masks: launches only, nothing is read by the host."""
        from . import device as D
        s, m = self._state(), self.model
        ctx, a_hat, mb = m.ctx, s["a_hat"], s["mbatch"]
        a_mt = s["op"][1]
        ces, cee, cns, cne = self._scales(s)
        bufs = self._masked(s)
        m._forward(mb, bufs, "grads", float(s["b"]))
        m._backward(mb, bufs)
        ctx._ck(ctx.lib.gcnx_d2d(ctx.h, s["last"].ptr, m.loss_acc.ptr, 8))
        D.gemm_dx(ctx, bufs["dz1"], m.p["w1"], s["t1"])      # T_1 = dZ1 W1^T
        if s["ne"]:
            D.gemm_dx(ctx, bufs["dz2"], m.p["w2"], s["t2"])  # T_2 = dZ2 W2^T
            D.sddmm(ctx, a_hat, s["t1"], mb.x, s["dv"])
            D.sddmm(ctx, a_hat, s["t2"], bufs["y1"], s["dv"], accumulate=True)
            D.edge_mask_bwd(ctx, a_hat, s["pe"], s["dv"], s["ge"], s["last"].flat(2, 2), s["escratch"], ces, cee)
        if s["nn"]:
            D.spmm(ctx, a_mt, s["t1"], None, s["dxm"])       # dL/dX' = A^_m^T T_1
            D.feat_mask_bwd(ctx, s["dxm"], s["batch"].x, s["pn"], s["gn"], s["last"].flat(4, 2), s["fscratch"], cns, cne)
        k = s["steps"] % self.epochs
        ctx._ck(ctx.lib.gcnx_d2d(ctx.h, s["ring"].ptr + 24 * k, s["last"].ptr, 24))
        s["steps"] += 1
        D.counter_add(ctx, s["t"], 1)
        D.adam(ctx, s["p"], s["g"], s["m"], s["v"], s["t"], self.lr)

    def _terms(self, s, raw):
        ces, cee, cns, cne = self._scales(s)
        raw = np.asarray(raw, np.float64).reshape(-1, 6)
        return np.stack([raw[:, 0], ces * raw[:, 2], cee * raw[:, 3], cns * raw[:, 4], cne * raw[:, 5]], 1)

    def objective(self):
        """{term: value} of the last step's forward (``explain.TERMS``) and their "total": one read."""
        s = self._state()
        v = self._terms(s, s["last"].numpy())[0]
        return {**dict(zip(TERMS, map(float, v))), "total": float(v.sum())}

    def gradients(self):
        """{"edge": dL/dm [nnz] in CSR order (0 on the diagonal) or None, "node": dL/df in the node logits' shape or None} of
        the last step's backward."""
        s = self._state()
        host = s["g"].numpy()
        return {"edge": host[:s["nnz"]].copy() if s["ne"] else None,
                "node": host[s["ne"]:].reshape(s["node_shape"]).copy() if s["nn"] else None}

    def history(self):
        """[steps, 5]: the terms of the steps taken since begin (the last ``epochs`` of them), from one read of the device ring."""
        s = self._state()
        taken = min(s["steps"], self.epochs)
        raw = s["ring"].numpy().reshape(self.epochs, 6)
        if s["steps"] > self.epochs:
            raw = np.roll(raw, -(s["steps"] % self.epochs), axis=0)
        return self._terms(s, raw[:taken])

    # ---- the whole run -------------------------------------------------------------------------------------------------------
    def __call__(self, inputs, target=None):
        self.begin(inputs, target)
        try:
            s = self._s
            for _ in range(self.epochs):
                self.step()
            lg, hist = self.logits(), self.history()
            edge = _sigmoid(lg["edge"][s["off"]]) if s["ne"] else None
            node = _sigmoid(lg["node"]) if s["nn"] else None
            return Explanation(edge, s["edge_index"], node, hist, s["target"].copy(), s["graph_of_edge"])
        finally:
            self.end()

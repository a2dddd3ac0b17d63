"""Host mirror of the Spektral / Keras layer call surface used on the hot path.

Upstream signatures kept: ``GCNConv(channels, activation=None, use_bias=True,
kernel_initializer="glorot_uniform", bias_initializer="zeros")`` called as ``layer([x, a])``;
``GCNConv.preprocess(a)``; ``GlobalSumPool()([x, i])`` (+ Avg/Max); ``Dense(units, activation)``.
Reference topology: GCNConv -> GCNConv -> global pool -> Linear (gcn_utills.py:805-808,
832-842); live model ctor gcn.py:320, forward gcn.py:334/351, gradients gcn.py:337.
``SAGEConv(channels, root_weight=True, use_bias=True)`` is PyG's layer of that name (aggr="mean"), which the reference
names as its next step (gcn_utills.py:804-806); ``GATConv(channels, heads=1)`` is PyG's attention layer for the same slot.
``GINConv(channels, mlp_hidden=None, eps=0.0, train_eps=False)`` is PyG's / Spektral's Graph Isomorphism Network layer for it.
``GINEConv(channels, edge_dim, mlp_hidden=None, eps=0.0, train_eps=False)`` is PyG's GINEConv: GIN whose neighbour sum reads the edge features (gcn.py:71).
``ChebConv(channels, K=3, lambda_max=2.0)`` is PyG's Chebyshev spectral convolution: K filter terms, one weight matrix per hop distance.
``RGCNConv(channels, num_relations=None, relations="nonzero", root_weight=True)`` is PyG's relational convolution (aggr="mean"): one weight matrix per edge type, the type read off the edge features.
``PNAConv(channels, deg=None, avg_deg_log=None)`` is PyG's PNAConv with the mean / min / max / std aggregators and the three degree scalers.
``GATv2Conv(channels, heads=1, edge_dim=None)`` is PyG's GATv2Conv: attention whose scores read the edge features (gcn.py:71).
``ResGatedGraphConv(channels, edge_dim=None, root_weight=True)`` is PyG's gated layer: per-channel sigmoid gates that read the edge features.
``TransformerConv(channels, heads=1, beta=False, edge_dim=None, root_weight=True)`` is PyG's dot-product attention with edge features in keys and values.
``TopKPool(ratio)`` is Spektral's pooling layer of that name, which the
reference's script imports (gcn.py:10), called as ``layer([x, a, seg])``.

There is no autograd here: every layer has ``backward(dy)`` that returns dx and leaves the
parameter gradients in ``layer.grads`` (what tape.gradient, gcn.py:337, would produce).
All arithmetic runs in libgcnx (HIP); these classes only own buffers and sequence calls.
"""
from __future__ import annotations

import os

import numpy as np

from . import convs
from . import device as D
from .convs import pna_backward, pna_forward     # (the models and the tests import the two from here)
from .params import block_views, from_pyg, join_blocks, to_pyg

_FUSED_KNOB = os.environ.get("GCNX_FUSED", "1") != "0"     # tuning knob, read once at import (diagnostics)


def glorot_uniform(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


class Layer:
    """Keras-like lazy build: parameters are created on the first call, when the input width
    is known.  ``storage`` lets a model place all parameters in one flat buffer."""

    ALIGN = 1           # floats between the starts of two tensors in a caller's store (4: every tensor on a 16-byte boundary)
    OWN_ALIGN = 1       # the same where the layer allocates its own storage
    # {attribute: its blocks}: the stacked tensors.  One stored tensor each, kept as ``self.<attribute>`` (its gradient as
    # ``<attribute>_grad``), allocated where _stored_spec lists its first block and initialised from the blocks' initial values
    # side by side; ``params`` / ``grads`` hold the named blocks as views.  A block is a name of _stored_spec (skipped where the
    # spec has none) or an int: that many unnamed zeros.  This table is the only statement of the block order.
    STACKS = {}
    LEADING_AXIS = ()   # the names that carry a leading axis of 1 in PyG ([1, heads, channels], [1, 3 heads channels])

    def __init__(self, ctx=None, seed=None):
        self.ctx = ctx
        self.built = False
        self.params, self.grads = {}, {}
        self._rng = np.random.default_rng(seed)
        self._seed = 0 if seed is None else int(seed)    # of the layer's Dropout streams
        self._scratch = {}

    # parameter spec: list of (name, shape, initial host array)
    def _param_spec(self, in_dim):
        return []

    def _stored_spec(self, in_dim):
        """_param_spec under the names and in the layouts of ``params`` (a layer whose _param_spec speaks PyG's converts here)."""
        return self._param_spec(in_dim)

    def _storage(self, in_dim):
        """(the stored spec, [(attribute or None, [(block name or None, initial value)])] in storage order)."""
        spec = [(name, np.asarray(init, np.float32).reshape(shape)) for name, shape, init in self._stored_spec(in_dim)]
        init, stored, seen = dict(spec), [], set()
        owner = {b: attr for attr, blocks in self.STACKS.items() for b in blocks if b in init}
        for name, v in spec:
            attr = owner.get(name)
            if attr is None:
                stored.append((None, [(name, v)]))
            elif attr not in seen:
                seen.add(attr)
                stored.append((attr, [(None, np.zeros(b, np.float32)) if isinstance(b, int) else (b, init[b])
                                      for b in self.STACKS[attr] if isinstance(b, int) or b in init]))
        return spec, stored

    def n_params(self, in_dim):
        """Floats of storage in a caller's store."""
        return sum(-(-sum(v.size for _, v in blocks) // self.ALIGN) * self.ALIGN for _, blocks in self._storage(in_dim)[1])

    def build(self, ctx, in_dim, p_store=None, g_store=None, offset=0):
        self.ctx = ctx
        spec, stored = self._storage(in_dim)
        align = self.ALIGN if p_store is not None else self.OWN_ALIGN
        pad = lambda n: -(-n // align) * align
        if p_store is None:
            total = max(sum(pad(sum(v.size for _, v in blocks)) for _, blocks in stored), 1)
            p_store, g_store, offset = ctx.zeros(total), ctx.zeros(total), 0
        off, views = offset, {}
        for attr in self.STACKS:                            # (a stack none of whose blocks is in the spec stays None)
            setattr(self, attr, None)
            setattr(self, attr + "_grad", None)
        for attr, blocks in stored:
            init = np.concatenate([v for _, v in blocks], axis=-1)
            pv, gv = p_store.flat(off, init.size, init.shape), g_store.flat(off, init.size, init.shape)
            pv.copy_from_host(init)
            off += pad(init.size)
            if attr is None:
                views[blocks[0][0]] = (pv, gv)
                continue
            setattr(self, attr, pv)
            setattr(self, attr + "_grad", gv)
            widths = [(name, v.shape[-1]) for name, v in blocks]
            pb, gb = block_views(pv, widths), block_views(gv, widths)
            views.update({name: (pb[name], gb[name]) for name in pb})
        for name, _ in spec:                                # ``params`` / ``grads`` list the spec's names in the spec's order
            self.params[name], self.grads[name] = views[name]
        self.in_dim, self.built = in_dim, True
        return off

    def _load(self, host):
        """{name in ``params``: array in the stored layout} into the storage; the blocks of a stacked tensor go up as one."""
        host = dict(host)
        for attr, blocks in self.STACKS.items():
            blocks = [b for b in blocks if isinstance(b, int) or b in host]
            if any(isinstance(b, str) for b in blocks):
                getattr(self, attr).copy_from_host(join_blocks(host, blocks))
        for k, v in host.items():
            self.params[k].copy_from_host(v)

    def _pyg_keys(self, t):
        """(PyG name, name in t, transposed) of a layer whose names are PyG's: a .weight is [out, in] there, [in, out] here."""
        return [(k, k, k.endswith(".weight")) for k in t], [k for k in self.LEADING_AXIS if k in t]

    def _pyg(self, t):
        """{PyG name: array in PyG's layout} of ``params`` or ``grads``."""
        return to_pyg(t, *self._pyg_keys(t))

    def _edge_inputs(self, inputs, optional=True, refuse_bipartite=False):
        """(x, a, e) of a call's [x, a] or [x, a, e], checked against the layer's edge_dim: e is [nnz, edge_dim], one row per
        stored entry of a, and is there exactly when the layer was built with edge_dim.  ``optional=False``: a layer that
        always reads e.  ``refuse_bipartite``: for PyG's layers that take an (x_source, x_target) pair."""
        name, d = type(self).__name__, self.edge_dim
        if len(inputs) not in ((2, 3) if optional else (3,)):
            raise ValueError(f"{name} takes [x, a] or [x, a, e]" if optional else f"{name}(edge_dim={d}) takes [x, a, e]")
        x, a = inputs[:2]
        if refuse_bipartite and isinstance(x, (tuple, list)):
            raise NotImplementedError(f"{name}: bipartite inputs (x_source, x_target) have no kernel")
        e = inputs[2] if len(inputs) == 3 else None
        if e is not None and d is None:
            raise ValueError(f"{name}: edge features given to a layer built without edge_dim")
        if e is None and d is not None:
            raise ValueError(f"{name}(edge_dim={d}) takes [x, a, e]")
        if e is not None and tuple(e.shape) != (a.nnz, d):
            raise ValueError(f"{name}(edge_dim={d}): e must be [{a.nnz}, {d}] (one row per stored entry), got {list(e.shape)}")
        return x, a, e

    def _buf(self, key, shape, dtype=np.float32):
        b = self._scratch.get(key)
        if b is None or b.shape != tuple(shape):
            b = self.ctx.empty(shape, dtype)
            self._scratch[key] = b
        return b

    def get_weights(self):
        return [self.params[k].numpy() for k in self.params]

    def set_weights(self, weights):
        """Arrays in the order and the stored layouts of ``params``."""
        self._load(dict(zip(self.params, weights)))

    @property
    def trainable_variables(self):
        return list(self.params.values())

    def __call__(self, inputs, **kw):
        return self.call(inputs, **kw)


def _unweighted(a):
    """The stored pattern of a DeviceCSR, unweighted: no loop added or removed, values ignored (the ``preprocess`` of the layers
    that use the adjacency exactly as stored)."""
    return a.unweighted()


class GCNConv(Layer):
    """out = activation(A^ (x W) + b)   -- bias after aggregation."""

    def __init__(self, channels, activation=None, use_bias=True, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", prec="f32", **kw):
        super().__init__(**kw)
        if activation not in (None, "linear", "relu"):
            raise NotImplementedError(f"GCNConv activation {activation!r}: only None/'relu' are fused in the SpMM epilogue")
        if kernel_initializer != "glorot_uniform" or bias_initializer != "zeros":
            raise NotImplementedError("only glorot_uniform / zeros initialisers (the Spektral defaults)")
        self.channels, self.activation, self.use_bias, self.prec = int(channels), activation, use_bias, prec

    @staticmethod
    def preprocess(a, mode="spektral"):
        """gcn_filter on one graph's scipy adjacency (a dataset transform in Spektral): adds I
        unconditionally (diagonal 2 where a self-loop exists), D^-1/2 A~ D^-1/2 (8.A.2)."""
        import scipy.sparse as sp

        a = sp.csr_matrix(a, dtype=np.float64)
        if mode == "spektral":
            a = a + sp.identity(a.shape[0], format="csr")
        else:  # PyG add_remaining_self_loops
            a = a + sp.diags(np.where(a.diagonal() == 0, 1.0, 0.0))
        a = sp.csr_matrix(a)
        deg = np.asarray(a.sum(1)).ravel()
        dinv = np.zeros_like(deg)
        dinv[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
        out = sp.csr_matrix(sp.diags(dinv) @ a @ sp.diags(dinv))
        out.sort_indices()
        return out

    def _param_spec(self, in_dim):
        spec = [("kernel", (in_dim, self.channels), glorot_uniform(self._rng, in_dim, self.channels))]
        if self.use_bias:
            spec.append(("bias", (self.channels,), np.zeros(self.channels, np.float32)))
        return spec

    def call(self, inputs, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n = x.shape[0]
        y = out if out is not None else self._buf("y", (n, self.channels))
        if self._one_launch(x, a):
            # small-feature regime: (A x) W in one launch (csrc/fused.hip); S = A x is kept for dW = S^T dZ
            s = self._buf("s", (n, x.shape[1]))
            D.gcn_conv_fwd(self.ctx, a, x, self.params["kernel"], self.params.get("bias"), y, act=self.activation, s=s,
                           prec=self.prec)
            self._saved = (x, a, y, s)
            return y
        h = self._buf("h", (n, self.channels))
        D.gemm(self.ctx, x, self.params["kernel"], None, h, prec=self.prec)
        D.spmm(self.ctx, a, h, self.params.get("bias"), y, act=self.activation)
        self._saved = (x, a, y, None)
        return y

    def _one_launch(self, x, a):
        return (self.prec in ("f32", "bf16x3") and getattr(a, "plan", None) is None and x.contiguous and _FUSED_KNOB
                and D.gcn_conv_fused_ok(self.ctx, x.shape[0], x.shape[1], self.channels, x.ld))

    def backward(self, dy, need_dx=True, dy_is_dz=False):
        """dy: gradient wrt the layer output.  dy_is_dz=True when the caller already applied the
        activation mask and filled grads['bias'] (fused upstream)."""
        x, a, y, s = self._saved
        n = x.shape[0]
        dz = dy
        if not dy_is_dz:
            dz = self._buf("dz", (n, self.channels))
            D.act_bias_grad(self.ctx, dy, y, dz, self.activation, db=self.grads.get("bias"))
        if s is not None:                        # forward was (A x) W: dW = S^T dZ, dx = A^T (dZ W^T)
            D.gemm_dw(self.ctx, s, dz, self.grads["kernel"], prec=self.prec)
            if not need_dx:
                return None
            t = self._buf("t", (n, self.in_dim))
            D.gemm_dx(self.ctx, dz, self.params["kernel"], t, prec=self.prec)
            dx = self._buf("dx", (n, self.in_dim))
            D.spmm(self.ctx, a.transpose(), t, None, dx)
            return dx
        dh = self._buf("h", (n, self.channels))  # forward scratch is dead by now
        D.spmm(self.ctx, a.transpose(), dz, None, dh)
        D.gemm_dw(self.ctx, x, dh, self.grads["kernel"], prec=self.prec)
        if not need_dx:
            return None
        dx = self._buf("dx", (n, self.in_dim))
        D.gemm_dx(self.ctx, dh, self.params["kernel"], dx, prec=self.prec)
        return dx


def _aligned16(*arrays):
    return all(a is None or a.ptr % 16 == 0 for a in arrays)


class SAGEConv(Layer):
    """torch_geometric.nn.SAGEConv(in, channels, aggr="mean"), the layer the reference's torch model names as its next step
    (gcn_utills.py:804-806):   out_i = mean_{j in N(i)} x_j W_l + b + x_i W_r

    ``SAGEConv(channels, root_weight=True, use_bias=True, activation=None)``, called as ``layer([x, a_mean])`` with
    ``a_mean = SAGEConv.preprocess(a)``: the stored pattern of ``a`` with 1 / (entries of the row) on every entry -- the
    adjacency is used exactly as stored, no loop is added or removed, values are ignored; a row without entries
    aggregates to 0.  Parameters under PyG's names and in its named_parameters() order: ``lin_l.weight``, ``lin_l.bias``,
    ``lin_r.weight``; the weights are stored [in, channels] (PyG: [channels, in]), initialised U(+-1/sqrt(in)) as torch's
    Linear.  ``backward(dy)`` returns dx and leaves the three gradients in ``grads``.

    One launch per direction where gcnx_sage_conv serves the shapes (csrc/sage.hip): the forward keeps S = A x, both weight
    gradients are one gcnx_gemm_dw2 (S^T dY, x^T dY), dx is the same kernel on the transposed operator with the weights as
    stored.  Otherwise (root_weight=False, widths the kernel refuses) the composed route: gcnx_spmm_csr, gcnx_gemm
    (twice, + gcnx_add) forward; gcnx_gemm_dx, gcnx_spmm_csr, gcnx_gemm_dx(accumulate) backward."""

    def __init__(self, channels, root_weight=True, use_bias=True, activation=None, fused=True, **kw):
        super().__init__(**kw)
        if activation not in (None, "linear"):
            raise NotImplementedError(f"SAGEConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        self.channels, self.root_weight, self.use_bias, self.activation = int(channels), bool(root_weight), bool(use_bias), activation
        self.fused = bool(fused)

    @staticmethod
    def preprocess(a):
        """The row-mean operator of a DeviceCSR: same pattern, 1 / (entries of the row) on every entry."""
        return a.unweighted().row_mean()

    def _param_spec(self, in_dim):
        lim, c = 1.0 / np.sqrt(in_dim), self.channels
        u = lambda *s: self._rng.uniform(-lim, lim, s).astype(np.float32)
        spec = [("lin_l.weight", (in_dim, c), u(in_dim, c))]
        if self.use_bias:
            spec.append(("lin_l.bias", (c,), u(c)))
        if self.root_weight:
            spec.append(("lin_r.weight", (in_dim, c), u(in_dim, c)))
        return spec

    def _one_launch(self, x, fo, *others):
        return (self.fused and self.root_weight and D.sage_conv_ok(self.ctx, x.shape[0], x.shape[1], fo, x.ld)
                and _aligned16(x, self.params["lin_l.weight"], self.params["lin_r.weight"], *others))

    def call(self, inputs, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, c, p = self.ctx, x.shape[0], self.channels, self.params
        y = out if out is not None else self._buf("y", (n, c))
        s = self._buf("s", (n, x.shape[1]))
        if self._one_launch(x, c, y, s):
            D.sage_conv(ctx, a, x, p["lin_l.weight"], p["lin_r.weight"], p.get("lin_l.bias"), y, s=s)
        else:
            D.spmm(ctx, a, x, None, s)
            D.gemm(ctx, s, p["lin_l.weight"], p.get("lin_l.bias"), y)
            if self.root_weight:
                h = self._buf("h", (n, c))
                D.gemm(ctx, x, p["lin_r.weight"], None, h)
                D.add(ctx, y, h, y)
        self._saved = (x, a, s)
        return y

    def backward(self, dy, need_dx=True):
        x, a, s = self._saved
        ctx, p, g = self.ctx, self.params, self.grads
        if self.use_bias:
            D.act_bias_grad(ctx, dy, None, dy, None, db=g["lin_l.bias"])            # column sums of dy
        if self.root_weight:
            D.gemm_dw2(ctx, s, dy, g["lin_l.weight"], x, dy, g["lin_r.weight"])      # dW_l = S^T dY, dW_r = x^T dY
        else:
            D.gemm_dw(ctx, s, dy, g["lin_l.weight"])
        if not need_dx:
            return None
        dx = self._buf("dx", x.shape)
        if self._one_launch(dy, self.in_dim, dx):
            D.sage_conv(ctx, a.transpose(), dy, p["lin_l.weight"], p["lin_r.weight"], None, dx, w_transposed=True)
            return dx
        t = self._buf("t", x.shape)
        D.gemm_dx(ctx, dy, p["lin_l.weight"], t)
        D.spmm(ctx, a.transpose(), t, None, dx)                                     # A^T (dY W_l^T)
        if self.root_weight:
            D.gemm_dx(ctx, dy, p["lin_r.weight"], dx, accumulate=True)              # + dY W_r^T
        return dx


class APPNPConv(Layer):
    """spektral.layers.APPNPConv, personalised-PageRank propagation behind a Dense layer (PyG: Linear + APPNP(K, alpha)):

        h = x W + b        z^0 = h        z^{k+1} = (1 - alpha) A^ z^k + alpha h        out = z^propagations

    ``APPNPConv(channels, alpha=0.2, propagations=1, mlp_hidden=None, dropout_rate=0.0, activation=None, use_bias=True)``, called
    as ``layer([x, a_hat])`` with ``a_hat`` the gcn_filter operator (``APPNPConv.preprocess`` = ``GCNConv.preprocess``, or
    ``DeviceCSR.gcn_norm``).  The signature follows Spektral's source from memory: Spektral could not be installed to confirm
    it against a live layer.  ``mlp_hidden`` other than None (hidden Dense layers ahead of the propagation) and
    ``dropout_rate != 0`` raise NotImplementedError; ``activation`` must be None / "linear".  Parameters ``kernel``
    [in, channels] (glorot_uniform) and ``bias`` (zeros), Keras' Dense defaults.

    Launches: gcnx_gemm, then gcnx_appnp_propagate (csrc/appnp.hip): one launch that keeps every graph's rows in LDS across all
    hops where the operator carries its graphs (a disjoint batch), the width is a multiple of 4 and there are enough hops to earn
    the staging back (3; 2 on graphs of up to 256 rows), otherwise one launch per hop.  Nothing is kept for the backward: it is the same propagation on the transposed operator applied to dy, then the
    Dense layer's gradients.  ``col_block``: gcnx_appnp_propagate's (0: the library's route, -1: one launch per hop)."""

    def __init__(self, channels, alpha=0.2, propagations=1, mlp_hidden=None, dropout_rate=0.0, activation=None, use_bias=True,
                 col_block=0, **kw):
        super().__init__(**kw)
        if mlp_hidden is not None:
            raise NotImplementedError(f"APPNPConv mlp_hidden={mlp_hidden!r}: only None (one Dense layer ahead of the propagation)")
        if float(dropout_rate) != 0.0:
            raise NotImplementedError(f"APPNPConv dropout_rate={dropout_rate!r}: only 0 (no dropout inside the layer)")
        if activation not in (None, "linear"):
            raise NotImplementedError(f"APPNPConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if isinstance(propagations, bool) or int(propagations) != propagations or not 0 <= int(propagations) <= 64:
            raise NotImplementedError(f"APPNPConv propagations={propagations!r} must be an int in 0 .. 64 (what gcnx_appnp_propagate serves)")
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"APPNPConv alpha={alpha!r} must be in [0, 1]")
        self.channels, self.alpha, self.propagations = int(channels), float(alpha), int(propagations)
        self.use_bias, self.activation, self.col_block = bool(use_bias), activation, int(col_block)

    preprocess = staticmethod(GCNConv.preprocess)

    def _param_spec(self, in_dim):
        spec = [("kernel", (in_dim, self.channels), glorot_uniform(self._rng, in_dim, self.channels))]
        if self.use_bias:
            spec.append(("bias", (self.channels,), np.zeros(self.channels, np.float32)))
        return spec

    def _scratch_buf(self, n):
        return self._buf("scratch", (max(D.appnp_scratch_floats(self.ctx, n, self.channels), 4),))

    def call(self, inputs, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n, c, p = x.shape[0], self.channels, self.params
        y = out if out is not None else self._buf("y", (n, c))
        convs.appnp_forward(self.ctx, a, x, p["kernel"], p.get("bias"), self._buf("h", (n, c)), y, self.propagations, self.alpha,
                            self._scratch_buf(n), col_block=self.col_block)
        self._saved = (x, a)
        return y

    def backward(self, dy, need_dx=True):
        x, a = self._saved
        p, g = self.params, self.grads
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.appnp_backward(self.ctx, a.transpose(), x, dy, p["kernel"], g["kernel"], g.get("bias"), self._buf("h", dy.shape),
                             self.propagations, self.alpha, self._scratch_buf(x.shape[0]), dx, col_block=self.col_block)
        return dx


class ChebConv(Layer):
    """torch_geometric.nn.ChebConv(in, channels, K, normalization="sym", lambda_max) (Defferrard et al. 2016), the Chebyshev
    spectral convolution: the K-hop layer with one weight matrix per hop distance, for the slot the reference's author left open
    (gcn_utills.py:804-806):

        out = sum_{k < K} T_k(L^) x W_k + b      T_0 = I   T_1 = L^   T_k = 2 L^ T_{k-1} - T_{k-2}      L^ = (2 / lambda_max) L - I

    with L = I - D^-1/2 A D^-1/2 on the adjacency without its loops (PyG's get_laplacian: loops removed, the degree taken on
    the source index), so L^ = -(2 / lambda_max) S + (2 / lambda_max - 1) I with S = ``ChebConv.preprocess(a)``.  K is PyG's:
    the NUMBER of terms, 1 .. 16 (spektral.layers.ChebConv(channels, K) counts one less: its K is the highest order).
    ``lambda_max`` is a number > 0 (default 2.0, which bounds the spectrum of the symmetric normalised Laplacian; nothing is
    estimated); a value below the operator's largest eigenvalue makes the terms grow with k.

    ``ChebConv(channels, K=3, lambda_max=2.0, use_bias=True, activation=None, col_block=0)``, called as ``layer([x, s])``.
    Parameters under PyG's names ``lins.{k}.weight`` ([in, channels] here, [channels, in] in PyG; glorot) and ``bias`` (zeros);
    the weights are the column blocks of one stacked tensor ``weight`` [in, K channels] (gradient ``weight_grad``).
    ``normalization`` other than "sym", an activation, or K outside 1 .. 16 raise NotImplementedError.

    Launches (cheb_forward / cheb_backward of gcnx/convs.py, which the model runs too; csrc/cheb.hip): gcnx_gemm (H = x W), then
    gcnx_cheb_sum -- Clenshaw summation, K - 1 gathers in one launch that keeps every graph's rows in LDS where the operator
    carries its graphs, the width is a multiple of 4 and there are enough gathers to earn the staging back (3; 2 on graphs of up
    to 256 rows), otherwise one launch per gather.  Nothing is kept for the backward: gcnx_cheb_basis on the transposed operator
    gives G = [T_k(L^^T) dy], then dW = x^T G (one gcnx_gemm_dw) and dx = G W^T (one gcnx_gemm_dx).  ``col_block``: the kernels'
    (0: the library's route, -1: one launch per gather)."""

    MAX_K = 16

    def __init__(self, channels, K=3, lambda_max=2.0, use_bias=True, activation=None, col_block=0, normalization="sym", **kw):
        super().__init__(**kw)
        if activation not in (None, "linear"):
            raise NotImplementedError(f"ChebConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if normalization != "sym":
            raise NotImplementedError(f"ChebConv normalization={normalization!r}: only \"sym\"")
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= self.MAX_K:
            raise NotImplementedError(f"ChebConv K={K!r} must be an int in 1 .. {self.MAX_K} (what the Chebyshev kernels serve)")
        if not float(lambda_max) > 0.0 or not np.isfinite(float(lambda_max)):
            raise ValueError(f"ChebConv lambda_max={lambda_max!r} must be a finite number > 0")
        self.channels, self.K, self.lambda_max = int(channels), int(K), float(lambda_max)
        self.use_bias, self.activation, self.col_block = bool(use_bias), activation, int(col_block)
        self.STACKS = {"weight": tuple(f"lins.{k}.weight" for k in range(self.K))}

    @staticmethod
    def preprocess(a):
        """The operator S of a DeviceCSR (DeviceCSR.cheb_norm): r_i w_ij r_j off the diagonal, 0 on a stored diagonal entry."""
        return a.cheb_norm()

    def _param_spec(self, in_dim):
        c = self.channels
        spec = [(f"lins.{k}.weight", (in_dim, c), glorot_uniform(self._rng, in_dim, c)) for k in range(self.K)]
        if self.use_bias:
            spec.append(("bias", (c,), np.zeros(c, np.float32)))
        return spec

    def _scratch_buf(self, n):
        return self._buf("scratch", (max(D.cheb_scratch_floats(self.ctx, n, self.channels), 4),))

    def call(self, inputs, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n, c = x.shape[0], self.channels
        y = out if out is not None else self._buf("y", (n, c))
        convs.cheb_forward(self.ctx, a, x, self.weight, self.params.get("bias"), self._buf("h", (n, self.K * c)), y, self.K,
                           self.lambda_max, self._scratch_buf(n), col_block=self.col_block)
        self._saved = (x, a)
        return y

    def backward(self, dy, need_dx=True):
        x, a = self._saved
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.cheb_backward(self.ctx, a.transpose(), x, dy, self.weight, self.weight_grad, self.grads.get("bias"),
                            self._buf("h", (x.shape[0], self.K * self.channels)), self.K, self.lambda_max,
                            self._scratch_buf(x.shape[0]), dx, col_block=self.col_block)
        return dx


class RGCNConv(Layer):
    """torch_geometric.nn.RGCNConv(in, channels, num_relations, aggr="mean", root_weight, bias) (Schlichtkrull et al. 2018)
    without a decomposition: every stored entry has one of R <= 4 relations and every relation its own weight matrix -- the layer
    that treats the reference's inter-chain DCA bridges differently from its intra-chain contacts (gcn_utills.py:319-443):

        out_i = x_i W_root + b + sum_{r < R} mean_{k in N_r(i)} x_col(k) W_r        N_r(i): the entries of row i with relation r

    ``RGCNConv(channels, num_relations=None, relations="nonzero", root_weight=True, use_bias=True, activation=None)``, called
    as ``layer([x, a, e])`` with ``a = RGCNConv.preprocess(a)`` (the stored pattern, unweighted: no loop added or removed) and
    e [nnz, edge_dim], one row per stored entry.  relations="nonzero": an entry's relation is the first non-zero column of its
    row of e, edge_dim where there is none, so R = edge_dim + 1 (num_relations, if given, must say so); "index": e has one
    column holding the relation as an integer-valued float, num_relations must be given, and a value outside 0 .. R - 1 is
    clamped into that range on the device.  Relations and mean weights are built on every call (DeviceCSR.rgcn_operator, two
    small launches): the layer keeps nothing that could outlive the contents of e (gcnx.RGCN keeps them per batch).  basis / block decomposition, aggr other than "mean" and an activation raise
    NotImplementedError.

    Parameters under PyG's names: ``weight`` ([R in, channels] here: PyG's [R, in, channels] with the first two axes merged;
    glorot per relation), ``root`` [in, channels] (glorot) and ``bias`` (zeros).  weight and root are the row blocks of one
    stored tensor ``stack`` [(R + 1) in, channels] (gradient ``stack_grad``), which the kernel reads as one matrix.

    Launches (rgcn_forward / rgcn_backward of gcnx/convs.py, which the model runs too; csrc/rgcn.hip): gcnx_rgcn_conv where it
    serves the shapes -- one launch, which keeps the panel M = [mean_0 x | .. | mean_{R-1} x] --, otherwise gcnx_rgcn_aggregate
    and gcnx_gemm; backward gcnx_gemm_dw2 over M and x, and for dx the same launch on the transposed pattern."""

    ALIGN = OWN_ALIGN = 4
    MAX_RELATIONS = 4

    def __init__(self, channels, num_relations=None, relations="nonzero", root_weight=True, use_bias=True, activation=None, fused=True,
                 num_bases=None, num_blocks=None, aggr="mean", **kw):
        super().__init__(**kw)
        if activation not in (None, "linear"):
            raise NotImplementedError(f"RGCNConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if num_bases is not None or num_blocks is not None or aggr != "mean":
            raise NotImplementedError("RGCNConv: basis / block decomposition and aggr other than \"mean\" have no kernel")
        if relations not in ("nonzero", "index"):
            raise ValueError(f"RGCNConv relations={relations!r} must be \"nonzero\" or \"index\"")
        if relations == "index" and num_relations is None:
            raise ValueError("RGCNConv relations=\"index\" needs num_relations")
        if num_relations is not None and (isinstance(num_relations, bool) or not isinstance(num_relations, (int, np.integer))
                                          or not 1 <= int(num_relations) <= self.MAX_RELATIONS):
            raise NotImplementedError(f"RGCNConv num_relations={num_relations!r} must be an int in 1 .. {self.MAX_RELATIONS}")
        self.channels, self.R, self.relations = int(channels), None if num_relations is None else int(num_relations), relations
        self.root_weight, self.use_bias, self.activation, self.fused = bool(root_weight), bool(use_bias), activation, bool(fused)

    @staticmethod
    def preprocess(a):
        return _unweighted(a)

    def _param_spec(self, in_dim):
        r, c = self.R, self.channels
        spec = [("weight", (r * in_dim, c), np.concatenate([glorot_uniform(self._rng, in_dim, c) for _ in range(r)], axis=0))]
        if self.root_weight:
            spec.append(("root", (in_dim, c), glorot_uniform(self._rng, in_dim, c)))
        if self.use_bias:
            spec.append(("bias", (c,), np.zeros(c, np.float32)))
        return spec

    def n_params(self, in_dim):
        return sum(-(-int(np.prod(s)) // self.ALIGN) * self.ALIGN for s in self._stored_shapes(in_dim))

    def _stored_shapes(self, in_dim):
        nb = self.R + (1 if self.root_weight else 0)
        return [(nb * in_dim, self.channels)] + ([(self.channels,)] if self.use_bias else [])

    def build(self, ctx, in_dim, p_store=None, g_store=None, offset=0):
        """weight and root go into one stored tensor, row blocks of ``stack``; then the bias."""
        self.ctx = ctx
        init = {name: np.asarray(v, np.float32).reshape(shape) for name, shape, v in self._param_spec(in_dim)}
        if p_store is None:
            p_store, g_store, offset = ctx.zeros(self.n_params(in_dim)), ctx.zeros(self.n_params(in_dim)), 0
        r, c, off = self.R, self.channels, offset
        nw = self._stored_shapes(in_dim)[0][0] * c
        self.stack, self.stack_grad = p_store.flat(off, nw, (nw // c, c)), g_store.flat(off, nw, (nw // c, c))
        parts = [("weight", 0, r * in_dim)] + ([("root", r * in_dim, in_dim)] if self.root_weight else [])
        for name, row, rows in parts:
            self.params[name] = self.stack.flat(row * c, rows * c, (rows, c))
            self.grads[name] = self.stack_grad.flat(row * c, rows * c, (rows, c))
        off += -(-nw // self.ALIGN) * self.ALIGN
        if self.use_bias:
            self.params["bias"], self.grads["bias"] = p_store.flat(off, c, (c,)), g_store.flat(off, c, (c,))
            off += -(-c // self.ALIGN) * self.ALIGN
        for name, v in init.items():
            self.params[name].copy_from_host(v)
        self.in_dim, self.built = in_dim, True
        return off

    def _pyg_keys(self, t):
        return [(k, k, False) for k in t], []                       # PyG stores weight and root [in, out] too

    def _pyg(self, t):
        d = super()._pyg(t)
        d["weight"] = d["weight"].reshape(self.R, -1, self.channels)
        return d

    def _one_launch(self, x, fo, *others):
        return (self.fused and D.rgcn_conv_ok(self.ctx, x.shape[0], x.shape[1], fo, self.R, x.ld)
                and all(v.ptr % 16 == 0 and v.ld % 4 == 0 for v in (x,) + others))

    def call(self, inputs, out=None):
        if len(inputs) != 3:
            raise ValueError("RGCNConv takes [x, a, e]")
        x, a, e = inputs
        if e is None or len(e.shape) != 2 or e.shape[0] != a.nnz or (self.relations == "index" and e.shape[1] != 1):
            raise ValueError(f"RGCNConv(relations={self.relations!r}): e must be [{a.nnz}, {'1' if self.relations == 'index' else 'edge_dim'}] "
                             f"(one row per stored entry), got {None if e is None else list(e.shape)}")
        if self.R is None:
            self.R = e.shape[1] + 1
            if not 1 <= self.R <= self.MAX_RELATIONS:
                raise NotImplementedError(f"RGCNConv: edge_dim + 1 = {self.R} relations; 1 .. {self.MAX_RELATIONS} are served")
        if self.relations == "nonzero" and self.R != e.shape[1] + 1:
            raise ValueError(f"RGCNConv(relations=\"nonzero\"): num_relations={self.R} must be edge_dim + 1 = {e.shape[1] + 1}")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n, c = x.shape[0], self.channels
        y = out if out is not None else self._buf("y", (n, c))
        m = self._buf("m", (n, self.R * x.shape[1]))
        ops = a.rgcn_operator(e, self.relations, self.R)             # every call: e may have been refilled in place
        convs.rgcn_forward(self.ctx, a, ops, x, self.stack, self.params.get("bias"), m, y, self._buf("h", (n, c)), self.R,
                           self.root_weight, self._one_launch(x, c, y, m))
        self._saved = (x, a, ops, m)
        return y

    def backward(self, dy, need_dx=True):
        x, a, ops, m = self._saved
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.rgcn_backward(self.ctx, a, ops, x, m, dy, self.stack, self.stack_grad, self.grads.get("bias"),
                            self._buf("mt", (x.shape[0], self.R * self.channels)), self.R, self.root_weight,
                            need_dx and self._one_launch(dy, self.in_dim, dx), dx)
        return dx


class GINConv(Layer):
    """torch_geometric.nn.GINConv(Sequential(Linear(in, mlp_hidden), ReLU(), Linear(mlp_hidden, channels)), eps, train_eps) --
    spektral.layers.GINConv(channels, mlp_hidden=[mlp_hidden]) is the same layer -- for the slot the reference's author left
    open (gcn_utills.py:804-806):   out_i = MLP((1 + eps) x_i + sum_{j in N(i)} x_j),   MLP = Linear -> ReLU -> Linear

    ``GINConv(channels, mlp_hidden=None, eps=0.0, train_eps=False, use_bias=True, activation=None, fused=True)``, called as
    ``layer([x, a])`` with ``a = GINConv.preprocess(a)``: the stored pattern of ``a``, unweighted -- the adjacency is used
    exactly as stored, no loop is added or removed (a stored self-loop counts as one more neighbour), values are ignored.
    ``mlp_hidden`` defaults to ``channels``.  Parameters under PyG's names and in its named_parameters() order: ``eps`` (only
    with train_eps; a device scalar either way), ``nn.0.weight``, ``nn.0.bias``, ``nn.2.weight``, ``nn.2.bias``; the weights
    are stored [in, out] (PyG: [out, in]), initialised U(+-1/sqrt(fan_in)) as torch's Linear.  When the layer allocates its own storage every
    tensor starts on a 4-float boundary (what gcnx_gin_conv needs of the weights); in a caller's ``p_store`` the tensors are
    packed as the base class packs them, and a call whose weights are then off a 16-byte boundary takes the composed route.
    ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves every
    gradient in ``grads``.

    Forward: one gcnx_gin_conv launch where it serves the shapes (csrc/gin.hip), which keeps T = (1 + eps) x + A x and
    U = relu(T W_a + b_a); otherwise gcnx_gin_aggregate, gcnx_gemm(act=relu), gcnx_gemm.  Backward, both routes:
    gcnx_act_bias_grad (db_b), gcnx_gemm_dx(dZ, W_b, y_mask=U, db=db_a) -> dU, gcnx_gemm_dw2 (dW_b = U^T dZ, dW_a = T^T dU).
    dX without train_eps: the single-stage gcnx_gin_conv on the transposed pattern with x = dU and W_a as stored, or
    gcnx_gemm_dx(dU, W_a) -> dT and gcnx_gin_aggregate(A^T, dT).  With train_eps dT = dU W_a^T is formed anyway for
    d eps = sum <x, dT> (gcnx_gin_eps_grad), and dX takes gcnx_gin_aggregate(A^T, dT): no second gather-and-product launch."""

    def __init__(self, channels, mlp_hidden=None, eps=0.0, train_eps=False, use_bias=True, activation=None, fused=True, **kw):
        super().__init__(**kw)
        if activation not in (None, "linear"):
            raise NotImplementedError(f"GINConv activation {activation!r}: the layer ends in its MLP's second Linear (follow it with "
                                      "BatchNorm1d / PReLU)")
        self.channels = int(channels)
        self.mlp_hidden = int(mlp_hidden) if mlp_hidden is not None else self.channels
        self.eps, self.train_eps, self.use_bias, self.activation = float(eps), bool(train_eps), bool(use_bias), activation
        self.fused = bool(fused)
        self._eps_dev = None

    OWN_ALIGN = 4                               # own storage: every tensor on a 4-float boundary (gcnx_gin_conv's weights)
    preprocess = staticmethod(_unweighted)

    def _param_spec(self, in_dim):
        c, m = self.channels, self.mlp_hidden
        u = lambda fan_in, *s: self._rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), s).astype(np.float32)
        spec = [("eps", (1,), np.full(1, self.eps, np.float32))] if self.train_eps else []
        spec.append(("nn.0.weight", (in_dim, m), u(in_dim, in_dim, m)))
        if self.use_bias:
            spec.append(("nn.0.bias", (m,), u(in_dim, m)))
        spec.append(("nn.2.weight", (m, c), u(m, m, c)))
        if self.use_bias:
            spec.append(("nn.2.bias", (c,), u(m, c)))
        return spec

    def build(self, ctx, in_dim, p_store=None, g_store=None, offset=0):
        off = super().build(ctx, in_dim, p_store, g_store, offset)
        if not self.train_eps and self.eps != 0.0:
            self._eps_dev = ctx.to_device(np.full(1, self.eps, np.float32))
        return off

    def _eps(self):
        return self.params["eps"] if self.train_eps else self._eps_dev

    def _one_launch(self, x, k1, k2, *others):
        p = self.params
        return (self.fused and D.gin_conv_ok(self.ctx, x.shape[0], x.shape[1], k1, k2, x.ld)
                and _aligned16(x, p["nn.0.weight"], p["nn.2.weight"], *others)
                and all(o is None or o.ld % 4 == 0 for o in others))

    def call(self, inputs, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, c, m, p = self.ctx, x.shape[0], self.channels, self.mlp_hidden, self.params
        y = out if out is not None else self._buf("y", (n, c))
        t, u = self._buf("t", (n, x.shape[1])), self._buf("u", (n, m))
        if self._one_launch(x, m, c, y, t, u):
            D.gin_conv(ctx, a, x, self._eps(), p["nn.0.weight"], p.get("nn.0.bias"), p["nn.2.weight"], p.get("nn.2.bias"), y, t=t, u=u)
        else:
            D.gin_aggregate(ctx, a, x, self._eps(), t)
            D.gemm(ctx, t, p["nn.0.weight"], p.get("nn.0.bias"), u, act="relu")
            D.gemm(ctx, u, p["nn.2.weight"], p.get("nn.2.bias"), y)
        self._saved = (x, a, t, u)
        return y

    def backward(self, dy, need_dx=True):
        x, a, t, u = self._saved
        ctx, p, g, n = self.ctx, self.params, self.grads, x.shape[0]
        if self.use_bias:
            D.act_bias_grad(ctx, dy, None, dy, None, db=g["nn.2.bias"])             # db_b: column sums of dy
        du = self._buf("du", u.shape)
        D.gemm_dx(ctx, dy, p["nn.2.weight"], du, y_mask=u, db=g.get("nn.0.bias"))    # dU = (dy W_b^T) * [U > 0], db_a
        D.gemm_dw2(ctx, u, dy, g["nn.2.weight"], t, du, g["nn.0.weight"])            # dW_b = U^T dY, dW_a = T^T dU
        if not (need_dx or self.train_eps):
            return None
        dx = self._buf("dx", x.shape) if need_dx else None
        if not self.train_eps and self._one_launch(du, self.in_dim, 0, dx):
            D.gin_conv(ctx, a.transpose(), du, self._eps(), p["nn.0.weight"], None, None, None, dx, w_transposed=True)
            return dx
        dt = self._buf("dt", x.shape)
        D.gemm_dx(ctx, du, p["nn.0.weight"], dt)                                    # dT = dU W_a^T
        if self.train_eps:
            parts = self._buf("eps_parts", (D.gin_eps_grad_parts(n),))
            D.gin_eps_grad(ctx, x, dt, parts, g["eps"])                             # d eps = sum <x, dT>
        if need_dx:
            D.gin_aggregate(ctx, a.transpose(), dt, self._eps(), dx)                # dX = (1 + eps) dT + A^T dT
        return dx


class GINEConv(GINConv):
    """torch_geometric.nn.GINEConv(Sequential(Linear(in, mlp_hidden), ReLU(), Linear(mlp_hidden, channels)), eps, train_eps,
    edge_dim) (Hu et al.): GINConv whose neighbour sum reads the edge features -- the dca / proximity values the reference
    computes on every contact and bridge and its model drops (gcn_utills.py:319-443; gcn.py:71):

        out_i = MLP((1 + eps) x_i + sum_{j in N(i)} relu(x_j + lin(e_ij))),   lin = Linear(edge_dim, in),  MLP = Linear -> ReLU -> Linear

    ``GINEConv(channels, edge_dim, mlp_hidden=None, eps=0.0, train_eps=False, use_bias=True, activation=None, fused=True)``,
    called as ``layer([x, a, e])`` with ``a = GINEConv.preprocess(a)`` and e [nnz, edge_dim], row k belonging to stored entry k
    of ``a``: the pattern and e are used as stored, no loop is added or removed, values are ignored.  edge_dim is 1 .. 8;
    ``edge_dim=None`` (PyG: e already as wide as x) and any activation raise NotImplementedError.  Parameters under PyG's names:
    ``eps`` (only with train_eps), ``nn.0.weight``, ``nn.0.bias``, ``nn.2.weight``, ``nn.2.bias``, ``lin.weight`` (stored
    [edge_dim, in]; PyG: [in, edge_dim]), ``lin.bias``; use_bias=False drops the three biases.  The order follows PyG's source
    (eps, nn.*, lin.*); it was not confirmed against a live torch_geometric: prefer the names.  Initialisation
    U(+-1/sqrt(fan_in)) as torch's Linear (lin: fan_in = edge_dim).  Own storage starts every tensor on a 4-float boundary, as
    GINConv's.  ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves every gradient in ``grads``.

    Launches (gine_forward / gine_backward of gcnx/convs.py, which the model runs too; csrc/gine.hip): one gcnx_gine_conv where
    it serves the shapes, otherwise gcnx_gine_aggregate, gcnx_gemm(act=relu), gcnx_gemm; backward gcnx_act_bias_grad,
    gcnx_gemm_dx(y_mask=U, db), gcnx_gemm_dw2, gcnx_gemm_dx -> dT, gcnx_gine_bwd_edges, gcnx_gin_eps_grad (train_eps),
    gcnx_gine_bwd_nodes (need_dx)."""

    def __init__(self, channels, edge_dim, mlp_hidden=None, eps=0.0, train_eps=False, use_bias=True, activation=None, fused=True, **kw):
        if activation not in (None, "linear"):
            raise NotImplementedError(f"GINEConv activation {activation!r}: the layer ends in its MLP's second Linear (follow it with "
                                      "BatchNorm1d / PReLU)")
        if edge_dim is None or not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"GINEConv edge_dim={edge_dim}: the kernels serve 1 to 8 edge features through lin = "
                                      "Linear(edge_dim, in) (None, e already as wide as x, has no kernel)")
        super().__init__(channels, mlp_hidden, eps, train_eps, use_bias, activation, fused, **kw)
        self.edge_dim = int(edge_dim)

    def _param_spec(self, in_dim):
        d = self.edge_dim
        u = lambda *s: self._rng.uniform(-1.0 / np.sqrt(d), 1.0 / np.sqrt(d), s).astype(np.float32)
        spec = super()._param_spec(in_dim)
        spec.append(("lin.weight", (d, in_dim), u(d, in_dim)))
        if self.use_bias:
            spec.append(("lin.bias", (in_dim,), u(in_dim)))
        return spec

    def _one_launch(self, x, k1, k2, *others):
        p = self.params
        return (self.fused and D.gine_conv_ok(self.ctx, x.shape[0], x.shape[1], k1, k2, x.ld, self.edge_dim)
                and _aligned16(x, p["nn.0.weight"], p["nn.2.weight"], p["lin.weight"], p.get("lin.bias"), *others)
                and all(o.ld % 4 == 0 for o in others))

    def call(self, inputs, out=None):
        x, a, e = self._edge_inputs(inputs, optional=False)
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, c, m, p = self.ctx, x.shape[0], self.channels, self.mlp_hidden, self.params
        y = out if out is not None else self._buf("y", (n, c))
        t, u = self._buf("t", (n, x.shape[1])), self._buf("u", (n, m))
        convs.gine_forward(ctx, a, x, e, self._eps(), p["lin.weight"], p.get("lin.bias"), p["nn.0.weight"], p.get("nn.0.bias"),
                           p["nn.2.weight"], p.get("nn.2.bias"), t, u, y, self._one_launch(x, m, c, y, t, u))
        self._saved = (x, a, e, t, u)
        return y

    def backward(self, dy, need_dx=True):
        x, a, e, t, u = self._saved
        ctx, p, g, (n, f) = self.ctx, self.params, self.grads, x.shape
        du, dt = self._buf("du", u.shape), self._buf("dt", x.shape)
        scratch = self._buf("scratch", (max(D.gine_bwd_scratch_floats(ctx, n, f, self.edge_dim), 4),))
        parts = self._buf("eps_parts", (D.gin_eps_grad_parts(n),)) if self.train_eps else None
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.gine_backward(ctx, a, x, e, self._eps(), t, u, dy, p["lin.weight"], p.get("lin.bias"), p["nn.0.weight"], p["nn.2.weight"],
                            g.get("eps"), g["lin.weight"], g.get("lin.bias"), g["nn.0.weight"], g.get("nn.0.bias"), g["nn.2.weight"],
                            g.get("nn.2.bias"), du, dt, scratch, parts, dx)
        return dx


class PDNConv(Layer):
    """torch_geometric.nn.PDNConv(in, channels, edge_dim, hidden_channels, add_self_loops=True, normalize=True, bias=True)
    (Pathfinder Discovery Networks, Rozemberczki et al. 2021): GCNConv on edge weights that a two-layer MLP with a sigmoid
    learns from the edge features -- the dca / proximity values the reference computes on every contact and bridge and its
    model drops (gcn_utills.py:319-443; gcn.py:71):

        w_e = sigmoid(mlp.2(relu(mlp.0(e_ij))))     out = D_w^-1/2 A_w D_w^-1/2 (x lin) + bias,   D_w = the row sums of the w_e

    ``PDNConv(channels, edge_dim, hidden_channels, add_self_loops=True, normalize=True, bias=True)``, called as
    ``layer([x, a, e])`` or ``layer([x, a, e, unit])`` with device operands: e [nnz, edge_dim], row k belonging to stored entry
    k of ``a``; unit (uint8 [nnz], optional) marks entries whose weight is exactly 1 and not learned.  The pattern is used as
    stored, values are ignored.  ``a, e, unit = layer.preprocess(a, e)`` is PyG's add_remaining_self_loops(fill_value=1) on a
    host matrix: missing loops added in sorted position with zero feature rows and their flags (unit None where none was
    missing); with add_self_loops=False it raises NotImplementedError (pass the matrix as stored), as normalize=False does at
    construction.  edge_dim 1 .. 8, hidden_channels 1 .. 64.  Parameters under PyG's names: ``bias``, ``lin.weight`` (stored
    [in, channels]), ``mlp.0.weight`` (stored [edge_dim, hidden]), ``mlp.0.bias``, ``mlp.2.weight`` (stored [hidden, 1]),
    ``mlp.2.bias``; glorot-uniform weights drawn lin, mlp.0, mlp.2, zero biases.  ``backward(dy, need_dx=True)`` returns dx and
    leaves every gradient in ``grads``; no gradient flows to e.  ``edge_weights()``: the gates of the last call, a host array.

    Launches (pdn_forward / pdn_backward of gcnx/convs.py, which the model runs too; csrc/pdn.hip): gcnx_pdn_operator, then
    GCNConv's one launch or gcnx_gemm + gcnx_spmm_csr; backward GCNConv's launches on the transposed operator, gcnx_gemm_dx,
    gcnx_sddmm_csr, gcnx_pdn_operator_bwd."""

    def __init__(self, channels, edge_dim, hidden_channels, add_self_loops=True, normalize=True, bias=True, **kw):
        super().__init__(**kw)
        if not normalize:
            raise NotImplementedError("PDNConv normalize=False: the kernels build the normalised operator (gcnx_pdn_operator)")
        if edge_dim is None or not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"PDNConv edge_dim={edge_dim}: the kernels serve 1 to 8 edge features")
        if not 1 <= int(hidden_channels) <= 64:
            raise NotImplementedError(f"PDNConv hidden_channels={hidden_channels}: the kernels serve a gate MLP of 1 to 64 hidden units")
        self.channels, self.edge_dim, self.hidden_channels = int(channels), int(edge_dim), int(hidden_channels)
        self.add_self_loops, self.use_bias = bool(add_self_loops), bool(bias)

    def preprocess(self, a, e):
        """(scipy CSR with unit values, e', unit) of a host adjacency and its per-entry features: the missing loops added."""
        if not self.add_self_loops:
            raise NotImplementedError("PDNConv add_self_loops=False has no host transform: pass the adjacency as stored")
        import scipy.sparse as sp
        from .models import _with_unit_self_loops
        t, e, unit = _with_unit_self_loops(a, e, a.shape[0])
        idx = np.asarray(t.indices, np.int64)
        return sp.csr_matrix((np.ones(idx.shape[0]), (idx[:, 0], idx[:, 1])), shape=a.shape), e, unit

    def _param_spec(self, in_dim):
        c, d, he = self.channels, self.edge_dim, self.hidden_channels
        lin, m0, m2 = glorot_uniform(self._rng, in_dim, c), glorot_uniform(self._rng, d, he), glorot_uniform(self._rng, he, 1)
        spec = [("bias", (c,), np.zeros(c, np.float32))] if self.use_bias else []
        return spec + [("lin.weight", (in_dim, c), lin), ("mlp.0.weight", (d, he), m0), ("mlp.0.bias", (he,), np.zeros(he, np.float32)),
                       ("mlp.2.weight", (he, 1), m2), ("mlp.2.bias", (1,), np.zeros(1, np.float32))]

    def _mlp(self, t):
        return t["mlp.0.weight"], t["mlp.0.bias"], t["mlp.2.weight"], t["mlp.2.bias"]

    def call(self, inputs, out=None):
        if len(inputs) not in (3, 4):
            raise ValueError(f"PDNConv(edge_dim={self.edge_dim}) takes [x, a, e] or [x, a, e, unit]")
        x, a, e = inputs[:3]
        unit = inputs[3] if len(inputs) == 4 else None
        if tuple(e.shape) != (a.nnz, self.edge_dim):
            raise ValueError(f"PDNConv(edge_dim={self.edge_dim}): e must be [{a.nnz}, {self.edge_dim}] (one row per stored entry), "
                             f"got {list(e.shape)}")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, c, p, ne = self.ctx, x.shape[0], self.channels, self.params, max(a.nnz, 1)
        a = a.unweighted()
        rp_t, ci_t, _ = a.transpose_perm()
        y = out if out is not None else self._buf("y", (n, c))
        gate, r, s = self._buf("gate", (ne,)), self._buf("r", (n,)), self._buf("s", (n, x.shape[1]))
        mk = lambda rp, ci, vals: D.DeviceCSR(ctx, a.n, a.nnz, rp, ci, vals, a.block_ptr, a.n_blocks, False, a.max_block_rows)
        a_v, a_vt = mk(a.rowptr, a.colidx, self._buf("v", (ne,))), mk(rp_t, ci_t, self._buf("vt", (ne,)))
        ok = convs.pdn_forward(ctx, a, a_v, a_vt, x, e, unit, *self._mlp(p), p["lin.weight"], p.get("bias"), gate, r, y,
                               self._buf("h", (n, c)), s=s)
        self._saved = (x, a, a_vt, e, unit, gate, r, s if ok else None)
        return y

    def edge_weights(self):
        """The gates w_e [nnz] of the last call (before normalisation; 1 on unit entries)."""
        a, gate = self._saved[1], self._saved[5]
        return gate.numpy()[:a.nnz].copy()

    def backward(self, dy, need_dx=True):
        x, a, a_vt, e, unit, gate, r, s = self._saved
        ctx, p, g, (n, f) = self.ctx, self.params, self.grads, x.shape
        dx = self._buf("dx", x.shape) if need_dx else None
        scratch = self._buf("scratch", (max(D.pdn_bwd_scratch_floats(ctx, n, a.nnz, self.edge_dim, self.hidden_channels), 4),))
        db = g["bias"] if self.use_bias else self._buf("db", (self.channels,))
        convs.pdn_backward(ctx, a, a_vt, x, e, unit, *self._mlp(p), gate, r, dy, p["lin.weight"], g["lin.weight"], db, *self._mlp(g),
                           self._buf("t", (n, self.channels if s is None or dx is None else f)), self._buf("tl", (n, f)),
                           self._buf("gv", (max(a.nnz, 1),)), scratch, dx, s)
        return dx


PNA_AGGREGATORS = ("mean", "min", "max", "std")
PNA_SCALERS = ("identity", "amplification", "attenuation")


def pna_avg_deg_log(deg):
    """delta of PyG's DegreeScalerAggregation from its in-degree histogram: sum_d hist[d] log(d + 1) / sum_d hist[d]."""
    hist = np.asarray(deg, np.float64).ravel()
    if hist.size == 0 or hist.sum() <= 0 or np.any(hist < 0):
        raise ValueError("PNAConv: deg must be a non-empty histogram of node counts per in-degree")
    return float((hist * np.log(np.arange(hist.size) + 1.0)).sum() / hist.sum())


def pna_delta(who, deg, avg_deg_log):
    """The one delta of a PNA layer: exactly one of the histogram and the value is given."""
    if (deg is None) == (avg_deg_log is None):
        raise ValueError(f"{who}: give exactly one of deg (the in-degree histogram) and avg_deg_log")
    delta = pna_avg_deg_log(deg) if deg is not None else float(avg_deg_log)
    if not (delta > 0.0 and np.isfinite(delta)):
        raise ValueError(f"{who}: avg_deg_log must be positive and finite, got {delta} (a training set without edges?)")
    return delta


def pna_refuse(who, aggregators=None, scalers=None, towers=1, pre_layers=1, post_layers=1, divide_input=False, edge_dim=None,
               train_norm=False):
    """NotImplementedError for every PNAConv option beside the one configuration csrc/pna.hip serves."""
    if aggregators is not None and tuple(aggregators) != PNA_AGGREGATORS:
        raise NotImplementedError(f"{who}: aggregators must be {list(PNA_AGGREGATORS)} (one gather computes exactly these)")
    if scalers is not None and tuple(scalers) != PNA_SCALERS:
        raise NotImplementedError(f"{who}: scalers must be {list(PNA_SCALERS)}")
    if int(towers) != 1 or int(pre_layers) != 1 or int(post_layers) != 1 or divide_input:
        raise NotImplementedError(f"{who}: towers = pre_layers = post_layers = 1 and divide_input = False only")
    if edge_dim is not None:
        raise NotImplementedError(f"{who}: edge features (edge_dim) are not supported")
    if train_norm:
        raise NotImplementedError(f"{who}: train_norm is not supported (avg_deg_log is a constant)")


class PNAConv(Layer):
    """torch_geometric.nn.PNAConv(in, channels, aggregators=['mean', 'min', 'max', 'std'], scalers=['identity', 'amplification',
    'attenuation'], deg, towers=1, pre_layers=1, post_layers=1, divide_input=False, edge_dim=None, train_norm=False): Principal
    Neighbourhood Aggregation, four statistics of the same messages, each scaled by the node's degree:

        M_ij = [x_i | x_j] W_pre + b_pre = P_i + Q_j              P = x W_pre[:F] + b_pre,  Q = x W_pre[F:]
        A_i  = [mean_j M_ij | min_j M_ij | max_j M_ij | sqrt(relu(var_j M_ij) + 1e-5)]     (a row without entries: [0 | 0 | 0 | sqrt(1e-5)])
        C_i  = [x_i | A_i | s_amp,i A_i | s_att,i A_i],  s_amp,i = log(max(d_i, 1) + 1) / delta = 1 / s_att,i
        out  = (C W_post + b_post) W_lin + b_lin

    ``PNAConv(channels, deg=None, avg_deg_log=None, use_bias=True, seed=0)``, called as ``layer([x, a])`` with
    ``a = PNAConv.preprocess(a)``: the stored pattern of ``a``, row = target -- used exactly as stored, no loop added or removed,
    values ignored.  Exactly one of ``deg`` (PyG's in-degree histogram; delta = sum hist[d] log(d + 1) / sum hist) and
    ``avg_deg_log`` (delta itself) is required.  Any other aggregator or scaler set, towers, edge_dim or train_norm raises
    NotImplementedError.  Parameters under PyG's names: ``pre_nns.0.0.weight`` (stored [2F, F]; PyG: [F, 2F]),
    ``pre_nns.0.0.bias``, ``post_nns.0.0.weight`` (stored [13F, H]; PyG: [H, 13F]), ``post_nns.0.0.bias``, ``lin.weight``,
    ``lin.bias``; initialised U(+-1/sqrt(fan_in)) as torch's Linear.

    Launches (pna_forward / pna_backward of gcnx/convs.py, which gcnx.PNA runs too).
    Forward: gcnx_gemm twice into the halves of one [N, 2F] array (the pre weight's row halves are contiguous views),
    gcnx_pna_aggregate (csrc/pna.hip: one gather for the four statistics, all 13 blocks of C), gcnx_gemm twice.  Backward:
    gcnx_act_bias_grad (db_lin), gcnx_gemm_dx (dT, db_post), gcnx_gemm_dw2 (dW_lin = T^T dZ, dW_post = C^T dT), gcnx_gemm_dx
    (dC), gcnx_pna_bwd (dP | dQ), gcnx_act_bias_grad (db_pre), gcnx_gemm_dw2 (dW_pre = x^T [dP | dQ]), and for dx two
    gcnx_gemm_dx and a gcnx_add of dC's first block.  ``backward(dy, need_dx=True)`` returns dx."""

    def __init__(self, channels, deg=None, avg_deg_log=None, use_bias=True, aggregators=None, scalers=None, towers=1, pre_layers=1,
                 post_layers=1, divide_input=False, edge_dim=None, train_norm=False, **kw):
        super().__init__(**kw)
        pna_refuse("PNAConv", aggregators, scalers, towers, pre_layers, post_layers, divide_input, edge_dim, train_norm)
        self.channels, self.use_bias = int(channels), bool(use_bias)
        self.avg_deg_log = pna_delta("PNAConv", deg, avg_deg_log)

    OWN_ALIGN = 4                               # own storage: every tensor on a 4-float boundary (float4 lanes, the dW launches)
    preprocess = staticmethod(_unweighted)

    def _param_spec(self, in_dim):
        f, h = in_dim, self.channels
        u = lambda fan_in, *s: self._rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), s).astype(np.float32)
        spec = []
        for name, fi, fo in (("pre_nns.0.0", 2 * f, f), ("post_nns.0.0", 13 * f, h), ("lin", h, h)):
            spec.append((name + ".weight", (fi, fo), u(fi, fi, fo)))
            if self.use_bias:
                spec.append((name + ".bias", (fo,), u(fi, fo)))
        return spec

    def call(self, inputs, out=None, training=True):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, p, n, f, h = self.ctx, self.params, x.shape[0], x.shape[1], self.channels
        y = out if out is not None else self._buf("y", (n, h))
        pq, c, t = self._buf("pq", (n, 2 * f)), self._buf("c", (n, 13 * f)), self._buf("t", (n, h))
        stats = self._buf("stats", (n, 6 * f)) if training else None
        pna_forward(ctx, a, x, p["pre_nns.0.0.weight"], p.get("pre_nns.0.0.bias"), p["post_nns.0.0.weight"], p.get("post_nns.0.0.bias"),
                    p["lin.weight"], p.get("lin.bias"), self.avg_deg_log, pq, c, stats, t, y)
        self._saved = (x, a, pq, c, stats, t)
        return y

    def backward(self, dy, need_dx=True):
        x, a, pq, c, stats, t = self._saved
        if stats is None:
            raise RuntimeError("PNAConv.backward: the forward ran with training=False (no statistics were kept)")
        ctx, p, g, n, f, h = self.ctx, self.params, self.grads, x.shape[0], x.shape[1], self.channels
        ns = D.pna_bwd_scratch_floats(ctx, n, f)
        dx = self._buf("dx", (n, f)) if need_dx else None
        pna_backward(ctx, a, a.transpose(), x, pq, c, stats, t, dy, p["pre_nns.0.0.weight"], p["post_nns.0.0.weight"], p["lin.weight"],
                     g["pre_nns.0.0.weight"], g.get("pre_nns.0.0.bias"), g["post_nns.0.0.weight"], g.get("post_nns.0.0.bias"),
                     g["lin.weight"], g.get("lin.bias"), self.avg_deg_log, self._buf("dt", (n, h)), self._buf("dc", (n, 13 * f)),
                     self._buf("dpq", (n, 2 * f)), self._buf("coef", (ns,)), dx)
        return dx


class GATConv(Layer):
    """torch_geometric.nn.GATConv(in, channels, heads, concat=True, negative_slope=0.2, dropout=0.0, bias=True) -- the attention
    layer for the slot the reference's author marked as open (gcn_utills.py:804-806); spektral.layers.GATConv is the same layer:

        Hf = x W    e_ij,h = LeakyReLU(<Hf[j,h,:], att_src[h,:]> + <Hf[i,h,:], att_dst[h,:]>)    alpha = softmax over the row's entries
        out[i,h,:] = sum_j alpha_ij,h Hf[j,h,:] + bias

    ``GATConv(channels, heads=1, concat=True, negative_slope=0.2, use_bias=True, activation=None)``, called as ``layer([x, a])``
    with ``a = GATConv.preprocess(a)``: the stored pattern of ``a`` (row = target), values ignored, no loop added or removed; a
    row without entries gives the bias.  Parameters under PyG's names and in its named_parameters() order: ``att_src``,
    ``att_dst`` (stored [heads, channels]; ``state_dict()`` gives PyG's [1, heads, channels]), ``bias`` [heads * channels],
    ``lin.weight`` (stored [in, heads * channels]; PyG: [heads * channels, in]); glorot-uniform as PyG, the bias zero.
    ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves the four gradients in ``grads``.

    Launches (gat_forward / gat_backward of gcnx/convs.py, which the model runs too; csrc/gat.hip):
    gcnx_gemm, gcnx_gat_scores, gcnx_gat_aggregate forward; gcnx_act_bias_grad, gcnx_gat_bwd_edges,
    gcnx_gat_bwd_nodes, gcnx_gemm_dw, gcnx_gemm_dx backward.  There is no composed route: what the kernels do not serve
    (concat=False, attention dropout, edge features, shapes gcnx_gat_conv_ok refuses) raises NotImplementedError."""

    def __init__(self, channels, heads=1, concat=True, negative_slope=0.2, use_bias=True, activation=None, dropout=0.0, edge_dim=None,
                 **kw):
        super().__init__(**kw)
        if not concat:
            raise NotImplementedError("GATConv concat=False (the mean over heads) has no kernel: only concat=True")
        if dropout:
            raise NotImplementedError(f"GATConv dropout={dropout}: attention dropout has no kernel (only dropout=0)")
        if edge_dim is not None:
            raise NotImplementedError("GATConv edge features (edge_dim / lin_edge) have no kernel")
        if activation not in (None, "linear"):
            raise NotImplementedError(f"GATConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        self.channels, self.heads, self.negative_slope = int(channels), int(heads), float(negative_slope)
        self.concat, self.use_bias, self.activation = True, bool(use_bias), activation

    preprocess = staticmethod(_unweighted)

    def _param_spec(self, in_dim):
        h, c = self.heads, self.channels
        lim = np.sqrt(6.0 / (h + c))                       # PyG's glorot on the [1, heads, channels] tensor
        att = lambda: self._rng.uniform(-lim, lim, (h, c)).astype(np.float32)
        spec = [("att_src", (h, c), att()), ("att_dst", (h, c), att())]
        if self.use_bias:
            spec.append(("bias", (h * c,), np.zeros(h * c, np.float32)))
        spec.append(("lin.weight", (in_dim, h * c), glorot_uniform(self._rng, in_dim, h * c)))
        return spec

    LEADING_AXIS = ("att_src", "att_dst")

    def state_dict(self):
        """{PyG name: array in PyG's layout}: att_* [1, heads, channels], lin.weight [heads * channels, in]."""
        return self._pyg(self.params)

    def call(self, inputs, out=None):
        if len(inputs) != 2:
            raise NotImplementedError("GATConv takes [x, a]: edge features have no kernel")
        x, a = inputs
        h, c = self.heads, self.channels
        if not D.gat_conv_ok(x.ctx, x.shape[0], h, c):
            raise NotImplementedError(f"GATConv heads={h} channels={c} on {x.shape[0]} rows: the kernels serve heads in {{1, 2, 4, 8}}, "
                                      "heads * channels in {16, 32, 64, 128}, channels >= 4 and rows * heads * channels * 4 < 2^32")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, p = self.ctx, x.shape[0], self.params
        y = out if out is not None else self._buf("y", (n, h * c))
        hf, o = self._buf("hf", (n, h * c)), self._buf("o", (n, h * c))
        asrc, adst, alpha = self._buf("asrc", (n, h)), self._buf("adst", (n, h)), self._buf("alpha", (a.nnz, h))
        convs.gat_forward(ctx, a, x, p["lin.weight"], p["att_src"], p["att_dst"], p.get("bias"), hf, asrc, adst, alpha, o, y,
                          self.negative_slope)
        self._saved = (x, a, hf, asrc, adst, alpha, o)
        return y

    def backward(self, dy, need_dx=True):
        x, a, hf, asrc, adst, alpha, o = self._saved
        ctx, p, g, h, c, n = self.ctx, self.params, self.grads, self.heads, self.channels, x.shape[0]
        dz, dadst, dasrc = self._buf("dz", (a.nnz, h)), self._buf("dadst", (n, h)), self._buf("dasrc", (n, h))
        dhf = self._buf("dhf", (n, h * c))
        scratch = self._buf("scratch", (max(D.gat_bwd_scratch_floats(ctx, n, h, c), 1),))
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.gat_backward(ctx, a, x, hf, asrc, adst, alpha, o, dy, p["lin.weight"], p["att_src"], p["att_dst"], g["lin.weight"],
                           g["att_src"], g["att_dst"], g.get("bias"), dz, dadst, dasrc, dhf, scratch, dx, self.negative_slope)
        return dx


class GATv2Conv(Layer):
    """torch_geometric.nn.GATv2Conv(in, channels, heads, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=False,
    edge_dim=D, bias=True, share_weights=False) (Brody et al.) -- attention whose scores read the edge features, the dca /
    proximity values the reference computes and its model drops (gcn_utills.py:319-443; gcn.py:71):

        Xl = x W_l + b_l    Xr = x W_r + b_r    s_ij = Xl[j] + Xr[i] + e_ij W_e    score_ij,h = <att[h,:], LeakyReLU(s_ij)[h,:]>
        alpha = softmax over the row's entries       out[i,h,:] = sum_j alpha_ij,h Xl[j,h,:] + bias

    The LeakyReLU comes before the dot with att: the score depends jointly on target, source and edge (GATConv's ordering of
    the sources is the same for every target).  ``GATv2Conv(channels, heads=1, ..., edge_dim=None)``, called as ``layer([x, a])``
    or, with edge_dim, ``layer([x, a, e])`` with ``a = GATv2Conv.preprocess(a)`` and e [nnz, edge_dim] in the entry order of a:
    the stored pattern (row = target) and e as stored, values ignored, no loop added or removed; a row without entries gives
    the bias.  Parameters under PyG's names and in this order: ``att`` (stored [heads, channels]), ``bias``, ``lin_l.weight``,
    ``lin_l.bias``, ``lin_r.weight``, ``lin_r.bias``, ``lin_edge.weight`` (with edge_dim).  The two lin weights are the column
    halves of ONE stacked tensor [in, 2 heads channels] (``lin_weight``; PyG: two [heads channels, in]) and the two biases the
    halves of ``lin_bias``: Xl | Xr is one gcnx_gemm, the layer's backward one gcnx_gemm_dw, one column sum, one gcnx_gemm_dx.
    ``params`` / ``grads`` hold per-name views; ``state_dict()`` gives PyG's layouts.  glorot-uniform as PyG, biases zero.
    ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves the gradients in ``grads``.

    Launches (gatv2_forward / gatv2_backward of gcnx/convs.py, which the model runs too; csrc/gatv2.hip):
    gcnx_gemm, gcnx_gatv2_aggregate forward; gcnx_act_bias_grad, gcnx_gatv2_bwd_edges,
    gcnx_gatv2_bwd_nodes, gcnx_gemm_dw, gcnx_act_bias_grad, gcnx_gemm_dx backward.  There is no composed route: what the kernels
    do not serve (concat=False, attention dropout, share_weights=True, shapes gcnx_gatv2_conv_ok refuses) raises
    NotImplementedError."""

    def __init__(self, channels, heads=1, concat=True, negative_slope=0.2, use_bias=True, activation=None, dropout=0.0, edge_dim=None,
                 share_weights=False, **kw):
        super().__init__(**kw)
        if not concat:
            raise NotImplementedError("GATv2Conv concat=False (the mean over heads) has no kernel: only concat=True")
        if dropout:
            raise NotImplementedError(f"GATv2Conv dropout={dropout}: attention dropout has no kernel (only dropout=0)")
        if share_weights:
            raise NotImplementedError("GATv2Conv share_weights=True has no kernel: lin_l and lin_r are separate")
        if activation not in (None, "linear"):
            raise NotImplementedError(f"GATv2Conv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if edge_dim is not None and not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"GATv2Conv edge_dim={edge_dim}: the kernels serve 1 to 8 edge features (or None)")
        self.channels, self.heads, self.negative_slope = int(channels), int(heads), float(negative_slope)
        self.concat, self.use_bias, self.activation = True, bool(use_bias), activation
        self.edge_dim = None if edge_dim is None else int(edge_dim)

    # Storage order: att, bias, the stacked weight [in, 2 heads channels], the stacked bias, lin_edge.weight -- every tensor on a
    # 16-byte boundary when ``offset`` is.
    STACKS = {"lin_weight": ("lin_l.weight", "lin_r.weight"), "lin_bias": ("lin_l.bias", "lin_r.bias")}
    LEADING_AXIS = ("att",)
    preprocess = staticmethod(_unweighted)

    def _param_spec(self, in_dim):
        """PyG's names in its named_parameters() order, with the stored shapes ([in, heads * channels] weights)."""
        h, c, d = self.heads, self.channels, self.edge_dim or 0
        hc, rng = h * c, self._rng
        u = lambda lim, *s: rng.uniform(-lim, lim, s).astype(np.float32)
        spec = [("att", (h, c), u(np.sqrt(6.0 / (h + c)), h, c))]             # PyG's glorot on the [1, heads, channels] tensor
        if self.use_bias:
            spec.append(("bias", (hc,), np.zeros(hc, np.float32)))
        for k in ("lin_l", "lin_r"):
            spec += [(k + ".weight", (in_dim, hc), glorot_uniform(rng, in_dim, hc)), (k + ".bias", (hc,), np.zeros(hc, np.float32))]
        if d:
            spec.append(("lin_edge.weight", (d, hc), glorot_uniform(rng, d, hc)))
        return spec

    def state_dict(self):
        """{PyG name: array in PyG's layout}: att [1, heads, channels], lin_l / lin_r / lin_edge .weight [heads * channels, in]."""
        return self._pyg(self.params)

    def call(self, inputs, out=None):
        x, a, e = self._edge_inputs(inputs)
        h, c, d = self.heads, self.channels, self.edge_dim
        if not D.gatv2_conv_ok(x.ctx, x.shape[0], h, c, edge_dim=d or 0):
            raise NotImplementedError(f"GATv2Conv heads={h} channels={c} on {x.shape[0]} rows: the kernels serve heads in {{1, 2, 4, 8}}, "
                                      "heads * channels in {16, 32, 64, 128}, channels >= 4 and rows * heads * channels * 8 < 2^32")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, p = self.ctx, x.shape[0], self.params
        y = out if out is not None else self._buf("y", (n, h * c))
        xlr, o, alpha = self._buf("xlr", (n, 2 * h * c)), self._buf("o", (n, h * c)), self._buf("alpha", (a.nnz, h))
        convs.gatv2_forward(ctx, a, x, e, self.lin_weight, self.lin_bias, p["att"], p.get("bias"), p.get("lin_edge.weight"), xlr, alpha,
                            o, y, self.negative_slope)
        self._saved = (x, a, e, xlr, alpha, o)
        return y

    def backward(self, dy, need_dx=True):
        x, a, e, xlr, alpha, o = self._saved
        ctx, p, g, h, c, n = self.ctx, self.params, self.grads, self.heads, self.channels, x.shape[0]
        dscore, dxlr = self._buf("dscore", (a.nnz, h)), self._buf("dxlr", (n, 2 * h * c))
        scratch = self._buf("scratch", (max(D.gatv2_bwd_scratch_floats(ctx, n, h, c, self.edge_dim or 0), 1),))
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.gatv2_backward(ctx, a, x, e, xlr, alpha, o, dy, self.lin_weight, p["att"], p.get("lin_edge.weight"), self.lin_weight_grad,
                             self.lin_bias_grad, g["att"], g.get("bias"), g.get("lin_edge.weight"), dscore, dxlr, scratch, dx,
                             self.negative_slope)
        return dx


class ResGatedGraphConv(Layer):
    """torch_geometric.nn.ResGatedGraphConv(in, channels, act=Sigmoid(), edge_dim=D, root_weight=True, bias=True) (Bresson &
    Laurent's GatedGCN), aggr = add -- every message multiplied channel by channel by a sigmoid gate that reads target, source
    and the edge features, the dca / proximity values the reference computes and its model drops (gcn_utills.py:319-443;
    gcn.py:71).  With z_ij = [x ‖ e_ij] fed to lin_key / lin_query / lin_value (each Linear(in + D, channels) with bias):

        out_i = lin_skip(x_i) + bias + sum_j sigmoid(lin_key([x_i ‖ e_ij]) + lin_query([x_j ‖ e_ij])) * lin_value([x_j ‖ e_ij])

    No softmax: a row's messages do not compete.  ``ResGatedGraphConv(channels, edge_dim=None, root_weight=True, use_bias=True)``,
    called as ``layer([x, a])`` or, with edge_dim, ``layer([x, a, e])`` with ``a = ResGatedGraphConv.preprocess(a)`` and e
    [nnz, edge_dim] in the entry order of a: the stored pattern (row = target) and e as stored, values ignored, no loop added
    or removed; a row without entries gives lin_skip(x_i) + bias.

    Parameters under PyG's names, ``_param_spec`` in its named_parameters() order and layouts: ``bias``, ``lin_key.weight``
    [channels, in + D], ``lin_key.bias``, ``lin_query.*``, ``lin_value.*``, ``lin_skip.weight`` [channels, in] (no bias).  The
    names and layouts follow PyG 2.3+'s source, not a live module (neither torch_geometric nor a checkpoint was available).
    Every Linear of a concatenation is a sum of two products, so the layer STORES (``params`` / ``grads``) ``bias``; ``weight``
    [in, 4 channels] = the node blocks W_k | W_q | W_v | W_s (3 channels wide without root_weight); ``lin_bias`` [3 channels] =
    b_k | b_q | b_v; ``edge_weight`` [D, 3 channels] = the edge blocks W_ke | W_qe | W_ve: P = K | Q | V | S is one gcnx_gemm,
    the layer's backward one gcnx_gemm_dw, one column sum, one gcnx_gemm_dx.  ``state_dict()`` / ``gradients()`` join them into
    PyG's tensors (dW_ke and dW_qe are the same numbers), ``load_state_dict()`` splits them.  Initialisation as torch's Linear:
    U(+-1 / sqrt(fan_in)) for every weight and bias (fan_in = in + D for key / query / value), ``bias`` zero.
    ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves the gradients in ``grads``.

    Launches (resgated_forward / resgated_backward of gcnx/convs.py, which the model runs too; csrc/resgated.hip):
    gcnx_gemm, gcnx_resgated_aggregate forward; gcnx_act_bias_grad, gcnx_resgated_bwd_targets,
    gcnx_resgated_bwd_sources, gcnx_gemm_dw, gcnx_act_bias_grad, gcnx_gemm_dx backward.  There is no composed route: what the
    kernels do not serve (a gate other than the sigmoid, bipartite inputs, shapes gcnx_resgated_conv_ok refuses) raises
    NotImplementedError."""

    LINS = ("lin_key", "lin_query", "lin_value")

    def __init__(self, channels, edge_dim=None, root_weight=True, use_bias=True, activation=None, act="sigmoid", **kw):
        super().__init__(**kw)
        if not (isinstance(act, str) and act.lower() == "sigmoid"):
            raise NotImplementedError(f"ResGatedGraphConv act={act!r}: the gate of the kernels is the sigmoid")
        if activation not in (None, "linear"):
            raise NotImplementedError(f"ResGatedGraphConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if edge_dim is not None and not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"ResGatedGraphConv edge_dim={edge_dim}: the kernels serve 1 to 8 edge features (or None)")
        if int(channels) not in (16, 32, 64, 128):
            raise NotImplementedError(f"ResGatedGraphConv channels={channels}: the kernels serve 16, 32, 64 and 128 (there is no composed route)")
        self.channels, self.root_weight, self.use_bias, self.activation = int(channels), bool(root_weight), bool(use_bias), activation
        self.edge_dim = None if edge_dim is None else int(edge_dim)
        # the product's bias: lin_bias and, for the S block, as many zeros behind it (whose gradient is never written)
        self.STACKS = {"_gemm_bias": ("lin_bias",) + ((self.channels,) if self.root_weight else ())}

    preprocess = staticmethod(_unweighted)

    def _param_spec(self, in_dim):
        """PyG's names in its named_parameters() order and its layouts ([channels, in + D] weights)."""
        h, d, rng = self.channels, self.edge_dim or 0, self._rng
        u = lambda fan_in, *s: rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), s).astype(np.float32)
        spec = [("bias", (h,), np.zeros(h, np.float32))] if self.use_bias else []
        for k in self.LINS:
            spec += [(k + ".weight", (h, in_dim + d), u(in_dim + d, h, in_dim + d)), (k + ".bias", (h,), u(in_dim + d, h))]
        if self.root_weight:
            spec.append(("lin_skip.weight", (h, in_dim), u(in_dim, h, in_dim)))
        return spec

    def _width(self):
        return (4 if self.root_weight else 3) * self.channels

    def _names(self):
        """PyG's names in _param_spec's order (without drawing the initial values)."""
        return (["bias"] if self.use_bias else []) + [k + t for k in self.LINS for t in (".weight", ".bias")] + \
            (["lin_skip.weight"] if self.root_weight else [])

    def _blocks(self):
        """{stored tensor: the names of its column blocks}, PyG's but for the edge blocks ("lin_key.edge": the rows of
        lin_key.weight that read e).  Storage order: bias, weight [in, 4 channels], lin_bias [3 channels] and the zero bias of the
        S block behind it (STACKS: the product's bias is the two together; its gradient is never written), edge_weight -- every
        tensor on a 16-byte boundary when ``offset`` is."""
        t = {"weight": [k + ".weight" for k in self.LINS] + ["lin_skip.weight"] * self.root_weight, "lin_bias": [k + ".bias" for k in self.LINS]}
        if self.edge_dim:
            t["edge_weight"] = [k + ".edge" for k in self.LINS]
        return t

    def _stored(self, d, in_dim, misfit=None):
        """{name in ``params``: array} of a {PyG name: array in PyG's layout}: the [channels, in + D] tensors split into their node
        and edge blocks, the blocks side by side."""
        h, keys = self.channels, [(n, n, n.endswith(".weight")) for n in self._names()]
        shapes = {n: (in_dim, h) if tr else (h,) for n, _, tr in keys}
        edge = {k + ".weight": k + ".edge" for k in self.LINS} if self.edge_dim else None
        host = from_pyg(d, keys, shapes, "ResGatedGraphConv", edge=edge, edge_dim=self.edge_dim or 0, misfit=misfit)
        stored = {"bias": host["bias"]} if self.use_bias else {}
        stored.update({k: join_blocks(host, names) for k, names in self._blocks().items()})
        return stored

    def _stored_spec(self, in_dim):
        self._param_spec(in_dim)                # (a seed's values are those of its second draw, as they always were: the first
        #                                          one used to size the storage)
        stored = self._stored({name: init for name, _, init in self._param_spec(in_dim)}, in_dim)
        return [(k, v.shape, v) for k, v in stored.items()]

    def load_state_dict(self, d):
        """{PyG name: array in PyG's layout}: the [channels, in + D] tensors are split into their node and edge blocks."""
        def misfit(tk, v, want):
            n = tk.rsplit(".", 1)[0]
            if n in self.LINS:
                return f"{n}: shapes {np.shape(d[n + '.weight'])}, {np.shape(d[n + '.bias'])} do not fit this layer"
            return f"{tk}: shape {np.shape(d[tk])} does not fit this layer"
        self._load(self._stored(d, self.in_dim, misfit))

    def _pyg(self, t):
        h, views = self.channels, {k: t[k] for k in ("bias",) if k in t}
        for k, names in self._blocks().items():
            views.update(block_views(t[k], [(n, h) for n in names]))
        edge = {k + ".weight": k + ".edge" for k in self.LINS} if self.edge_dim else None
        return to_pyg(views, [(n, n, n.endswith(".weight")) for n in self._names()], edge=edge)

    def state_dict(self):
        """{PyG name: array in PyG's layout}: lin_key / lin_query / lin_value .weight [channels, in + D] = [node block ‖ edge block]."""
        return self._pyg(self.params)

    def gradients(self):
        """The gradients of the last backward under the names and in the layouts of state_dict()."""
        return self._pyg(self.grads)

    def call(self, inputs, out=None):
        x, a, e = self._edge_inputs(inputs, refuse_bipartite=True)
        h, d = self.channels, self.edge_dim
        w = self._width()
        if not D.resgated_conv_ok(x.ctx, x.shape[0], h, ldp=w, edge_dim=d or 0):
            raise NotImplementedError(f"ResGatedGraphConv channels={h} on {x.shape[0]} rows: the kernels serve channels in "
                                      "{16, 32, 64, 128} and rows * channels * 16 < 2^32")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, p = self.ctx, x.shape[0], self.params
        y = out if out is not None else self._buf("y", (n, h))
        pk = self._buf("p", (n, w))
        convs.resgated_forward(ctx, a, x, e, p["weight"], self._gemm_bias, p.get("bias"), p.get("edge_weight"), pk, y)
        self._saved = (x, a, e, pk)
        return y

    def backward(self, dy, need_dx=True):
        x, a, e, pk = self._saved
        ctx, p, g, h, n, w = self.ctx, self.params, self.grads, self.channels, x.shape[0], self._width()
        dp = self._buf("dp", (n, w))
        scratch = self._buf("scratch", (max(D.resgated_bwd_scratch_floats(ctx, n, h, self.edge_dim or 0), 1),))
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.resgated_backward(ctx, a, x, e, pk, dy, p["weight"], p.get("edge_weight"), g["weight"], g["lin_bias"], g.get("bias"),
                                g.get("edge_weight"), dp, scratch, dx)
        return dx


class TransformerConv(Layer):
    """torch_geometric.nn.TransformerConv(in, channels, heads=H, concat=True, beta, dropout=0, edge_dim=D, bias, root_weight)
    (Shi et al., UniMP) -- scaled dot-product attention whose keys and values carry the edge features, the dca / proximity
    values the reference computes and its model drops (gcn_utills.py:319-443; gcn.py:71).  Per head h, with C = channels:

        t_ij = lin_edge(e_ij)        k_ij = lin_key(x_j) + t_ij        v_ij = lin_value(x_j) + t_ij
        alpha_ij = softmax_j(<lin_query(x_i), k_ij> / sqrt(C))         O_i = sum_j alpha_ij v_ij
        out_i = O_i + lin_skip(x_i)                                    (root_weight; beta=False)
        out_i = b_i lin_skip(x_i) + (1 - b_i) O_i,  b_i = sigmoid(lin_beta([O_i ‖ S_i ‖ O_i - S_i]))       (beta=True)

    ``TransformerConv(channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, use_bias=True, root_weight=True)``,
    called as ``layer([x, a])`` or, with edge_dim, ``layer([x, a, e])`` with ``a = TransformerConv.preprocess(a)`` and e
    [nnz, edge_dim] in the entry order of a: the stored pattern (row = target) and e as stored, values ignored, no loop added
    or removed (TransformerConv has no add_self_loops); a row without entries has O = 0.

    Parameters under PyG's names in its named_parameters() order: ``lin_key.weight`` / ``.bias``, ``lin_query.*``,
    ``lin_value.*``, ``lin_edge.weight`` (no bias), ``lin_skip.*``, ``lin_beta.weight`` (no bias).  ``use_bias=False`` drops all
    four biases, as PyG >= 2.5's ``bias=False`` does (older releases kept lin_skip's).  The names and layouts follow PyG's
    source, not a live module (torch_geometric was not available).  STORED are ONE stacked weight [in, 4 heads channels] =
    W_q | W_k | W_v | W_s (3 blocks without root_weight) and ONE stacked bias; ``params`` / ``grads`` hold per-name views
    ([in, heads channels] weights, lin_edge.weight [D, heads channels], lin_beta.weight [3 heads channels]).  ``state_dict()`` /
    ``gradients()`` give PyG's layouts ([out, in]; lin_beta.weight [1, 3 heads channels]), ``load_state_dict()`` takes them.
    Initialisation as torch's Linear: U(+-1 / sqrt(fan_in)) for every weight and bias.
    ``backward(dy, need_dx=True)`` returns dx (None with need_dx=False) and leaves the gradients in ``grads``.

    Launches (transformer_forward / transformer_backward of gcnx/convs.py, which the model runs too; csrc/transformer.hip):
    gcnx_gemm, gcnx_transformer_aggregate forward; gcnx_transformer_beta_bwd (beta only),
    gcnx_transformer_bwd_targets, gcnx_transformer_bwd_sources, gcnx_gemm_dw, gcnx_act_bias_grad, gcnx_gemm_dx backward.  There
    is no composed route: what the kernels do not serve (concat=False, attention dropout, bipartite inputs, beta without
    root_weight, shapes gcnx_transformer_conv_ok refuses) raises NotImplementedError."""

    BLOCKS = ("lin_query", "lin_key", "lin_value", "lin_skip")         # the stacked tensors' column blocks, in storage order

    def __init__(self, channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, use_bias=True, root_weight=True,
                 activation=None, **kw):
        super().__init__(**kw)
        if not concat:
            raise NotImplementedError("TransformerConv concat=False (the mean over heads) has no kernel: only concat=True")
        if dropout:
            raise NotImplementedError(f"TransformerConv dropout={dropout}: attention dropout has no kernel (only dropout=0)")
        if beta and not root_weight:
            raise NotImplementedError("TransformerConv beta=True gates the root connection: it needs root_weight=True")
        if activation not in (None, "linear"):
            raise NotImplementedError(f"TransformerConv activation {activation!r}: the layer is linear (follow it with BatchNorm1d / PReLU)")
        if edge_dim is not None and not 1 <= int(edge_dim) <= 8:
            raise NotImplementedError(f"TransformerConv edge_dim={edge_dim}: the kernels serve 1 to 8 edge features (or None)")
        h, c = int(heads), int(channels)
        if h not in (1, 2, 4, 8) or h * c not in (16, 32, 64, 128) or c < 4:
            raise NotImplementedError(f"TransformerConv heads={heads} channels={channels}: the kernels serve heads in {{1, 2, 4, 8}}, "
                                      "heads * channels in {16, 32, 64, 128} and channels >= 4 (there is no composed route)")
        self.channels, self.heads, self.beta, self.root_weight = c, h, bool(beta), bool(root_weight)
        self.concat, self.use_bias, self.activation = True, bool(use_bias), activation
        self.edge_dim = None if edge_dim is None else int(edge_dim)

    # Storage order: the stacked weight [in, 4 heads channels], the stacked bias, lin_edge.weight, lin_beta.weight -- every tensor on
    # a 16-byte boundary when ``offset`` is.
    STACKS = {"lin_weight": tuple(k + ".weight" for k in BLOCKS), "lin_bias": tuple(k + ".bias" for k in BLOCKS)}
    LEADING_AXIS = ("lin_beta.weight",)
    preprocess = staticmethod(_unweighted)

    def _blocks(self):
        return self.BLOCKS if self.root_weight else self.BLOCKS[:3]

    def _names(self):
        """PyG's names in its named_parameters() order."""
        lin = lambda k: [k + ".weight"] + ([k + ".bias"] if self.use_bias else [])
        return lin("lin_key") + lin("lin_query") + lin("lin_value") + (["lin_edge.weight"] if self.edge_dim else []) + \
            (lin("lin_skip") if self.root_weight else []) + (["lin_beta.weight"] if self.beta else [])

    def _param_spec(self, in_dim):
        """PyG's names in its named_parameters() order, with the stored shapes ([in, heads * channels] weights)."""
        hc, d, rng = self.heads * self.channels, self.edge_dim or 0, self._rng
        u = lambda fan_in, *s: rng.uniform(-1.0 / np.sqrt(fan_in), 1.0 / np.sqrt(fan_in), s).astype(np.float32)
        shapes = {"lin_edge.weight": ((d, hc), d), "lin_beta.weight": ((3 * hc,), 3 * hc)}
        spec = []
        for name in self._names():
            shape, fan_in = shapes.get(name, ((in_dim, hc) if name.endswith(".weight") else (hc,), in_dim))
            spec.append((name, shape, u(fan_in, *shape)))
        return spec

    def _width(self):
        return len(self._blocks()) * self.heads * self.channels

    def _fit(self, d, keys, leading=()):
        """from_pyg against the shapes of ``params``, with the layer's words for an array that does not fit."""
        shapes = {k: v.shape for k, v in self.params.items()}
        return from_pyg(d, keys, shapes, "TransformerConv", leading,
                        misfit=lambda tk, v, want: f"{tk}: shape {v.shape} does not fit this layer ({want})")

    def set_weights(self, weights):
        """Arrays in the order and the stored layouts of ``params`` (weights [in, heads channels])."""
        self._load(self._fit(dict(zip(self.params, weights)), [(k, k, False) for k in self.params]))

    def load_state_dict(self, d):
        """{PyG name: array in PyG's layout ([out, in] weights, lin_beta.weight [1, 3 heads channels])}."""
        self._load(self._fit(d, *self._pyg_keys(self.params)))

    def state_dict(self):
        """{PyG name: array in PyG's layout}: weights [heads * channels, in], lin_edge.weight [heads * channels, D],
        lin_beta.weight [1, 3 heads * channels]."""
        return self._pyg(self.params)

    def gradients(self):
        """The gradients of the last backward under the names and in the layouts of state_dict()."""
        return self._pyg(self.grads)

    def call(self, inputs, out=None):
        x, a, e = self._edge_inputs(inputs, refuse_bipartite=True)
        h, c, d = self.heads, self.channels, self.edge_dim
        hc, w = h * c, self._width()
        if not D.transformer_conv_ok(x.ctx, x.shape[0], h, c, ldp=w, edge_dim=d or 0):
            raise NotImplementedError(f"TransformerConv heads={h} channels={c} on {x.shape[0]} rows: the kernels serve heads in "
                                      "{1, 2, 4, 8}, heads * channels in {16, 32, 64, 128}, channels >= 4 and rows * heads * channels * 16 < 2^32")
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, p = self.ctx, x.shape[0], self.params
        y = out if out is not None else self._buf("y", (n, hc))
        pk, o, alpha = self._buf("p", (n, w)), self._buf("o", (n, hc)), self._buf("alpha", (a.nnz, h))
        convs.transformer_forward(ctx, a, x, e, self.lin_weight, self.lin_bias, p.get("lin_edge.weight"), p.get("lin_beta.weight"), pk,
                                  alpha, o, y, h)
        self._saved = (x, a, e, pk, alpha, o)
        return y

    def backward(self, dy, need_dx=True):
        x, a, e, pk, alpha, o = self._saved
        ctx, p, g, h, c, n = self.ctx, self.params, self.grads, self.heads, self.channels, x.shape[0]
        hc, w, ed = h * c, self._width(), self.edge_dim or 0
        dp, dscore = self._buf("dp", (n, w)), self._buf("dscore", (a.nnz, h))       # dQ | dK | dV | dS
        scratch = self._buf("scratch", (max(D.transformer_bwd_scratch_floats(ctx, n, h, c, ed, self.beta), 1),))
        d_o = self._buf("d_o", (n, hc)) if self.beta else None
        dx = self._buf("dx", x.shape) if need_dx else None
        convs.transformer_backward(ctx, a, x, e, pk, alpha, o, dy, self.lin_weight, p.get("lin_edge.weight"), p.get("lin_beta.weight"),
                                   self.lin_weight_grad, self.lin_bias_grad, g.get("lin_edge.weight"), g.get("lin_beta.weight"), dp,
                                   dscore, d_o, scratch, dx, h)
        return dx


class GeneralConv(Layer):
    """spektral.layers.GeneralConv -- the message-passing layer inside the model the reference trains (gcn.py:320
    -> GeneralGNN):

        h = activation(BatchNormalization(x W + b));   out[t] = sum_{(t, s) in a.indices} h[s]

    ``GeneralConv(channels=256, batch_norm=True, dropout=0.0, aggregate="sum", activation="prelu", use_bias=True)``,
    called as ``layer([x, a], training=bool)``.  The adjacency VALUES are ignored, no self-loop is added and nothing
    is normalised (Spektral's ``propagate`` gathers by a.indices and segment-sums).  Only what the reference uses is
    built: aggregate="sum", dropout=0.0; activation "prelu" (per-feature slopes, initial 0), "relu" or None.
    Keras BatchNormalization semantics: momentum 0.99, eps 1e-3, biased batch variance, moving statistics updated in
    training.  ``backward(dy)`` returns dx and leaves kernel / bias / gamma / beta / alpha gradients in ``grads``.
    get_weights() order: kernel, bias, alpha, gamma, beta, moving_mean, moving_variance (the layer's own variables,
    then its children's; non-trainables last -- see GeneralGNN.GNN_ORDERS; PARITY UNPINNED)."""

    def __init__(self, channels=256, batch_norm=True, dropout=0.0, aggregate="sum", activation="prelu", use_bias=True,
                 prec="f32", **kw):
        super().__init__(**kw)
        if aggregate not in ("sum", "mean", "max", "min", "prod"):
            raise ValueError(f"GeneralConv(aggregate={aggregate!r}): Spektral's aggregations are 'sum' (what gcn.py:320 uses), 'mean', 'max', 'min', 'prod'")
        self.aggregate = aggregate
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"GeneralConv(dropout={dropout!r}): a rate in [0, 1)")
        if activation not in (None, "linear", "relu", "prelu"):
            raise NotImplementedError(f"GeneralConv activation {activation!r}")
        self.channels, self.batch_norm, self.activation, self.use_bias, self.prec = int(channels), bool(batch_norm), activation, use_bias, prec
        # Dropout(rate) between BatchNormalization and the activation (8.A.4), training only: applied as its factor on the
        # activation's output (act(s u) = s act(u) for PReLU / ReLU / linear) and on the incoming gradient; the mask of call
        # number t is a stateless hash of (seed, t) -- this library's generator, not TensorFlow's
        self.dropout, self._drop_calls = float(dropout), 0
        self.state = {}

    def _param_spec(self, in_dim):
        c = self.channels
        spec = [("kernel", (in_dim, c), glorot_uniform(self._rng, in_dim, c))]
        if self.use_bias:
            spec.append(("bias", (c,), np.zeros(c, np.float32)))
        if self.activation == "prelu":
            spec.append(("alpha", (c,), np.zeros(c, np.float32)))
        if self.batch_norm:
            spec += [("gamma", (c,), np.ones(c, np.float32)), ("beta", (c,), np.zeros(c, np.float32))]
        return spec

    def build(self, ctx, in_dim, p_store=None, g_store=None, offset=0):
        off = super().build(ctx, in_dim, p_store, g_store, offset)
        if self.batch_norm:
            c = self.channels
            self.state = {"moving_mean": ctx.zeros(c), "moving_var": ctx.to_device(np.ones(c, np.float32))}
            self._mean, self._inv, self._sums, self._bn_scratch = ctx.zeros(c), ctx.zeros(c), ctx.zeros(2 * c), ctx.zeros(3 * c)
        elif self.activation == "prelu":
            # PReLU without BatchNormalization: the fused batch-norm + activation pass with the identity transform
            c = self.channels
            self._mean, self._inv, self._bn_scratch = ctx.zeros(c), ctx.to_device(np.ones(c, np.float32)), ctx.zeros(3 * c)
            self._dummy = (ctx.zeros(c), ctx.zeros(c))
        return off

    def get_weights(self):
        return [self.params[k].numpy() for k in self.params] + [self.state[k].numpy() for k in self.state]

    def set_weights(self, weights):
        for k, w in zip(list(self.params) + list(self.state), weights):
            (self.params[k] if k in self.params else self.state[k]).copy_from_host(np.asarray(w, np.float32))

    def call(self, inputs, training=False, out=None):
        x, a = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, n, c = self.ctx, x.shape[0], self.channels
        z, h = self._buf("z", (n, c)), self._buf("h", (n, c))
        ident = not self.batch_norm and self.activation == "prelu"
        D.gemm(ctx, x, self.params["kernel"], self.params.get("bias"), z, prec=self.prec,
               act=None if (self.batch_norm or ident) else self.activation)
        if ident:
            D.bn_act(ctx, z, self._mean, self._inv, self._inv, self._mean, h, act="prelu", alpha=self.params["alpha"])
        elif self.batch_norm:
            if training:
                D.bn_moments(ctx, z, self._sums, self._mean, self._inv, self.state["moving_mean"], self.state["moving_var"])
            else:
                D.bn_finalize(ctx, None, 1, self._mean, self._inv, self.state["moving_mean"], self.state["moving_var"])
            D.bn_act(ctx, z, self._mean, self._inv, self.params["gamma"], self.params["beta"], h, act=self.activation,
                     alpha=self.params.get("alpha"))
        else:
            h = z
        drop_id = None
        if training and self.dropout > 0.0:
            drop_id = self._drop_calls = self._drop_calls + 1
            D.dropout(ctx, h, self.dropout, self._seed, drop_id)
        y = out if out is not None else self._buf("y", (n, c))
        au = a.row_mean() if self.aggregate == "mean" else a.unweighted()  # values ignored (8.A.4); "mean": 1 / row length
        cnt = None
        if self.aggregate in ("max", "min", "prod"):        # unsorted_segment_max / _min / _prod; + what their gradients need
            cnt = self._buf("aggcnt", (n, c))
            D.spmm_minmax(ctx, au, h, y, cnt, self.aggregate)
        else:
            D.spmm(ctx, au, h, None, y)
        self._saved = (x, au, z, h, bool(training), drop_id, y, cnt)
        return y

    def backward(self, dy, need_dx=True):
        x, au, z, h, training, drop_id, y, cnt = self._saved
        ctx = self.ctx
        dh = self._buf("dh", dy.shape)
        if cnt is not None:
            D.spmm_minmax_bwd(ctx, au.transpose(), h, y, cnt, dy, dh, self.aggregate)
        else:
            D.spmm(ctx, au.transpose(), dy, None, dh)        # dH = S^T dY
        if drop_id is not None:
            D.dropout(ctx, dh, self.dropout, self._seed, drop_id)
        if not self.batch_norm and self.activation == "prelu":
            D.bn_act_bwd(ctx, dh, z, self._mean, self._inv, self._inv, self._mean, dh, self._bn_scratch, act="prelu",
                         alpha=self.params["alpha"], training=False, dgamma=self._dummy[0], dbeta=self._dummy[1],
                         dalpha=self.grads["alpha"])
            D.act_bias_grad(ctx, dh, None, dh, None, db=self.grads.get("bias"))
        elif self.batch_norm:
            D.bn_act_bwd(ctx, dh, z, self._mean, self._inv, self.params["gamma"], self.params["beta"], dh, self._bn_scratch,
                         act=self.activation, alpha=self.params.get("alpha"), training=training,
                         dgamma=self.grads["gamma"], dbeta=self.grads["beta"], dalpha=self.grads.get("alpha"))
            D.act_bias_grad(ctx, dh, None, dh, None, db=self.grads.get("bias"))
        else:
            D.act_bias_grad(ctx, dh, h, dh, self.activation, db=self.grads.get("bias"), alpha=self.params.get("alpha"),
                            dalpha=self.grads.get("alpha"))
        D.gemm_dw(ctx, x, dh, self.grads["kernel"], prec=self.prec)
        if not need_dx:
            return None
        dx = self._buf("dx", x.shape)
        D.gemm_dx(ctx, dh, self.params["kernel"], dx, prec=self.prec)
        return dx


class Dense(Layer):
    """Keras Dense: act(x W + b); activation None / 'relu' (softmax is fused with the loss)."""

    def __init__(self, units, activation=None, use_bias=True, prec="f32", **kw):
        super().__init__(**kw)
        if activation not in (None, "linear", "relu"):
            raise NotImplementedError(f"Dense activation {activation!r}")
        self.units, self.activation, self.use_bias, self.prec = int(units), activation, use_bias, prec

    def _param_spec(self, in_dim):
        spec = [("kernel", (in_dim, self.units), glorot_uniform(self._rng, in_dim, self.units))]
        if self.use_bias:
            spec.append(("bias", (self.units,), np.zeros(self.units, np.float32)))
        return spec

    def call(self, x, out=None):
        if not self.built:
            self.build(x.ctx, x.shape[1])
        y = out if out is not None else self._buf("y", (x.shape[0], self.units))
        D.gemm(self.ctx, x, self.params["kernel"], self.params.get("bias"), y, act=self.activation, prec=self.prec)
        self._saved = (x, y)
        return y

    def backward(self, dy, need_dx=True):
        x, y = self._saved
        dz = self._buf("dz", dy.shape)
        D.act_bias_grad(self.ctx, dy, y, dz, self.activation, db=self.grads.get("bias"))
        D.gemm_dw(self.ctx, x, dz, self.grads["kernel"], prec=self.prec)
        if not need_dx:
            return None
        dx = self._buf("dx", (x.shape[0], self.in_dim))
        D.gemm_dx(self.ctx, dz, self.params["kernel"], dx, prec=self.prec)
        return dx


class _GlobalPool(Layer):
    mode = "sum"

    def call(self, inputs, out=None):
        x, seg = inputs
        if not isinstance(seg, D.Segments):
            seg = D.Segments.from_ids(x.ctx, seg)
        self.ctx = x.ctx
        pooled = out if out is not None else self._buf("p", (seg.n_graphs, x.shape[1]))
        arg = self._buf("arg", (seg.n_graphs, x.shape[1]), np.int32) if self.mode == "max" else None
        D.segment_pool(self.ctx, seg, x, pooled, self.mode, arg)
        self._saved = (x.shape, seg, arg)
        return pooled

    def backward(self, dp, y_mask=None, db=None, out=None):
        shape, seg, arg = self._saved
        dx = out if out is not None else self._buf("dx", shape)
        D.segment_pool_bwd(self.ctx, seg, dp, dx, self.mode, arg, y=y_mask, db=db)
        return dx


class GlobalSumPool(_GlobalPool):
    """P[g] = sum_{n: i[n]=g} X[n]  (tf.math.segment_sum; GeneralGNN pool='sum', gcn.py:320)."""
    mode = "sum"


class GlobalAvgPool(_GlobalPool):
    mode = "avg"


class GlobalMaxPool(_GlobalPool):
    """global_max_pool of the reference's torch topology (gcn_utills.py:842)."""
    mode = "max"


class GlobalAttnSumPool(Layer):
    """spektral.layers.pooling.GlobalAttnSumPool in disjoint mode, the learned readout of the module the reference imports its
    pools from (gcn.py:10); PyG's AttentionalAggregation(gate_nn=Linear(F, 1, bias=False)):

        s_i = <x_i, attn_kernel>        alpha = softmax of s over the rows of each graph        P[g] = sum_i alpha_i x_i

    One parameter, ``attn_kernel`` [F, 1], glorot-uniform (``attn_kernel_initializer="glorot_uniform"``, the Spektral default).
    ``layer((x, seg))`` with graph ids or a Segments returns pooled [B, F]; an empty graph pools to a zero row.
    ``backward(dp)`` returns dx [N, F] and leaves d attn_kernel in ``grads``.  Launches: gcnx_attn_pool, gcnx_attn_pool_bwd
    (csrc/attn_pool.hip): one pass over x forward, one backward, each with a small second launch where it sums parts."""

    def __init__(self, attn_kernel_initializer="glorot_uniform", **kw):
        super().__init__(**kw)
        if attn_kernel_initializer != "glorot_uniform":
            raise NotImplementedError("only the glorot_uniform initialiser (the Spektral default)")

    def _param_spec(self, in_dim):
        return [("attn_kernel", (in_dim, 1), glorot_uniform(self._rng, in_dim, 1))]

    def call(self, inputs, out=None):
        x, seg = inputs
        if not isinstance(seg, D.Segments):
            seg = D.Segments.from_ids(x.ctx, seg)
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n, f = x.shape
        pooled = out if out is not None else self._buf("p", (seg.n_graphs, f))
        alpha = self._buf("alpha", (max(n, 1),))
        scratch = self._buf("scratch", (max(D.attn_pool_scratch_floats(self.ctx, n, seg.n_graphs, f), 4),))
        D.attn_pool(self.ctx, seg, x, self.params["attn_kernel"], pooled, alpha.flat(0, n), scratch)
        self._saved = (x, seg, pooled, alpha.flat(0, n), scratch)
        return pooled

    def backward(self, dp, need_dx=True, out=None):
        x, seg, pooled, alpha, scratch = self._saved
        dx = (out if out is not None else self._buf("dx", x.shape)) if need_dx else None
        D.attn_pool_bwd(self.ctx, seg, x, self.params["attn_kernel"], alpha, pooled, dp, dx, self.grads["attn_kernel"], scratch)
        return dx


class TopKPool(Layer):
    """spektral.layers.pooling.TopKPool in disjoint mode, the one Spektral layer the reference's script imports (gcn.py:10)
    besides the ones above: hierarchical pooling that keeps the ceil(ratio * n_g) highest-scoring nodes of every graph.

        y = X p / ||p||        idx = the k_g rows of graph g with the largest y        X' = (X * gate(y))[idx]
        A' = A[idx][:, idx]    values copied, NOT renormalised (as Spektral)           graph_ptr' = prefix sums of k_g

    ``TopKPool(ratio, return_selection=False, return_score=False, sigmoid_gating=False, kernel_initializer="glorot_uniform")``,
    called as ``layer([x, a, seg])`` with a DeviceCSR and a Segments; returns ``(x', a', seg')`` (+ ``idx`` int32[N'] and / or
    ``y`` [N] if asked, in that order).  One parameter, ``kernel`` [F, 1]; gate = tanh, or sigmoid with ``sigmoid_gating``.
    ``backward(dx')`` returns dx [N, F] (zero rows for dropped nodes) and leaves d kernel in ``grads``; nothing flows through
    the selection or through the values of A'.

    Two decisions that differ from, or go beyond, Spektral:
      1. Kept rows stay in their ORIGINAL relative order (Spektral and PyG order them by descending score).  Every layer that
         can follow (GCNConv, SAGEConv, the global pools) is permutation-equivariant or -invariant, so model outputs and all
         gradients are the same; the map old -> new is monotone, so A' keeps sorted columns and its diagonal blocks, and a
         symmetric A gives a symmetric A' (the flag is passed on, nothing is inspected per step).
      2. Scores compare as IEEE numbers (-0.0 equals +0.0); among equal scores the LOWER row index wins.  NaN scores are
         outside the contract: all that is promised then is k_g distinct rows of every graph.

    k_g is computed on the host in float64 from ``seg.host``, so N' and graph_ptr' are known up front; the one
    synchronisation of the layer is the 4-byte read-back of nnz' = rowptr'[N'].  colidx' / vals' live in buffers sized for the
    parent's nnz (no allocation per step) and ``a'.nnz`` is set from the read-back.  x', a', seg' and idx are views of the
    layer's buffers: valid until its next call.  Launches: gcnx_topk_select, gcnx_csr_induce (3), gcnx_topk_gather;
    backward gcnx_topk_bwd (2) -- csrc/topk.hip.  A graph of more than 16384 rows raises NotImplementedError."""

    def __init__(self, ratio, return_selection=False, return_score=False, sigmoid_gating=False,
                 kernel_initializer="glorot_uniform", **kw):
        super().__init__(**kw)
        if not (isinstance(ratio, (int, float, np.integer, np.floating)) and 0.0 < float(ratio) <= 1.0):
            raise ValueError(f"TopKPool(ratio={ratio!r}): a number in (0, 1]")
        if kernel_initializer != "glorot_uniform":
            raise NotImplementedError("only the glorot_uniform initialiser (the Spektral default)")
        self.ratio, self.return_selection, self.return_score = float(ratio), bool(return_selection), bool(return_score)
        self.sigmoid_gating = bool(sigmoid_gating)
        self._store, self._kept = {}, None

    def _param_spec(self, in_dim):
        return [("kernel", (in_dim, 1), glorot_uniform(self._rng, in_dim, 1))]

    def _cap(self, key, shape, dtype=np.float32):
        """Grow-only storage behind a view of ``shape`` (a streamed epoch brings a new N with every batch)."""
        shape = tuple(int(s) for s in shape)
        need = int(np.prod(shape))
        cur = self._store.get(key)
        if cur is None or cur.size < need:
            cur = self.ctx.empty(max(need, int(1.25 * cur.size) if cur is not None else 0, 4), dtype)
            self._store[key] = cur
        return D.DeviceArray._view(cur, 0, shape)

    def _segments(self, seg):
        """(graph_ptr' on the host, Segments'), kept while the same Segments object comes back."""
        if self._kept is None or self._kept[0] is not seg:
            kp = D.topk_kept_ptr(seg.host, self.ratio)
            self._kept = (seg, kp, D.Segments.from_device(self.ctx, self.ctx.to_device(kp, np.int32), kp))
        return self._kept[1], self._kept[2]

    def call(self, inputs, out=None):
        x, a, seg = inputs
        if not self.built:
            self.build(x.ctx, x.shape[1])
        ctx, (n, f) = self.ctx, x.shape
        if a.n != n or seg.n != n:
            raise ValueError(f"TopKPool: x has {n} rows, a {a.n}, the segments {seg.n}")
        kp, seg2 = self._segments(seg)
        nk = int(kp[-1])
        y, pos, idx = self._cap("y", (n,)), self._cap("pos", (n,), np.int32), self._cap("idx", (nk,), np.int32)
        D.topk_select(ctx, seg, seg2.dev, nk, x, self.params["kernel"], y, idx, pos)
        rp = self._cap("rowptr", (nk + 1,), np.int32)
        ci = self._cap("colidx", (max(a.nnz, 1),), np.int32)
        v = self._cap("vals", (max(a.nnz, 1),)) if a.vals is not None else None
        D.csr_induce(ctx, a, idx, pos, nk, rp, ci, v)
        x2 = out if out is not None else self._cap("x2", (nk, f))
        D.topk_gather(ctx, x, y, idx, nk, x2, self.sigmoid_gating)
        nnz2 = D.read_int32(ctx, rp, nk)                       # the layer's one synchronisation
        a2 = D.DeviceCSR(ctx, nk, nnz2, rp, ci, v, seg2.dev, seg2.n_graphs, a.symmetric, D._max_block(kp))
        # The buffers behind a' are reused from step to step, and a transposed CSR built for last step's a' may have been freed
        # and its address handed out again: a plan kept on graph_ptr' forgets every row order it holds and learns the new rows.
        plan = getattr(seg2.dev, "_spmm_plan", None)
        if plan is not None:
            plan.bound.clear()
        a2.rebind()
        self._saved = (x, y, pos, nk, idx)
        res = (x2, a2, seg2)
        if self.return_selection:
            res += (idx,)
        if self.return_score:
            res += (y,)
        return res

    def backward(self, dy, need_dx=True):
        x, y, pos, nk, _ = self._saved
        assert dy.shape == (nk, x.shape[1])
        dx = self._cap("dx", x.shape)
        D.topk_bwd(self.ctx, x, y, pos, self.params["kernel"], dy, dx, self.grads["kernel"], self.sigmoid_gating)
        return dx if need_dx else None


class BatchNorm1d(Layer):
    """torch.nn.BatchNorm1d(F, track_running_stats=False, momentum=None) -- the reference's torch GCN
    (gcn_utills.py:816-826): batch mean and biased variance, eps 1e-5, in training AND evaluation (no running
    statistics); weight (gamma) 1, bias (beta) 0.  One row raises ValueError, as torch does.  ``backward(dy)`` is the
    training-mode backward; the parameter gradients land in ``grads["weight"]`` / ``grads["bias"]``."""

    def __init__(self, eps=D.TORCH_BN_EPS, **kw):
        super().__init__(**kw)
        self.eps = float(eps)

    def _param_spec(self, in_dim):
        return [("weight", (in_dim,), np.ones(in_dim, np.float32)), ("bias", (in_dim,), np.zeros(in_dim, np.float32))]

    def call(self, x, training=False, out=None):
        n, f = x.shape
        if n < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{n}, {f}]")
        if not self.built:
            self.build(x.ctx, f)
        mean, inv = self._buf("mean", (f,)), self._buf("inv", (f,))
        D.bn_moments(self.ctx, x, None, mean, inv, eps=self.eps)
        y = out if out is not None else self._buf("y", (n, f))
        D.bn_act(self.ctx, x, mean, inv, self.params["weight"], self.params["bias"], y)
        self._saved = (x, mean, inv)
        return y

    def backward(self, dy, need_dx=True):
        x, mean, inv = self._saved
        dx = self._buf("dx", x.shape)
        D.bn_act_bwd(self.ctx, dy, x, mean, inv, self.params["weight"], self.params["bias"], dx, self._buf("sums", (3 * x.shape[1],)),
                     dgamma=self.grads["weight"], dbeta=self.grads["bias"])
        return dx


class GraphNorm(Layer):
    """torch_geometric.nn.GraphNorm(F, eps=1e-5) (Cai et al. 2021) in disjoint mode: per graph and per channel

        mu = mean_i x_i        o_i = x_i - mean_scale * mu        y_i = weight * o_i / sqrt(mean_i o_i^2 + eps) + bias

    Parameters ``weight`` (1), ``bias`` (0), ``mean_scale`` (1), each [F], in PyG's registration order.  Training and
    evaluation are the same.  ``layer((x, seg))`` with graph ids or a Segments returns y [N, F]; one row is legal (a one-row
    graph gives y = bias at mean_scale = 1), an empty graph contributes nothing.  ``backward(dy)`` returns dx [N, F] and leaves
    the three gradients in ``grads``.  Launches: gcnx_graph_norm_act, gcnx_graph_norm_act_bwd (csrc/graph_norm.hip)."""

    def __init__(self, eps=D.TORCH_BN_EPS, **kw):
        super().__init__(**kw)
        self.eps = float(eps)

    def _param_spec(self, in_dim):
        one = np.ones(in_dim, np.float32)
        return [("weight", (in_dim,), one), ("bias", (in_dim,), np.zeros(in_dim, np.float32)), ("mean_scale", (in_dim,), one)]

    def call(self, inputs, out=None):
        x, seg = inputs
        if not isinstance(seg, D.Segments):
            seg = D.Segments.from_ids(x.ctx, seg)
        if not self.built:
            self.build(x.ctx, x.shape[1])
        n, f = x.shape
        b, p = seg.n_graphs, self.params
        mean, inv = self._buf("mean", (b, f)), self._buf("inv", (b, f))
        scratch = self._buf("scratch", (max(D.graph_norm_scratch_floats(self.ctx, n, b, f), 4),))
        y = out if out is not None else self._buf("y", (n, f))
        D.graph_norm_act(self.ctx, seg, x, p["mean_scale"], p["weight"], p["bias"], y, mean, inv, scratch=scratch, eps=self.eps)
        self._saved = (x, seg, mean, inv, scratch)
        return y

    def backward(self, dy, need_dx=True):
        x, seg, mean, inv, scratch = self._saved
        p, g = self.params, self.grads
        dx = self._buf("dx", x.shape)
        D.graph_norm_act_bwd(self.ctx, seg, dy, x, mean, inv, p["mean_scale"], p["weight"], p["bias"], dx, dgamma=g["weight"],
                             dbeta=g["bias"], dmean_scale=g["mean_scale"], scratch=scratch)
        return dx


class PReLU(Layer):
    """torch.nn.PReLU(): y = max(0, x) + a * min(0, x) with ONE slope a for every feature (init 0.25);
    ``grads["weight"]`` = sum over all elements of dY * min(x, 0).  Runs on gcnx_bn_act(_bwd) with an identity
    normalisation (mean 0, inv 1, gamma 1, beta 0: fma(x - 0, 1, 0) == x exactly) and GCNX_ACT_PRELU_SHARED."""

    def __init__(self, init=0.25, **kw):
        super().__init__(**kw)
        self.init = float(init)

    def _param_spec(self, in_dim):
        return [("weight", (1,), np.full(1, self.init, np.float32))]

    def _identity(self, f):
        key = ("id", f)
        if key not in self._scratch:
            self._scratch[key] = (self.ctx.zeros(f), self.ctx.to_device(np.ones(f, np.float32)))
        return self._scratch[key]

    def call(self, x, out=None):
        if not self.built:
            self.build(x.ctx, x.shape[1])
        zero, one = self._identity(x.shape[1])
        y = out if out is not None else self._buf("y", x.shape)
        D.bn_act(self.ctx, x, zero, one, one, zero, y, act="prelu_shared", alpha=self.params["weight"])
        self._saved = x
        return y

    def backward(self, dy, need_dx=True):
        x = self._saved
        zero, one = self._identity(x.shape[1])
        dx = self._buf("dx", x.shape)
        D.bn_act_bwd(self.ctx, dy, x, zero, one, one, zero, dx, self._buf("sums", (3 * x.shape[1],)), act="prelu_shared",
                     alpha=self.params["weight"], training=False, dalpha=self.grads["weight"])
        return dx


# ---- ECCConv: Keras shapes <-> the stacked weight of the factorised form (host arrays only) ------------------------------------
def ecc_weight_names(kernel_network=None, root=True, use_bias=True):
    """The Keras variable names of an ECCConv in the order get_weights() lists them: the kernel network's hidden Dense layers
    "FGN_<m>_kernel" / "FGN_<m>_bias", its output Dense "FGN_out_kernel" / "FGN_out_bias", then "root_kernel" and "bias"."""
    names = []
    for m in range(len(kernel_network or ())):
        names += [f"FGN_{m}_kernel", f"FGN_{m}_bias"]
    names += ["FGN_out_kernel", "FGN_out_bias"]
    if root:
        names.append("root_kernel")
    if use_bias:
        names.append("bias")
    return names


def ecc_pack_weights(weights, f_in, channels, root=True):
    """{Keras name: array} -> the arrays libgcnx holds: "wstack" [(S' + 1 (+ 1 with root)) * F, F_out] =
    [W_0; ..; W_{S'-1}; B; W_root] with W_c = reshape(FGN_out_kernel[c], (F, F_out)), B = reshape(FGN_out_bias, (F, F_out));
    every other entry ("bias", "FGN_<m>_kernel", "FGN_<m>_bias") unchanged."""
    w = {k: np.asarray(v, np.float32) for k, v in weights.items()}
    wk, bk = w.pop("FGN_out_kernel"), w.pop("FGN_out_bias")
    f, fo = int(f_in), int(channels)
    if wk.ndim != 2 or wk.shape[1] != f * fo or bk.shape != (f * fo,):
        raise ValueError(f"FGN_out kernel {wk.shape} / bias {bk.shape}: expected [S', {f * fo}] and [{f * fo}]")
    parts = [wk.reshape(wk.shape[0] * f, fo), bk.reshape(f, fo)]
    rk = w.pop("root_kernel", None)
    if root:
        if rk is None or rk.shape != (f, fo):
            raise ValueError(f"root_kernel: expected [{f}, {fo}]")
        parts.append(rk)
    elif rk is not None:
        raise ValueError("root_kernel given for a layer built with root=False")
    w["wstack"] = np.ascontiguousarray(np.concatenate(parts, 0))
    return w


def ecc_unpack_weights(params, f_in, channels, root=True):
    """Inverse of ecc_pack_weights: the arrays libgcnx holds -> {Keras name: array in its Keras shape}."""
    w = {k: np.asarray(v) for k, v in params.items()}
    ws = w.pop("wstack")
    f, fo = int(f_in), int(channels)
    sp = ws.shape[0] // f - 1 - (1 if root else 0)
    if ws.shape != ((sp + 1 + (1 if root else 0)) * f, fo) or sp < 0:
        raise ValueError(f"wstack {ws.shape} does not fit F = {f}, F_out = {fo}, root = {root}")
    w["FGN_out_kernel"] = ws[:sp * f].reshape(sp, f * fo).copy()
    w["FGN_out_bias"] = ws[sp * f:(sp + 1) * f].reshape(f * fo).copy()
    if root:
        w["root_kernel"] = ws[(sp + 1) * f:].copy()
    return w


class ECCConv(Layer):
    """spektral.layers.ECCConv (edge-conditioned convolution) in single / disjoint mode, called as ``layer([x, a, e])``:

        u_0 = e,  u_m = relu(u_{m-1} V_m + v_m)  per hidden width of kernel_network;  K_k = reshape(u_M[k] Wk + bk, (F, F_out))
        out[c_k] += x[r_k] K_k  over the stored entries k = (r_k, c_k) of a;   out = activation(out + x W_root + bias)

    ``a``: DeviceCSR of the batch (values ignored); ``e``: DeviceArray [nnz, S], row k belonging to stored entry k (row-major).
    Evaluated in the factorised form of DESIGN.md ("ECCConv"): gcnx_ecc_expand writes [Scat | x], one gcnx_gemm with the
    stacked weight gives the output; the per-entry kernels are never formed.  ``backward(dy, need_dx=True)`` returns dx and
    leaves the gradients in ``grads`` ("wstack" holds those of FGN_out's kernel, its bias and root_kernel in the stacked
    layout; ``gradients()`` converts to the Keras shapes).  Activation None / "relu"; Keras default initialisers (glorot
    uniform on every kernel in its Keras shape, zero biases).  S' + 1 <= 17 (S' = the last hidden width, or S).

    ``get_weights(as_dict=True)`` / ``set_weights(dict)``: keyed by the Keras names (ecc_weight_names) -- the primary form.
    The list form follows ecc_weight_names' order; Keras' own order was not confirmed against a live layer (PARITY UNPINNED)."""

    MAX_C = 17

    def __init__(self, channels, kernel_network=None, root=True, activation=None, use_bias=True, **kw):
        super().__init__(**kw)
        if activation not in (None, "linear", "relu"):
            raise NotImplementedError(f"ECCConv activation {activation!r}: only None / 'relu'")
        if int(channels) < 1:
            raise ValueError(f"ECCConv(channels={channels!r}): a positive width")
        kn = list(kernel_network) if kernel_network is not None else []
        if any((not isinstance(w, (int, np.integer))) or int(w) < 1 for w in kn):
            raise ValueError(f"ECCConv(kernel_network={kernel_network!r}): a list of positive hidden widths (or None)")
        if kn and int(kn[-1]) + 1 > self.MAX_C:
            raise NotImplementedError(f"ECCConv: last kernel_network width {kn[-1]} + 1 exceeds C = {self.MAX_C}")
        self.channels, self.kernel_network, self.root = int(channels), [int(w) for w in kn], bool(root)
        self.activation = None if activation == "linear" else activation
        self.use_bias = bool(use_bias)
        self.edge_dim = None

    @property
    def sp(self):
        """S': channels per entry that reach the aggregation."""
        return self.kernel_network[-1] if self.kernel_network else self.edge_dim

    def _param_spec(self, in_dim):
        if self.edge_dim is None:
            raise ValueError("ECCConv: the edge feature width is not known yet (set edge_dim, or call the layer)")
        if self.sp + 1 > self.MAX_C:
            raise NotImplementedError(f"ECCConv: {self.sp} edge channels + 1 exceed C = {self.MAX_C}; reduce them with a kernel_network")
        f, fo, spec, w_in = int(in_dim), self.channels, [], self.edge_dim
        for m, w in enumerate(self.kernel_network):
            spec += [(f"FGN_{m}_kernel", (w_in, w), glorot_uniform(self._rng, w_in, w)), (f"FGN_{m}_bias", (w,), np.zeros(w, np.float32))]
            w_in = w
        keras = {"FGN_out_kernel": glorot_uniform(self._rng, w_in, f * fo), "FGN_out_bias": np.zeros(f * fo, np.float32)}
        if self.root:
            keras["root_kernel"] = glorot_uniform(self._rng, f, fo)
        ws = ecc_pack_weights(keras, f, fo, self.root)["wstack"]
        spec.append(("wstack", ws.shape, ws))
        if self.use_bias:
            spec.append(("bias", (fo,), np.zeros(fo, np.float32)))
        return spec

    # every parameter on a 16-byte boundary (the padding floats have zero gradients, so a single SGD launch over a model's flat
    # buffer leaves them at zero)
    ALIGN = OWN_ALIGN = 4

    # ---- weights in the Keras shapes ----------------------------------------------------------------------------------
    def get_weights(self, as_dict=False):
        d = ecc_unpack_weights({k: v.numpy() for k, v in self.params.items()}, self.in_dim, self.channels, self.root)
        return d if as_dict else [d[k] for k in ecc_weight_names(self.kernel_network, self.root, self.use_bias)]

    def set_weights(self, weights):
        names = ecc_weight_names(self.kernel_network, self.root, self.use_bias)
        if not isinstance(weights, dict):
            weights = dict(zip(names, weights))
        missing = [k for k in names if k not in weights]
        if missing:
            raise KeyError(f"ECCConv.set_weights: missing {missing}")
        packed = ecc_pack_weights({k: weights[k] for k in names}, self.in_dim, self.channels, self.root)
        for k, v in packed.items():
            if v.shape != self.params[k].shape:
                raise ValueError(f"ECCConv.set_weights: {k} has shape {v.shape}, the layer holds {self.params[k].shape}")
            self.params[k].copy_from_host(v)

    def gradients(self):
        """{Keras name: gradient of the last backward()} in the Keras shapes."""
        return ecc_unpack_weights({k: v.numpy() for k, v in self.grads.items()}, self.in_dim, self.channels, self.root)

    # ---- forward / backward -------------------------------------------------------------------------------------------
    def _buf(self, key, shape, dtype=np.float32):
        """Grow-only scratch: a view of exactly ``shape`` on storage that is replaced only when it is too small.  A streamed
        epoch brings a new (N, nnz) with every batch, and Layer._buf would allocate [Scat | x] (15 MB at the config-2 batch
        shape) and the rest again on every step."""
        shape = tuple(int(d) for d in shape)
        need = int(np.prod(shape, dtype=np.int64))
        cur = self._scratch.get(key)
        if cur is None or cur.size < need or cur.dtype != np.dtype(dtype):
            cur = self.ctx.empty(max(need, int(1.25 * cur.size) if cur is not None else 0, 1), dtype)
            self._scratch[key] = cur
        return D.DeviceArray._view(cur, 0, shape)

    def call(self, inputs, out=None):
        x, a, e = inputs
        if e is None:
            raise ValueError("ECCConv needs edge features: layer([x, a, e])")
        if not self.built:
            self.edge_dim = int(e.shape[1])
            self.build(x.ctx, x.shape[1])
        ctx, n, f = self.ctx, x.shape[0], x.shape[1]
        if e.shape != (a.nnz, self.edge_dim):
            raise ValueError(f"ECCConv: e has shape {e.shape}, expected ({a.nnz}, {self.edge_dim}): one row per stored entry of a")
        us = [e]
        for m, w in enumerate(self.kernel_network):
            u = self._buf(f"u{m}", (a.nnz, w))
            D.gemm(ctx, us[-1], self.params[f"FGN_{m}_kernel"], self.params[f"FGN_{m}_bias"], u, act="relu")
            us.append(u)
        cols = (self.sp + 1 + (1 if self.root else 0)) * f
        sx = self._buf("sx", (n, cols))
        D.ecc_expand(ctx, a, us[-1], x, sx, root=self.root)
        y = out if out is not None else self._buf("y", (n, self.channels))
        D.gemm(ctx, sx, self.params["wstack"], self.params.get("bias"), y, act=self.activation)
        self._saved = (x, a, us, sx, y)
        return y

    def backward(self, dy, need_dx=True):
        x, a, us, sx, y = self._saved
        ctx, n, f, fo, sp = self.ctx, x.shape[0], x.shape[1], self.channels, self.sp
        dz = dy
        if self.activation is not None:
            dz = self._buf("dz", (n, fo))
            D.act_bias_grad(ctx, dy, y, dz, self.activation, db=self.grads.get("bias"))
        elif self.use_bias:
            D.act_bias_grad(ctx, dy, None, dy, None, db=self.grads["bias"])         # a pure column sum
        D.gemm_dw(ctx, sx, dz, self.grads["wstack"])
        need_du = bool(self.kernel_network)
        if not need_dx and not need_du:
            return None
        cf = (sp + 1) * f
        take_root = self.root and need_dx
        rows = cf + (f if take_root else 0)
        g = self._buf("g", (n, rows))                                               # [dScat | dx_root] = dZ Wstack^T
        D.gemm_dx(ctx, dz, self.params["wstack"].flat(0, rows * fo, (rows, fo)), g)
        dx = self._buf("dx", (n, f)) if need_dx else None
        du = self._buf("du", (a.nnz, sp)) if need_du else None
        D.ecc_bwd(ctx, a, us[-1], x, g.cols(0, cf), g.cols(cf, cf + f) if take_root else None, dx, du)
        for m in reversed(range(len(self.kernel_network))):
            dzu = self._buf(f"dzu{m}", us[m + 1].shape)
            D.act_bias_grad(ctx, du, us[m + 1], dzu, "relu", db=self.grads[f"FGN_{m}_bias"])
            D.gemm_dw(ctx, us[m], dzu, self.grads[f"FGN_{m}_kernel"])
            if m > 0:
                du = self._buf(f"du{m - 1}", us[m].shape)
                D.gemm_dx(ctx, dzu, self.params[f"FGN_{m}_kernel"], du)
        return dx

"""float64 NumPy restatement of Spektral's ECCConv (single / disjoint mode) and of gcnx.ECCNet: forward, loss, accuracy,
every gradient and an SGD step (the spec of record is DESIGN.md, "ECCConv").  No torch, no Spektral.

Two forms of the layer, which must agree to rounding:
  * ``materialised``: what Spektral runs -- gather x by indices[:, 0], one [F, F_out] kernel per stored entry out of the
    kernel network, einsum("ab,abc->ac"), index-add by indices[:, 1];
  * ``factorised``:   what libgcnx runs -- Scat = the edge-channel-weighted aggregation, one GEMM with
    Wstack = [W_0; ..; W_{S'-1}; B; W_root], and the matching backward.

Parameters are a dict in the Keras shapes: "FGN_<m>_kernel" / "FGN_<m>_bias" for the hidden layers of kernel_network,
"FGN_out_kernel" [S', F * F_out] / "FGN_out_bias" [F * F_out], "root_kernel" [F, F_out], "bias" [F_out].

Kink sides: every ReLU (the layer's activation and the kernel network's) can be evaluated on the DEVICE's side through
``masks`` = {"act": bool [N, F_out], "kn": [bool [nnz, width_m], ...]} (True = the pre-activation counts as positive), as
tests/gcn_bn_ref.py does; ``kink_report`` then tells where the device's sides differ from the oracle's own.
"""
import numpy as np


def param_names(hidden, root=True, use_bias=True):
    names = []
    for m in range(len(hidden or ())):
        names += [f"FGN_{m}_kernel", f"FGN_{m}_bias"]
    names += ["FGN_out_kernel", "FGN_out_bias"]
    if root:
        names.append("root_kernel")
    if use_bias:
        names.append("bias")
    return names


def init_params(f_in, channels, s, hidden=None, root=True, use_bias=True, seed=0):
    """Random parameters of every kind, biases included (not the Keras initialisation: every gradient term is exercised)."""
    rng = np.random.default_rng(seed)
    p, w_in = {}, s
    for m, w in enumerate(hidden or ()):
        p[f"FGN_{m}_kernel"] = rng.uniform(-1, 1, (w_in, w)) * np.sqrt(3.0 / w_in)
        p[f"FGN_{m}_bias"] = rng.uniform(-0.3, 0.3, w)
        w_in = w
    lim = np.sqrt(3.0 / (w_in * f_in))
    p["FGN_out_kernel"] = rng.uniform(-lim, lim, (w_in, f_in * channels))
    p["FGN_out_bias"] = rng.uniform(-lim, lim, f_in * channels)
    if root:
        p["root_kernel"] = rng.uniform(-1, 1, (f_in, channels)) * np.sqrt(3.0 / f_in)
    if use_bias:
        p["bias"] = rng.uniform(-0.2, 0.2, channels)
    return p


def _relu(z, pos=None):
    pos = z > 0 if pos is None else np.asarray(pos, bool)
    return np.where(pos, z, 0.0), pos


def kernel_network(e, p, hidden, masks=None):
    """u_0 = e, u_m = relu(u_{m-1} V_m + v_m).  Returns ([u_0 .. u_M], [pre-activations], [sides])."""
    us, pres, sides = [np.asarray(e, np.float64)], [], []
    for m in range(len(hidden or ())):
        z = us[-1] @ p[f"FGN_{m}_kernel"] + p[f"FGN_{m}_bias"]
        u, pos = _relu(z, masks[m] if masks is not None else None)
        us.append(u); pres.append(z); sides.append(pos)
    return us, pres, sides


def _kn_backward(du, us, sides, p, hidden, g):
    for m in reversed(range(len(hidden or ()))):
        dz = np.where(sides[m], du, 0.0)
        g[f"FGN_{m}_kernel"] = us[m].T @ dz
        g[f"FGN_{m}_bias"] = dz.sum(0)
        du = dz @ p[f"FGN_{m}_kernel"].T
    return du          # gradient wrt e


def layer(x, indices, e, p, hidden=None, activation=None, root=True, use_bias=True, dy=None, form="factorised",
          masks=None, flip=False):
    """One ECCConv.  indices [nnz, 2] (row, column) of the stored entries, e [nnz, S] in the same order.  Messages go from
    indices[:, 0] to indices[:, 1] (flip=True: the other reading, GeneralConv's).  Returns a dict: out, pre (the
    pre-activation), act_side, kn_pre, kn_sides and, with dy, dx, de and grads {Keras name: array}."""
    masks = masks or {}
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    indices = np.asarray(indices, np.int64).reshape(-1, 2)
    src, dst = (indices[:, 1], indices[:, 0]) if flip else (indices[:, 0], indices[:, 1])
    n, f = x.shape
    wk, bk = p["FGN_out_kernel"], p["FGN_out_bias"]
    fo = wk.shape[1] // f
    us, kn_pre, kn_sides = kernel_network(e, p, hidden, masks.get("kn"))
    um = us[-1]
    sp = um.shape[1]
    if form == "materialised":
        kern = (um @ wk + bk).reshape(-1, f, fo)
        msg = np.einsum("ab,abc->ac", x[src], kern)
        pre = np.zeros((n, fo))
        np.add.at(pre, dst, msg)
    else:
        uh = np.concatenate([um, np.ones((um.shape[0], 1))], 1)                 # u^ = [u, 1]
        scat = np.zeros((n, (sp + 1) * f))
        np.add.at(scat, dst, (uh[:, :, None] * x[src][:, None, :]).reshape(-1, (sp + 1) * f))
        wstack = np.concatenate([wk.reshape(sp * f, fo), bk.reshape(f, fo)], 0)
        pre = scat @ wstack
    if root:
        pre = pre + x @ p["root_kernel"]
    if use_bias:
        pre = pre + p["bias"]
    if activation == "relu":
        out, side = _relu(pre, masks.get("act"))
    else:
        out, side = pre, np.ones(pre.shape, bool)
    r = {"out": out, "pre": pre, "act_side": side, "kn_pre": kn_pre, "kn_sides": kn_sides, "u": us}
    if dy is None:
        return r
    dz = np.where(side, np.asarray(dy, np.float64), 0.0)
    g = {}
    if use_bias:
        g["bias"] = dz.sum(0)
    dx = np.zeros_like(x)
    if root:
        g["root_kernel"] = x.T @ dz
        dx += dz @ p["root_kernel"].T
    if form == "materialised":
        dmsg = dz[dst]
        np.add.at(dx, src, np.einsum("abc,ac->ab", kern, dmsg))
        dkern = (x[src][:, :, None] * dmsg[:, None, :]).reshape(-1, f * fo)
        g["FGN_out_kernel"] = um.T @ dkern
        g["FGN_out_bias"] = dkern.sum(0)
        du = dkern @ wk.T
    else:
        dws = scat.T @ dz
        g["FGN_out_kernel"] = dws[:sp * f].reshape(sp, f * fo)
        g["FGN_out_bias"] = dws[sp * f:].reshape(f * fo)
        dscat = (dz @ wstack.T).reshape(n, sp + 1, f)
        np.add.at(dx, src, np.einsum("ac,aci->ai", uh, dscat[dst]))
        du = np.einsum("ai,aci->ac", x[src], dscat[dst][:, :sp])
    r["de"] = _kn_backward(du, us, kn_sides, p, hidden, g)
    r["dx"], r["grads"] = dx, g
    return r


def softmax_cce(logits, y, denom):
    """The "logits" form of keras categorical_crossentropy inside tf.function (gcnx_cce_mode): loss = sum CCE / denom,
    dlogits = (p - y) / denom, hits = rows whose argmax matches the label's."""
    z = logits - logits.max(1, keepdims=True)
    ex = np.exp(z)
    pr = ex / ex.sum(1, keepdims=True)
    y = np.asarray(y, np.float64)
    loss = -np.sum(y * (z - np.log(ex.sum(1, keepdims=True)))) / denom
    hits = float(np.sum(pr.argmax(1) == y.argmax(1))) if y.shape[0] else 0.0
    return pr, loss, hits, (pr - y) / denom


def model(x, indices, e, graph_ptr, params, hidden=None, y=None, denom=None, masks=None, flip=False, form="factorised"):
    """gcnx.ECCNet: ECCConv(relu) -> ECCConv(relu) -> GlobalSumPool -> Dense(softmax), categorical cross-entropy.
    params = {"conv1": {...}, "conv2": {...}, "dense_kernel": [H, n_labels], "dense_bias": [n_labels]};
    masks = {"conv1": {...}, "conv2": {...}} (the device's ReLU sides).  Returns probs, pooled, the two layer records
    and, with labels, loss, hits and grads in the same nesting as params."""
    masks = masks or {}
    gp = np.asarray(graph_ptr, np.int64)
    b = len(gp) - 1
    l1 = layer(x, indices, e, params["conv1"], hidden, "relu", masks=masks.get("conv1"), flip=flip, form=form)
    l2 = layer(l1["out"], indices, e, params["conv2"], hidden, "relu", masks=masks.get("conv2"), flip=flip, form=form)
    pooled = np.stack([l2["out"][gp[g]:gp[g + 1]].sum(0) for g in range(b)]) if b else np.zeros((0, l2["out"].shape[1]))
    w3, b3 = np.asarray(params["dense_kernel"], np.float64), np.asarray(params["dense_bias"], np.float64)
    logits = pooled @ w3 + b3
    r = {"pooled": pooled, "conv1": l1, "conv2": l2}
    if y is None:
        r["probs"] = softmax_cce(logits, np.zeros_like(logits), 1.0)[0]
        return r
    denom = float(denom or b)
    r["probs"], r["loss"], r["hits"], dlog = softmax_cce(logits, y, denom)
    g = {"dense_kernel": pooled.T @ dlog, "dense_bias": dlog.sum(0)}
    dpooled = dlog @ w3.T
    dy2 = np.repeat(dpooled, np.diff(gp), axis=0)
    b2 = layer(l1["out"], indices, e, params["conv2"], hidden, "relu", dy=dy2, flip=flip, form=form,
               masks={"act": l2["act_side"], "kn": l2["kn_sides"]})
    b1 = layer(x, indices, e, params["conv1"], hidden, "relu", dy=b2["dx"], flip=flip, form=form,
               masks={"act": l1["act_side"], "kn": l1["kn_sides"]})
    g["conv1"], g["conv2"] = b1["grads"], b2["grads"]
    r["grads"] = g
    return r


def sgd(params, grads, lr):
    out = {}
    for k, v in params.items():
        out[k] = sgd(v, grads[k], lr) if isinstance(v, dict) else np.asarray(v, np.float64) - lr * grads[k]
    return out


def kink_report(pre, device_side):
    """Where the device's ReLU side differs from the oracle's own (pre > 0): (number of differing elements, the largest
    |pre| among them relative to max |pre|, number of elements).  The GPU tests bound both: sides may differ only where
    the oracle's pre-activation is within 1e-5 of the tensor's largest magnitude, and on at most 1e-4 of its elements."""
    pre = np.asarray(pre, np.float64)
    diff = (pre > 0) != np.asarray(device_side, bool)
    top = max(float(np.max(np.abs(pre))), 1e-30) if pre.size else 1.0
    worst = float(np.max(np.abs(pre[diff]))) / top if diff.any() else 0.0
    return int(diff.sum()), worst, int(pre.size)


# ---- test inputs ---------------------------------------------------------------------------------------------------------
def random_batch(sizes, f, s=2, density=0.3, directed=False, seed=0, self_loops=True):
    """A disjoint batch: x [N, f], indices [nnz, 2] row-major, e [nnz, s], graph_ptr.  Undirected: the pattern is symmetric
    and e is equal in both directions of an edge (as the reference's graphs); directed: neither."""
    rng = np.random.default_rng(seed)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(gp[-1])
    rows, cols = [], []
    for g, m in enumerate(sizes):
        if m == 0:
            continue
        a = rng.random((m, m)) < density
        if not directed:
            a = np.triu(a, 1)
            a = a | a.T
        np.fill_diagonal(a, self_loops and not directed)
        r, c = np.nonzero(a)
        rows.append(r + gp[g]); cols.append(c + gp[g])
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    order = np.lexsort((cols, rows))
    idx = np.stack([rows[order], cols[order]], 1).astype(np.int64)
    e = rng.random((idx.shape[0], s))
    if not directed and idx.shape[0]:
        lo, hi = np.minimum(idx[:, 0], idx[:, 1]), np.maximum(idx[:, 0], idx[:, 1])
        _, inv = np.unique(lo * n + hi, return_inverse=True)
        e = rng.random((inv.max() + 1, s))[inv]
    x = rng.standard_normal((n, f))
    return x, idx, e, gp

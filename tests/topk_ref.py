"""float64 NumPy / SciPy restatement of TopKPool (spektral.layers.pooling.TopKPool in disjoint mode, gcn.py:10) as
gcnx.TopKPool defines it, and of gcnx.TopKNet: selection, gated gather, induced adjacency, backward, the whole step.  No torch.

    y = X p / ||p||      k_g = ceil(ratio n_g)      idx = the k_g rows of graph g with the largest y, IN ROW ORDER
    X' = (X * gate(y))[idx]      A' = A[idx][:, idx] (values copied)

Scores compare as IEEE numbers (-0.0 == +0.0); among equal scores the lower row index wins.
"""
import numpy as np


def kept_counts(graph_ptr, ratio):
    """k_g = ceil(ratio * n_g) in float64 (an empty graph keeps nothing)."""
    n_g = np.diff(np.asarray(graph_ptr, np.int64))
    return np.minimum(np.ceil(np.float64(ratio) * n_g.astype(np.float64)).astype(np.int64), n_g)


def kept_ptr(graph_ptr, ratio):
    return np.concatenate([[0], np.cumsum(kept_counts(graph_ptr, ratio))]).astype(np.int64)


def scores(x, p):
    p = np.asarray(p, np.float64).reshape(-1)
    return np.asarray(x, np.float64) @ p / np.sqrt(np.sum(p * p))


def _ranked(y_g):
    """Rows of one graph from the best down: descending score, ties by ascending row (a stable sort of -y; adding 0.0
    turns -0.0 into +0.0, and the two compare equal anyway)."""
    return np.argsort(-(np.asarray(y_g, np.float64) + 0.0), kind="stable")


def select(y, graph_ptr, ratio):
    """(idx [N'], pos [N], graph_ptr'): kept rows as global row numbers in ascending order, their new numbers (-1: dropped)."""
    gp = np.asarray(graph_ptr, np.int64)
    k = kept_counts(gp, ratio)
    idx = [gp[g] + np.sort(_ranked(y[gp[g]:gp[g + 1]])[:k[g]]) for g in range(len(gp) - 1)]
    idx = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    pos = np.full(int(gp[-1]), -1, np.int64)
    pos[idx] = np.arange(idx.size)
    return idx, pos, kept_ptr(gp, ratio)


def threshold_gap(y, graph_ptr, ratio):
    """The smallest distance between the k-th and the (k+1)-th best score of a graph, relative to max |y| (inf where every
    graph keeps all or none of its rows): how far a perturbation of y is from changing the selection."""
    gp = np.asarray(graph_ptr, np.int64)
    k = kept_counts(gp, ratio)
    y = np.asarray(y, np.float64)
    top = max(float(np.max(np.abs(y))), 1e-300) if y.size else 1.0
    gap = np.inf
    for g in range(len(gp) - 1):
        n_g = gp[g + 1] - gp[g]
        if 0 < k[g] < n_g:
            s = y[gp[g]:gp[g + 1]][_ranked(y[gp[g]:gp[g + 1]])]
            gap = min(gap, float(s[k[g] - 1] - s[k[g]]) / top)
    return gap


def gate(y, sigmoid=False):
    y = np.asarray(y, np.float64)
    return 1.0 / (1.0 + np.exp(-y)) if sigmoid else np.tanh(y)


def dgate(y, sigmoid=False):
    g = gate(y, sigmoid)
    return g * (1.0 - g) if sigmoid else 1.0 - g * g


def pool_fwd(x, p, graph_ptr, ratio, sigmoid=False, idx=None):
    """The layer's forward: {"y", "idx", "pos", "kept_ptr", "out"}.  idx: a selection to use instead of the oracle's own."""
    x = np.asarray(x, np.float64)
    y = scores(x, p)
    own_idx, pos, kp = select(y, graph_ptr, ratio)
    if idx is not None:
        idx = np.asarray(idx, np.int64)
        pos = np.full(x.shape[0], -1, np.int64)
        pos[idx] = np.arange(idx.size)
    else:
        idx = own_idx
    return {"y": y, "idx": idx, "pos": pos, "kept_ptr": kp, "out": x[idx] * gate(y[idx], sigmoid)[:, None]}


def pool_bwd(x, p, y, idx, dout, sigmoid=False):
    """(dx [N, F], dp [F]) from dout = dLoss / dX' [N', F]; nothing flows through the selection."""
    x, dout = np.asarray(x, np.float64), np.asarray(dout, np.float64)
    p = np.asarray(p, np.float64).reshape(-1)
    norm = np.sqrt(np.sum(p * p))
    ph = p / norm
    dy = np.zeros(x.shape[0])
    dy[idx] = dgate(y[idx], sigmoid) * np.sum(dout * x[idx], 1)
    dx = np.zeros_like(x)
    dx[idx] = gate(y[idx], sigmoid)[:, None] * dout
    dx += dy[:, None] * ph[None, :]
    v = x.T @ dy
    return dx, (v - ph * (ph @ v)) / norm


def induce(a, idx):
    """A[idx][:, idx] of a scipy matrix as CSR with sorted indices; stored entries are kept (also explicit zeros)."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a)
    n = a.shape[0]
    idx = np.asarray(idx, np.int64)
    pos = np.full(n, -1, np.int64)
    pos[idx] = np.arange(idx.size)
    rows = np.repeat(np.arange(n), np.diff(a.indptr))
    keep = (pos[rows] >= 0) & (pos[a.indices] >= 0)
    r, c, v = pos[rows[keep]], pos[a.indices[keep]], a.data[keep]
    order = np.lexsort((c, r))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=idx.size))]).astype(np.int64)
    out = sp.csr_matrix((v[order], c[order], rowptr), shape=(idx.size, idx.size))
    return out


# ---- GCNConv and the model -----------------------------------------------------------------------------------------------
def _relu(pre, side=None):
    side = (pre > 0) if side is None else np.asarray(side, bool)
    return np.where(side, pre, 0.0), side


def gcn_conv_fwd(a, x, w, b, side=None):
    pre = a @ (np.asarray(x, np.float64) @ np.asarray(w, np.float64)) + np.asarray(b, np.float64)
    out, side = _relu(pre, side)
    return out, pre, side


def gcn_conv_bwd(a, x, w, side, dout):
    dz = np.where(side, np.asarray(dout, np.float64), 0.0)
    t = a.T @ dz
    return t @ np.asarray(w, np.float64).T, np.asarray(x, np.float64).T @ t, dz.sum(0)


def softmax_cce(logits, y, denom):
    """The "logits" form of the categorical cross-entropy: loss = sum CCE / denom, dlogits = (p - y) / denom."""
    z = logits - logits.max(1, keepdims=True)
    ex = np.exp(z)
    pr = ex / ex.sum(1, keepdims=True)
    y = np.asarray(y, np.float64)
    loss = -np.sum(y * (z - np.log(ex.sum(1, keepdims=True)))) / denom
    hits = float(np.sum(pr.argmax(1) == y.argmax(1))) if y.shape[0] else 0.0
    return pr, loss, hits, (pr - y) / denom


KEYS = ("conv1_kernel", "conv1_bias", "pool_kernel", "conv2_kernel", "conv2_bias", "dense_kernel", "dense_bias")


def init_params(f_in, hidden, n_labels=2, seed=0):
    rng = np.random.default_rng(seed)
    u = lambda fi, fo: rng.uniform(-1, 1, (fi, fo)) * np.sqrt(6.0 / (fi + fo))
    return {"conv1_kernel": u(f_in, hidden), "conv1_bias": rng.uniform(-0.1, 0.1, hidden), "pool_kernel": u(hidden, 1),
            "conv2_kernel": u(hidden, hidden), "conv2_bias": rng.uniform(-0.1, 0.1, hidden),
            "dense_kernel": u(hidden, n_labels), "dense_bias": rng.uniform(-0.1, 0.1, n_labels)}


def model(x, a, graph_ptr, params, ratio, y=None, pool="sum", sigmoid=False, denom=None, masks=None, idx=None):
    """gcnx.TopKNet: GCNConv(relu) -> TopKPool(ratio) -> GCNConv(relu) -> global sum / avg pool -> Dense(softmax), CCE.
    a: scipy CSR (used with its values).  masks = {"m1", "m2"}: ReLU sides to use instead of the oracle's own (pre > 0);
    idx: a selection to use instead of the oracle's own.  Returns probs, the intermediates and, with labels, loss, hits
    and grads keyed as KEYS."""
    import scipy.sparse as sp
    m = masks or {}
    q = {k: np.asarray(v, np.float64) for k, v in params.items()}
    a = sp.csr_matrix(a).astype(np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    b = len(gp) - 1
    y1, pre1, s1 = gcn_conv_fwd(a, x, q["conv1_kernel"], q["conv1_bias"], m.get("m1"))
    pl = pool_fwd(y1, q["pool_kernel"], gp, ratio, sigmoid, idx)
    a2 = induce(a, pl["idx"])
    kp = pl["kept_ptr"]
    y2, pre2, s2 = gcn_conv_fwd(a2, pl["out"], q["conv2_kernel"], q["conv2_bias"], m.get("m2"))
    cnt = np.diff(kp).astype(np.float64)
    scale = np.ones(b) if pool == "sum" else np.where(cnt > 0, 1.0 / np.maximum(cnt, 1.0), 0.0)
    pooled = np.stack([y2[kp[g]:kp[g + 1]].sum(0) * scale[g] for g in range(b)]) if b else np.zeros((0, y2.shape[1]))
    logits = pooled @ q["dense_kernel"] + q["dense_bias"]
    r = {"pooled": pooled, "y1": y1, "pre1": pre1, "pre2": pre2, "y2": y2, "pool": pl, "a2": a2, "gap": threshold_gap(pl["y"], gp, ratio)}
    if y is None:
        r["probs"] = softmax_cce(logits, np.zeros_like(logits), 1.0)[0]
        return r
    denom = float(denom or b)
    r["probs"], r["loss"], r["hits"], dlog = softmax_cce(logits, y, denom)
    g = {"dense_kernel": pooled.T @ dlog, "dense_bias": dlog.sum(0)}
    dpooled = dlog @ q["dense_kernel"].T
    dy2 = np.repeat(dpooled * scale[:, None], np.diff(kp), axis=0)
    dx2, g["conv2_kernel"], g["conv2_bias"] = gcn_conv_bwd(a2, pl["out"], q["conv2_kernel"], s2, dy2)
    dy1, dp = pool_bwd(y1, q["pool_kernel"], pl["y"], pl["idx"], dx2, sigmoid)
    g["pool_kernel"] = dp.reshape(-1, 1)
    _, g["conv1_kernel"], g["conv1_bias"] = gcn_conv_bwd(a, x, q["conv1_kernel"], s1, dy1)
    r["grads"] = g
    return r


def sgd(params, grads, lr):
    return {k: np.asarray(v, np.float64) - lr * np.asarray(grads[k], np.float64).reshape(np.shape(v)) for k, v in params.items()}

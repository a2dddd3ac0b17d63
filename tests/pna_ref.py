"""float64 NumPy restatement of PyG's PNAConv(aggregators=['mean', 'min', 'max', 'std'], scalers=['identity', 'amplification',
'attenuation'], deg, towers=1, pre_layers=1, post_layers=1, divide_input=False) and of gcnx.PNA -- the reference's torch GCN
(gcn_utills.py:795-853) with its two GCNConv layers replaced by PNAConv -- with BCEWithLogitsLoss: forward, loss, accuracy,
every gradient.  No torch.

    M_ij = [x_i | x_j] W_pre^T + b_pre = P_i + Q_j        row i of the CSR is the target, its stored entries j the sources;
    A_i  = [mean | min | max | sqrt(relu(var) + 1e-5)]    values ignored, no self-loop added or removed; a row without entries
    C_i  = [x_i | A_i | s_amp,i A_i | s_att,i A_i]        has A_i = [0 | 0 | 0 | sqrt(1e-5)];  s_amp,i = log(max(d_i, 1) + 1) / delta
    out  = (C W_post^T + b_post) W_lin^T + b_lin          = 1 / s_att,i

Ties of the minimum / maximum share the gradient evenly (torch.scatter_reduce("amin" / "amax")).  BatchNorm, PReLU, the
max-pool, the head, BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's.  Parameters use the torch key
names and layouts: conv*.pre_nns.0.0.weight [F, 2F], conv*.post_nns.0.0.weight [H, 13F], conv*.lin.weight [H, H], biases [out].
"""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401

STD_EPS = 1e-5
_CONV = ("pre_nns.0.0.weight", "pre_nns.0.0.bias", "post_nns.0.0.weight", "post_nns.0.0.bias", "lin.weight", "lin.bias")
CONV_KEYS = tuple(f"conv{k}.{s}" for k in (1, 2) for s in _CONV)
KEYS = CONV_KEYS + ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
                    "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
                    "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")
DELTA_KEYS = ("conv1.aggr_module.avg_deg_log", "conv2.aggr_module.avg_deg_log")
STATE_KEYS = (DELTA_KEYS[0],) + CONV_KEYS[:6] + (DELTA_KEYS[1],) + CONV_KEYS[6:] + KEYS[12:]     # state_dict() order


def conv_params(fi, h, rng, bias=True):
    """Random parameters of one PNAConv(fi -> h) in torch's layouts: (w_pre, b_pre, w_post, b_post, w_lin, b_lin)."""
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    b = (lambda *s: u(0.1, *s)) if bias else (lambda *s: None)
    return (u(1 / np.sqrt(2 * fi), fi, 2 * fi), b(fi), u(1 / np.sqrt(13 * fi), h, 13 * fi), b(h), u(1 / np.sqrt(h), h, h), b(h))


def init_params(f_in, h=64, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = _gcn_params(f_in, h, seed)
    for k in ("conv1.bias", "conv1.lin.weight", "conv2.bias", "conv2.lin.weight"):
        del p[k]
    rng = np.random.default_rng(seed + 3000)
    for c, fi in (("conv1", f_in), ("conv2", h)):
        for s, v in zip(_CONV, conv_params(fi, h, rng)):
            p[f"{c}.{s}"] = v
    return {k: p[k] for k in KEYS}


def pattern(a, n=None):
    """(rowptr, colidx) of the stored pattern of `a` (scipy; row = target): values ignored, duplicates counted once."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a, shape=None if n is None else (n, n)).copy()
    a.sum_duplicates()
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int64)


def avg_deg_log(hist):
    """delta from PyG's in-degree histogram: sum_d hist[d] log(d + 1) / sum_d hist[d]."""
    hist = np.asarray(hist, np.float64)
    return float((hist * np.log(np.arange(hist.size) + 1.0)).sum() / hist.sum())


def _segsum(vals, ids, n):
    """out[k] = the sum of vals[e] over ids[e] == k; vals [E, F], out [n, F]."""
    out = np.zeros((n,) + vals.shape[1:])
    if len(ids):
        order = np.argsort(ids, kind="stable")
        cnt = np.bincount(ids, minlength=n)
        starts = (np.cumsum(cnt) - cnt)[cnt > 0]
        out[cnt > 0] = np.add.reduceat(vals[order], starts, axis=0)
    return out


def scalers(d, delta):
    l = np.log(np.maximum(d, 1) + 1.0)
    return l / delta, delta / l


def aggregate(rowptr, colidx, x, pq, delta):
    """The contract of gcnx_pna_aggregate in float64: (c [n, 13f], stats [n, 6f] = meanQ | minQ | maxQ | std | cmin | cmax)."""
    x, pq = np.asarray(x, np.float64), np.asarray(pq, np.float64)
    n, f = x.shape
    P, Q = pq[:, :f], pq[:, f:]
    d = np.diff(rowptr)
    ne = d > 0
    mean, mn, mx, var, cmin, cmax = (np.zeros((n, f)) for _ in range(6))
    if len(colidx):
        t = np.repeat(np.arange(n), d)
        qe = Q[colidx]
        starts = rowptr[:-1][ne]                                  # the rows between two non-empty ones hold no entries
        dn = d[ne][:, None].astype(np.float64)
        mean[ne] = np.add.reduceat(qe, starts, axis=0) / dn
        mn[ne], mx[ne] = np.minimum.reduceat(qe, starts, axis=0), np.maximum.reduceat(qe, starts, axis=0)
        var[ne] = np.add.reduceat((qe - mean[t]) ** 2, starts, axis=0) / dn
        cmin[ne] = np.add.reduceat((qe == mn[t]).astype(np.float64), starts, axis=0)
        cmax[ne] = np.add.reduceat((qe == mx[t]).astype(np.float64), starts, axis=0)
    var[mx == mn] = 0.0                                           # all entries equal: exactly zero, not a rounding of it
    std = np.sqrt(np.maximum(var, 0.0) + STD_EPS)
    m = ne[:, None]
    A = np.concatenate([m * (P + mean), m * (P + mn), m * (P + mx), std], axis=1)
    amp, att = scalers(d, delta)
    c = np.concatenate([x, A, amp[:, None] * A, att[:, None] * A], axis=1)
    return c, np.concatenate([mean, mn, mx, std, cmin, cmax], axis=1)


def aggregate_bwd(rowptr, colidx, pq, stats, dc, delta):
    """The contract of gcnx_pna_bwd in float64: dpq [n, 2f] = dP | dQ from dc [n, 13f] (block 0 is not read).  Also returns
    the largest |term| of every dQ sum (the scale its error is measured against)."""
    pq, stats, dc = np.asarray(pq, np.float64), np.asarray(stats, np.float64), np.asarray(dc, np.float64)
    n, f = pq.shape[0], pq.shape[1] // 2
    Q = pq[:, f:]
    mean, mn, mx, std, cmin, cmax = (stats[:, k * f:(k + 1) * f] for k in range(6))
    d = np.diff(rowptr)
    ne = (d > 0)[:, None]
    amp, att = scalers(d, delta)
    g = dc[:, f:5 * f] + amp[:, None] * dc[:, 5 * f:9 * f] + att[:, None] * dc[:, 9 * f:13 * f]
    g_mean, g_min, g_max, g_std = (g[:, k * f:(k + 1) * f] for k in range(4))
    dP = ne * (g_mean + g_min + g_max)
    dQ, big = np.zeros((n, f)), np.zeros((n, f))
    if len(colidx):
        t = np.repeat(np.arange(n), d)
        qe = Q[colidx]
        dd = d[t][:, None].astype(np.float64)
        terms = (g_mean[t] / dd, g_min[t] * (qe == mn[t]) / np.maximum(cmin[t], 1), g_max[t] * (qe == mx[t]) / np.maximum(cmax[t], 1),
                 g_std[t] * (mx[t] > mn[t]) * (qe - mean[t]) / (dd * std[t]))
        dQ = _segsum(sum(terms), colidx, n)
        for term in terms:
            np.maximum.at(big, colidx, np.abs(term))
    return np.concatenate([dP, dQ], axis=1), big


def pna_conv_fwd(rowptr, colidx, x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, delta):
    """One layer; weights in torch's layouts, biases may be None.  Returns (out, cache)."""
    x = np.asarray(x, np.float64)
    f = x.shape[1]
    w_pre = np.asarray(w_pre, np.float64)
    P = x @ w_pre[:, :f].T + (0.0 if b_pre is None else np.asarray(b_pre, np.float64))
    Q = x @ w_pre[:, f:].T
    pq = np.concatenate([P, Q], axis=1)
    c, stats = aggregate(rowptr, colidx, x, pq, delta)
    t = c @ np.asarray(w_post, np.float64).T + (0.0 if b_post is None else np.asarray(b_post, np.float64))
    out = t @ np.asarray(w_lin, np.float64).T + (0.0 if b_lin is None else np.asarray(b_lin, np.float64))
    return out, dict(x=x, pq=pq, c=c, stats=stats, t=t)


def pna_conv_bwd(rowptr, colidx, cache, w_pre, w_post, w_lin, delta, dz):
    """(dx, dW_pre, db_pre, dW_post, db_post, dW_lin, db_lin) of pna_conv_fwd from dz = dLoss / dout."""
    dz = np.asarray(dz, np.float64)
    x, f = cache["x"], cache["x"].shape[1]
    w_pre = np.asarray(w_pre, np.float64)
    dt = dz @ np.asarray(w_lin, np.float64)
    dc = dt @ np.asarray(w_post, np.float64)
    dpq, _ = aggregate_bwd(rowptr, colidx, cache["pq"], cache["stats"], dc, delta)
    dP, dQ = dpq[:, :f], dpq[:, f:]
    dx = dc[:, :f] + dP @ w_pre[:, :f] + dQ @ w_pre[:, f:]
    return dx, np.concatenate([dP.T @ x, dQ.T @ x], axis=1), dP.sum(0), dt.T @ cache["c"], dt.sum(0), dz.T @ cache["t"], dz.sum(0)


def model(x, a, graph_ptr, p, delta, y=None, denom=None, masks=None, argmax=None):
    """gcn_bn_ref.model with the two convolutions replaced and no self-loops added: same arguments (+ delta, one value or one
    per convolution), same result dict."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    rp, ci = pattern(a, x.shape[0])
    dl = [float(v) for v in np.broadcast_to(np.asarray(delta, np.float64).reshape(-1), (2,))]
    cw = lambda c: tuple(q[f"{c}.{s}"] for s in _CONV)
    z1, k1 = pna_conv_fwd(rp, ci, x, *cw("conv1"), dl[0])
    zb1, c1 = bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2, k2 = pna_conv_fwd(rp, ci, y1, *cw("conv2"), dl[1])
    zb2, c2 = bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = prelu_fwd(zb2, q["prelu_2.weight"][0], m.get("m2"))
    arg = first_argmax(y2, graph_ptr) if argmax is None else np.asarray(argmax, np.int64)
    cols = np.arange(y2.shape[1])
    P = np.stack([y2[arg[g], cols] if graph_ptr[g + 1] > graph_ptr[g] else np.zeros(y2.shape[1])
                  for g in range(len(graph_ptr) - 1)])
    r = head(P, p, y, denom, m)
    r.update(m1=p1, m2=p2, argmax=arg, pooled=P, y2=y2, z1=z1, z2=z2, stats1=k1["stats"], stats2=k2["stats"])
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    names = lambda c: [f"{c}.{s}" for s in _CONV]
    w = lambda c: (q[f"{c}.pre_nns.0.0.weight"], q[f"{c}.post_nns.0.0.weight"], q[f"{c}.lin.weight"])
    dy1, *gs = pna_conv_bwd(rp, ci, k2, *w("conv2"), dl[1], dz2)
    g.update(zip(names("conv2"), gs))
    dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    _, *gs = pna_conv_bwd(rp, ci, k1, *w("conv1"), dl[0], dz1)
    g.update(zip(names("conv1"), gs))
    return r


def graphs(kind, n_graphs=8, f=16, seed=0, lo=8, hi=40):
    """One disjoint batch for the PNA tests: x, scipy adjacency (row = target), graph_ptr, y.  "symmetric": an undirected
    pattern, most rows with a stored self-loop; "directed": a directed pattern without loops.  Both hold a graph of a single
    node without entries, in every larger graph a node without entries (node 1) and a row with exactly one entry (node 2),
    and duplicated feature rows: the upper half of every graph's nodes repeats three rows, so minima and maxima tie."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    sizes = rng.integers(lo, hi + 1, n_graphs)
    sizes[min(3, n_graphs - 1)] = 1
    gp = np.concatenate([[0], np.cumsum(sizes)])
    x = rng.normal(size=(gp[-1], f))
    blocks = []
    for gi, s in enumerate(sizes):
        m = np.triu(rng.random((s, s)) < 0.25, 1)
        m = m | (np.tril(rng.random((s, s)) < 0.25, -1) if kind == "directed" else m.T)
        if kind == "symmetric":
            m[np.diag_indices(s)] = rng.random(s) < 0.7
        if s == 1:
            m[:] = False
        if s > 3:
            m[1, :] = False                                   # a node without entries ...
            m[:, 1] = False
            m[2, :] = False                                   # ... and a row with exactly one
            m[2, 0] = True
            if kind == "symmetric":
                m[:, 2] = False
                m[0, 2] = True
            half = np.arange(s // 2, s)
            x[gp[gi] + half] = x[gp[gi] + half[:3]][np.arange(len(half)) % min(3, len(half))]
        blocks.append(sp.csr_matrix(m.astype(np.float64) * rng.uniform(0.5, 2.0, (s, s))))   # values are ignored
    a = sp.block_diag(blocks, format="csr")
    y = np.eye(2)[rng.integers(0, 2, n_graphs)]
    return x, a, gp, y

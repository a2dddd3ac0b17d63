"""float64 NumPy restatement of PyG's GATv2Conv(heads=H, concat=True, negative_slope=0.2, dropout=0, add_self_loops=False,
edge_dim=D, bias=True, share_weights=False) and of gcnx.GATv2 -- the reference's torch GCN (gcn_utills.py:795-853) with its
two GCNConv layers replaced by GATv2Conv, which reads the dca / proximity edge features the reference computes and drops
(gcn_utills.py:319-443; gcn.py:71) -- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient.  No torch.

    Xl = x W_l + b_l    Xr = x W_r + b_r    t_ij = e_ij W_e    s_ij = (Xl[j] + Xr[i]) + t_ij    g = s > 0 ? s : slope s
    score_ij,h = <att[h,:], g_ij[h,:]>     alpha = softmax over the stored entries j of row i (row = target)
    out[i,h,:] = sum_j alpha_ij,h Xl[j,h,:] + bias            (a row without entries: out = bias)

The pattern (rowptr, colidx) and e [nnz, D] are used as stored; mean_self_loops is PyG's add_self_loops=True rule for a host
adjacency.  BatchNorm, PReLU, the max-pool, the head, BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's;
``masks`` takes "s1" / "s2" [nnz, H C] beside them: the side of s of every entry and channel (CSR entry order), as the device
decided it (device_sides).  Parameters use PyG's key names and layouts: conv*.att [1, H, C], conv*.bias [H C], conv*.lin_l.weight
/ lin_r.weight [H C, in], conv*.lin_l.bias / lin_r.bias [H C], conv*.lin_edge.weight [H C, D]."""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401
from gat_ref import _per_head

CONV_PARTS = ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "lin_edge.weight")
TAIL_KEYS = ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
             "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
             "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")


def keys(edge_dim=None):
    """The state_dict keys of gcnx.GATv2 in order (lin_edge.weight only with edge features)."""
    parts = CONV_PARTS if edge_dim else CONV_PARTS[:-1]
    return tuple(f"conv{k}.{t}" for k in (1, 2) for t in parts) + TAIL_KEYS


def init_params(f_in, h=64, heads=1, edge_dim=None, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    assert h % heads == 0
    p = _gcn_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 3000)
    c = h // heads
    for k, fi in (("conv1", f_in), ("conv2", h)):
        p[f"{k}.att"] = rng.normal(size=(1, heads, c)) / np.sqrt(c)
        p[f"{k}.bias"] = rng.uniform(-0.1, 0.1, h)
        for s in ("lin_l", "lin_r"):
            p[f"{k}.{s}.weight"] = rng.uniform(-1, 1, (h, fi)) * np.sqrt(6 / (fi + h))
            p[f"{k}.{s}.bias"] = rng.uniform(-0.1, 0.1, h)
        if edge_dim:
            p[f"{k}.lin_edge.weight"] = rng.uniform(-1, 1, (h, edge_dim)) * np.sqrt(6 / (edge_dim + h))
    return {k: p[k] for k in keys(edge_dim)}


def stored_pattern(a, e=None):
    """(rowptr, colidx, e) of a scipy / COO adjacency as stored (row = target), entries row-major; e [nnz, D] follows them."""
    import scipy.sparse as sp
    a = sp.coo_matrix(a)
    order = np.lexsort((a.col, a.row))
    n = a.shape[0]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(a.row, minlength=n))]).astype(np.int64)
    return rowptr, a.col[order].astype(np.int64), (None if e is None else np.asarray(e)[order])


def mean_self_loops(rowptr, colidx, e, n=None):
    """PyG's add_self_loops(fill_value="mean") on a stored pattern: the stored loops are removed, one loop per node is added,
    its feature row the mean of the feature rows of that row's remaining entries (zeros if none).  Returns (rowptr, colidx, e)."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n = len(rowptr) - 1 if n is None else n
    row = np.repeat(np.arange(n), np.diff(rowptr))
    keep = row != colidx
    r2, c2 = np.concatenate([row[keep], np.arange(n)]), np.concatenate([colidx[keep], np.arange(n)])
    order = np.lexsort((c2, r2))
    e2 = None
    if e is not None:
        e = np.asarray(e, np.float64)
        fill = np.zeros((n, e.shape[1]))
        for i in range(n):                                # (plain loops: this is the statement of the rule)
            mine = e[keep & (row == i)]
            if len(mine):
                fill[i] = mine.mean(0)
        e2 = np.concatenate([e[keep], fill])[order]
    return np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int64), c2[order], e2


def conv_fwd(rowptr, colidx, x, Wl, bl, Wr, br, att, bias, e=None, We=None, slope=0.2, sides=None):
    """Wl, Wr [in, H C]; bl, br [H C] (or None); att [H, C] (or [1, H, C]); bias [H C] or None; e [nnz, D] and We [D, H C] or both
    None; sides [nnz, H C] (bool): the side of s of every entry and channel (None: s > 0).  Returns (out [n, H C], cache)."""
    x, Wl, Wr = (np.asarray(t, np.float64) for t in (x, Wl, Wr))
    att = np.asarray(att, np.float64).reshape(-1, np.shape(att)[-1])
    H, C = att.shape
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n = x.shape[0]
    row = np.repeat(np.arange(n), np.diff(rowptr))
    Xl = (x @ Wl + (0.0 if bl is None else np.asarray(bl, np.float64))).reshape(n, H, C)
    Xr = (x @ Wr + (0.0 if br is None else np.asarray(br, np.float64))).reshape(n, H, C)
    if e is not None:
        e, We = np.asarray(e, np.float64), np.asarray(We, np.float64)
        t = (e @ We).reshape(-1, H, C)
    else:
        t = 0.0
    s = (Xl[colidx] + Xr[row]) + t
    pos = s > 0 if sides is None else np.asarray(sides, bool).reshape(s.shape)
    g = np.where(pos, s, slope * s)
    score = np.einsum("ehc,hc->eh", g, att)
    m = np.full((n, H), -np.inf)
    np.maximum.at(m, row, score)
    w = np.exp(score - m[row])
    l = np.zeros((n, H))
    np.add.at(l, row, w)
    alpha = w / l[row]
    O = _per_head(rowptr, colidx, n, alpha, Xl)
    out = O.reshape(n, H * C) + (0.0 if bias is None else np.asarray(bias, np.float64))
    cache = dict(rowptr=rowptr, colidx=colidx, row=row, x=x, Wl=Wl, Wr=Wr, att=att, slope=slope, Xl=Xl, Xr=Xr, e=e, We=We, s=s, pos=pos,
                 g=g, score=score, alpha=alpha, O=O, n=n, H=H, C=C)
    return out, cache


def conv_bwd(cache, dout):
    """{name: gradient} of conv_fwd from dout = dLoss / dout: x, Wl, bl, Wr, br, att, bias, We (None without edge features).
    Leaves dscore, dXl and dXr in the cache (what the kernels are compared with)."""
    c = cache
    n, H, C, row, col = c["n"], c["H"], c["C"], c["row"], c["colidx"]
    dO = np.asarray(dout, np.float64).reshape(n, H, C)
    r = np.einsum("nhc,nhc->nh", dO, c["O"])
    dalpha = np.einsum("ehc,ehc->eh", dO[row], c["Xl"][col])
    dscore = c["alpha"] * (dalpha - r[row])
    ds = dscore[:, :, None] * c["att"][None] * np.where(c["pos"], 1.0, c["slope"])
    datt = np.einsum("eh,ehc->hc", dscore, c["g"])
    dXr, dXl = np.zeros((n, H, C)), _per_head(c["rowptr"], col, n, c["alpha"], dO, transpose=True)
    np.add.at(dXr, row, ds)
    np.add.at(dXl, col, ds)
    dXl2, dXr2, ds2 = dXl.reshape(n, H * C), dXr.reshape(n, H * C), ds.reshape(-1, H * C)
    c.update(dscore=dscore, ds=ds2, dXl=dXl2, dXr=dXr2)
    return dict(x=dXl2 @ c["Wl"].T + dXr2 @ c["Wr"].T, Wl=c["x"].T @ dXl2, bl=dXl2.sum(0), Wr=c["x"].T @ dXr2, br=dXr2.sum(0), att=datt,
                bias=dO.reshape(n, H * C).sum(0), We=None if c["e"] is None else c["e"].T @ ds2)


def device_sides(Xlr, e, W_e, rowptr, colidx):
    """The side of s of every entry and channel [nnz, H C] as the device decides it, from the STORED float32 Xl | Xr [n, 2 H C],
    e [nnz, D] and W_e [D, H C] (both None: no edge features), in float32 by the contract of include/gcnx.h: t starts from the
    rounded product of d = 0 and adds the separately rounded products of d = 1 .. D - 1 in that order (no FMA; D = 0: t = 0),
    one add forms Xl + Xr, one more adds t; positive is s > 0."""
    Xlr = np.asarray(Xlr, np.float32)
    hc = Xlr.shape[1] // 2
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    t = np.zeros((len(colidx), hc), np.float32)
    if e is not None:
        e, W_e = np.asarray(e, np.float32), np.asarray(W_e, np.float32)
        for d in range(e.shape[1]):
            pr = e[:, d:d + 1] * W_e[d][None, :]
            t = pr if d == 0 else t + pr
    s = (Xlr[colidx, :hc] + Xlr[row, hc:]) + t
    assert s.dtype == np.float32
    return s > 0


def model(x, rowptr, colidx, e, graph_ptr, p, y=None, denom=None, masks=None, argmax=None, heads=1):
    """gcn_bn_ref.model with the two convolutions replaced, on the pattern and e as given: same result dict; masks["s1"],
    masks["s2"]: the sides of s of the two convolutions."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)

    def conv(k, inp):
        c = f"conv{k}."
        we = q.get(c + "lin_edge.weight")
        return conv_fwd(rowptr, colidx, inp, q[c + "lin_l.weight"].T, q[c + "lin_l.bias"], q[c + "lin_r.weight"].T, q[c + "lin_r.bias"],
                        q[c + "att"].reshape(heads, -1), q[c + "bias"], e if we is not None else None, None if we is None else we.T,
                        0.2, m.get(f"s{k}"))

    z1, k1 = conv(1, x)
    zb1, c1 = bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2, k2 = conv(2, y1)
    zb2, c2 = bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = prelu_fwd(zb2, q["prelu_2.weight"][0], m.get("m2"))
    arg = first_argmax(y2, graph_ptr) if argmax is None else np.asarray(argmax, np.int64)
    cols = np.arange(y2.shape[1])
    P = np.stack([y2[arg[g], cols] if graph_ptr[g + 1] > graph_ptr[g] else np.zeros(y2.shape[1])
                  for g in range(len(graph_ptr) - 1)])
    r = head(P, p, y, denom, m)
    r.update(m1=p1, m2=p2, s1=k1["pos"], s2=k2["pos"], argmax=arg, pooled=P, y2=y2, conv1=k1, conv2=k2)
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    dzk = {2: dz2}
    for k, cache in ((2, k2), (1, k1)):
        if k == 1:
            dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
            dzk[1], g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
        d = conv_bwd(cache, dzk[k])
        dy1 = d["x"]
        c = f"conv{k}."
        g[c + "att"], g[c + "bias"] = d["att"][None], d["bias"]
        g[c + "lin_l.weight"], g[c + "lin_l.bias"], g[c + "lin_r.weight"], g[c + "lin_r.bias"] = d["Wl"].T, d["bl"], d["Wr"].T, d["br"]
        if d["We"] is not None:
            g[c + "lin_edge.weight"] = d["We"].T
    return r

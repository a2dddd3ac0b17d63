"""float64 NumPy restatement of PyG's GATConv(heads=H, concat=True, negative_slope=0.2, dropout=0, bias=True) and of
gcnx.GAT -- the reference's torch GCN (gcn_utills.py:795-853) with its two GCNConv layers replaced by GATConv, the slot the
comment above them leaves open (gcn_utills.py:804-806) -- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient.
No torch.

    Hf = x W   a_src[j,h] = <Hf[j,h,:], att_src[h,:]>   a_dst[i,h] = <Hf[i,h,:], att_dst[h,:]>   z = a_src[j,h] + a_dst[i,h]
    e = z > 0 ? z : slope z     alpha = softmax of e over the stored entries j of row i (row = target)
    out[i,h,:] = sum_j alpha_ij,h Hf[j,h,:] + bias            (a row without entries: out = bias)

BatchNorm, PReLU, the max-pool, the head, BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's; ``masks``
takes "e1" / "e2" [nnz, heads] beside them: the side of z of every entry (CSR entry order), as the device decided it.
Parameters use PyG's key names and layouts: conv*.att_src / att_dst [1, H, C], conv*.bias [H C], conv*.lin.weight [H C, in].
"""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401

CONV_KEYS = ("conv1.att_src", "conv1.att_dst", "conv1.bias", "conv1.lin.weight",
             "conv2.att_src", "conv2.att_dst", "conv2.bias", "conv2.lin.weight")
KEYS = CONV_KEYS + ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
                    "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
                    "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")


def init_params(f_in, h=64, heads=1, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    assert h % heads == 0
    p = _gcn_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 2000)
    c = h // heads
    for k, fi in (("conv1", f_in), ("conv2", h)):
        p[f"{k}.att_src"], p[f"{k}.att_dst"] = rng.normal(size=(1, heads, c)) / np.sqrt(c), rng.normal(size=(1, heads, c)) / np.sqrt(c)
        p[f"{k}.bias"] = rng.uniform(-0.1, 0.1, h)
        p[f"{k}.lin.weight"] = rng.uniform(-1, 1, (h, fi)) * np.sqrt(6 / (fi + h))
    return {k: p[k] for k in KEYS}


def pattern(a, n=None, loops=True):
    """(rowptr, colidx) of the stored pattern of `a` (scipy; row = target), duplicates counted once, columns ascending;
    loops: PyG's remaining self-loops (GATConv removes and re-adds them: the same pattern once values are ignored)."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a, shape=None if n is None else (n, n)).copy()
    a.sum_duplicates()
    a.data[:] = 1.0
    if loops:
        a = sp.csr_matrix(a + sp.diags(np.where(a.diagonal() == 0, 1.0, 0.0)))
    a.sort_indices()
    return a.indptr.astype(np.int64), a.indices.astype(np.int64)


def _per_head(rowptr, colidx, n, w, m, transpose=False):
    """[n, H, C]: for every head h, A_h m[:, h, :] with A_h = the pattern carrying w[:, h] (transpose: A_h^T)."""
    import scipy.sparse as sp
    out = np.zeros_like(m)
    for h in range(w.shape[1]):
        A = sp.csr_matrix((w[:, h], colidx, rowptr), shape=(n, n))
        out[:, h, :] = (A.T if transpose else A) @ m[:, h, :]
    return out


def softmax_aggregate(rowptr, colidx, Hf, a_src, a_dst, slope=0.2, sides=None):
    """The attention half of the layer from given score halves: Hf [n, H, C], a_src, a_dst [n, H].  Returns (O [n, H, C], alpha
    [nnz, H], z, pos): the softmax runs over the stored entries of every row; a row without entries gives O = 0."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    Hf, a_src, a_dst = np.asarray(Hf, np.float64), np.asarray(a_src, np.float64), np.asarray(a_dst, np.float64)
    n, H = a_src.shape
    row = np.repeat(np.arange(n), np.diff(rowptr))
    z = a_src[colidx] + a_dst[row]
    pos = z > 0 if sides is None else np.asarray(sides, bool).reshape(z.shape)
    e = np.where(pos, z, slope * z)
    m = np.full((n, H), -np.inf)
    np.maximum.at(m, row, e)
    w = np.exp(e - m[row])
    l = np.zeros((n, H))
    np.add.at(l, row, w)
    alpha = w / l[row]
    return _per_head(rowptr, colidx, n, alpha, Hf), alpha, z, pos


def gat_conv_fwd(rowptr, colidx, x, W, att_src, att_dst, bias, slope=0.2, sides=None):
    """W [in, H C] (Hf = x W); att_src, att_dst [H, C] (or [1, H, C]); bias [H C] or None; sides [nnz, H] (bool): the side of
    z of every entry (None: z > 0).  Returns (out [n, H C], cache)."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    att_src, att_dst = (np.asarray(t, np.float64).reshape(-1, np.shape(t)[-1]) for t in (att_src, att_dst))
    H, C = att_src.shape
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n = x.shape[0]
    row = np.repeat(np.arange(n), np.diff(rowptr))
    Hf = (x @ W).reshape(n, H, C)
    a_src, a_dst = np.einsum("nhc,hc->nh", Hf, att_src), np.einsum("nhc,hc->nh", Hf, att_dst)
    O, alpha, z, pos = softmax_aggregate(rowptr, colidx, Hf, a_src, a_dst, slope, sides)
    out = O.reshape(n, H * C) + (0.0 if bias is None else np.asarray(bias, np.float64))
    cache = dict(rowptr=rowptr, colidx=colidx, row=row, x=x, W=W, att_src=att_src, att_dst=att_dst, slope=slope, Hf=Hf, a_src=a_src,
                 a_dst=a_dst, z=z, pos=pos, alpha=alpha, O=O, n=n, H=H, C=C)
    return out, cache


def gat_conv_bwd(cache, dout):
    """(dx, dW, datt_src, datt_dst, dbias) of gat_conv_fwd from dout = dLoss / dout.  Leaves dz, da_dst, da_src and dHf in the
    cache (what the kernels are compared with)."""
    c = cache
    n, H, C, row, col = c["n"], c["H"], c["C"], c["row"], c["colidx"]
    dO = np.asarray(dout, np.float64).reshape(n, H, C)
    r = np.einsum("nhc,nhc->nh", dO, c["O"])
    dalpha = np.empty(c["alpha"].shape)
    for s in range(0, len(col), 16384):                 # <dO[i,h,:], Hf[j,h,:]> per entry, in cache-sized pieces
        dalpha[s:s + 16384] = np.einsum("ehc,ehc->eh", dO[row[s:s + 16384]], c["Hf"][col[s:s + 16384]])
    dz = c["alpha"] * (dalpha - r[row]) * np.where(c["pos"], 1.0, c["slope"])
    da_dst, da_src = np.zeros((n, H)), np.zeros((n, H))
    np.add.at(da_dst, row, dz)
    np.add.at(da_src, col, dz)
    dHf = _per_head(c["rowptr"], col, n, c["alpha"], dO, transpose=True)
    dHf += da_src[:, :, None] * c["att_src"][None] + da_dst[:, :, None] * c["att_dst"][None]
    datt_src, datt_dst = np.einsum("nh,nhc->hc", da_src, c["Hf"]), np.einsum("nh,nhc->hc", da_dst, c["Hf"])
    dHf2 = dHf.reshape(n, H * C)
    c.update(dz=dz, da_dst=da_dst, da_src=da_src, dHf=dHf2)
    return dHf2 @ c["W"].T, c["x"].T @ dHf2, datt_src, datt_dst, dO.reshape(n, H * C).sum(0)


def device_score_sides(a_src32, a_dst32, rowptr, colidx):
    """The side of z of every entry as the device decides it: (a_src32[col] + a_dst32[row]) > 0 evaluated in float32."""
    a_src32, a_dst32 = np.asarray(a_src32, np.float32), np.asarray(a_dst32, np.float32)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(np.asarray(rowptr, np.int64)))
    z = a_src32[np.asarray(colidx, np.int64)] + a_dst32[row]
    assert z.dtype == np.float32
    return z > 0


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, argmax=None, heads=1):
    """gcn_bn_ref.model with the two convolutions replaced (on the pattern of `a` with PyG's remaining self-loops): same
    arguments, same result dict; masks["e1"], masks["e2"]: the score sides of the two convolutions."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    rp, ci = pattern(a, x.shape[0])
    conv = lambda k, inp: gat_conv_fwd(rp, ci, inp, q[f"conv{k}.lin.weight"].T, q[f"conv{k}.att_src"].reshape(heads, -1),
                                       q[f"conv{k}.att_dst"].reshape(heads, -1), q[f"conv{k}.bias"], 0.2, m.get(f"e{k}"))
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
    r.update(m1=p1, m2=p2, e1=k1["pos"], e2=k2["pos"], argmax=arg, pooled=P, y2=y2)
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    dy1, dw2, das2, dad2, g["conv2.bias"] = gat_conv_bwd(k2, dz2)
    g["conv2.lin.weight"], g["conv2.att_src"], g["conv2.att_dst"] = dw2.T, das2[None], dad2[None]
    dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    _, dw1, das1, dad1, g["conv1.bias"] = gat_conv_bwd(k1, dz1)
    g["conv1.lin.weight"], g["conv1.att_src"], g["conv1.att_dst"] = dw1.T, das1[None], dad1[None]
    return r

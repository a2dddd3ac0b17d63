"""float64 NumPy restatement of PyG's TransformerConv(in, C, heads=H, concat=True, beta, dropout=0, edge_dim=D, bias=True,
root_weight) (Shi et al., UniMP) and of gcnx.Transformer -- the reference's torch GCN (gcn_utills.py:795-853) with its two
GCNConv layers replaced by it, which reads the dca / proximity edge features the reference computes and drops
(gcn_utills.py:319-443; gcn.py:71) -- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient.  No torch.

The decomposed form the device uses (head h owns columns [h C, h C + C) of every H C wide block):

    P = x [W_q | W_k | W_v | W_s] + [b_q | b_k | b_v | b_s] = Q | K | V | S
    T_ij = e_ij W_e      k_ij = K[j] + T_ij      v_ij = V[j] + T_ij      score_ij,h = <Q[i,h,:], k_ij[h,:]> / sqrt(C)
    alpha = softmax over the stored entries of row i      O[i,h,:] = sum_j alpha_ij,h v_ij[h,:]      (no entries: O = 0)
    out = O | O + S | b S + (1 - b) O,  b_i = sigmoid(<w1, O_i> + <w2, S_i> + <w3, O_i - S_i>)

The pattern (rowptr, colidx) and e [nnz, D] are used as stored: no self-loop is added.  BatchNorm, PReLU, the max-pool, the head,
BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's; softmax, dot and sigmoid have no kink, so the
convolutions take no mask.  Parameters use PyG's key names and layouts: conv*.lin_key / lin_query / lin_value / lin_skip .weight
[H C, in] and .bias [H C], conv*.lin_edge.weight [H C, D], conv*.lin_beta.weight [1, 3 H C]."""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401
from gatv2_ref import TAIL_KEYS, stored_pattern  # noqa: F401

BLOCKS = ("lin_query", "lin_key", "lin_value", "lin_skip")          # the stored column blocks, in order


def conv_keys(edge_dim=None, beta=False, root_weight=True):
    """PyG's parameter names of one TransformerConv in its named_parameters() order."""
    lin = lambda k: (k + ".weight", k + ".bias")
    return lin("lin_key") + lin("lin_query") + lin("lin_value") + (("lin_edge.weight",) if edge_dim else ()) + \
        (lin("lin_skip") if root_weight else ()) + (("lin_beta.weight",) if beta else ())


def keys(edge_dim=None, beta=False, root_weight=True):
    """The state_dict keys of gcnx.Transformer in order."""
    return tuple(f"conv{k}.{t}" for k in (1, 2) for t in conv_keys(edge_dim, beta, root_weight)) + TAIL_KEYS


def init_params(f_in, h=64, edge_dim=None, beta=False, root_weight=True, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = _gcn_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 5000)
    for k, fi in (("conv1", f_in), ("conv2", h)):
        for s in BLOCKS[:4 if root_weight else 3]:
            p[f"{k}.{s}.weight"] = rng.uniform(-1, 1, (h, fi)) / np.sqrt(fi)
            p[f"{k}.{s}.bias"] = rng.uniform(-0.1, 0.1, h)
        if edge_dim:
            p[f"{k}.lin_edge.weight"] = rng.uniform(-1, 1, (h, edge_dim)) / np.sqrt(edge_dim)
        if beta:
            p[f"{k}.lin_beta.weight"] = rng.uniform(-1, 1, (1, 3 * h)) / np.sqrt(3 * h)
    return {k: p[k] for k in keys(edge_dim, beta, root_weight)}


def sigmoid(a):
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))


def conv_fwd(rowptr, colidx, P, heads, c, e=None, We=None, skip=None, w_beta=None):
    """P [n, >= 3 HC] = Q | K | V in its first 3 HC columns; e [nnz, D] and We [D, HC] or both None; skip [n, HC] or None; w_beta
    [3 HC] = w1 | w2 | w3 or None (needs skip).  Returns (out [n, HC], cache); the cache holds alpha [nnz, heads], O, score."""
    P = np.asarray(P, np.float64)
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n, hc = P.shape[0], heads * c
    row = np.repeat(np.arange(n), np.diff(rowptr))
    nnz = len(colidx)
    Q, K, V = P[:, :hc], P[:, hc:2 * hc], P[:, 2 * hc:3 * hc]
    T = np.zeros((nnz, hc))
    if e is not None:
        e, We = np.asarray(e, np.float64), np.asarray(We, np.float64)
        T = e @ We
    s = 1.0 / np.sqrt(c)
    kk, vv = K[colidx] + T, V[colidx] + T
    score = (Q[row] * kk).reshape(nnz, heads, c).sum(2) * s
    mx = np.full((n, heads), -np.inf)
    np.maximum.at(mx, row, score)
    ex = np.exp(score - mx[row])
    den = np.zeros((n, heads))
    np.add.at(den, row, ex)
    alpha = ex / den[row]
    O = np.zeros((n, hc))
    np.add.at(O, row, (alpha[:, :, None] * vv.reshape(nnz, heads, c)).reshape(nnz, hc))
    b, S = None, None
    if skip is not None:
        S = np.asarray(skip, np.float64)
    if w_beta is not None:
        w = np.asarray(w_beta, np.float64).reshape(3, hc)
        b = sigmoid(O @ w[0] + S @ w[1] + (O - S) @ w[2])
        out = b[:, None] * S + (1.0 - b[:, None]) * O
    elif S is not None:
        out = O + S
    else:
        out = O.copy()
    cache = dict(rowptr=rowptr, colidx=colidx, row=row, n=n, heads=heads, c=c, s=s, e=e, Q=Q, kk=kk, vv=vv, score=score, alpha=alpha, O=O,
                 S=S, b=b, w_beta=None if w_beta is None else np.asarray(w_beta, np.float64).reshape(3, hc))
    return out, cache


def conv_bwd(cache, dout):
    """{dQ, dK, dV, dS (None without skip), dWe [D, HC] (None without edge features), dw_beta [3 HC] (None without beta), dO,
    dscore [nnz, heads]} from dout = dLoss / dout."""
    k = cache
    n, heads, c, row, col, s = k["n"], k["heads"], k["c"], k["row"], k["colidx"], k["s"]
    hc, nnz = heads * c, len(col)
    d = np.asarray(dout, np.float64)
    O, S = k["O"], k["S"]
    dw_beta = None
    if k["b"] is not None:
        b, w = k["b"], k["w_beta"]
        g = ((d * (S - O)).sum(1)) * b * (1.0 - b)
        dO = (1.0 - b)[:, None] * d + g[:, None] * (w[0] + w[2])
        dS = b[:, None] * d + g[:, None] * (w[1] - w[2])
        dw_beta = np.concatenate([g @ O, g @ S, g @ (O - S)])
    else:
        dO, dS = d, (d.copy() if S is not None else None)
    r = (dO * O).reshape(n, heads, c).sum(2)
    dalpha = (dO[row] * k["vv"]).reshape(nnz, heads, c).sum(2)
    dscore = k["alpha"] * (dalpha - r[row])
    rep = lambda a: np.repeat(a, c, axis=1)                          # [nnz, heads] -> [nnz, HC]
    dkk = s * rep(dscore) * k["Q"][row]
    dvv = rep(k["alpha"]) * dO[row]
    dQ, dK, dV = np.zeros((n, hc)), np.zeros((n, hc)), np.zeros((n, hc))
    np.add.at(dQ, row, s * rep(dscore) * k["kk"])
    np.add.at(dK, col, dkk)
    np.add.at(dV, col, dvv)
    dWe = k["e"].T @ (dkk + dvv) if k["e"] is not None else None
    return dict(dQ=dQ, dK=dK, dV=dV, dS=dS, dWe=dWe, dw_beta=dw_beta, dO=dO, dscore=dscore)


def split(p, k):
    """PyG's tensors of conv{k} -> the stored form: (W [in, 3 HC or 4 HC], b likewise, We [D, HC] or None, w_beta [3 HC] or None)."""
    c = f"conv{k}."
    blocks = [s for s in BLOCKS if c + s + ".weight" in p]
    W = np.hstack([np.asarray(p[c + s + ".weight"], np.float64).T for s in blocks])
    b = np.concatenate([np.asarray(p[c + s + ".bias"], np.float64) for s in blocks])
    We = np.asarray(p[c + "lin_edge.weight"], np.float64).T if c + "lin_edge.weight" in p else None
    wb = np.asarray(p[c + "lin_beta.weight"], np.float64).reshape(-1) if c + "lin_beta.weight" in p else None
    return W, b, We, wb


def layer_fwd(rowptr, colidx, x, W, b, We, w_beta, heads, hc, e=None):
    """The layer from the stored form: W [in, 3 HC or 4 HC] (4 HC: the last block is W_s), b likewise (or None), We [D, HC] or
    None, w_beta [3 HC] or None."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    root = W.shape[1] == 4 * hc
    P = x @ W
    if b is not None:
        P = P + np.asarray(b, np.float64)
    out, cache = conv_fwd(rowptr, colidx, P, heads, hc // heads, e if We is not None else None, We, P[:, 3 * hc:] if root else None, w_beta)
    cache.update(x=x, W=W, P=P, hc=hc)
    return out, cache


def layer_bwd(cache, dout):
    """{x, W, b, We, w_beta}: the gradients of layer_fwd's operands."""
    r = conv_bwd(cache, dout)
    dP = np.hstack([r["dQ"], r["dK"], r["dV"]] + ([r["dS"]] if r["dS"] is not None else []))
    cache["dP"] = dP
    return dict(x=dP @ cache["W"].T, W=cache["x"].T @ dP, b=dP.sum(0), We=r["dWe"], w_beta=r["dw_beta"])


def join(d, k, hc):
    """layer_bwd's gradients of conv{k} under PyG's names and layouts."""
    c = f"conv{k}."
    out = {}
    for i, s in enumerate(BLOCKS[:d["W"].shape[1] // hc]):
        out[c + s + ".weight"], out[c + s + ".bias"] = d["W"][:, i * hc:(i + 1) * hc].T, d["b"][i * hc:(i + 1) * hc]
    if d["We"] is not None:
        out[c + "lin_edge.weight"] = d["We"].T
    if d["w_beta"] is not None:
        out[c + "lin_beta.weight"] = d["w_beta"][None]
    return out


def model(x, rowptr, colidx, e, graph_ptr, p, heads=1, y=None, denom=None, masks=None, argmax=None):
    """gcn_bn_ref.model with the two convolutions replaced, on the pattern and e as given: same result dict."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    hc = q["batch_norm_1.weight"].shape[0]

    def conv(k, inp):
        W, b, We, wb = split(q, k)
        return layer_fwd(rowptr, colidx, inp, W, b, We, wb, heads, hc, e)

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
    r.update(m1=p1, m2=p2, argmax=arg, pooled=P, y2=y2, conv1=k1, conv2=k2)
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    d2 = layer_bwd(k2, dz2)
    g.update(join(d2, 2, hc))
    dzb1, g["prelu_1.weight"] = prelu_bwd(d2["x"], zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    g.update(join(layer_bwd(k1, dz1), 1, hc))
    return r

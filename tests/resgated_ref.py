"""float64 NumPy restatement of PyG's ResGatedGraphConv(in, H, act=Sigmoid(), edge_dim=D, root_weight, bias=True), aggr = add
(Bresson & Laurent's GatedGCN), and of gcnx.ResGated -- the reference's torch GCN (gcn_utills.py:795-853) with its two GCNConv
layers replaced by it, which reads the dca / proximity edge features the reference computes and drops (gcn_utills.py:319-443;
gcn.py:71) -- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient.  No torch.

The decomposed form the device uses (every Linear of the concatenation [x ‖ e_ij] is a sum of two products):

    P = x [W_k | W_q | W_v | W_s] + [b_k | b_q | b_v | 0] = K | Q | V | S
    a_ij = K[i] + Q[j] + e_ij (W_ke + W_qe)     g_ij = sigmoid(a_ij)     m_ij = V[j] + e_ij W_ve
    out[i] = S[i] + bias + sum_j g_ij * m_ij            (row i = target, its stored entries j = sources; no entries: S[i] + bias)

The pattern (rowptr, colidx) and e [nnz, D] are used as stored: no self-loop is added.  BatchNorm, PReLU, the max-pool, the head,
BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's; the sigmoid has no kink, so the convolutions take no
mask.  Parameters use PyG's key names and layouts: conv*.bias [H], conv*.lin_key / lin_query / lin_value .weight [H, in + D] =
[node block ‖ edge block] and .bias [H], conv*.lin_skip.weight [H, in] (with root_weight)."""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401
from gatv2_ref import TAIL_KEYS, stored_pattern  # noqa: F401

LINS = ("lin_key", "lin_query", "lin_value")
CONV_PARTS = ("bias", "lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
              "lin_skip.weight")


def keys(root_weight=True):
    """The state_dict keys of gcnx.ResGated in order (lin_skip.weight only with root_weight; edge_dim changes shapes, not keys)."""
    parts = CONV_PARTS if root_weight else CONV_PARTS[:-1]
    return tuple(f"conv{k}.{t}" for k in (1, 2) for t in parts) + TAIL_KEYS


def init_params(f_in, h=64, edge_dim=None, root_weight=True, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = _gcn_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 4000)
    d = edge_dim or 0
    for k, fi in (("conv1", f_in), ("conv2", h)):
        p[f"{k}.bias"] = rng.uniform(-0.1, 0.1, h)
        for s in LINS:
            p[f"{k}.{s}.weight"] = rng.uniform(-1, 1, (h, fi + d)) / np.sqrt(fi + d)
            p[f"{k}.{s}.bias"] = rng.uniform(-0.1, 0.1, h)
        if root_weight:
            p[f"{k}.lin_skip.weight"] = rng.uniform(-1, 1, (h, fi)) / np.sqrt(fi)
    return {k: p[k] for k in keys(root_weight)}


def sigmoid(a):
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))


def conv_fwd(rowptr, colidx, P, H, e=None, We=None, skip=None, bias=None):
    """P [n, >= 3 H] = K | Q | V in its first 3 H columns; e [nnz, D] and We [D, 3 H] = W_ke | W_qe | W_ve or both None; skip
    [n, H] or None; bias [H] or None.  Returns (out [n, H], cache)."""
    P = np.asarray(P, np.float64)
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n = P.shape[0]
    row = np.repeat(np.arange(n), np.diff(rowptr))
    K, Q, V = P[:, :H], P[:, H:2 * H], P[:, 2 * H:3 * H]
    a, m = K[row] + Q[colidx], V[colidx].copy()
    if e is not None:
        e, We = np.asarray(e, np.float64), np.asarray(We, np.float64)
        a = a + e @ (We[:, :H] + We[:, H:2 * H])
        m = m + e @ We[:, 2 * H:]
    g = sigmoid(a)
    out = np.zeros((n, H))
    np.add.at(out, row, g * m)
    if skip is not None:
        out = out + np.asarray(skip, np.float64)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out, dict(rowptr=rowptr, colidx=colidx, row=row, n=n, H=H, e=e, a=a, g=g, m=m, has_skip=skip is not None)


def conv_bwd(cache, dout):
    """{dK, dQ, dV, dS (None without skip), dbias, dWe [D, 3 H] (None without edge features; its first two blocks equal)} from
    dout = dLoss / dout.  Leaves da and dm [nnz, H] in the cache."""
    c = cache
    n, H, row, col = c["n"], c["H"], c["row"], c["colidx"]
    dO = np.asarray(dout, np.float64)
    da = dO[row] * c["m"] * c["g"] * (1.0 - c["g"])
    dm = dO[row] * c["g"]
    dK, dQ, dV = np.zeros((n, H)), np.zeros((n, H)), np.zeros((n, H))
    np.add.at(dK, row, da)
    np.add.at(dQ, col, da)
    np.add.at(dV, col, dm)
    dWe = None
    if c["e"] is not None:
        gate = c["e"].T @ da
        dWe = np.hstack([gate, gate, c["e"].T @ dm])
    c.update(da=da, dm=dm)
    return dict(dK=dK, dQ=dQ, dV=dV, dS=dO.copy() if c["has_skip"] else None, dbias=dO.sum(0), dWe=dWe)


def split(p, k, edge_dim=None):
    """PyG's tensors of conv{k} -> the stored form: (W [in, 3 H or 4 H], b [3 H], We [D, 3 H] or None, bias [H], root_weight)."""
    c, d = f"conv{k}.", edge_dim or 0
    w = [np.asarray(p[c + s + ".weight"], np.float64) for s in LINS]
    f = w[0].shape[1] - d
    root = c + "lin_skip.weight" in p
    node = [t[:, :f].T for t in w] + ([np.asarray(p[c + "lin_skip.weight"], np.float64).T] if root else [])
    We = np.hstack([t[:, f:].T for t in w]) if d else None
    return np.hstack(node), np.concatenate([np.asarray(p[c + s + ".bias"], np.float64) for s in LINS]), We, np.asarray(p[c + "bias"], np.float64), root


def layer_fwd(rowptr, colidx, x, W, b, We, bias, e=None):
    """The layer from the stored form: W [in, 3 H or 4 H] (4 H: the last block is W_s), b [3 H], We [D, 3 H] or None."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    H = np.asarray(b).shape[0] // 3
    root = W.shape[1] == 4 * H
    P = x @ W
    P[:, :3 * H] += np.asarray(b, np.float64)
    out, cache = conv_fwd(rowptr, colidx, P, H, e if We is not None else None, We, P[:, 3 * H:] if root else None, bias)
    cache.update(x=x, W=W, P=P)
    return out, cache


def layer_bwd(cache, dout):
    """{x, W, b, We, bias}: the gradients of layer_fwd's operands."""
    r = conv_bwd(cache, dout)
    dP = np.hstack([r["dK"], r["dQ"], r["dV"]] + ([r["dS"]] if r["dS"] is not None else []))
    H = cache["H"]
    cache["dP"] = dP
    return dict(x=dP @ cache["W"].T, W=cache["x"].T @ dP, b=dP[:, :3 * H].sum(0), We=r["dWe"], bias=r["dbias"])


def join(d, k, edge_dim=None):
    """layer_bwd's gradients of conv{k} under PyG's names and layouts (dW_ke == dW_qe)."""
    c, H = f"conv{k}.", d["b"].shape[0] // 3
    out = {c + "bias": d["bias"]}
    for i, s in enumerate(LINS):
        blocks = [d["W"][:, i * H:(i + 1) * H].T] + ([d["We"][:, i * H:(i + 1) * H].T] if edge_dim else [])
        out[c + s + ".weight"], out[c + s + ".bias"] = np.hstack(blocks), d["b"][i * H:(i + 1) * H]
    if d["W"].shape[1] == 4 * H:
        out[c + "lin_skip.weight"] = d["W"][:, 3 * H:].T
    return out


def model(x, rowptr, colidx, e, graph_ptr, p, y=None, denom=None, masks=None, argmax=None, edge_dim=None):
    """gcn_bn_ref.model with the two convolutions replaced, on the pattern and e as given: same result dict."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)

    def conv(k, inp):
        W, b, We, bias, _ = split(q, k, edge_dim)
        return layer_fwd(rowptr, colidx, inp, W, b, We, bias, e)

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
    g.update(join(d2, 2, edge_dim))
    dzb1, g["prelu_1.weight"] = prelu_bwd(d2["x"], zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    g.update(join(layer_bwd(k1, dz1), 1, edge_dim))
    return r

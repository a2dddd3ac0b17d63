"""float64 NumPy restatement of SAGEConv(aggr="mean") and of gcnx.SAGE -- the reference's torch GCN (gcn_utills.py:795-853)
with its two GCNConv layers replaced by SAGEConv, as the comment above them suggests (gcn_utills.py:804-806) -- with
BCEWithLogitsLoss: forward, loss, accuracy, every gradient.  No torch.

    out_i = mean_{j in N(i)} x_j W_l^T + b + x_i W_r^T        N(i): the stored entries of row i (row = target), as stored:
                                                              no self-loop is added or removed; an empty row aggregates to 0

BatchNorm, PReLU, the max-pool, the head, BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's.
Parameters use the torch key names and layouts: conv*.lin_l.weight / conv*.lin_r.weight [out, in], conv*.lin_l.bias [out].
"""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401

CONV_KEYS = ("conv1.lin_l.weight", "conv1.lin_l.bias", "conv1.lin_r.weight",
             "conv2.lin_l.weight", "conv2.lin_l.bias", "conv2.lin_r.weight")
KEYS = CONV_KEYS + ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
                    "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
                    "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")


def init_params(f_in, h=64, seed=0):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = _gcn_params(f_in, h, seed)
    for k in ("conv1.bias", "conv1.lin.weight", "conv2.bias", "conv2.lin.weight"):
        del p[k]
    rng = np.random.default_rng(seed + 1000)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for c, fi in (("conv1", f_in), ("conv2", h)):
        p[f"{c}.lin_l.weight"], p[f"{c}.lin_r.weight"] = u(1 / np.sqrt(fi), h, fi), u(1 / np.sqrt(fi), h, fi)
        p[f"{c}.lin_l.bias"] = u(0.1, h)
    return {k: p[k] for k in KEYS}


def mean_operator(a, n=None):
    """The row-mean operator of the stored pattern of `a` (scipy; row = target): 1 / (entries of the row) on every stored
    entry, values ignored, duplicates counted once, rows without entries left empty."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a, shape=None if n is None else (n, n)).copy()
    a.sum_duplicates()
    a.data[:] = 1.0
    deg = np.diff(a.indptr)
    a.data[:] = np.repeat(1.0 / np.maximum(deg, 1), deg)
    return a


def sage_conv_fwd(A, x, w_l, w_r, b):
    """A: the aggregation operator (scipy CSR, any values); w_l, w_r [out, in] (w_r None: no root weight); b [out] or None.
    Returns (out, S = A x)."""
    x = np.asarray(x, np.float64)
    s = A @ x
    out = s @ np.asarray(w_l, np.float64).T
    if w_r is not None:
        out = out + x @ np.asarray(w_r, np.float64).T
    if b is not None:
        out = out + np.asarray(b, np.float64)
    return out, s


def sage_conv_bwd(A, x, s, w_l, w_r, dz):
    """(dx, dW_l, dW_r, db) of sage_conv_fwd from dz = dLoss / dout (dW_r None without a root weight)."""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    dx = A.T @ (dz @ np.asarray(w_l, np.float64))
    dwr = None
    if w_r is not None:
        dx = dx + dz @ np.asarray(w_r, np.float64)
        dwr = dz.T @ x
    return dx, dz.T @ s, dwr, dz.sum(0)


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, argmax=None):
    """gcn_bn_ref.model with the two convolutions replaced and no self-loops added: same arguments, same result dict."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    A = mean_operator(a, x.shape[0])
    z1, s1 = sage_conv_fwd(A, x, q["conv1.lin_l.weight"], q["conv1.lin_r.weight"], q["conv1.lin_l.bias"])
    zb1, c1 = bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2, s2 = sage_conv_fwd(A, y1, q["conv2.lin_l.weight"], q["conv2.lin_r.weight"], q["conv2.lin_l.bias"])
    zb2, c2 = bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = prelu_fwd(zb2, q["prelu_2.weight"][0], m.get("m2"))
    arg = first_argmax(y2, graph_ptr) if argmax is None else np.asarray(argmax, np.int64)
    cols = np.arange(y2.shape[1])
    P = np.stack([y2[arg[g], cols] if graph_ptr[g + 1] > graph_ptr[g] else np.zeros(y2.shape[1])
                  for g in range(len(graph_ptr) - 1)])
    r = head(P, p, y, denom, m)
    r.update(m1=p1, m2=p2, argmax=arg, pooled=P, y2=y2)
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    dy1, g["conv2.lin_l.weight"], g["conv2.lin_r.weight"], g["conv2.lin_l.bias"] = sage_conv_bwd(
        A, y1, s2, q["conv2.lin_l.weight"], q["conv2.lin_r.weight"], dz2)
    dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    _, g["conv1.lin_l.weight"], g["conv1.lin_r.weight"], g["conv1.lin_l.bias"] = sage_conv_bwd(
        A, x, s1, q["conv1.lin_l.weight"], q["conv1.lin_r.weight"], dz1)
    return r

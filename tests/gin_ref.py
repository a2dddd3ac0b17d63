"""float64 NumPy restatement of GINConv(Sequential(Linear, ReLU, Linear), train_eps) and of gcnx.GIN -- the reference's torch
GCN (gcn_utills.py:795-853) with its two GCNConv layers replaced by GINConv, in the slot its author left open
(gcn_utills.py:804-806) -- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient, eps included.  No torch.

    out_i = MLP((1 + eps) x_i + sum_{j in N(i)} x_j)          N(i): the stored entries of row i (row = target), as stored:
    MLP = Linear -> ReLU -> Linear                            no self-loop is added or removed, values are ignored

BatchNorm, PReLU, the max-pool, the head, BCE and the kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's; ``masks``
also takes ``relu1`` / ``relu2``, the device's side of the two inner ReLUs (bool [N, H], True = the ReLU passes).
Parameters use the torch key names and layouts: conv*.eps [1], conv*.nn.{0,2}.weight [out, in], conv*.nn.{0,2}.bias [out].
"""
import numpy as np

from gcn_bn_ref import bn_bwd, bn_fwd, device_prelu_sides, first_argmax, head, init_params as _gcn_params, prelu_bwd, prelu_fwd, sgd  # noqa: F401

CONV_KEYS = ("conv1.eps", "conv1.nn.0.weight", "conv1.nn.0.bias", "conv1.nn.2.weight", "conv1.nn.2.bias",
             "conv2.eps", "conv2.nn.0.weight", "conv2.nn.0.bias", "conv2.nn.2.weight", "conv2.nn.2.bias")
KEYS = CONV_KEYS + ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
                    "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
                    "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")
EPS_KEYS = ("conv1.eps", "conv2.eps")


def init_params(f_in, h=64, seed=0, eps=(0.0, 0.0)):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = _gcn_params(f_in, h, seed)
    for k in ("conv1.bias", "conv1.lin.weight", "conv2.bias", "conv2.lin.weight"):
        del p[k]
    rng = np.random.default_rng(seed + 2000)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for i, (c, fi) in enumerate((("conv1", f_in), ("conv2", h))):
        p[f"{c}.eps"] = np.array([float(eps[i])])
        p[f"{c}.nn.0.weight"], p[f"{c}.nn.0.bias"] = u(1 / np.sqrt(fi), h, fi), u(0.1, h)
        p[f"{c}.nn.2.weight"], p[f"{c}.nn.2.bias"] = u(1 / np.sqrt(h), h, h), u(0.1, h)
    return {k: p[k] for k in KEYS}


def sum_operator(a, n=None):
    """The stored pattern of `a` (scipy; row = target) as all ones: values ignored, duplicates counted once."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a, shape=None if n is None else (n, n)).copy()
    a.sum_duplicates()
    a.data[:] = 1.0
    return a


def gin_conv_fwd(A, x, eps, w_a, b_a, w_b, b_b, relu_mask=None):
    """A: the aggregation operator (scipy CSR); w_a [hidden, in], w_b [out, hidden]; b_a, b_b may be None.  relu_mask (bool,
    the shape of U; None: the pre-activation's own sign) picks the side of the inner ReLU.
    Returns (out, T = (1 + eps) x + A x, U = relu(T w_a^T + b_a), mask)."""
    x = np.asarray(x, np.float64)
    t = (1.0 + float(np.asarray(eps).reshape(-1)[0])) * x + A @ x
    v = t @ np.asarray(w_a, np.float64).T
    if b_a is not None:
        v = v + np.asarray(b_a, np.float64)
    mask = v > 0 if relu_mask is None else np.asarray(relu_mask, bool)
    u = np.where(mask, v, 0.0)
    out = u @ np.asarray(w_b, np.float64).T
    if b_b is not None:
        out = out + np.asarray(b_b, np.float64)
    return out, t, u, mask


def gin_conv_bwd(A, x, eps, t, u, mask, w_a, w_b, dz):
    """(dx, d eps [1], dW_a, db_a, dW_b, db_b) of gin_conv_fwd from dz = dLoss / dout; mask: the ReLU mask of the forward."""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    du = np.where(mask, dz @ np.asarray(w_b, np.float64), 0.0)
    dt = du @ np.asarray(w_a, np.float64)
    dx = (1.0 + float(np.asarray(eps).reshape(-1)[0])) * dt + A.T @ dt
    return dx, np.array([np.sum(x * dt)]), du.T @ t, du.sum(0), dz.T @ u, dz.sum(0)


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, argmax=None):
    """gcn_bn_ref.model with the two convolutions replaced and no self-loops added: same arguments, same result dict
    (+ relu1 / relu2, the inner ReLU masks used)."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    A = sum_operator(a, x.shape[0])
    cw = lambda c: (q[f"{c}.eps"], q[f"{c}.nn.0.weight"], q[f"{c}.nn.0.bias"], q[f"{c}.nn.2.weight"], q[f"{c}.nn.2.bias"])
    z1, t1, u1, r1 = gin_conv_fwd(A, x, *cw("conv1"), relu_mask=m.get("relu1"))
    zb1, c1 = bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2, t2, u2, r2 = gin_conv_fwd(A, y1, *cw("conv2"), relu_mask=m.get("relu2"))
    zb2, c2 = bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = prelu_fwd(zb2, q["prelu_2.weight"][0], m.get("m2"))
    arg = first_argmax(y2, graph_ptr) if argmax is None else np.asarray(argmax, np.int64)
    cols = np.arange(y2.shape[1])
    P = np.stack([y2[arg[g], cols] if graph_ptr[g + 1] > graph_ptr[g] else np.zeros(y2.shape[1])
                  for g in range(len(graph_ptr) - 1)])
    r = head(P, p, y, denom, m)
    r.update(m1=p1, m2=p2, relu1=r1, relu2=r2, argmax=arg, pooled=P, y2=y2)
    if y is None:
        return r
    g = r["grads"]
    dy2 = np.zeros_like(y2)
    for gi in range(len(graph_ptr) - 1):
        if graph_ptr[gi + 1] > graph_ptr[gi]:
            dy2[arg[gi], cols] += r["dP"][gi]
    dzb2, g["prelu_2.weight"] = prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    (dy1, g["conv2.eps"], g["conv2.nn.0.weight"], g["conv2.nn.0.bias"], g["conv2.nn.2.weight"], g["conv2.nn.2.bias"]) = gin_conv_bwd(
        A, y1, q["conv2.eps"], t2, u2, r2, q["conv2.nn.0.weight"], q["conv2.nn.2.weight"], dz2)
    dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    (_, g["conv1.eps"], g["conv1.nn.0.weight"], g["conv1.nn.0.bias"], g["conv1.nn.2.weight"], g["conv1.nn.2.bias"]) = gin_conv_bwd(
        A, x, q["conv1.eps"], t1, u1, r1, q["conv1.nn.0.weight"], q["conv1.nn.2.weight"], dz1)
    return r

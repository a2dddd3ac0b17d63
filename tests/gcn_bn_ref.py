"""float64 NumPy restatement of the reference's torch GCN (src/utilities/gcn_utills.py:795-853) with BCEWithLogitsLoss:
forward, loss, accuracy, every gradient and an SGD step (the spec of record is DESIGN.md, "torch GCN").  No torch.

Kink sides: every non-smooth point can be evaluated on the DEVICE's side -- ``masks`` = {"m1", "m2", "m3", "m4"} (bool
arrays, True = the PReLU input counts as positive) and ``argmax`` [B, H] (the max-pool rows).  A PReLU input or a pooled
maximum within an fp32 rounding of a kink then takes the device's branch, so that the comparison measures arithmetic,
not a coin toss.

Parameters use the torch key names and layouts (state_dict): conv*.lin.weight [out, in], linear_*.weight [out, in],
prelu_*.weight [1], batch_norm_*.weight / .bias.
"""
import numpy as np

EPS = 1e-5
KEYS = ("conv1.bias", "conv1.lin.weight", "conv2.bias", "conv2.lin.weight", "linear_1.weight", "linear_1.bias",
        "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight", "prelu_3.weight", "prelu_4.weight",
        "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight", "batch_norm_2.bias",
        "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")


def init_params(f_in, h=64, seed=0):
    """Random parameters of every kind (not torch's initialisation: slopes, gammas and betas away from their defaults so
    that every gradient term is exercised)."""
    rng = np.random.default_rng(seed)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    return {"conv1.bias": u(0.1, h), "conv1.lin.weight": u(np.sqrt(6 / (f_in + h)), h, f_in),
            "conv2.bias": u(0.1, h), "conv2.lin.weight": u(np.sqrt(6 / (2 * h)), h, h),
            "linear_1.weight": u(1 / np.sqrt(h), h, h), "linear_1.bias": u(1 / np.sqrt(h), h),
            "linear_2.weight": u(1 / np.sqrt(h), 1, h), "linear_2.bias": u(1 / np.sqrt(h), 1),
            "prelu_1.weight": np.array([0.25]), "prelu_2.weight": np.array([0.1]), "prelu_3.weight": np.array([0.3]),
            "prelu_4.weight": np.array([0.2]),
            "batch_norm_1.weight": 1 + u(0.2, h), "batch_norm_1.bias": u(0.2, h),
            "batch_norm_2.weight": 1 + u(0.2, h), "batch_norm_2.bias": u(0.2, h),
            "batch_norm_3.weight": 1 + u(0.2, h), "batch_norm_3.bias": u(0.2, h),
            "batch_norm_4.weight": 1 + u(0.2, 1), "batch_norm_4.bias": u(0.2, 1)}


def pyg_norm(a, n):
    """A^ = D^-1/2 (A + I_missing) D^-1/2 of the pattern of `a` (scipy, row = target, column = source; values
    ignored), as PyG's gcn_norm with add_remaining_self_loops and no edge_weight."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a, shape=(n, n)).copy()
    a.data[:] = 1.0
    a.sum_duplicates()
    a.data[:] = 1.0
    diag = a.diagonal()
    a = sp.csr_matrix(a + sp.diags(np.where(diag == 0, 1.0, 0.0)))
    deg = np.asarray(a.sum(1)).ravel()
    dinv = 1.0 / np.sqrt(deg)
    return sp.csr_matrix(sp.diags(dinv) @ a @ sp.diags(dinv))


def targets(y):
    """t of BCEWithLogits: y[:, 1] of one-hot [B, 2], y[:, 0] of [B, 1], y of [B]."""
    y = np.asarray(y, np.float64)
    return y[:, 1] if y.ndim == 2 and y.shape[1] == 2 else y.reshape(-1)


def bn_fwd(z, g, b, eps=EPS):
    if z.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(z.shape)}")
    mu, var = z.mean(0), z.var(0)
    xh = (z - mu) / np.sqrt(var + eps)
    return g * xh + b, (xh, var)


def bn_bwd(dzb, cache, g, eps=EPS):
    xh, var = cache
    n = dzb.shape[0]
    db, dg = dzb.sum(0), (dzb * xh).sum(0)
    return g / np.sqrt(var + eps) * (dzb - db / n - xh * dg / n), dg, db


def prelu_fwd(zb, a, pos=None):
    pos = zb > 0 if pos is None else np.asarray(pos, bool)
    return np.where(pos, zb, a * zb), pos


def prelu_bwd(dy, zb, a, pos):
    return np.where(pos, dy, a * dy), np.array([np.sum(dy * np.where(pos, 0.0, zb))])


def first_argmax(y, graph_ptr):
    b, f = len(graph_ptr) - 1, y.shape[1]
    arg = np.zeros((b, f), np.int64)
    for g in range(b):
        lo, hi = graph_ptr[g], graph_ptr[g + 1]
        arg[g] = lo + np.argmax(y[lo:hi], 0) if hi > lo else lo
    return arg


def bce(out, t, denom):
    z = out.reshape(-1)
    loss = np.sum(np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))) / denom
    hits = float(np.sum((z > 0) == (t > 0.5)))
    dout = (1 / (1 + np.exp(-z)) - t) / denom
    return loss, hits, dout.reshape(-1, 1)


def head(P, p, y=None, denom=None, masks=None):
    """The post-pool half (Linear·BN·PReLU twice) + BCE: the arithmetic of gcnx_bn_prelu_bce_head.  Returns a dict with
    out, probs and, with labels, loss, hits, dP and the head's parameter gradients (torch keys)."""
    m = masks or {}
    P = np.asarray(P, np.float64)
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    z3 = P @ q["linear_1.weight"].T + q["linear_1.bias"]
    zb3, c3 = bn_fwd(z3, q["batch_norm_3.weight"], q["batch_norm_3.bias"])
    y3, p3 = prelu_fwd(zb3, q["prelu_3.weight"][0], m.get("m3"))
    z4 = y3 @ q["linear_2.weight"].T + q["linear_2.bias"]
    zb4, c4 = bn_fwd(z4, q["batch_norm_4.weight"], q["batch_norm_4.bias"])
    out, p4 = prelu_fwd(zb4, q["prelu_4.weight"][0], m.get("m4"))
    r = {"out": out, "probs": 1 / (1 + np.exp(-out)), "m3": p3, "m4": p4}
    if y is None:
        return r
    t = targets(y)
    denom = float(denom or P.shape[0])
    r["loss"], r["hits"], dout = bce(out, t, denom)
    g = {}
    dzb4, g["prelu_4.weight"] = prelu_bwd(dout, zb4, q["prelu_4.weight"][0], p4)
    dz4, g["batch_norm_4.weight"], g["batch_norm_4.bias"] = bn_bwd(dzb4, c4, q["batch_norm_4.weight"])
    g["linear_2.weight"], g["linear_2.bias"] = dz4.T @ y3, dz4.sum(0)
    dy3 = dz4 @ q["linear_2.weight"]
    dzb3, g["prelu_3.weight"] = prelu_bwd(dy3, zb3, q["prelu_3.weight"][0], p3)
    dz3, g["batch_norm_3.weight"], g["batch_norm_3.bias"] = bn_bwd(dzb3, c3, q["batch_norm_3.weight"])
    g["linear_1.weight"], g["linear_1.bias"] = dz3.T @ P, dz3.sum(0)
    r["dP"] = dz3 @ q["linear_1.weight"]
    r["grads"] = g
    return r


def bn_act_pool_bwd(dP, argmax, z, gamma, beta, alpha, n_graph_ptr, pos=None, eps=EPS):
    """Backward of BN·PReLU(shared or per-feature slope)·max-pool from dPooled: (dZ, dgamma, dbeta, dalpha).  `pos`: the
    device's PReLU sides (default: this function's own)."""
    z = np.asarray(z, np.float64)
    zb, c = bn_fwd(z, gamma, beta, eps)
    pos = zb > 0 if pos is None else np.asarray(pos, bool)
    dy = np.zeros_like(z)
    cols = np.arange(z.shape[1])
    for g in range(len(n_graph_ptr) - 1):
        if n_graph_ptr[g + 1] > n_graph_ptr[g]:
            dy[argmax[g], cols] += dP[g]
    alpha = np.asarray(alpha, np.float64)
    dzb = np.where(pos, dy, alpha * dy)
    term = dy * np.where(pos, 0.0, zb)
    dalpha = np.array([term.sum()]) if alpha.size == 1 else term.sum(0)
    dz, dg, db = bn_bwd(dzb, c, gamma, eps)
    return dz, dg, db, dalpha


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, argmax=None):
    """Forward (+ loss, accuracy and every gradient with labels) of the whole model.  a: scipy adjacency (row = target);
    graph_ptr [B + 1].  Returns a dict: out [B, 1], probs, loss, hits, grads {torch key: array}, the kink sides it used
    (m1..m4, argmax), the pooled rows and the second layer's activation y2 [N, H].  The adjacency may be directed: A^ is
    then not symmetric and the backward pass aggregates with A^T."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    A = pyg_norm(a, n)
    z1 = A @ (x @ q["conv1.lin.weight"].T) + q["conv1.bias"]
    zb1, c1 = bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2 = A @ (y1 @ q["conv2.lin.weight"].T) + q["conv2.bias"]
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
    g["conv2.bias"] = dz2.sum(0)
    t2 = A.T @ dz2
    g["conv2.lin.weight"] = t2.T @ y1
    dy1 = t2 @ q["conv2.lin.weight"]
    dzb1, g["prelu_1.weight"] = prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    g["conv1.bias"] = dz1.sum(0)
    g["conv1.lin.weight"] = (A.T @ dz1).T @ x
    return r


def sgd(p, grads, lr):
    return {k: np.asarray(p[k], np.float64) - lr * grads[k] for k in p}


def device_prelu_sides(z, mean, inv, gamma, beta):
    """The device's PReLU branch after gcnx_bn_act: sign of the exact fma(fl32(z - mean), fl32(gamma * inv), beta)."""
    z, mean, inv, gamma, beta = (np.asarray(v, np.float32) for v in (z, mean, inv, gamma, beta))
    d = (z - mean).astype(np.float64)
    sc = (gamma * inv).astype(np.float64)
    return d * sc + beta.astype(np.float64) > 0

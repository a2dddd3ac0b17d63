"""float64 NumPy restatement of GINEConv(Sequential(Linear, ReLU, Linear), train_eps, edge_dim) and of gcnx.GINE -- gcnx.GIN
whose neighbour sum reads the dca / proximity edge features the reference computes and drops (gcn_utills.py:319-443; gcn.py:71)
-- with BCEWithLogitsLoss: forward, loss, accuracy, every gradient, eps included.  No torch.

    out_i = MLP((1 + eps) x_i + sum_{j in N(i)} relu(x_j + lin(e_ij)))      N(i): the stored entries of row i (row = target), as
    lin = Linear(edge_dim, in)      MLP = Linear -> ReLU -> Linear          stored; e [nnz, edge_dim] in the CSR's entry order

The pattern is (rowptr, colidx) as stored: nothing is sorted or merged, since e belongs to the entries in their order.
The side of every message kink is an argument (``msg_mask``, bool [nnz, in]); ``contract_m`` is the float32 restatement of the
contract of include/gcnx.h (every product and sum rounded on its own, in the stated order), whose sign is the side the device
takes -- by construction, so no entry is ever excluded from a comparison.  BatchNorm, PReLU, the pools, the head, BCE and the
other kink-side arguments (``masks``, ``argmax``) are gcn_bn_ref's / graph_norm_ref's / attn_pool_ref's; ``masks`` also takes
``relu1`` / ``relu2`` (the inner ReLUs, as gin_ref) and ``msg1`` / ``msg2`` (the message kinks).
Parameters use the torch key names and layouts: gin_ref's and conv*.lin.weight [in, edge_dim], conv*.lin.bias [in].
"""
import numpy as np

import attn_pool_ref as AR
import gcn_bn_ref as R
import graph_norm_ref as GN
from gcn_bn_ref import sgd  # noqa: F401

_CONV = ("eps", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "lin.weight", "lin.bias")
CONV_KEYS = tuple(f"conv{k}.{s}" for k in (1, 2) for s in _CONV)
KEYS = CONV_KEYS + ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "prelu_1.weight", "prelu_2.weight",
                    "prelu_3.weight", "prelu_4.weight", "batch_norm_1.weight", "batch_norm_1.bias", "batch_norm_2.weight",
                    "batch_norm_2.bias", "batch_norm_3.weight", "batch_norm_3.bias", "batch_norm_4.weight", "batch_norm_4.bias")
EPS_KEYS = ("conv1.eps", "conv2.eps")


def keys(readout="max", norm="batch"):
    """The state_dict order of gcnx.GINE: mean_scale directly behind its norm's bias, the attention gate last."""
    out = []
    for k in KEYS:
        out.append(k)
        if norm == "graph" and k in ("batch_norm_1.bias", "batch_norm_2.bias"):
            out.append(k.replace(".bias", ".mean_scale"))
    return tuple(out) + ((AR.GATE_KEY,) if readout == "attention" else ())


def init_params(f_in, h=64, edge_dim=2, seed=0, eps=(0.0, 0.0), readout="max", norm="batch"):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced (random, every kind away from its default)."""
    p = R.init_params(f_in, h, seed)
    for k in ("conv1.bias", "conv1.lin.weight", "conv2.bias", "conv2.lin.weight"):
        del p[k]
    rng = np.random.default_rng(seed + 2500)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for i, (c, fi) in enumerate((("conv1", f_in), ("conv2", h))):
        p[f"{c}.eps"] = np.array([float(eps[i])])
        p[f"{c}.nn.0.weight"], p[f"{c}.nn.0.bias"] = u(1 / np.sqrt(fi), h, fi), u(0.1, h)
        p[f"{c}.nn.2.weight"], p[f"{c}.nn.2.bias"] = u(1 / np.sqrt(h), h, h), u(0.1, h)
        p[f"{c}.lin.weight"], p[f"{c}.lin.bias"] = u(1 / np.sqrt(edge_dim), fi, edge_dim), u(0.3, fi)
    if norm == "graph":
        r2 = np.random.default_rng(seed + 4000)
        for k in GN.SCALE_KEYS:
            p[k] = r2.uniform(0.5, 1.5, h)
    if readout == "attention":
        p[AR.GATE_KEY] = np.random.default_rng(seed + 3000).uniform(-0.5, 0.5, (1, h))
    return {k: p[k] for k in keys(readout, norm)}


def rows_of(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def contract_m(colidx, x, e, lin_w, lin_b):
    """m [nnz, in] in float32 exactly as the contract writes it: t = e[0] w[0]; t = t + e[d] w[d] for d = 1 ..; v = t + b
    (lin_b None: v = t); m = x_j + v -- every product and every sum rounded to float32 on its own (NumPy fuses nothing).
    x [n, in], e [nnz, edge_dim], lin_w [in, edge_dim] (torch's layout), lin_b [in]: all taken as float32 values."""
    x, e, w = np.asarray(x, np.float32), np.asarray(e, np.float32), np.asarray(lin_w, np.float32).T       # w [edge_dim, in]
    t = e[:, 0:1] * w[0][None, :]
    for d in range(1, e.shape[1]):
        t = t + e[:, d:d + 1] * w[d][None, :]
    v = t + np.asarray(lin_b, np.float32)[None, :] if lin_b is not None else t
    m = x[np.asarray(colidx, np.int64)] + v
    assert m.dtype == np.float32
    return m


def contract_mask(colidx, x, e, lin_w, lin_b):
    """The device's side of every message kink: m > 0 (m == 0 is the zero side)."""
    return contract_m(colidx, x, e, lin_w, lin_b) > 0


def gine_aggregate(rowptr, colidx, x, e, eps, lin_w, lin_b, msg_mask=None):
    """(T = (1 + eps) x + sum_j [mask] (x_j + e_ij lin_w^T + lin_b), mask) in float64; msg_mask None: m's own sign in float64."""
    x, e = np.asarray(x, np.float64), np.asarray(e, np.float64)
    m = x[np.asarray(colidx, np.int64)] + e @ np.asarray(lin_w, np.float64).T
    if lin_b is not None:
        m = m + np.asarray(lin_b, np.float64)
    mask = m > 0 if msg_mask is None else np.asarray(msg_mask, bool)
    s = np.zeros_like(x)
    np.add.at(s, rows_of(rowptr), np.where(mask, m, 0.0))
    return (1.0 + float(np.asarray(eps).reshape(-1)[0])) * x + s, mask


def gine_conv_fwd(rowptr, colidx, x, e, eps, lin_w, lin_b, w_a, b_a, w_b, b_b, msg_mask=None, relu_mask=None):
    """w_a [hidden, in], w_b [out, hidden], lin_w [in, edge_dim]; the biases may be None.  Returns (out, T, U, msg_mask, relu_mask)."""
    t, mm = gine_aggregate(rowptr, colidx, x, e, eps, lin_w, lin_b, msg_mask)
    v = t @ np.asarray(w_a, np.float64).T
    if b_a is not None:
        v = v + np.asarray(b_a, np.float64)
    mask = v > 0 if relu_mask is None else np.asarray(relu_mask, bool)
    u = np.where(mask, v, 0.0)
    out = u @ np.asarray(w_b, np.float64).T
    if b_b is not None:
        out = out + np.asarray(b_b, np.float64)
    return out, t, u, mm, mask


def gine_edge_bwd(rowptr, colidx, x, e, eps, msg_mask, dt):
    """(dx, d eps [1], d lin.weight [in, edge_dim], d lin.bias [in]) from dT."""
    x, e, dt = np.asarray(x, np.float64), np.asarray(e, np.float64), np.asarray(dt, np.float64)
    g = np.where(np.asarray(msg_mask, bool), dt[rows_of(rowptr)], 0.0)                  # [nnz, in]
    dx = (1.0 + float(np.asarray(eps).reshape(-1)[0])) * dt
    np.add.at(dx, np.asarray(colidx, np.int64), g)
    return dx, np.array([np.sum(x * dt)]), g.T @ e, g.sum(0)


def gine_conv_bwd(rowptr, colidx, x, e, eps, t, u, msg_mask, relu_mask, w_a, w_b, dz):
    """(dx, d eps [1], dW_a, db_a, dW_b, db_b, d lin.weight, d lin.bias) of gine_conv_fwd from dz, at the forward's masks."""
    dz = np.asarray(dz, np.float64)
    du = np.where(relu_mask, dz @ np.asarray(w_b, np.float64), 0.0)
    dt = du @ np.asarray(w_a, np.float64)
    dx, deps, dwe, dbe = gine_edge_bwd(rowptr, colidx, x, e, eps, msg_mask, dt)
    return dx, deps, du.T @ t, du.sum(0), dz.T @ u, dz.sum(0), dwe, dbe


def model(x, rowptr, colidx, e, graph_ptr, p, y=None, denom=None, masks=None, argmax=None, readout="max", norm="batch"):
    """gcnx.GINE: gcn_bn_ref.model's result dict (+ relu1 / relu2 / msg1 / msg2, the masks used; y1: conv2's input).  masks:
    m1 .. m4 (PReLU sides), relu1 / relu2, msg1 / msg2; a missing one is the float64 value's own sign."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    cw = lambda c: (q[f"{c}.eps"], q[f"{c}.lin.weight"], q[f"{c}.lin.bias"], q[f"{c}.nn.0.weight"], q[f"{c}.nn.0.bias"],
                    q[f"{c}.nn.2.weight"], q[f"{c}.nn.2.bias"])
    if norm == "graph":
        def nfwd(k, z):
            yk, c = GN.forward(z, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"],
                               q[f"prelu_{k}.weight"][0], m.get(f"m{k}"))
            return yk, c["pos"], c
    else:
        def nfwd(k, z):
            zb, c = R.bn_fwd(z, q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"])
            yk, pos = R.prelu_fwd(zb, q[f"prelu_{k}.weight"][0], m.get(f"m{k}"))
            return yk, pos, (zb, c)
    z1, t1, u1, s1, r1 = gine_conv_fwd(rowptr, colidx, x, e, *cw("conv1"), msg_mask=m.get("msg1"), relu_mask=m.get("relu1"))
    y1, p1, c1 = nfwd(1, z1)
    z2, t2, u2, s2, r2 = gine_conv_fwd(rowptr, colidx, y1, e, *cw("conv2"), msg_mask=m.get("msg2"), relu_mask=m.get("relu2"))
    y2, p2, c2 = nfwd(2, z2)
    cols = np.arange(y2.shape[1])
    head_p = {k: v for k, v in p.items() if k not in GN.SCALE_KEYS and k != AR.GATE_KEY}
    if readout == "attention":
        gate = q[AR.GATE_KEY].reshape(-1)
        P, alpha = AR.forward(y2, gate, gp)
        r = R.head(P, head_p, y, denom, m)
        arg = None
    else:
        arg = R.first_argmax(y2, gp) if argmax is None else np.asarray(argmax, np.int64)
        P = np.stack([y2[arg[g], cols] if gp[g + 1] > gp[g] else np.zeros(y2.shape[1]) for g in range(len(gp) - 1)])
        r = R.head(P, head_p, y, denom, m)
    r.update(m1=p1, m2=p2, relu1=r1, relu2=r2, msg1=s1, msg2=s2, argmax=arg, pooled=P, y1=y1, y2=y2)
    if y is None:
        return r
    g = r["grads"]
    if readout == "attention":
        dy2, dgate = AR.backward(y2, gate, gp, r["dP"], alpha, P)
        g[AR.GATE_KEY] = dgate[None, :]
    else:
        dy2 = np.zeros_like(y2)
        for gi in range(len(gp) - 1):
            if gp[gi + 1] > gp[gi]:
                dy2[arg[gi], cols] += r["dP"][gi]

    def nbwd(k, dyk, zk, c, pos):
        if norm == "graph":
            dz, dg, db, da, ds = GN.backward(dyk, zk, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"],
                                             q[f"batch_norm_{k}.bias"], q[f"prelu_{k}.weight"][0], pos)
            g[f"batch_norm_{k}.mean_scale"] = da
        else:
            dzb, ds = R.prelu_bwd(dyk, c[0], q[f"prelu_{k}.weight"][0], pos)
            dz, dg, db = R.bn_bwd(dzb, c[1], q[f"batch_norm_{k}.weight"])
        g[f"batch_norm_{k}.weight"], g[f"batch_norm_{k}.bias"], g[f"prelu_{k}.weight"] = dg, db, ds
        return dz

    def cbwd(c, xin, t, u, s, rm, dz):
        dx, g[f"{c}.eps"], g[f"{c}.nn.0.weight"], g[f"{c}.nn.0.bias"], g[f"{c}.nn.2.weight"], g[f"{c}.nn.2.bias"], \
            g[f"{c}.lin.weight"], g[f"{c}.lin.bias"] = gine_conv_bwd(rowptr, colidx, xin, e, q[f"{c}.eps"], t, u, s, rm,
                                                                     q[f"{c}.nn.0.weight"], q[f"{c}.nn.2.weight"], dz)
        return dx

    dy1 = cbwd("conv2", y1, t2, u2, s2, r2, nbwd(2, dy2, z2, c2, p2))
    cbwd("conv1", x, t1, u1, s1, r1, nbwd(1, dy1, z1, c1, p1))
    return r

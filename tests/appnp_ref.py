"""float64 NumPy restatement of APPNP propagation (include/gcnx.h, gcnx_appnp_propagate), of gcnx.APPNPConv and of
gcnx.APPNP -- gcnx.GCN with each GCNConv replaced by Linear + APPNP(K, alpha) -- with BCEWithLogitsLoss: forward, loss, every
gradient.  No torch (tests/test_appnp_host.py pins it to torch autograd).

    h = x W^T + b      z^0 = h      z^{k+1} = (1 - alpha) A^ z^k + alpha h      Z = z^K      A^ = gcn_bn_ref.pyg_norm

The backward of the propagation is the same recursion on A^^T: P = M^K + alpha sum_{k<K} M^k with M = (1 - alpha) A^.
BatchNorm, GraphNorm, PReLU, the pools, the head and BCE are gcn_bn_ref's / graph_norm_ref's / attn_pool_ref's, with their kink
sides (``masks`` m1 .. m4, ``argmax``).  Parameters use the torch key names and layouts: lin*.weight [out, in], lin*.bias [out]."""
import numpy as np

import attn_pool_ref as AR
import gcn_bn_ref as R
import graph_norm_ref as GN
from gcn_bn_ref import sgd  # noqa: F401

CONV_KEYS = ("lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias")
KEYS = CONV_KEYS + R.KEYS[4:]


def keys(readout="max", norm="batch"):
    """The state_dict order of gcnx.APPNP: mean_scale directly behind its norm's bias, the attention gate last."""
    out = []
    for k in KEYS:
        out.append(k)
        if norm == "graph" and k in ("batch_norm_1.bias", "batch_norm_2.bias"):
            out.append(k.replace(".bias", ".mean_scale"))
    return tuple(out) + ((AR.GATE_KEY,) if readout == "attention" else ())


def init_params(f_in, h=64, seed=0, readout="max", norm="batch"):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced by the two Linears (random, biases away from zero)."""
    p = R.init_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 2700)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for c, fi in (("lin1", f_in), ("lin2", h)):
        p[f"{c}.weight"], p[f"{c}.bias"] = u(1 / np.sqrt(fi), h, fi), u(0.3, h)
    if norm == "graph":
        r2 = np.random.default_rng(seed + 4000)
        for k in GN.SCALE_KEYS:
            p[k] = r2.uniform(0.5, 1.5, h)
    if readout == "attention":
        p[AR.GATE_KEY] = np.random.default_rng(seed + 3000).uniform(-0.5, 0.5, (1, h))
    return {k: p[k] for k in keys(readout, norm)}


def propagate(A, x, K, alpha):
    """z^K of z^0 = x, z^{k+1} = (1 - alpha) A z^k + alpha x.  A: scipy sparse or dense [n, n]; the adjoint is
    propagate(A.T, ., K, alpha)."""
    x = np.asarray(x, np.float64)
    z = x
    for _ in range(int(K)):
        z = (1.0 - alpha) * (A @ z) + alpha * x
    return z


def conv_fwd(A, x, w, b, K, alpha):
    """APPNPConv: (out, h = x W^T + b).  w [out, in]; b [out] or None."""
    h = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    if b is not None:
        h = h + np.asarray(b, np.float64)
    return propagate(A, h, K, alpha), h


def conv_bwd(A, x, w, dz, K, alpha):
    """(dx, dW [out, in], db) of conv_fwd from dz = dLoss / dout."""
    dh = propagate(A.T, dz, K, alpha)
    return dh @ np.asarray(w, np.float64), dh.T @ np.asarray(x, np.float64), dh.sum(0)


def model(x, a, graph_ptr, p, K, alpha, y=None, denom=None, masks=None, argmax=None, readout="max", norm="batch"):
    """gcnx.APPNP: gcn_bn_ref.model's arguments (+ K, alpha, readout, norm) and result dict (+ z1, z2, y1).  a: scipy adjacency
    (row = target), normalised here as GCNConv's operator."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    A = R.pyg_norm(a, x.shape[0])
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

    z1, _ = conv_fwd(A, x, q["lin1.weight"], q["lin1.bias"], K, alpha)
    y1, p1, c1 = nfwd(1, z1)
    z2, _ = conv_fwd(A, y1, q["lin2.weight"], q["lin2.bias"], K, alpha)
    y2, p2, c2 = nfwd(2, z2)
    cols = np.arange(y2.shape[1])
    head_p = {k: v for k, v in p.items() if k not in GN.SCALE_KEYS and k != AR.GATE_KEY and k not in CONV_KEYS}
    if readout == "attention":
        agate = q[AR.GATE_KEY].reshape(-1)
        P, att = AR.forward(y2, agate, gp)
        arg = None
    else:
        arg = R.first_argmax(y2, gp) if argmax is None else np.asarray(argmax, np.int64)
        P = np.stack([y2[arg[g], cols] if gp[g + 1] > gp[g] else np.zeros(y2.shape[1]) for g in range(len(gp) - 1)])
    r = R.head(P, head_p, y, denom, m)
    r.update(m1=p1, m2=p2, argmax=arg, pooled=P, z1=z1, z2=z2, y1=y1, y2=y2)
    if y is None:
        return r
    g = r["grads"]
    if readout == "attention":
        dy2, dgate = AR.backward(y2, agate, gp, r["dP"], att, P)
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

    dy1, g["lin2.weight"], g["lin2.bias"] = conv_bwd(A, y1, q["lin2.weight"], nbwd(2, dy2, z2, c2, p2), K, alpha)
    _, g["lin1.weight"], g["lin1.bias"] = conv_bwd(A, x, q["lin1.weight"], nbwd(1, dy1, z1, c1, p1), K, alpha)
    return r

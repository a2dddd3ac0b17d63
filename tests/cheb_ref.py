"""float64 NumPy restatement of the Chebyshev convolution (include/gcnx.h, gcnx_cheb_norm / gcnx_cheb_basis / gcnx_cheb_sum;
DESIGN.md 4.24), of gcnx.ChebConv and of gcnx.Cheb -- gcnx.GCN with each GCNConv replaced by PyG's ChebConv(K, "sym",
lambda_max) -- with BCEWithLogitsLoss: forward, loss, every gradient.  No torch (tests/test_cheb_host.py pins it to torch
autograd of PyG's steps).

    S[i, j] = r_i w_ij r_j (i != j), S[i, i] = 0      r_j = deg_j^-1/2, deg_j = sum_{i != j} w_ij over column j (0 where deg_j <= 0)
    L^ z = c_s S z + c_d z      c_s = -2 / lambda_max      c_d = 2 / lambda_max - 1
    T_0 = I   T_1 = L^   T_k = 2 L^ T_{k-1} - T_{k-2}         out = sum_{k < K} T_k(L^) x W_k^T + b

K is PyG's: the number of terms.  ``fp32=True`` rounds lambda_max, c_s and c_d once to fp32 as the library's host code does
(the contract of include/gcnx.h); the default keeps them exact, as PyG computes them.  BatchNorm, GraphNorm, PReLU, the pools,
the head and BCE are gcn_bn_ref's / graph_norm_ref's / attn_pool_ref's, with their kink sides (``masks`` m1 .. m4, ``argmax``).
Parameters use PyG's key names and layouts: conv*.lins.k.weight [out, in], conv*.bias [out]."""
import numpy as np

import attn_pool_ref as AR
import gcn_bn_ref as R
import graph_norm_ref as GN
from gcn_bn_ref import sgd  # noqa: F401


def conv_keys(K):
    return tuple(k for c in (1, 2) for k in tuple(f"conv{c}.lins.{j}.weight" for j in range(K)) + (f"conv{c}.bias",))


def keys(K, readout="max", norm="batch"):
    """The state_dict order of gcnx.Cheb: mean_scale directly behind its norm's bias, the attention gate last."""
    out = []
    for k in conv_keys(K) + R.KEYS[4:]:
        out.append(k)
        if norm == "graph" and k in ("batch_norm_1.bias", "batch_norm_2.bias"):
            out.append(k.replace(".bias", ".mean_scale"))
    return tuple(out) + ((AR.GATE_KEY,) if readout == "attention" else ())


def init_params(f_in, h=64, K=3, seed=0, readout="max", norm="batch"):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced by ChebConv's (random, biases away from zero)."""
    p = R.init_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 2800)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for c, fi in ((1, f_in), (2, h)):
        for j in range(K):
            p[f"conv{c}.lins.{j}.weight"] = u(np.sqrt(6 / (fi + h)), h, fi)
        p[f"conv{c}.bias"] = u(0.3, h)
    if norm == "graph":
        r2 = np.random.default_rng(seed + 4000)
        for k in GN.SCALE_KEYS:
            p[k] = r2.uniform(0.5, 1.5, h)
    if readout == "attention":
        p[AR.GATE_KEY] = np.random.default_rng(seed + 3000).uniform(-0.5, 0.5, (1, h))
    return {k: p[k] for k in keys(K, readout, norm)}


def hand_batch(seed=5):
    """(rowptr, colidx, vals, graph_ptr) of three graphs and an empty one, 12 nodes: an asymmetric pattern, stored diagonals
    (0, 2, 7, 10, 11), an isolated node (4), a one-node graph without entries (5), an empty graph, and a row holding only its
    diagonal (11, whose column does hold an entry).  Row = target, column = source; random weights."""
    entries = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 3), (2, 1), (2, 2), (2, 3), (3, 0),
               (6, 7), (6, 8), (7, 6), (7, 7), (7, 9), (8, 6), (8, 10), (9, 7), (9, 8), (9, 11), (10, 8), (10, 9), (10, 10), (11, 11)]
    rows, cols = np.array(entries).T
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=12))]).astype(np.int32)
    vals = np.random.default_rng(seed).uniform(0.2, 1.5, len(entries)).astype(np.float32)
    return rowptr, cols.astype(np.int32), vals, np.array([0, 5, 6, 6, 12], np.int32)


def coefs(lambda_max, fp32=False):
    """(c_s, c_d) as float64; fp32: lambda_max and both coefficients rounded once to fp32."""
    if not fp32:
        return -2.0 / lambda_max, 2.0 / lambda_max - 1.0
    lam = np.float64(np.float32(lambda_max))
    return np.float64(np.float32(-2.0 / lam)), np.float64(np.float32(2.0 / lam - 1.0))


def operator_values(rowptr, colidx, vals, n):
    """The values of S on the stored pattern (vals None: ones): exactly 0 on a stored diagonal entry."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    w = np.ones(colidx.size) if vals is None else np.asarray(vals, np.float64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    off = rows != colidx
    deg = np.bincount(colidx[off], weights=w[off], minlength=n)            # the column sums without the diagonal
    r = np.zeros(n)
    r[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return np.where(off, r[rows] * w * r[colidx], 0.0)


def operator(a, n=None):
    """S of a scipy adjacency (row = target, column = source), as a CSR on the same stored pattern."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a)
    a.sort_indices()
    n = a.shape[0] if n is None else n
    return sp.csr_matrix((operator_values(a.indptr, a.indices, a.data, n), a.indices.copy(), a.indptr.copy()), shape=(n, n))


def basis(S, x, K, lambda_max=2.0, fp32=False):
    """[T_0(L^) x | .. | T_{K-1}(L^) x], [n, K f]; the adjoint of cheb_sum's linear part is basis(S.T, .)."""
    cs, cd = coefs(lambda_max, fp32)
    lhat = lambda z: cs * (S @ z) + cd * z
    t = [np.asarray(x, np.float64)]
    if K > 1:
        t.append(lhat(t[0]))
    for _ in range(2, K):
        t.append(2.0 * lhat(t[-1]) - t[-2])
    return np.concatenate(t, axis=1)


def cheb_sum(S, H, bias, K, lambda_max=2.0, fp32=False):
    """sum_k T_k(L^) H_k + bias by Clenshaw summation: b_K = b_{K+1} = 0, b_j = H_j + 2 L^ b_{j+1} - b_{j+2},
    out = H_0 + L^ b_1 - b_2 + bias.  H [n, K f]."""
    cs, cd = coefs(lambda_max, fp32)
    lhat = lambda z: cs * (S @ z) + cd * z
    H = np.asarray(H, np.float64)
    f = H.shape[1] // K
    blk = lambda j: H[:, j * f:(j + 1) * f]
    b1, b2 = np.zeros_like(blk(0)), np.zeros_like(blk(0))
    for j in range(K - 1, 0, -1):
        b1, b2 = blk(j) + 2.0 * lhat(b1) - b2, b1
    out = blk(0) + lhat(b1) - b2
    return out if bias is None else out + np.asarray(bias, np.float64)


def cheb_sum_explicit(S, H, bias, K, lambda_max=2.0, fp32=False):
    """The same as the explicit sum over the basis of every block."""
    H = np.asarray(H, np.float64)
    f = H.shape[1] // K
    out = sum(basis(S, H[:, j * f:(j + 1) * f], K, lambda_max, fp32)[:, j * f:(j + 1) * f] for j in range(K))
    return out if bias is None else out + np.asarray(bias, np.float64)


def conv_fwd(S, x, ws, b, K, lambda_max=2.0, fp32=False):
    """ChebConv: ws = [lins.k.weight [out, in]], b [out] or None."""
    x = np.asarray(x, np.float64)
    H = np.concatenate([x @ np.asarray(w, np.float64).T for w in ws], axis=1)
    return cheb_sum(S, H, b, K, lambda_max, fp32)


def conv_bwd(S, x, ws, dz, K, lambda_max=2.0, fp32=False):
    """(dx, [dW_k [out, in]], db) of conv_fwd from dz = dLoss / dout."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    c = dz.shape[1]
    G = basis(S.T, dz, K, lambda_max, fp32)
    gk = [G[:, j * c:(j + 1) * c] for j in range(K)]
    return sum(g @ np.asarray(w, np.float64) for g, w in zip(gk, ws)), [g.T @ x for g in gk], dz.sum(0)


def model(x, a, graph_ptr, p, K, lambda_max=2.0, y=None, denom=None, masks=None, argmax=None, readout="max", norm="batch", fp32=False):
    """gcnx.Cheb: gcn_bn_ref.model's arguments (+ K, lambda_max, readout, norm) and result dict (+ z1, z2, y1).  a: scipy adjacency
    (row = target), used unweighted as stored."""
    import scipy.sparse as sp
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    a = sp.csr_matrix(a, shape=(x.shape[0], x.shape[0])).copy()
    a.data[:] = 1.0
    S = operator(a, x.shape[0])
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

    ws = lambda c: [q[f"conv{c}.lins.{j}.weight"] for j in range(K)]
    z1 = conv_fwd(S, x, ws(1), q["conv1.bias"], K, lambda_max, fp32)
    y1, p1, c1 = nfwd(1, z1)
    z2 = conv_fwd(S, y1, ws(2), q["conv2.bias"], K, lambda_max, fp32)
    y2, p2, c2 = nfwd(2, z2)
    cols = np.arange(y2.shape[1])
    ck = set(conv_keys(K))
    head_p = {k: v for k, v in p.items() if k not in GN.SCALE_KEYS and k != AR.GATE_KEY and k not in ck}
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

    def cbwd(c, xin, dz):
        dx, dws, db = conv_bwd(S, xin, ws(c), dz, K, lambda_max, fp32)
        for j, dw in enumerate(dws):
            g[f"conv{c}.lins.{j}.weight"] = dw
        g[f"conv{c}.bias"] = db
        return dx

    dy1 = cbwd(2, y1, nbwd(2, dy2, z2, c2, p2))
    cbwd(1, x, nbwd(1, dy1, z1, c1, p1))
    return r

"""float64 NumPy restatement of the relational convolution (include/gcnx.h, gcnx_rgcn_operator / gcnx_rgcn_conv /
gcnx_rgcn_aggregate), of gcnx.RGCNConv and of gcnx.RGCN -- gcnx.GCN with each GCNConv replaced by PyG's
RGCNConv(num_relations, aggr="mean", root_weight) -- with BCEWithLogitsLoss: forward, loss, every gradient.  No torch
(tests/test_rgcn_host.py pins it to torch autograd of PyG's steps).

    out_i = x_i W_root + b + sum_{r < R} mean_{k in N_r(i)} x_col(k) W_r       N_r(i): the stored entries of row i of relation r
    rel[k]: "nonzero": the first column d with e[k, d] != 0, edge_dim where there is none (R = edge_dim + 1)
            "index":   e[k, 0] as an integer, clamped to 0 .. R - 1 (a NaN reads 0), as the kernel does
    val[k] = 1 / |N_rel(k)(row(k))|                                            the mean over no entry is 0

The adjacency is used as stored, unweighted (row = target, column = source): no loop is added or removed.  BatchNorm, GraphNorm,
PReLU, the pools, the head and BCE are gcn_bn_ref's / graph_norm_ref's / attn_pool_ref's, with their kink sides (``masks``
m1 .. m4, ``argmax``).  Parameters use PyG's key names and layouts: conv*.weight [R, in, out], conv*.root [in, out],
conv*.bias [out]."""
import numpy as np

import attn_pool_ref as AR
import gcn_bn_ref as R
import graph_norm_ref as GN
from gcn_bn_ref import sgd  # noqa: F401


def conv_keys(root_weight=True):
    return tuple(k for c in (1, 2) for k in (f"conv{c}.weight",) + ((f"conv{c}.root",) if root_weight else ()) + (f"conv{c}.bias",))


def keys(root_weight=True, readout="max", norm="batch"):
    """The state_dict order of gcnx.RGCN: mean_scale directly behind its norm's bias, the attention gate last."""
    out = []
    for k in conv_keys(root_weight) + R.KEYS[4:]:
        out.append(k)
        if norm == "graph" and k in ("batch_norm_1.bias", "batch_norm_2.bias"):
            out.append(k.replace(".bias", ".mean_scale"))
    return tuple(out) + ((AR.GATE_KEY,) if readout == "attention" else ())


def init_params(f_in, h=64, num_relations=3, seed=0, root_weight=True, readout="max", norm="batch"):
    """gcn_bn_ref.init_params with the convolutions' parameters replaced by RGCNConv's (random, biases away from zero)."""
    p = R.init_params(f_in, h, seed)
    rng = np.random.default_rng(seed + 2900)
    u = lambda lim, *s: rng.uniform(-lim, lim, s)
    for c, fi in ((1, f_in), (2, h)):
        p[f"conv{c}.weight"] = u(np.sqrt(6 / (fi + h)), num_relations, fi, h)
        p[f"conv{c}.root"] = u(np.sqrt(6 / (fi + h)), fi, h)
        p[f"conv{c}.bias"] = u(0.3, h)
    if norm == "graph":
        r2 = np.random.default_rng(seed + 4000)
        for k in GN.SCALE_KEYS:
            p[k] = r2.uniform(0.5, 1.5, h)
    if readout == "attention":
        p[AR.GATE_KEY] = np.random.default_rng(seed + 3000).uniform(-0.5, 0.5, (1, h))
    return {k: p[k] for k in keys(root_weight, readout, norm)}


def hand_batch():
    """(rowptr, colidx, e, graph_ptr) of three graphs and an empty one, 12 nodes (graphs: rows 0-4, row 5, none, rows 6-11), with
    reference-style edge features e = (dca, proximity): an asymmetric pattern, stored loops (0, 2, 7, 10, 11: neither feature
    set, so relation 2 under "nonzero"), an isolated node (4), a one-node graph without entries (5), rows holding only one
    relation (1, 3: contacts only; 11: its loop only), bridges (relation 0) in the last graph only -- no row of the first
    graph holds relation 0 --, and one contact whose proximity is exactly 0 (entry (8, 10): relation 2)."""
    entries = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 3), (2, 1), (2, 2), (2, 3), (3, 0),
               (6, 7), (6, 8), (7, 6), (7, 7), (7, 9), (8, 6), (8, 10), (9, 7), (9, 8), (9, 11), (10, 8), (10, 9), (10, 10), (11, 11)]
    bridges = {(6, 8), (8, 6), (7, 9), (9, 7), (9, 11)}
    rows, cols = np.array(entries).T
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=12))]).astype(np.int32)
    rng = np.random.default_rng(5)
    e = np.zeros((len(entries), 2), np.float32)
    for k, (i, j) in enumerate(entries):
        if i == j or (i, j) == (8, 10):
            continue
        e[k, 0 if (i, j) in bridges else 1] = rng.uniform(0.2, 1.5)
    return rowptr, cols.astype(np.int32), e, np.array([0, 5, 6, 6, 12], np.int32)


# ---- relations and values ----------------------------------------------------------------------------------------------------
def relations(e, rule="nonzero", num_relations=None):
    """rel [nnz] int64 of the edge features e [nnz, edge_dim]."""
    e = np.asarray(e, np.float64)
    if rule == "nonzero":
        nz = e != 0
        return np.where(nz.any(1), nz.argmax(1), e.shape[1]).astype(np.int64)
    v = np.nan_to_num(e[:, 0], nan=0.0, posinf=np.inf, neginf=-np.inf)
    return np.clip(np.trunc(np.clip(v, 0, num_relations - 1)), 0, num_relations - 1).astype(np.int64)


def check_index(e, num_relations):
    """What the model checks on a host batch under relations="index": one column of integers in 0 .. R - 1."""
    e = np.asarray(e, np.float64)
    return e.ndim == 2 and e.shape[1] == 1 and bool(np.all(e == np.floor(e)) and (e.size == 0 or (e.min() >= 0 and e.max() <= num_relations - 1)))


def values(rowptr, rel, num_relations):
    """val [nnz] = 1 / (entries of the entry's row with the entry's relation)."""
    rowptr = np.asarray(rowptr, np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    cnt = np.zeros((len(rowptr) - 1, num_relations))
    np.add.at(cnt, (rows, rel), 1.0)
    return 1.0 / cnt[rows, rel]


def operators(rowptr, colidx, rel, num_relations):
    """[A_0, .., A_{R-1}]: the row-mean operator of every relation as scipy CSR [n, n] (row = target)."""
    import scipy.sparse as sp
    rowptr, colidx, rel = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64), np.asarray(rel, np.int64)
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    val = values(rowptr, rel, num_relations)
    return [sp.csr_matrix((val[rel == r], (rows[rel == r], colidx[rel == r])), shape=(n, n)) for r in range(num_relations)]


def panel(ops, x):
    """M = [A_0 x | .. | A_{R-1} x], [n, R f]."""
    x = np.asarray(x, np.float64)
    return np.concatenate([A @ x for A in ops], axis=1)


# ---- the convolution ---------------------------------------------------------------------------------------------------------
def conv_fwd(ops, x, weight, root, bias):
    """weight [R, in, out], root [in, out] or None, bias [out] or None.  Returns (out, M)."""
    x, weight = np.asarray(x, np.float64), np.asarray(weight, np.float64)
    m = panel(ops, x)
    out = m @ weight.reshape(-1, weight.shape[2])
    if root is not None:
        out = out + x @ np.asarray(root, np.float64)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out, m


def conv_bwd(ops, x, weight, root, dz):
    """(dx, dweight [R, in, out], droot or None, dbias) of conv_fwd from dz = dLoss / dout."""
    x, dz, weight = np.asarray(x, np.float64), np.asarray(dz, np.float64), np.asarray(weight, np.float64)
    dx = sum(A.T @ (dz @ weight[r].T) for r, A in enumerate(ops))
    dw = np.stack([(A @ x).T @ dz for A in ops])
    droot = None
    if root is not None:
        dx = dx + dz @ np.asarray(root, np.float64).T
        droot = x.T @ dz
    return dx, dw, droot, dz.sum(0)


def model(x, rowptr, colidx, e, graph_ptr, p, y=None, rule="nonzero", num_relations=None, denom=None, masks=None, argmax=None,
          readout="max", norm="batch"):
    """gcnx.RGCN: gcn_bn_ref.model's result dict (+ z1, z2, y1, y2) on the CSR (rowptr, colidx) with edge features e.  p without
    conv*.root: root_weight=False."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    nrel = q["conv1.weight"].shape[0] if num_relations is None else num_relations
    ops = operators(rowptr, colidx, relations(e, rule, nrel), nrel)
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

    z1, _ = conv_fwd(ops, x, q["conv1.weight"], q.get("conv1.root"), q["conv1.bias"])
    y1, p1, c1 = nfwd(1, z1)
    z2, _ = conv_fwd(ops, y1, q["conv2.weight"], q.get("conv2.root"), q["conv2.bias"])
    y2, p2, c2 = nfwd(2, z2)
    cols = np.arange(y2.shape[1])
    ck = set(conv_keys(True))
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
        dx, dw, droot, db = conv_bwd(ops, xin, q[f"conv{c}.weight"], q.get(f"conv{c}.root"), dz)
        g[f"conv{c}.weight"], g[f"conv{c}.bias"] = dw, db
        if droot is not None:
            g[f"conv{c}.root"] = droot
        return dx

    dy1 = cbwd(2, y1, nbwd(2, dy2, z2, c2, p2))
    cbwd(1, x, nbwd(1, dy1, z1, c1, p1))
    return r

"""float64 restatement of the sync-BN training step of gcnx.GCN over graph shards ("torch GCN", multi-GPU): every
shard works on its own rows, and the column sums of each BatchNorm -- both moment passes and the backward's two sums -- are
added over the shards between the phases, as the all-reduces of the device step add them.  Each shard returns its LOCAL
gradient parts and loss / hit parts; summed over the shards they are the whole batch's (tests/gcn_bn_ref.py's model).

Kink sides: ``masks`` and ``argmax`` are the WHOLE batch's (rows in batch order, argmax in global row numbers), as
gcn_bn_ref takes them; each shard reads its own rows.
"""
import numpy as np

import gcn_bn_ref as R

EPS = R.EPS


def _bn_fwd(zs, g, b, eps=EPS):
    """BatchNorm over the rows of every shard: the two moment passes with their sums added over the shards."""
    n = sum(z.shape[0] for z in zs)
    if n < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size [{n}, {zs[0].shape[1]}]")
    mu = sum(z.sum(0) for z in zs) / n
    var = sum(((z - mu) ** 2).sum(0) for z in zs) / n
    inv = 1.0 / np.sqrt(var + eps)
    xhs = [(z - mu) * inv for z in zs]
    return [g * xh + b for xh in xhs], (xhs, inv, n)


def _bn_bwd(dzbs, cache, g):
    """-> dz per shard, and the LOCAL dgamma / dbeta parts; dz uses the sums added over the shards and the global count."""
    xhs, inv, n = cache
    dbs = [d.sum(0) for d in dzbs]
    dgs = [(d * xh).sum(0) for d, xh in zip(dzbs, xhs)]
    db, dg = sum(dbs), sum(dgs)
    return [g * inv * (d - db / n - xh * dg / n) for d, xh in zip(dzbs, xhs)], dgs, dbs


def _split(rows, offs):
    return [rows[offs[s]:offs[s + 1]] for s in range(len(offs) - 1)]


def head(Ps, p, ys=None, denom=None, masks=None):
    """The head (Linear·BN·PReLU twice + BCE) over row shards Ps [b_s, h]: the arithmetic of the seven phases of
    gcnx_bce_head_phase with the partial sums added between them.  Returns one dict per shard: out, probs and, with labels
    ys (one per shard), the loss and hit parts, dP and the LOCAL gradient parts (torch keys)."""
    m = masks or {}
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    Ps = [np.asarray(P, np.float64) for P in Ps]
    offs = np.concatenate([[0], np.cumsum([P.shape[0] for P in Ps])])
    S = len(Ps)
    m3 = _split(m["m3"], offs) if "m3" in m else [None] * S
    m4 = _split(m["m4"], offs) if "m4" in m else [None] * S
    z3 = [P @ q["linear_1.weight"].T + q["linear_1.bias"] for P in Ps]
    zb3, c3 = _bn_fwd(z3, q["batch_norm_3.weight"], q["batch_norm_3.bias"])
    y3, p3 = zip(*[R.prelu_fwd(zb, q["prelu_3.weight"][0], mm) for zb, mm in zip(zb3, m3)])
    z4 = [y @ q["linear_2.weight"].T + q["linear_2.bias"] for y in y3]
    zb4, c4 = _bn_fwd(z4, q["batch_norm_4.weight"], q["batch_norm_4.bias"])
    out, p4 = zip(*[R.prelu_fwd(zb, q["prelu_4.weight"][0], mm) for zb, mm in zip(zb4, m4)])
    res = [{"out": o, "probs": 1 / (1 + np.exp(-o)), "m3": a, "m4": b} for o, a, b in zip(out, p3, p4)]
    if ys is None:
        return res
    denom = float(denom or offs[-1])
    dout = []
    for r, o, y in zip(res, out, ys):
        r["loss"], r["hits"], d = R.bce(o, R.targets(y), denom)
        dout.append(d)
        r["grads"] = {}
    dzb4 = []
    for r, d, zb, pos in zip(res, dout, zb4, p4):
        dz, r["grads"]["prelu_4.weight"] = R.prelu_bwd(d, zb, q["prelu_4.weight"][0], pos)
        dzb4.append(dz)
    dz4, dg4, db4 = _bn_bwd(dzb4, c4, q["batch_norm_4.weight"])
    dzb3 = []
    for s, r in enumerate(res):
        g = r["grads"]
        g["batch_norm_4.weight"], g["batch_norm_4.bias"] = dg4[s], db4[s]
        g["linear_2.weight"], g["linear_2.bias"] = dz4[s].T @ y3[s], dz4[s].sum(0)
        dz, g["prelu_3.weight"] = R.prelu_bwd(dz4[s] @ q["linear_2.weight"], zb3[s], q["prelu_3.weight"][0], p3[s])
        dzb3.append(dz)
    dz3, dg3, db3 = _bn_bwd(dzb3, c3, q["batch_norm_3.weight"])
    for s, r in enumerate(res):
        g = r["grads"]
        g["batch_norm_3.weight"], g["batch_norm_3.bias"] = dg3[s], db3[s]
        g["linear_1.weight"], g["linear_1.bias"] = dz3[s].T @ Ps[s], dz3[s].sum(0)
        r["dP"] = dz3[s] @ q["linear_1.weight"]
        r["dz3"], r["dz4"], r["y3"], r["dzb3"], r["xh3"] = dz3[s], dz4[s], y3[s], dzb3[s], c3[0][s]
    return res


def model(x, a, graph_ptr, p, y, bounds, denom=None, masks=None, argmax=None):
    """The whole step over graph shards: shard s holds graphs [bounds[s], bounds[s + 1]) (each with its own block of the
    block-diagonal adjacency).  Returns {"parts": [per-shard dict], "out": [B, 1], "loss", "hits", "grads": {torch key: sum
    of the shards' parts}, "argmax"} -- the last four as gcn_bn_ref.model returns them."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    gp = np.asarray(graph_ptr, np.int64)
    bounds = np.asarray(bounds, np.int64)
    S = len(bounds) - 1
    lo = [int(gp[bounds[s]]) for s in range(S)]
    hi = [int(gp[bounds[s + 1]]) for s in range(S)]
    a = a.tocsr()
    A = [R.pyg_norm(a[lo[s]:hi[s], lo[s]:hi[s]], hi[s] - lo[s]) for s in range(S)]
    X = [x[lo[s]:hi[s]] for s in range(S)]
    noffs = np.array(lo + [hi[-1]])
    m1 = _split(m["m1"], noffs) if "m1" in m else [None] * S
    m2 = _split(m["m2"], noffs) if "m2" in m else [None] * S
    z1 = [A[s] @ (X[s] @ q["conv1.lin.weight"].T) + q["conv1.bias"] for s in range(S)]
    zb1, c1 = _bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = zip(*[R.prelu_fwd(zb1[s], q["prelu_1.weight"][0], m1[s]) for s in range(S)])
    z2 = [A[s] @ (y1[s] @ q["conv2.lin.weight"].T) + q["conv2.bias"] for s in range(S)]
    zb2, c2 = _bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = zip(*[R.prelu_fwd(zb2[s], q["prelu_2.weight"][0], m2[s]) for s in range(S)])
    args, Ps, lgps = [], [], []
    for s in range(S):
        lgp = gp[bounds[s]:bounds[s + 1] + 1] - lo[s]
        arg = (R.first_argmax(y2[s], lgp) if argmax is None
               else np.asarray(argmax, np.int64)[bounds[s]:bounds[s + 1]] - lo[s])
        cols = np.arange(y2[s].shape[1])
        Ps.append(np.stack([y2[s][arg[g], cols] if lgp[g + 1] > lgp[g] else np.zeros(y2[s].shape[1])
                            for g in range(len(lgp) - 1)]))
        args.append(arg)
        lgps.append(lgp)
    ys = [np.asarray(y)[bounds[s]:bounds[s + 1]] for s in range(S)]
    res = head(Ps, p, ys, denom or gp.size - 1, m)
    dzb2 = []
    for s, r in enumerate(res):
        dy2 = np.zeros_like(y2[s])
        cols = np.arange(y2[s].shape[1])
        for gi in range(len(lgps[s]) - 1):
            if lgps[s][gi + 1] > lgps[s][gi]:
                dy2[args[s][gi], cols] += r["dP"][gi]
        dz, r["grads"]["prelu_2.weight"] = R.prelu_bwd(dy2, zb2[s], q["prelu_2.weight"][0], p2[s])
        dzb2.append(dz)
    dz2, dg2, db2 = _bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    dzb1 = []
    for s, r in enumerate(res):
        g = r["grads"]
        g["batch_norm_2.weight"], g["batch_norm_2.bias"] = dg2[s], db2[s]
        g["conv2.bias"] = dz2[s].sum(0)
        t2 = A[s].T @ dz2[s]
        g["conv2.lin.weight"] = t2.T @ y1[s]
        dz, g["prelu_1.weight"] = R.prelu_bwd(t2 @ q["conv2.lin.weight"], zb1[s], q["prelu_1.weight"][0], p1[s])
        dzb1.append(dz)
    dz1, dg1, db1 = _bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    for s, r in enumerate(res):
        g = r["grads"]
        g["batch_norm_1.weight"], g["batch_norm_1.bias"] = dg1[s], db1[s]
        g["conv1.bias"] = dz1[s].sum(0)
        g["conv1.lin.weight"] = (A[s].T @ dz1[s]).T @ X[s]
    grads = {k: sum(r["grads"][k] for r in res) for k in res[0]["grads"]}
    return {"parts": res, "out": np.concatenate([r["out"] for r in res]), "loss": sum(r["loss"] for r in res),
            "hits": sum(r["hits"] for r in res), "grads": grads,
            "argmax": np.concatenate([args[s] + lo[s] for s in range(S)])}

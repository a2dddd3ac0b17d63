"""float64 NumPy restatement of gcnx.Explainer: the masked gcnx.GCN -- either norm, either readout -- its
five-term objective, dL/d(edge logits), dL/d(feature logits), dL/dX' and one Adam step.  Built on the pieces of gcn_bn_ref,
graph_norm_ref and attn_pool_ref.  No torch (tests/test_explain_host.py pins it to torch autograd).

    v_e = A^_e sigma(m_e) off the diagonal, A^_e on it        X' = X * sigma(f)        Z_k = A^_m (X_k W_k^T) + b_k
    L = BCE(out, t) / B + c_es sum_off s + c_ee / E_off sum_off ent(s) + c_ns mean sigma(f) + c_ne mean ent(sigma(f))
    ent(p) = -p log(p + 1e-15) - (1 - p) log(1 - p + 1e-15)

Entries are in CSR order of the operator's pattern (row = target, sorted columns): edge logits and their gradient are [nnz]
arrays, diagonal entries never read and with gradient 0.  Kink sides (``masks`` m1 .. m4, ``argmax``) as gcn_bn_ref.model takes
them, so that a comparison with the device runs on the device's side of every kink."""
import numpy as np

import attn_pool_ref as AR
import gcn_bn_ref as R
import graph_norm_ref as GN

ENT_EPS = 1e-15
COEFFS = {"edge_size": 0.005, "edge_ent": 1.0, "node_feat_size": 1.0, "node_feat_ent": 0.1}
TERMS = ("loss", "edge_size", "edge_ent", "node_feat_size", "node_feat_ent")


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-np.asarray(a, np.float64)))


def ent(p):
    return -p * np.log(p + ENT_EPS) - (1 - p) * np.log(1 - p + ENT_EPS)


def dent(p):
    return -np.log(p + ENT_EPS) - p / (p + ENT_EPS) + np.log(1 - p + ENT_EPS) + (1 - p) / (1 - p + ENT_EPS)


def operator(a, n):
    """(A^ as a scipy CSR with sorted columns, rows [nnz], off [nnz] bool) of the pattern of `a`."""
    A = R.pyg_norm(a, n)
    A.sort_indices()
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    return A, rows, rows != A.indices


def initial_logits(n, nnz, node_shape, seed=0, edge=True):
    """The explainer's initial logits: the draws of np.random.default_rng(seed) in its order."""
    rng = np.random.default_rng(seed)
    e = rng.normal(0.0, np.sqrt(2.0) * np.sqrt(2.0 / (2.0 * n)), nnz) if edge else None
    f = rng.normal(0.0, 0.1, int(np.prod(node_shape))).reshape(node_shape) if node_shape else None
    return e, f


def model(x, a, graph_ptr, p, t, edge_logits=None, node_logits=None, coeffs=None, masks=None, argmax=None, norm="batch",
          readout="max"):
    """The masked forward, the objective and its gradients.  t [B]: the targets.  edge_logits [nnz] or None (no edge mask),
    node_logits [1, F] / [N, F] or None.  Returns a dict: out [B, 1], terms {name: value}, total, d_edge [nnz] / None, d_node
    (the logits' shape) / None, dxm [N, F] = dL/dX', dv [nnz] = dL/d(masked values), vals [nnz] and the kink sides it used."""
    import scipy.sparse as sp
    c = {**COEFFS, **(coeffs or {})}
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    gp = np.asarray(graph_ptr, np.int64)
    b = len(gp) - 1
    A, rows, off = operator(a, n)
    cols = A.indices
    if edge_logits is not None:
        s_e = sigmoid(np.asarray(edge_logits, np.float64).reshape(-1))
        vals = A.data * np.where(off, s_e, 1.0)
    else:
        vals = A.data.copy()
    Am = sp.csr_matrix((vals, cols, A.indptr), shape=(n, n))
    if node_logits is not None:
        fl = np.asarray(node_logits, np.float64)
        s_f = sigmoid(fl)
        xm = x * s_f
    else:
        xm = x
    w1, w2 = q["conv1.lin.weight"], q["conv2.lin.weight"]
    graph_norm = norm == "graph"

    def norm_fwd(k, z):
        if graph_norm:
            y, cache = GN.forward(z, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"],
                                  q[f"prelu_{k}.weight"][0], m.get(f"m{k}"))
            return y, cache["pos"], None
        zb, cache = R.bn_fwd(z, q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"])
        y, pos = R.prelu_fwd(zb, q[f"prelu_{k}.weight"][0], m.get(f"m{k}"))
        return y, pos, (zb, cache)

    def norm_bwd(k, dy, z, pos, kept):
        if graph_norm:
            return GN.backward(dy, z, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"],
                               q[f"prelu_{k}.weight"][0], pos)[0]
        zb, cache = kept
        dzb, _ = R.prelu_bwd(dy, zb, q[f"prelu_{k}.weight"][0], pos)
        return R.bn_bwd(dzb, cache, q[f"batch_norm_{k}.weight"])[0]

    h1 = xm @ w1.T
    z1 = Am @ h1 + q["conv1.bias"]
    y1, p1, k1 = norm_fwd(1, z1)
    h2 = y1 @ w2.T
    z2 = Am @ h2 + q["conv2.bias"]
    y2, p2, k2 = norm_fwd(2, z2)
    fcols = np.arange(y2.shape[1])
    head_p = {k: v for k, v in p.items() if k not in GN.SCALE_KEYS and k != AR.GATE_KEY}
    if readout == "attention":
        gate = q[AR.GATE_KEY].reshape(-1)
        P, alpha = AR.forward(y2, gate, gp)
        arg = None
    else:
        arg = R.first_argmax(y2, gp) if argmax is None else np.asarray(argmax, np.int64)
        P = np.stack([y2[arg[g], fcols] if gp[g + 1] > gp[g] else np.zeros(y2.shape[1]) for g in range(b)])
    r = R.head(P, head_p, np.asarray(t, np.float64).reshape(-1), float(b), m)
    if readout == "attention":
        dy2, _ = AR.backward(y2, gate, gp, r["dP"], alpha, P)
    else:
        dy2 = np.zeros_like(y2)
        for g in range(b):
            if gp[g + 1] > gp[g]:
                dy2[arg[g], fcols] += r["dP"][g]
    dz2 = norm_bwd(2, dy2, z2, p2, k2)
    dy1 = (Am.T @ dz2) @ w2
    dz1 = norm_bwd(1, dy1, z1, p1, k1)
    dv = np.einsum("ek,ek->e", dz1[rows], h1[cols]) + np.einsum("ek,ek->e", dz2[rows], h2[cols])
    dxm = (Am.T @ dz1) @ w1
    terms = dict.fromkeys(TERMS, 0.0)
    terms["loss"] = float(r["loss"])
    d_edge = d_node = None
    if edge_logits is not None:
        e_off = max(int(off.sum()), 1)
        so = s_e[off]
        terms["edge_size"] = c["edge_size"] * float(so.sum())
        terms["edge_ent"] = c["edge_ent"] / e_off * float(ent(so).sum())
        d_edge = np.where(off, (dv * A.data + c["edge_size"] + c["edge_ent"] / e_off * dent(s_e)) * s_e * (1 - s_e), 0.0)
    if node_logits is not None:
        cnt = s_f.size
        terms["node_feat_size"] = c["node_feat_size"] * float(s_f.mean())
        terms["node_feat_ent"] = c["node_feat_ent"] * float(ent(s_f).mean())
        data = dxm * x
        if fl.shape[0] == 1 and n != 1:
            data = data.sum(0, keepdims=True)
        d_node = (data + c["node_feat_size"] / cnt + c["node_feat_ent"] / cnt * dent(s_f)) * s_f * (1 - s_f)
    return {"out": r["out"], "terms": terms, "total": float(sum(terms.values())), "d_edge": d_edge, "d_node": d_node, "dxm": dxm,
            "dv": dv, "vals": vals, "m1": p1, "m2": p2, "m3": r["m3"], "m4": r["m4"], "argmax": arg, "y1": y1, "y2": y2}


def make_batch(sizes, f, seed=0, directed=False, p_edge=0.15):
    """A small disjoint batch: (x [N, f] float32, a scipy CSR [N, N] with every self-loop and sorted columns, graph_ptr, labels
    [B]).  Random undirected graphs (``directed``: about a third of the edges keep one direction only); the LAST node of the
    first graph is isolated (its loop is its only entry)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    blocks = []
    for gi, m in enumerate(sizes):
        up = np.triu(rng.random((m, m)) < p_edge, 1)
        up[np.arange(m - 1), np.arange(1, m)] = True          # a path: no graph falls apart
        d = up | up.T
        if directed:
            d &= ~(np.triu(rng.random((m, m)) < 0.33, 1) & up)
        if gi == 0:
            d[m - 1, :] = d[:, m - 1] = False
        np.fill_diagonal(d, True)
        blocks.append(sp.csr_matrix(d.astype(np.float64)))
    a = sp.block_diag(blocks, format="csr")
    a.sort_indices()
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = rng.normal(size=(int(gp[-1]), f)).astype(np.float32)
    return x, a, gp, rng.integers(0, 2, len(sizes)).astype(np.float32)


def adam_init(*arrays):
    """Fresh Adam state for the given logit arrays (None entries stay None): {"t": 0, "m": [...], "v": [...]}."""
    z = lambda a: None if a is None else np.zeros_like(np.asarray(a, np.float64))
    return {"t": 0, "m": [z(a) for a in arrays], "v": [z(a) for a in arrays]}


def adam_step(params, grads, state, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam without weight decay on the arrays of ``params`` (None entries skipped); returns the new list and
    advances ``state`` in place."""
    state["t"] += 1
    t = state["t"]
    out = []
    for i, (p, g) in enumerate(zip(params, grads)):
        if p is None:
            out.append(None)
            continue
        p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
        state["m"][i] = beta1 * state["m"][i] + (1 - beta1) * g
        state["v"][i] = beta2 * state["v"][i] + (1 - beta2) * g * g
        out.append(p - lr / (1 - beta1 ** t) * state["m"][i] / (np.sqrt(state["v"][i]) / np.sqrt(1 - beta2 ** t) + eps))
    return out


def optimise(x, a, graph_ptr, p, t, edge_logits, node_logits, steps, lr=0.01, **kw):
    """``steps`` Adam steps on the ref's own kink sides: the history [steps, 5] and the final logits."""
    state = adam_init(edge_logits, node_logits)
    hist = []
    for _ in range(steps):
        r = model(x, a, graph_ptr, p, t, edge_logits, node_logits, **kw)
        hist.append([r["terms"][k] for k in TERMS])
        edge_logits, node_logits = adam_step([edge_logits, node_logits], [r["d_edge"], r["d_node"]], state, lr)
    return np.asarray(hist), edge_logits, node_logits


OPT_CASE = dict(sizes=(14, 22, 30, 17), f=16, h=32, seed=5)          # the batch, weights and seed of "it optimises"


def opt_case():
    """(x, a, graph_ptr, p) of the run whose objective must go down: checked on the restatement by the host test, on the device
    by the GPU test."""
    c = OPT_CASE
    x, a, gp, _ = make_batch(c["sizes"], c["f"], seed=c["seed"])
    return x, a, gp, R.init_params(c["f"], c["h"], seed=c["seed"])

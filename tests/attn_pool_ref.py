"""float64 NumPy restatement of the learned readout -- spektral.layers.pooling.GlobalAttnSumPool, PyG's
AttentionalAggregation(gate_nn=Linear(F, 1, bias=False)) -- forward and backward, and of gcnx.GCN / gcnx.GAT with
``readout="attention"``: gcn_bn_ref.model / gat_ref.model with the max-pool replaced.  No torch.

    s_i = <x_i, a>        alpha_i = softmax of s over the rows i of graph g        P[g] = sum_i alpha_i x_i
    t_i = <dP[g], x_i> - <dP[g], P[g]>      dx_i = alpha_i dP[g] + (alpha_i t_i) a      da = sum_i (alpha_i t_i) x_i

An empty graph pools to a zero row.  The readout has no kink: the models' kink sides are the PReLU masks (and the GAT score
sides) of the restatements they are built from."""
import numpy as np

import gat_ref as GR
import gcn_bn_ref as R

GATE_KEY = "pool.gate_nn.weight"          # [1, H], last in state_dict()


def forward(x, a, graph_ptr):
    """(pooled [B, F], alpha [N]) of x [N, F], a [F] (or [F, 1] / [1, F]) over the graphs of graph_ptr [B + 1]."""
    x, a = np.asarray(x, np.float64), np.asarray(a, np.float64).reshape(-1)
    gp = np.asarray(graph_ptr, np.int64)
    s = x @ a
    pooled, alpha = np.zeros((len(gp) - 1, x.shape[1])), np.zeros(x.shape[0])
    for g in range(len(gp) - 1):
        lo, hi = gp[g], gp[g + 1]
        if hi > lo:
            w = np.exp(s[lo:hi] - s[lo:hi].max())
            alpha[lo:hi] = w / w.sum()
            pooled[g] = alpha[lo:hi] @ x[lo:hi]
    return pooled, alpha


def backward(x, a, graph_ptr, dpooled, alpha=None, pooled=None):
    """(dx [N, F], da [F]) from dpooled [B, F]; alpha / pooled: the forward's (recomputed when not given)."""
    x, a = np.asarray(x, np.float64), np.asarray(a, np.float64).reshape(-1)
    gp, dP = np.asarray(graph_ptr, np.int64), np.asarray(dpooled, np.float64)
    if alpha is None or pooled is None:
        pooled, alpha = forward(x, a, gp)
    gid = np.repeat(np.arange(len(gp) - 1), np.diff(gp))
    t = np.einsum("nf,nf->n", dP[gid], x) - np.einsum("bf,bf->b", dP, pooled)[gid]
    w = np.asarray(alpha, np.float64) * t
    return np.asarray(alpha, np.float64)[:, None] * dP[gid] + w[:, None] * a[None, :], w @ x


def init_params(f_in, h=64, seed=0, heads=None):
    """gcn_bn_ref.init_params (heads=None) or gat_ref.init_params with the gate's weight added last, at the scale of torch's
    Linear initialisation."""
    p = R.init_params(f_in, h, seed) if heads is None else GR.init_params(f_in, h, heads, seed)
    p[GATE_KEY] = np.random.default_rng(seed + 3000).uniform(-1, 1, (1, h)) / np.sqrt(h)
    return p


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, heads=None):
    """gcnx.GCN(readout="attention") (heads=None) or gcnx.GAT(heads, readout="attention"): the arguments and the result dict
    of gcn_bn_ref.model / gat_ref.model (no argmax), p with GATE_KEY; grads carries GATE_KEY [1, H] too."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    gat = heads is not None
    if gat:
        rp, ci = GR.pattern(a, n)
        conv = lambda k, inp: GR.gat_conv_fwd(rp, ci, inp, q[f"conv{k}.lin.weight"].T, q[f"conv{k}.att_src"].reshape(heads, -1),
                                              q[f"conv{k}.att_dst"].reshape(heads, -1), q[f"conv{k}.bias"], 0.2, m.get(f"e{k}"))
    else:
        A = R.pyg_norm(a, n)
        conv = lambda k, inp: (A @ (inp @ q[f"conv{k}.lin.weight"].T) + q[f"conv{k}.bias"], inp)
    z1, k1 = conv(1, x)
    zb1, c1 = R.bn_fwd(z1, q["batch_norm_1.weight"], q["batch_norm_1.bias"])
    y1, p1 = R.prelu_fwd(zb1, q["prelu_1.weight"][0], m.get("m1"))
    z2, k2 = conv(2, y1)
    zb2, c2 = R.bn_fwd(z2, q["batch_norm_2.weight"], q["batch_norm_2.bias"])
    y2, p2 = R.prelu_fwd(zb2, q["prelu_2.weight"][0], m.get("m2"))
    gate = q[GATE_KEY].reshape(-1)
    P, alpha = forward(y2, gate, graph_ptr)
    r = R.head(P, {k: v for k, v in p.items() if k != GATE_KEY}, y, denom, m)
    r.update(m1=p1, m2=p2, pooled=P, alpha=alpha, y2=y2)
    if gat:
        r.update(e1=k1["pos"], e2=k2["pos"])
    if y is None:
        return r
    g = r["grads"]
    dy2, dgate = backward(y2, gate, graph_ptr, r["dP"], alpha, P)
    g[GATE_KEY] = dgate[None, :]
    dzb2, g["prelu_2.weight"] = R.prelu_bwd(dy2, zb2, q["prelu_2.weight"][0], p2)
    dz2, g["batch_norm_2.weight"], g["batch_norm_2.bias"] = R.bn_bwd(dzb2, c2, q["batch_norm_2.weight"])
    if gat:
        dy1, dw2, das2, dad2, g["conv2.bias"] = GR.gat_conv_bwd(k2, dz2)
        g["conv2.lin.weight"], g["conv2.att_src"], g["conv2.att_dst"] = dw2.T, das2[None], dad2[None]
    else:
        g["conv2.bias"] = dz2.sum(0)
        t2 = A.T @ dz2
        g["conv2.lin.weight"] = t2.T @ y1
        dy1 = t2 @ q["conv2.lin.weight"]
    dzb1, g["prelu_1.weight"] = R.prelu_bwd(dy1, zb1, q["prelu_1.weight"][0], p1)
    dz1, g["batch_norm_1.weight"], g["batch_norm_1.bias"] = R.bn_bwd(dzb1, c1, q["batch_norm_1.weight"])
    if gat:
        _, dw1, das1, dad1, g["conv1.bias"] = GR.gat_conv_bwd(k1, dz1)
        g["conv1.lin.weight"], g["conv1.att_src"], g["conv1.att_dst"] = dw1.T, das1[None], dad1[None]
    else:
        g["conv1.bias"] = dz1.sum(0)
        g["conv1.lin.weight"] = (A.T @ dz1).T @ x
    return r

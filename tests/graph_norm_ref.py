"""float64 NumPy restatement of GraphNorm (Cai et al. 2021; torch_geometric.nn.GraphNorm(F, eps=1e-5)) fused with a shared-slope
PReLU -- forward and backward -- and of gcnx.GCN / gcnx.GAT with ``norm="graph"``: gcn_bn_ref.model / gat_ref.model with the two
node-level norms replaced (either readout).  No torch.

Per graph g with m rows and per channel, with mean_scale a, weight gamma, bias beta:

    mu = mean_i z_i     o_i = z_i - a mu     v = mean_i o_i^2     r = 1 / sqrt(v + eps)     xh_i = o_i r     t_i = gamma xh_i + beta
    y_i = act(t_i)      act: none | PReLU with one shared slope s

    dt_i = dy_i act'(t_i)        S1 = sum_i dt_i        S2 = sum_i dt_i xh_i        X = sum_i xh_i
    do_i = r gamma (dt_i - xh_i S2 / m)                 D = r gamma (S1 - S2 X / m)
    dz_i = do_i - a D / m
    dgamma = sum_g S2      dbeta = sum_g S1      da = - sum_g mu D      ds = sum_i dy_i min(t_i, 0)

An empty graph has no rows and contributes nothing; its mean and inv rows are zero.  The PReLU side mask ``pos`` (True: t counts
as positive) is an argument, so that a comparison with the device runs on the device's side of every kink."""
import numpy as np

import attn_pool_ref as AR
import gat_ref as GR
import gcn_bn_ref as R

EPS = 1e-5
SCALE_KEYS = ("batch_norm_1.mean_scale", "batch_norm_2.mean_scale")


def forward(z, graph_ptr, a, gamma, beta, slope=None, pos=None, eps=EPS):
    """(y [N, F], cache) of z [N, F]; cache: mean [B, F], inv [B, F], xh, t [N, F], pos [N, F] (None without a slope)."""
    z, a, gamma, beta = (np.asarray(v, np.float64) for v in (z, a, gamma, beta))
    gp = np.asarray(graph_ptr, np.int64)
    b, f = len(gp) - 1, z.shape[1]
    mean, inv, xh = np.zeros((b, f)), np.zeros((b, f)), np.zeros_like(z)
    for g in range(b):
        lo, hi = gp[g], gp[g + 1]
        if hi > lo:
            mean[g] = z[lo:hi].mean(0)
            o = z[lo:hi] - a * mean[g]
            inv[g] = 1.0 / np.sqrt((o * o).mean(0) + eps)
            xh[lo:hi] = o * inv[g]
    t = gamma * xh + beta
    if slope is None:
        return t, {"mean": mean, "inv": inv, "xh": xh, "t": t, "pos": None}
    pos = t > 0 if pos is None else np.asarray(pos, bool)
    return np.where(pos, t, float(slope) * t), {"mean": mean, "inv": inv, "xh": xh, "t": t, "pos": pos}


def backward(dy, z, graph_ptr, a, gamma, beta, slope=None, pos=None, eps=EPS):
    """(dz [N, F], dgamma [F], dbeta [F], da [F], dslope [1]) from dy [N, F]."""
    dy, a, gamma = (np.asarray(v, np.float64) for v in (dy, a, gamma))
    _, c = forward(z, graph_ptr, a, gamma, beta, slope, pos, eps)
    gp = np.asarray(graph_ptr, np.int64)
    xh, t = c["xh"], c["t"]
    if slope is None:
        dt, ds = dy, np.zeros(1)
    else:
        dt = np.where(c["pos"], dy, float(slope) * dy)
        ds = np.array([np.sum(dy * np.where(c["pos"], 0.0, t))])
    f = dy.shape[1]
    dz, dgamma, dbeta, da = np.zeros_like(dy), np.zeros(f), np.zeros(f), np.zeros(f)
    for g in range(len(gp) - 1):
        lo, hi = gp[g], gp[g + 1]
        m = hi - lo
        if m == 0:
            continue
        r, mu = c["inv"][g], c["mean"][g]
        s1, s2, x = dt[lo:hi].sum(0), (dt[lo:hi] * xh[lo:hi]).sum(0), xh[lo:hi].sum(0)
        do = r * gamma * (dt[lo:hi] - xh[lo:hi] * s2 / m)
        d = r * gamma * (s1 - s2 * x / m)
        dz[lo:hi] = do - a * d / m
        dgamma += s2
        dbeta += s1
        da -= mu * d
    return dz, dgamma, dbeta, da, ds


def init_params(f_in, h=64, seed=0, heads=None, readout="max"):
    """The parameters of gcn_bn_ref / gat_ref (with the attention gate for readout="attention") and the two mean_scale vectors,
    away from their initial value 1."""
    if readout == "attention":
        p = AR.init_params(f_in, h, seed, heads)
    else:
        p = R.init_params(f_in, h, seed) if heads is None else GR.init_params(f_in, h, heads, seed)
    rng = np.random.default_rng(seed + 4000)
    for k in SCALE_KEYS:
        p[k] = rng.uniform(0.5, 1.5, h)
    return p


def model(x, a, graph_ptr, p, y=None, denom=None, masks=None, argmax=None, heads=None, readout="max"):
    """gcnx.GCN(norm="graph") (heads=None) or gcnx.GAT(heads, norm="graph") with either readout: the arguments and the result
    dict of gcn_bn_ref.model / gat_ref.model / attn_pool_ref.model; p and grads carry SCALE_KEYS too."""
    m = dict(masks or {})
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    gp = np.asarray(graph_ptr, np.int64)
    gat = heads is not None
    if gat:
        rp, ci = GR.pattern(a, n)
        conv = lambda k, inp: GR.gat_conv_fwd(rp, ci, inp, q[f"conv{k}.lin.weight"].T, q[f"conv{k}.att_src"].reshape(heads, -1),
                                              q[f"conv{k}.att_dst"].reshape(heads, -1), q[f"conv{k}.bias"], 0.2, m.get(f"e{k}"))
    else:
        A = R.pyg_norm(a, n)
        conv = lambda k, inp: (A @ (inp @ q[f"conv{k}.lin.weight"].T) + q[f"conv{k}.bias"], inp)
    norm = lambda k, z: forward(z, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"], q[f"batch_norm_{k}.bias"],
                                q[f"prelu_{k}.weight"][0], m.get(f"m{k}"))
    z1, k1 = conv(1, x)
    y1, c1 = norm(1, z1)
    z2, k2 = conv(2, y1)
    y2, c2 = norm(2, z2)
    cols = np.arange(y2.shape[1])
    head_p = {k: v for k, v in p.items() if k not in SCALE_KEYS and k != AR.GATE_KEY}
    if readout == "attention":
        gate = q[AR.GATE_KEY].reshape(-1)
        P, alpha = AR.forward(y2, gate, gp)
        r = R.head(P, head_p, y, denom, m)
        r.update(alpha=alpha)
    else:
        arg = R.first_argmax(y2, gp) if argmax is None else np.asarray(argmax, np.int64)
        P = np.stack([y2[arg[g], cols] if gp[g + 1] > gp[g] else np.zeros(y2.shape[1]) for g in range(len(gp) - 1)])
        r = R.head(P, head_p, y, denom, m)
        r.update(argmax=arg)
    r.update(m1=c1["pos"], m2=c2["pos"], pooled=P, y1=y1, y2=y2)
    if gat:
        r.update(e1=k1["pos"], e2=k2["pos"])
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

    def norm_bwd(k, dyk, zk, c):
        dz, dg, db, da, ds = backward(dyk, zk, gp, q[f"batch_norm_{k}.mean_scale"], q[f"batch_norm_{k}.weight"],
                                      q[f"batch_norm_{k}.bias"], q[f"prelu_{k}.weight"][0], c["pos"])
        g[f"batch_norm_{k}.weight"], g[f"batch_norm_{k}.bias"], g[f"batch_norm_{k}.mean_scale"], g[f"prelu_{k}.weight"] = dg, db, da, ds
        return dz

    dz2 = norm_bwd(2, dy2, z2, c2)
    if gat:
        dy1, dw2, das2, dad2, g["conv2.bias"] = GR.gat_conv_bwd(k2, dz2)
        g["conv2.lin.weight"], g["conv2.att_src"], g["conv2.att_dst"] = dw2.T, das2[None], dad2[None]
    else:
        g["conv2.bias"] = dz2.sum(0)
        t2 = A.T @ dz2
        g["conv2.lin.weight"] = t2.T @ y1
        dy1 = t2 @ q["conv2.lin.weight"]
    dz1 = norm_bwd(1, dy1, z1, c1)
    if gat:
        _, dw1, das1, dad1, g["conv1.bias"] = GR.gat_conv_bwd(k1, dz1)
        g["conv1.lin.weight"], g["conv1.bias"] = dw1.T, g["conv1.bias"]
        g["conv1.att_src"], g["conv1.att_dst"] = das1[None], dad1[None]
    else:
        g["conv1.bias"] = dz1.sum(0)
        g["conv1.lin.weight"] = (A.T @ dz1).T @ x
    return r

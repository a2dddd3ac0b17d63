"""Host-side checks of the edge-conditioned convolution (no GPU): the fp64 oracle of tests/ecc_ref.py against torch autograd,
its factorised form against its materialised one, the per-entry edge features of the loader, the Keras-shape round trip of
the layer's weights, constructor errors and the ABI version."""
import itertools

import numpy as np
import pytest

import ecc_ref as R
from conftest import rel_err

NETS = (None, [4], [6, 3])
GRID = [(kn, d, root, ub) for kn, d, root, ub in itertools.product(NETS, (False, True), (True, False), (True, False))]


def _case(kn, directed, root, use_bias, seed):
    f, fo, s = 5, 7, 2
    x, idx, e, gp = R.random_batch([6, 0, 9, 4], f, s, density=0.35, directed=directed, seed=seed)
    p = R.init_params(f, fo, s, kn, root, use_bias, seed=seed + 1)
    dy = np.random.default_rng(seed + 2).standard_normal((x.shape[0], fo))
    return x, idx, e, p, dy


def _torch_layer(x, idx, e, p, kn, activation, root, use_bias, dy):
    """Spektral's ECCConv.call (single mode) written with torch ops: gather, einsum, index-add by indices[:, 1]."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)
    tx, te = t(x), t(e)
    tp = {k: t(v) for k, v in p.items()}
    f = x.shape[1]
    fo = p["FGN_out_kernel"].shape[1] // f
    u = te
    for m in range(len(kn or ())):
        u = torch.relu(u @ tp[f"FGN_{m}_kernel"] + tp[f"FGN_{m}_bias"])
    kern = (u @ tp["FGN_out_kernel"] + tp["FGN_out_bias"]).reshape(-1, f, fo)
    src, dst = torch.tensor(idx[:, 0]), torch.tensor(idx[:, 1])
    msg = torch.einsum("ab,abc->ac", tx[src], kern)
    out = torch.zeros((x.shape[0], fo), dtype=torch.float64).index_add(0, dst, msg)
    if root:
        out = out + tx @ tp["root_kernel"]
    if use_bias:
        out = out + tp["bias"]
    if activation == "relu":
        out = torch.relu(out)
    (out * torch.tensor(dy)).sum().backward()
    g = {k: v.grad.numpy() for k, v in tp.items()}
    return out.detach().numpy(), tx.grad.numpy(), te.grad.numpy(), g


@pytest.mark.parametrize("kn,directed,root,use_bias", GRID)
def test_oracle_materialised_form_equals_torch_autograd(kn, directed, root, use_bias):
    for seed, act in ((3, None), (11, "relu")):
        x, idx, e, p, dy = _case(kn, directed, root, use_bias, seed)
        out, dx, de, g = _torch_layer(x, idx, e, p, kn, act, root, use_bias, dy)
        r = R.layer(x, idx, e, p, kn, act, root, use_bias, dy=dy, form="materialised")
        assert rel_err(r["out"], out) < 1e-10
        assert rel_err(r["dx"], dx) < 1e-10
        assert rel_err(r["de"], de) < 1e-10
        assert set(r["grads"]) == set(g) == set(R.param_names(kn, root, use_bias))
        for k in g:
            assert rel_err(r["grads"][k], g[k]) < 1e-10, k


@pytest.mark.parametrize("kn,directed,root,use_bias", GRID)
def test_oracle_factorised_form_equals_materialised_form(kn, directed, root, use_bias):
    for seed, act in ((5, None), (17, "relu")):
        x, idx, e, p, dy = _case(kn, directed, root, use_bias, seed)
        a = R.layer(x, idx, e, p, kn, act, root, use_bias, dy=dy, form="materialised")
        b = R.layer(x, idx, e, p, kn, act, root, use_bias, dy=dy, form="factorised")
        for k in ("out", "pre", "dx", "de"):
            assert rel_err(b[k], a[k]) < 1e-12, k
        for k in a["grads"]:
            assert rel_err(b["grads"][k], a["grads"][k]) < 1e-12, k


def test_oracle_model_gradients_equal_finite_differences_and_both_forms_agree():
    x, idx, e, gp = R.random_batch([5, 7, 0, 4], 3, 2, density=0.4, seed=2)
    h, c = 4, 2
    rng = np.random.default_rng(0)
    params = {"conv1": R.init_params(3, h, 2, [3], seed=1), "conv2": R.init_params(h, h, 2, [3], seed=2),
              "dense_kernel": rng.standard_normal((h, c)), "dense_bias": rng.standard_normal(c)}
    y = np.eye(c)[[0, 1, 1, 0]]
    r = R.model(x, idx, e, gp, params, [3], y=y)
    m = R.model(x, idx, e, gp, params, [3], y=y, form="materialised")
    assert abs(r["loss"] - m["loss"]) < 1e-12 and rel_err(r["grads"]["conv1"]["FGN_0_kernel"], m["grads"]["conv1"]["FGN_0_kernel"]) < 1e-11
    for path in (("conv1", "FGN_0_kernel"), ("conv1", "FGN_out_bias"), ("conv2", "root_kernel"), ("conv2", "bias"), ("dense_kernel",)):
        def get(d):
            for k in path:
                d = d[k]
            return d
        w = get(params)
        it = np.unravel_index(np.argmax(np.abs(get(r["grads"]))), w.shape)
        eps, w0 = 1e-6, w[it]
        w[it] = w0 + eps; lp = R.model(x, idx, e, gp, params, [3], y=y)["loss"]
        w[it] = w0 - eps; lm = R.model(x, idx, e, gp, params, [3], y=y)["loss"]
        w[it] = w0
        assert abs((lp - lm) / (2 * eps) - get(r["grads"])[it]) < 1e-6 * max(1.0, abs(get(r["grads"])[it])), path


def test_oracle_directions_agree_on_undirected_batches_with_symmetric_edge_features():
    """The claim of DESIGN.md ("ECCConv", direction): on the reference's graphs -- undirected, e equal in both directions of an
    edge -- reading the messages as indices[:, 0] -> indices[:, 1] or the other way gives the same layer."""
    x, idx, e, gp = R.random_batch([8, 5], 4, 2, density=0.4, seed=7)
    p = R.init_params(4, 6, 2, [4], seed=8)
    dy = np.random.default_rng(9).standard_normal((13, 6))
    a = R.layer(x, idx, e, p, [4], "relu", dy=dy)
    b = R.layer(x, idx, e, p, [4], "relu", dy=dy, flip=True)
    assert rel_err(b["out"], a["out"]) < 1e-12 and rel_err(b["dx"], a["dx"]) < 1e-12
    xd, idxd, ed, _ = R.random_batch([8, 5], 4, 2, density=0.4, directed=True, seed=7)
    assert rel_err(R.layer(xd, idxd, ed, p, [4], "relu", flip=True)["out"], R.layer(xd, idxd, ed, p, [4], "relu")["out"]) > 1e-3


# ---- loader ------------------------------------------------------------------------------------------------------------------
def _linked_graph(na, nb, bridges, seed):
    """Two chains ``a-*`` / ``b-*`` with self-loops and ``proximity`` on their contacts, joined by bridges that carry ``dca``:
    the shape link_graphs + populate_edge_dca / populate_edge_proximity give a pair (every edge carries both keys, the
    other one 0.0), plus the ``weight`` attribute the loader strips."""
    import networkx as nx
    rng = np.random.default_rng(seed)
    g = nx.Graph()
    for tag, m in (("a", na), ("b", nb)):
        for k in range(m):
            g.add_node(f"{tag}-{k}", x=rng.standard_normal(3))
    for tag, m in (("a", na), ("b", nb)):
        for k in range(m):
            g.add_edge(f"{tag}-{k}", f"{tag}-{k}", weight=0.0)
            if k + 1 < m:
                g.add_edge(f"{tag}-{k}", f"{tag}-{k + 1}", weight=float(rng.random()))
    for i, j in bridges:
        g.add_edge(f"a-{i}", f"b-{j}", weight=1.0)
    for u, v in g.edges:
        bridge = u[0] != v[0]
        g.edges[u, v]["dca"] = float(rng.random()) + 0.5 if bridge else 0.0
    for u, v in g.edges:
        bridge = u[0] != v[0]
        g.edges[u, v]["proximity"] = 0.0 if bridge else float(rng.random()) + 0.5
    return g


def test_entry_edge_features_follow_the_stored_entries():
    import networkx as nx
    from gcnx import DisjointLoader, NetworkxDataset, entry_edge_features, format_graph, from_networkx
    from gcnx.loader import collate_disjoint
    g1, g2 = _linked_graph(3, 2, [(0, 1), (2, 0)], 1), _linked_graph(2, 4, [(1, 3)], 2)
    for g in (g1, g2):
        gr = from_networkx(g, [1, 0], use_edge_data="entries")
        a = gr.a.tocoo()
        nnz = a.nnz
        assert gr.e.shape == (nnz, 2) and nnz == 2 * g.number_of_edges() - nx.number_of_selfloops(g)
        fg = format_graph(g)
        dense = {n: np.zeros(a.shape) for n in ("dca", "proximity")}
        for u, v, d in fg.edges(data=True):
            for n in dense:
                dense[n][u, v] = dense[n][v, u] = d[n]
        order = np.lexsort((a.col, a.row))
        rows, cols = a.row[order], a.col[order]
        assert np.array_equal(gr.e[:, 0], dense["dca"][rows, cols]) and np.array_equal(gr.e[:, 1], dense["proximity"][rows, cols])
        # both directions of an edge carry the same row; bridges have dca only, contacts proximity only
        lut = {(r, c): gr.e[k] for k, (r, c) in enumerate(zip(rows, cols))}
        assert all(np.array_equal(lut[(r, c)], lut[(c, r)]) for r, c in lut)
        assert np.all((gr.e[:, 0] > 0) != (gr.e[:, 1] > 0))
        assert np.array_equal(entry_edge_features(fg, gr.a, names=["proximity"])[:, 0], gr.e[:, 1])
        # use_edge_data=True keeps the reference's per-edge rows (fewer than the stored entries: its TODO's mismatch)
        per_edge = from_networkx(g, [1, 0], use_edge_data=True)
        assert per_edge.e.shape == (g.number_of_edges(), 2) and per_edge.e.shape[0] < nnz
    ds = NetworkxDataset([g1, g2], [[1, 0], [0, 1]], use_edge_data="entries")
    (x, a, e, i), y = collate_disjoint([ds[0], ds[1]])
    assert e.shape == (a.indices.shape[0], 2) and a.indices.shape[0] == ds[0].a.nnz + ds[1].a.nnz
    assert np.array_equal(e, np.vstack([ds[0].e, ds[1].e]))
    n0 = ds[0].n_nodes
    first = a.indices[:, 0] < n0                                     # entry order: graph 0's entries, then graph 1's, row-major
    assert np.array_equal(a.indices[first], np.stack(np.nonzero(ds[0].a.toarray()), 1))
    assert np.array_equal(a.indices[~first] - n0, np.stack(np.nonzero(ds[1].a.toarray()), 1))
    (bx, ba, be, bi), by = next(DisjointLoader(ds, batch_size=2, epochs=1, shuffle=False))
    assert np.array_equal(be, e)
    with pytest.raises(ValueError):
        from_networkx(g1, [1, 0], use_edge_data="edges")


# ---- layer weights, constructor, ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kn,root,use_bias", [(None, True, True), ([4], True, False), ([6, 3], False, True)])
def test_keras_shape_round_trip_of_the_stacked_weight(kn, root, use_bias):
    from gcnx.layers import ecc_pack_weights, ecc_unpack_weights, ecc_weight_names
    f, fo, s = 5, 7, 2
    p = R.init_params(f, fo, s, kn, root, use_bias, seed=4)
    assert ecc_weight_names(kn, root, use_bias) == R.param_names(kn, root, use_bias) == list(p)
    packed = ecc_pack_weights(p, f, fo, root)
    sp = kn[-1] if kn else s
    assert packed["wstack"].shape == ((sp + 1 + root) * f, fo) and packed["wstack"].dtype == np.float32
    # Wk[c, i * F_out + j] = W_c[i, j];  B = reshape(bk);  W_root last
    c, i, j = sp - 1, 3, 2
    assert packed["wstack"][c * f + i, j] == np.float32(p["FGN_out_kernel"][c, i * fo + j])
    assert packed["wstack"][sp * f + i, j] == np.float32(p["FGN_out_bias"][i * fo + j])
    if root:
        assert packed["wstack"][(sp + 1) * f + i, j] == np.float32(p["root_kernel"][i, j])
    back = ecc_unpack_weights(packed, f, fo, root)
    assert set(back) == set(p)
    for k in p:
        assert back[k].shape == np.asarray(p[k]).shape and np.array_equal(back[k], np.asarray(p[k], np.float32)), k
    # the stacked weight is the factorised form's operand: [Scat | x] @ wstack equals the oracle's pre-activation
    x, idx, e, _ = R.random_batch([6, 5], f, s, seed=1)
    r = R.layer(x, idx, e, p, kn, None, root, False)
    um = r["u"][-1]
    uh = np.concatenate([um, np.ones((um.shape[0], 1))], 1)
    scat = np.zeros((x.shape[0], (sp + 1) * f))
    np.add.at(scat, idx[:, 1], (uh[:, :, None] * x[idx[:, 0]][:, None, :]).reshape(-1, (sp + 1) * f))
    sx = np.concatenate([scat, x], 1) if root else scat
    assert rel_err(sx @ packed["wstack"].astype(np.float64), r["pre"]) < 1e-6
    with pytest.raises(ValueError):
        ecc_pack_weights({**p, "FGN_out_bias": np.zeros(3)}, f, fo, root)


def test_constructor_errors():
    from gcnx.layers import ECCConv
    with pytest.raises(NotImplementedError):
        ECCConv(8, activation="tanh")
    with pytest.raises(ValueError):
        ECCConv(0)
    with pytest.raises(ValueError):
        ECCConv(8, kernel_network=[4, 0])
    with pytest.raises(ValueError):
        ECCConv(8, kernel_network=[2.5])
    with pytest.raises(NotImplementedError):
        ECCConv(8, kernel_network=[8, 17])               # C = 18 > 17
    layer = ECCConv(8, kernel_network=[8, 16], activation="relu")
    assert layer.sp == 16 and layer.kernel_network == [8, 16]
    with pytest.raises(ValueError):
        layer._param_spec(4)                             # edge width unknown until the first call
    wide = ECCConv(8)
    wide.edge_dim = 17
    with pytest.raises(NotImplementedError):
        wide._param_spec(4)                              # 17 raw edge channels + 1 > 17
    layer.edge_dim = 2
    spec = {k: s for k, s, _ in layer._param_spec(4)}
    assert spec == {"FGN_0_kernel": (2, 8), "FGN_0_bias": (8,), "FGN_1_kernel": (8, 16), "FGN_1_bias": (16,),
                    "wstack": (18 * 4, 8), "bias": (8,)}
    init = {k: v for k, _, v in layer._param_spec(4)}
    assert np.all(init["bias"] == 0) and np.all(init["wstack"][16 * 4:17 * 4] == 0)       # FGN_out bias starts at zero
    lim = np.sqrt(6.0 / (16 + 4 * 8))                                                    # glorot on FGN_out's Keras shape
    assert np.abs(init["wstack"][:16 * 4]).max() <= lim and np.abs(init["wstack"][:16 * 4]).max() > 0.8 * lim


def test_eccnet_constructor_errors_need_no_device():
    """The arguments ECCNet refuses are refused before the context is touched (the undecorated constructor, ctx = None)."""
    from gcnx.models import ECCNet
    init = ECCNet.__init__.__wrapped__
    for kw in ({"comm": object()}, {"prec": "bf16"}, {"prec": "bf16x3"}, {"pool": "max"}):
        with pytest.raises(NotImplementedError):
            init(object.__new__(ECCNet), None, **kw)
    with pytest.raises(ValueError):
        init(object.__new__(ECCNet), None, kernel_network=[0])
    m = object.__new__(ECCNet)
    init(m, None, n_labels=2, channels=64, kernel_network=[8])
    assert (m.channels, m.kernel_network, m.conv1.activation, m.conv2.sp, m.built) == (64, [8], "relu", 8, False)


def test_abi_version_and_entry_points():
    from gcnx import _lib
    lib = _lib.load()
    assert lib.gcnx_version() >= 403
    for name in ("gcnx_ecc_expand", "gcnx_ecc_bwd", "gcnx_csr_transpose_perm"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

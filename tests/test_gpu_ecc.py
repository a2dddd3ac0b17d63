"""GPU tests of the edge-conditioned convolution: the two gathers of csrc/ecc.hip through the C ABI, gcnx.layers.ECCConv and
gcnx.ECCNet against the fp64 oracle of tests/ecc_ref.py at the project's fp32 bar (assert_close 1e-4), reproducibility, the
message direction, edge features in the batch, and the older models fed batches that carry e.

ReLU kinks (the layers' activation, the kernel network's) are evaluated on the device's side (``masks``), as
tests/gcn_bn_ref.py does, and ``_kinks_ok`` bounds what that may hide: per tensor the device's sides differ from the oracle's
own only where the oracle's pre-activation is within 1e-5 of the tensor's largest magnitude, and on at most 1e-4 of its
elements."""
import itertools

import numpy as np
import pytest

import ecc_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _csr(ctx, idx, n, gp=None):
    from gcnx import device as D
    return D.DeviceCSR.from_coo(ctx, idx, None, n, graph_ptr=gp, weighted=False)


def _gather_ref(x, idx, u, root):
    """fp64 reference of gcnx_ecc_expand: [Scat | x]."""
    n, f = x.shape
    uh = np.concatenate([u, np.ones((idx.shape[0], 1))], 1)
    scat = np.zeros((n, uh.shape[1] * f))
    np.add.at(scat, idx[:, 1], (uh[:, :, None] * x[idx[:, 0]][:, None, :]).reshape(-1, uh.shape[1] * f))
    return np.concatenate([scat, x], 1) if root else scat


def _bwd_ref(x, idx, u, dscat, dx_root):
    n, f = x.shape
    sp = u.shape[1]
    uh = np.concatenate([u, np.ones((idx.shape[0], 1))], 1)
    d = dscat.reshape(n, sp + 1, f)[idx[:, 1]]
    dx = dx_root.copy()
    np.add.at(dx, idx[:, 0], np.einsum("ac,aci->ai", uh, d))
    return dx, np.einsum("ai,aci->ac", x[idx[:, 0]], d[:, :sp])


def _kernel_inputs(f, c, directed, seed, sizes=(7, 0, 12, 3, 1)):
    sp = c - 1
    x, idx, e, gp = R.random_batch(list(sizes), f, max(sp, 1), density=0.25, directed=directed, seed=seed, self_loops=False)
    rng = np.random.default_rng(seed + 100)
    u = e[:, :sp] - 0.3
    n = x.shape[0]
    assert np.any(np.bincount(idx[:, 0], minlength=n) == 0) and np.any(np.bincount(idx[:, 1], minlength=n) == 0)   # empty rows
    return (x.astype(np.float32), idx, u.astype(np.float32), gp, rng.standard_normal((n, c * f)).astype(np.float32),
            rng.standard_normal((n, f)).astype(np.float32))


@pytest.mark.parametrize("f", [1, 4, 10, 16, 64, 100])
@pytest.mark.parametrize("c", [1, 3, 9, 17])
@pytest.mark.parametrize("directed", [False, True])
def test_ecc_kernels_against_the_oracle(ctx, f, c, directed):
    """gcnx_ecc_expand and gcnx_ecc_bwd: float4 and plain paths, empty rows and graphs, every NULL combination of dx / du,
    with and without the root copy, twice (bit-identical)."""
    from gcnx import device as D
    x, idx, u, gp, dscat, dxr = _kernel_inputs(f, c, directed, seed=f * 31 + c)
    n, sp = x.shape[0], c - 1
    a = _csr(ctx, idx, n, gp)
    assert a.symmetric == (not directed)
    d_x, d_u = ctx.to_device(x), (ctx.to_device(u) if sp else None)
    for root in (False, True):
        ref = _gather_ref(x.astype(np.float64), idx, u.astype(np.float64), root)
        out = ctx.to_device(np.full(ref.shape, 7.0, np.float32))
        D.ecc_expand(ctx, a, d_u, d_x, out, root=root)
        got = out.numpy()
        assert_close(got, ref, TOL, f"ecc_expand f={f} c={c} root={root}")
        D.ecc_expand(ctx, a, d_u, d_x, out, root=root)
        assert np.array_equal(out.numpy(), got)
    d_ds, d_dxr = ctx.to_device(dscat), ctx.to_device(dxr)
    rdx, rdu = _bwd_ref(x.astype(np.float64), idx, u.astype(np.float64), dscat.astype(np.float64), dxr.astype(np.float64))
    rdx0, _ = _bwd_ref(x.astype(np.float64), idx, u.astype(np.float64), dscat.astype(np.float64), np.zeros_like(rdx))
    dx, du = ctx.empty((n, f)), (ctx.empty((idx.shape[0], sp)) if sp else None)
    D.ecc_bwd(ctx, a, d_u, d_x, d_ds, d_dxr, dx, du)
    g_dx, g_du = dx.numpy(), (du.numpy() if sp else None)
    assert_close(g_dx, rdx, TOL, f"ecc_bwd dx f={f} c={c}")
    if sp:
        assert_close(g_du, rdu, TOL, f"ecc_bwd du f={f} c={c}")
    dx2 = ctx.empty((n, f))
    D.ecc_bwd(ctx, a, d_u, d_x, d_ds, d_dxr, dx2, None)                    # dx alone: the same bits
    assert np.array_equal(dx2.numpy(), g_dx)
    D.ecc_bwd(ctx, a, d_u, d_x, d_ds, None, dx2, None)                     # no root term
    assert_close(dx2.numpy(), rdx0, TOL, "ecc_bwd dx without dx_root")
    if sp:
        du2 = ctx.empty((idx.shape[0], sp))
        D.ecc_bwd(ctx, a, d_u, d_x, d_ds, None, None, du2)                 # du alone: the same bits
        assert np.array_equal(du2.numpy(), g_du)
    D.ecc_bwd(ctx, a, d_u, d_x, d_ds, d_dxr, d_dxr, None)                  # dx may alias dx_root
    assert np.array_equal(d_dxr.numpy(), g_dx)


@pytest.mark.parametrize("f,off", [(16, 4), (16, 1), (10, 3), (64, 8)])
def test_ecc_kernels_honour_leading_dimensions(ctx, f, off):
    """Every operand as a column view of a wider buffer (off % 4 == 0 keeps the float4 path, otherwise the plain one); what
    lies outside the views is left untouched."""
    from gcnx import device as D
    c = 3
    x, idx, u, gp, dscat, dxr = _kernel_inputs(f, c, True, seed=5)
    n, sp, nnz = x.shape[0], c - 1, idx.shape[0]
    a = _csr(ctx, idx, n, gp)

    def wide(arr, extra=8):
        host = np.full((arr.shape[0], arr.shape[1] + off + extra), -3.0, np.float32)
        host[:, off:off + arr.shape[1]] = arr
        big = ctx.to_device(host)
        return big, big.cols(off, off + arr.shape[1])
    _, vx = wide(x)
    _, vu = wide(u)
    bo, vo = wide(np.zeros((n, (c + 1) * f), np.float32))
    D.ecc_expand(ctx, a, vu, vx, vo, root=True)
    ref = _gather_ref(x.astype(np.float64), idx, u.astype(np.float64), True)
    full = bo.numpy()
    assert_close(full[:, off:off + ref.shape[1]], ref, TOL, "strided ecc_expand")
    assert np.all(full[:, :off] == -3.0) and np.all(full[:, off + ref.shape[1]:] == -3.0)
    _, vds = wide(dscat)
    _, vdr = wide(dxr)
    bdx, vdx = wide(np.zeros((n, f), np.float32))
    bdu, vdu = wide(np.zeros((nnz, sp), np.float32))
    D.ecc_bwd(ctx, a, vu, vx, vds, vdr, vdx, vdu)
    rdx, rdu = _bwd_ref(x.astype(np.float64), idx, u.astype(np.float64), dscat.astype(np.float64), dxr.astype(np.float64))
    fdx, fdu = bdx.numpy(), bdu.numpy()
    assert_close(fdx[:, off:off + f], rdx, TOL, "strided dx")
    assert_close(fdu[:, off:off + sp], rdu, TOL, "strided du")
    assert np.all(fdx[:, :off] == -3.0) and np.all(fdx[:, off + f:] == -3.0)
    assert np.all(fdu[:, :off] == -3.0) and np.all(fdu[:, off + sp:] == -3.0)


def test_ecc_expand_identity_and_explicit_entry_permutation(ctx):
    """eperm NULL (the CSR handed in is the destination side and u is in its order) against the permuted form on the
    transposed pattern: the same bits; and gcnx_csr_transpose_perm returns a permutation that maps entries to entries."""
    from gcnx import device as D
    x, idx, u, gp, _, _ = _kernel_inputs(16, 3, True, seed=9)
    n = x.shape[0]
    a = _csr(ctx, idx, n, gp)
    rp, ci, pm = (v.numpy() for v in a.transpose_perm())
    nnz = idx.shape[0]
    assert sorted(pm[:nnz].tolist()) == list(range(nnz))
    dst = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(idx[pm[:nnz]], np.stack([ci[:nnz], dst], 1))        # transposed entry p = original entry perm[p]
    assert np.all(np.diff(pm[:nnz].reshape(-1))[np.diff(dst) == 0] > 0)       # stable: a row's entries keep their order
    d_x = ctx.to_device(x)
    out1, out2 = ctx.empty((n, 48)), ctx.empty((n, 48))
    D.ecc_expand(ctx, a, ctx.to_device(u), d_x, out1)
    at = _csr(ctx, np.stack([dst, ci[:nnz]], 1), n, gp)                        # the destination-side CSR as an operator
    D.ecc_expand(ctx, at, ctx.to_device(u[pm[:nnz]]), d_x, out2, identity_perm=True)
    assert np.array_equal(out1.numpy(), out2.numpy())


def test_ecc_long_row_of_4096_entries(ctx):
    """A hub with 4096 incoming and 4096 outgoing entries (the row length of synth.power_law_batch's hubs): the chunk
    outgrows the LDS staging and the tail is read from memory."""
    from gcnx import device as D
    n, f, sp = 4097, 16, 2
    rng = np.random.default_rng(0)
    leaves = np.arange(1, n)
    idx = np.concatenate([np.stack([np.zeros(n - 1, np.int64), leaves], 1), np.stack([leaves, np.zeros(n - 1, np.int64)], 1),
                          np.stack([np.arange(n), np.arange(n)], 1)])
    idx = idx[np.lexsort((idx[:, 1], idx[:, 0]))]
    x = rng.standard_normal((n, f)).astype(np.float32)
    u = rng.random((idx.shape[0], sp)).astype(np.float32)
    a = _csr(ctx, idx, n)
    assert np.diff(a.rowptr.numpy()).max() == 4097 - 0
    out = ctx.empty((n, 3 * f))
    D.ecc_expand(ctx, a, ctx.to_device(u), ctx.to_device(x), out)
    assert_close(out.numpy(), _gather_ref(x.astype(np.float64), idx, u.astype(np.float64), False), TOL, "hub expand")
    dscat = rng.standard_normal((n, 3 * f)).astype(np.float32)
    dx, du = ctx.empty((n, f)), ctx.empty((idx.shape[0], sp))
    D.ecc_bwd(ctx, a, ctx.to_device(u), ctx.to_device(x), ctx.to_device(dscat), None, dx, du)
    rdx, rdu = _bwd_ref(x.astype(np.float64), idx, u.astype(np.float64), dscat.astype(np.float64), np.zeros((n, f)))
    assert_close(dx.numpy(), rdx, TOL, "hub dx")
    assert_close(du.numpy(), rdu, TOL, "hub du")


def test_ecc_more_than_17_channels_are_refused_before_any_launch(ctx):
    from gcnx import _lib
    from gcnx import device as D
    x, idx, _, gp, _, _ = _kernel_inputs(4, 3, False, seed=2)
    n, nnz = x.shape[0], idx.shape[0]
    a = _csr(ctx, idx, n, gp)
    u = ctx.to_device(np.ones((nnz, 17), np.float32))                        # C = 18
    out = ctx.to_device(np.full((n, 18 * 4), 5.0, np.float32))
    with pytest.raises(_lib.GcnxError) as ei:
        D.ecc_expand(ctx, a, u, ctx.to_device(x), out)
    assert ei.value.code == _lib.ERR_UNSUPPORTED and "17" in str(ei.value)
    assert np.all(out.numpy() == 5.0)
    dx = ctx.to_device(np.full((n, 4), 5.0, np.float32))
    with pytest.raises(_lib.GcnxError) as ei:
        D.ecc_bwd(ctx, a, u, ctx.to_device(x), out, None, dx, None)
    assert ei.value.code == _lib.ERR_UNSUPPORTED and "gcnx_ecc_bwd" in str(ei.value)
    assert np.all(dx.numpy() == 5.0)
    u16 = ctx.to_device(np.ones((nnz, 16), np.float32))                      # C = 17: served
    D.ecc_expand(ctx, a, u16, ctx.to_device(x), ctx.empty((n, 17 * 4)))


def test_message_direction_is_row_to_column(ctx):
    """One directed stored entry (0, 1): the message lands in row 1, row 0 holds its root term only."""
    from gcnx.layers import ECCConv
    x = np.array([[1.0, 2.0], [3.0, -1.0]], np.float32)
    idx = np.array([[0, 1]], np.int64)
    e = np.array([[0.5, 2.0]], np.float32)
    a = _csr(ctx, idx, 2, np.array([0, 2]))
    layer = ECCConv(3, seed=1)
    y = layer([ctx.to_device(x), a, ctx.to_device(e)]).numpy()
    p = layer.get_weights(as_dict=True)
    p["bias"] = np.array([0.1, -0.2, 0.3], np.float32)
    p["FGN_out_bias"] = np.linspace(-1, 1, 6).astype(np.float32)
    layer.set_weights(p)
    y = layer([ctx.to_device(x), a, ctx.to_device(e)]).numpy()
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    kern = (e.astype(np.float64) @ p64["FGN_out_kernel"] + p64["FGN_out_bias"]).reshape(2, 3)
    root = x.astype(np.float64) @ p64["root_kernel"] + p64["bias"]
    assert_close(y[0], root[0], TOL, "row 0: root term only")
    assert_close(y[1], root[1] + x[0].astype(np.float64) @ kern, TOL, "row 1: root + the message from row 0")
    assert np.abs(x[0].astype(np.float64) @ kern).max() > 0.1


# ---- batches with edge features ------------------------------------------------------------------------------------------------------
def _host_inputs(x, idx, e, gp, ctx=None):
    """(x, a, e, i) as DisjointLoader yields it; with ctx the graph segments themselves stand for i (an id vector cannot
    say that the LAST graph has no rows)."""
    from gcnx import device as D
    from gcnx.loader import SparseTensor
    n = x.shape[0]
    i = D.Segments(ctx, gp) if ctx is not None else np.repeat(np.arange(len(gp) - 1), np.diff(gp))
    return (x, SparseTensor(idx, np.ones(idx.shape[0]), (n, n)), e, i)


def test_device_batch_keeps_e_in_csr_entry_order(ctx):
    import scipy.sparse as sp
    from gcnx.models import DeviceBatch
    x, idx, e, gp = R.random_batch([6, 9, 4], 5, 2, directed=True, seed=3)
    b = DeviceBatch.from_host(ctx, _host_inputs(x, idx, e, gp), np.eye(2)[[0, 1, 0]])
    rp, ci = b.a.rowptr.numpy(), b.a.colidx.numpy()
    assert np.array_equal(np.stack([np.repeat(np.arange(x.shape[0]), np.diff(rp)), ci[:idx.shape[0]]], 1), idx)   # CSR entry k = COO entry k
    assert b.e.shape == e.shape and np.array_equal(b.e.numpy(), e.astype(np.float32))
    assert DeviceBatch.from_host(ctx, (x, _host_inputs(x, idx, e, gp)[1], _host_inputs(x, idx, e, gp)[3])).e is None
    with pytest.raises(ValueError):
        DeviceBatch.from_host(ctx, _host_inputs(x, idx, e[:-1], gp))                       # one row per undirected edge, say
    # an explicitly stored zero of a scipy adjacency is dropped by the COO build: e with a row for it is refused
    m = sp.csr_matrix((np.array([1.0, 0.0, 1.0]), (np.array([0, 0, 1]), np.array([0, 1, 1]))), shape=(2, 2))
    i2 = np.zeros(2, np.int64)
    with pytest.raises(ValueError):
        DeviceBatch.from_host(ctx, (x[:2], m, np.ones((3, 2)), i2))
    assert DeviceBatch.from_host(ctx, (x[:2], m, np.ones((2, 2)), i2)).e.shape == (2, 2)


# ---- ECCConv -------------------------------------------------------------------------------------------------------------------------
def _kinks_ok(pre, side, what):
    cnt, worst, size = R.kink_report(pre, side)
    assert worst <= 1e-5, (what, "a ReLU side differs where the oracle's pre-activation is not near zero", worst)
    assert cnt <= 1e-4 * size, (what, "too many ReLU sides differ", cnt, size)


def _layer_masks(layer):
    _, _, us, _, y = layer._saved
    return {"act": y.numpy() > 0, "kn": [u.numpy() > 0 for u in us[1:]]}


def _check_layer_kinks(rec, masks, what):
    if masks.get("act") is not None:
        _kinks_ok(rec["pre"], masks["act"], what + " activation")
    for m, pre in enumerate(rec["kn_pre"]):
        _kinks_ok(pre, masks["kn"][m], f"{what} kernel network {m}")


NETS = (None, [4], [6, 3])


@pytest.mark.parametrize("kn,directed,root,use_bias", list(itertools.product(NETS, (False, True), (True, False), (True, False))))
def test_eccconv_forward_and_backward(ctx, kn, directed, root, use_bias):
    from gcnx.layers import ECCConv
    f, fo, s = 5, 8, 2
    for seed, act in ((3, None), (11, "relu")):
        x, idx, e, gp = R.random_batch([16, 0, 23, 9], f, s, density=0.3, directed=directed, seed=seed)
        n = x.shape[0]
        p = {k: v.astype(np.float32) for k, v in R.init_params(f, fo, s, kn, root, use_bias, seed=seed + 1).items()}
        dy = np.random.default_rng(seed + 2).standard_normal((n, fo)).astype(np.float32)
        x32, e32 = x.astype(np.float32), e.astype(np.float32)
        a = _csr(ctx, idx, n, gp)
        layer = ECCConv(fo, kn, root=root, activation=act, use_bias=use_bias, seed=0)
        d_x, d_e = ctx.to_device(x32), ctx.to_device(e32)
        layer([d_x, a, d_e])
        layer.set_weights(p)
        back = layer.get_weights(as_dict=True)
        assert all(np.array_equal(back[k], p[k]) for k in p) and set(back) == set(p)
        y = layer([d_x, a, d_e]).numpy()
        masks = _layer_masks(layer) if (act or kn) else {}
        if not act:
            masks.pop("act", None)
        ref = R.layer(x32, idx, e32, p, kn, act, root, use_bias, dy=dy, masks=masks)
        _check_layer_kinks(ref, masks, f"ECCConv {kn} {act}")
        assert_close(y, ref["out"], TOL, "ECCConv out")
        dx = layer.backward(ctx.to_device(dy)).numpy()
        assert_close(dx, ref["dx"], TOL, "ECCConv dx")
        g = layer.gradients()
        assert set(g) == set(ref["grads"])
        for k in g:
            assert_close(g[k], ref["grads"][k], TOL, f"ECCConv d{k}")
        assert layer.backward(ctx.to_device(dy), need_dx=False) is None                    # the first layer of a model
        g2 = layer.gradients()
        for k in g:
            assert_close(g2[k], ref["grads"][k], TOL, f"ECCConv d{k} (need_dx=False)")
        if not kn:                                                                         # no gather at all then: the same launches
            assert all(np.array_equal(g2[k], g[k]) for k in g)


def test_kernel_network_shapes_run_on_the_weight_gemms(ctx):
    """The hidden layers of the kernel network are [nnz, 2] -> [nnz, 8] products and the like: gcnx_gemm /
    gcnx_act_bias_grad / gcnx_gemm_dw / gcnx_gemm_dx take such shapes (ragged widths, rows in the tens of thousands)."""
    from gcnx import device as D
    rng = np.random.default_rng(0)
    for n, fi, fo in ((30011, 2, 8), (1000, 6, 3), (7, 2, 1)):
        x, w, b = rng.standard_normal((n, fi)).astype(np.float32), rng.standard_normal((fi, fo)).astype(np.float32), rng.standard_normal(fo).astype(np.float32)
        dy = rng.standard_normal((n, fo)).astype(np.float32)
        d_x, d_w, out = ctx.to_device(x), ctx.to_device(w), ctx.empty((n, fo))
        D.gemm(ctx, d_x, d_w, ctx.to_device(b), out, act="relu")
        z = x.astype(np.float64) @ w + b
        y = out.numpy()
        side = y > 0
        _kinks_ok(z, side, "kernel network layer")
        assert_close(y, np.where(side, z, 0), TOL, "kn gemm")
        dz, db, dw, dxo = ctx.empty((n, fo)), ctx.empty(fo), ctx.empty((fi, fo)), ctx.empty((n, fi))
        D.act_bias_grad(ctx, ctx.to_device(dy), out, dz, "relu", db=db)
        rdz = np.where(side, dy.astype(np.float64), 0)
        assert_close(dz.numpy(), rdz, TOL, "kn dz")
        assert_close(db.numpy(), rdz.sum(0), TOL, "kn db")
        D.gemm_dw(ctx, d_x, dz, dw)
        assert_close(dw.numpy(), x.astype(np.float64).T @ rdz, TOL, "kn dW")
        D.gemm_dx(ctx, dz, d_w, dxo)
        assert_close(dxo.numpy(), rdz @ w.astype(np.float64).T, TOL, "kn dx")


# ---- ECCNet ----------------------------------------------------------------------------------------------------------------------
def _net_batch(b, f, seed, with_empty=False):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(10, 40, b).tolist()
    if with_empty:
        sizes[1] = 0
        sizes[-1] = 0
    x, idx, e, gp = R.random_batch(sizes, f, 2, density=0.15, seed=seed)
    y = np.eye(2)[rng.integers(0, 2, b)]
    return x.astype(np.float32), idx, e.astype(np.float32), gp, y.astype(np.float32)


def _net_params(f, h, kn, seed):
    rng = np.random.default_rng(seed)
    p = {"conv1": R.init_params(f, h, 2, kn, seed=seed + 1), "conv2": R.init_params(h, h, 2, kn, seed=seed + 2),
         "dense_kernel": rng.uniform(-1, 1, (h, 2)) * np.sqrt(6.0 / (h + 2)), "dense_bias": rng.uniform(-0.1, 0.1, 2)}
    # activations of a sum-pooled, unnormalised two-layer model grow with the degree: keep the logits of order one
    for c in ("conv1", "conv2"):
        p[c]["FGN_out_kernel"] *= 0.3
        p[c]["FGN_out_bias"] *= 0.3
        p[c]["root_kernel"] *= 0.5
    p["dense_kernel"] *= 0.1
    f32 = lambda d: {k: (f32(v) if isinstance(v, dict) else np.asarray(v, np.float32)) for k, v in d.items()}
    return f32(p)


def _net_masks(model):
    return {"conv1": _layer_masks(model.conv1), "conv2": _layer_masks(model.conv2)}


def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "/"))
        else:
            out[prefix + k] = np.asarray(v)
    return out


def _cce_probs_loss(probs, y, denom):
    p = probs / probs.sum(1, keepdims=True)
    return float(-np.sum(y * np.log(np.clip(p, 1e-7, 1 - 1e-7))) / denom)


@pytest.mark.parametrize("h,b,kn,with_empty", [(32, 12, None, False), (64, 50, None, False), (32, 8, [8], False), (64, 20, [6, 3], True),
                                               (32, 9, None, True)])
def test_eccnet_step_against_the_oracle(ctx, h, b, kn, with_empty):
    """Loss, probabilities, every gradient, and the weights after five SGD steps at the reference's first learning rate
    (0.02, gcn.py:321-324) on a reference-sized batch (F_in 16); evaluate_batch in both cross-entropy readings."""
    import gcnx
    from gcnx.models import DeviceBatch
    f = 16
    x, idx, e, gp, y = _net_batch(b, f, seed=h + b, with_empty=with_empty)
    params = _net_params(f, h, kn, seed=b)
    model = gcnx.ECCNet(ctx, 2, channels=h, kernel_network=kn, seed=1)
    batch = DeviceBatch.from_host(ctx, _host_inputs(x, idx, e, gp, ctx), y)
    assert batch.n_graphs == b
    model.build(f, 2)
    model.set_weights(params)
    got = _flat(model.get_weights(as_dict=True))
    assert all(np.array_equal(got[k], v) for k, v in _flat(params).items())
    probs = model(batch)
    masks = _net_masks(model)
    ref = R.model(x, idx, e, gp, params, kn, y=y, masks=masks)
    for c in ("conv1", "conv2"):
        _check_layer_kinks(ref[c], masks[c], f"ECCNet {c}")
    assert_close(probs, ref["probs"], TOL, "ECCNet probabilities")
    # evaluate_batch: the eager ("probs") and the from-logits reading of the loss
    loss, acc, pr = model.evaluate_batch(batch, None)
    assert np.array_equal(pr, probs)
    assert abs(loss - _cce_probs_loss(ref["probs"], y, b)) < TOL * max(1.0, ref["loss"]) and acc == ref["hits"] / b
    model.cce_eval = "logits"
    loss, acc, _ = model.evaluate_batch(batch, None)
    assert abs(loss - ref["loss"]) < TOL * max(1.0, ref["loss"]) and acc == ref["hits"] / b
    # gradients
    model.loss_and_grads(batch)
    la = model.loss_acc.numpy()
    assert abs(la[0] - ref["loss"]) < TOL * max(1.0, ref["loss"]) and la[1] == ref["hits"]
    g, rg = _flat(model.gradients()), _flat(ref["grads"])
    assert set(g) == set(rg)
    for k in rg:
        assert_close(g[k], rg[k], TOL, f"ECCNet d{k}")
    before = _flat(model.get_weights(as_dict=True))
    assert all(np.array_equal(before[k], v) for k, v in _flat(params).items())            # no update without a rate
    # five SGD steps
    cur = params
    for step in range(5):
        loss, acc = model.train_step(batch, None, lr=0.02)
        masks = _net_masks(model)
        r = R.model(x, idx, e, gp, cur, kn, y=y, masks=masks)
        for c in ("conv1", "conv2"):
            _check_layer_kinks(r[c], masks[c], f"ECCNet step {step} {c}")
        assert abs(loss - r["loss"]) < TOL * max(1.0, r["loss"]), (step, loss, r["loss"])
        cur = R.sgd(cur, r["grads"], 0.02)
    got, want = _flat(model.get_weights(as_dict=True)), _flat(cur)
    for k in want:
        assert_close(got[k], want[k], TOL, f"ECCNet {k} after five steps")
    assert len(model.get_weights()) == len(want)


def test_eccnet_reads_e(ctx):
    """The output changes when the rows of e are permuted (an implementation that ignores e, or pairs rows with the wrong
    entries, fails), and by what the oracle says it should."""
    import gcnx
    from gcnx.models import DeviceBatch
    x, idx, e, gp, y = _net_batch(10, 16, seed=4)
    params = _net_params(16, 32, None, seed=5)
    model = gcnx.ECCNet(ctx, 2, channels=32, seed=0)
    model.build(16, 2)
    model.set_weights(params)
    p0 = model(DeviceBatch.from_host(ctx, _host_inputs(x, idx, e, gp)))
    perm = np.random.default_rng(0).permutation(e.shape[0])
    p1 = model(DeviceBatch.from_host(ctx, _host_inputs(x, idx, e[perm], gp)))
    r0 = R.model(x, idx, e, gp, params, masks=None)["probs"]
    r1 = R.model(x, idx, e[perm], gp, params, masks=None)["probs"]
    assert np.abs(r1 - r0).max() > 1e-3 and np.abs(p1 - p0).max() > 0.5 * np.abs(r1 - r0).max()
    # each side is held to 1e-4 of max |p| <= 1 by the project's bar, so their difference to 2e-4 absolute
    assert np.abs((p1 - p0) - (r1 - r0)).max() < 2e-4
    with pytest.raises(ValueError):
        model((x, _host_inputs(x, idx, e, gp)[1], _host_inputs(x, idx, e, gp)[3]))        # no e
    with pytest.raises(NotImplementedError):
        gcnx.ECCNet(ctx, 2, comm=object())
    with pytest.raises(NotImplementedError):
        gcnx.ECCNet(ctx, 2, prec="bf16")


def test_fit_over_a_host_loader_equals_the_steps_by_hand(ctx):
    """gcnx.fit / gcnx.evaluate drive ECCNet unchanged: two epochs over a DisjointLoader of Graph(e=...) leave the same bits
    as the same train_step calls made by hand with the reference's schedule."""
    import scipy.sparse as sp
    import gcnx
    from gcnx.models import DeviceBatch
    rng = np.random.default_rng(3)
    graphs = []
    for k in range(10):
        x, idx, e, gp = R.random_batch([int(rng.integers(8, 20))], 16, 2, density=0.3, seed=100 + k)
        n = x.shape[0]
        a = sp.csr_matrix((np.ones(idx.shape[0]), (idx[:, 0], idx[:, 1])), shape=(n, n))
        graphs.append(gcnx.Graph(x=x, a=a, e=e, y=np.eye(2)[k % 2]))
    ds = gcnx.ListDataset(graphs)

    def make():
        m = gcnx.ECCNet(ctx, 2, channels=32, kernel_network=[8], seed=7)
        return m
    m1 = make()
    out = gcnx.fit(m1, gcnx.DisjointLoader(ds, batch_size=4, epochs=2, shuffle=False),
                   gcnx.DisjointLoader(ds, batch_size=5, shuffle=False), epochs=2, verbose=False)
    m2 = make()
    sched = gcnx.PiecewiseConstantDecay.reference(2)
    losses = []
    for it, (inputs, target) in enumerate(gcnx.DisjointLoader(ds, batch_size=4, epochs=2, shuffle=False)):
        assert len(inputs) == 4
        losses.append(m2.train_step(DeviceBatch.from_host(ctx, inputs, target), None, lr=sched(it)))
    w1, w2 = m1.get_weights(), m2.get_weights()
    assert len(w1) == len(w2) and all(np.array_equal(u, v) for u, v in zip(w1, w2))
    assert all(np.array_equal(u, v) for u, v in zip(out["weights"][-1], w2))
    per_epoch = np.array(losses, np.float64).reshape(2, 3, 2).mean(1)
    assert np.allclose(np.array(out["history"])[:, :2], per_epoch, rtol=1e-6, atol=0)
    (te_loss, te_acc), preds = gcnx.train.evaluate(m2, gcnx.DisjointLoader(ds, batch_size=5, shuffle=False))
    assert np.allclose(out["history"][-1][2:], (te_loss, te_acc), rtol=1e-6, atol=0) and len(preds) == 2


# ---- the other models ignore e -------------------------------------------------------------------------------------------------------
def test_other_models_ignore_e_bit_for_bit(ctx):
    """GCN2, GeneralGNN, GCN and DeviceDataset fed batches that carry e give the results of the batches without it."""
    import scipy.sparse as sp
    import gcnx
    from gcnx.device_loader import collate_on_device
    x, idx, e, gp, y = _net_batch(9, 16, seed=21)
    x4 = _host_inputs(x, idx, e, gp)
    x3 = (x4[0], x4[1], x4[3])

    def run(make, inputs, target):
        m = make()
        loss = m.train_step(inputs, target, lr=0.02)
        return [np.asarray(w) for w in m.get_weights()] + [np.asarray(loss), np.asarray(m(inputs))]
    makers = {"GCN2": lambda: gcnx.GCN2(ctx, 2, hidden=32, seed=1),
              "GeneralGNN": lambda: gcnx.GeneralGNN(ctx, 2, activation="softmax", hidden=32, message_passing=2, seed=1),
              "GCN": lambda: gcnx.GCN(ctx, hidden_channels=32, seed=1)}
    per_edge = (x4[0], x4[1], e[:e.shape[0] // 2 + 1], x4[3])      # use_edge_data=True: one row per undirected edge, not per entry
    for name, make in makers.items():
        ra, rb, rc = run(make, x3, y), run(make, x4, y), run(make, per_edge, y)
        assert len(ra) == len(rb) == len(rc), name
        assert all(np.array_equal(u, v) and np.array_equal(u, w) for u, v, w in zip(ra, rb, rc)), name
    ds = gcnx.ListDataset([gcnx.Graph(x=x, a=sp.csr_matrix((np.ones(idx.shape[0]), (idx[:, 0], idx[:, 1])), shape=(x.shape[0],) * 2),
                                      e=e[:5], y=y[0]) for _ in range(2)])
    m = makers["GCN2"]()
    gcnx.fit(m, gcnx.DisjointLoader(ds, batch_size=2, epochs=1, shuffle=False), epochs=1, verbose=False)   # fit drops e for such a model
    graphs3, graphs4 = [], []
    for g in range(len(gp) - 1):
        lo, hi = gp[g], gp[g + 1]
        sel = (idx[:, 0] >= lo) & (idx[:, 0] < hi)
        a = sp.csr_matrix((np.ones(sel.sum()), (idx[sel, 0] - lo, idx[sel, 1] - lo)), shape=(hi - lo, hi - lo))
        graphs3.append(gcnx.Graph(x=x[lo:hi], a=a, y=y[g]))
        graphs4.append(gcnx.Graph(x=x[lo:hi], a=a, e=e[sel], y=y[g]))
    d3, d4 = gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs3)), gcnx.DeviceDataset(ctx, gcnx.ListDataset(graphs4))
    b3, b4 = collate_on_device(d3, [4, 0, 7]), collate_on_device(d4, [4, 0, 7])
    for u, v in ((b3.x, b4.x), (b3.a.rowptr, b4.a.rowptr), (b3.a.colidx, b4.a.colidx), (b3.y, b4.y), (b3.seg.dev, b4.seg.dev)):
        assert np.array_equal(u.numpy(), v.numpy())
    assert b4.e is None

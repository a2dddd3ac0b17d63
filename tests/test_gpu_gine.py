"""GPU tests of GINEConv: the one-launch kernel gcnx_gine_conv (csrc/gine.hip), gcnx_gine_aggregate, gcnx_gine_bwd_edges,
gcnx_gine_bwd_nodes, the layer gcnx.GINEConv and the model gcnx.GINE on both of its routes (GCNX_GINE_FUSED) with and without
train_eps -- each against the float64 oracle tests/gine_ref.py on the side of every message kink that the float32 restatement
of the contract (gine_ref.contract_mask) gives: device and oracle agree on every mask by construction, so no entry is excluded
from any comparison.  The inner ReLU masks and the PReLU sides are the device's, as in test_gpu_gin.py.
Tolerances: TIGHT = 2e-5 for a single fp32 kernel, 1e-4 for a whole step and for the weights after five SGD steps."""
import functools

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import gine_ref as ER
from gpu_frames import Frame
from test_gpu_gcn_bn import _tiny_host

pytestmark = pytest.mark.gpu

TIGHT = 2e-5

# gradients that are analytically zero (see test_gpu_gcn_bn.UNDER_BN): compared relative to the weight gradient named here
UNDER_BN = {"conv1.nn.2.bias": "conv1.nn.2.weight", "conv2.nn.2.bias": "conv2.nn.2.weight", "linear_1.bias": "linear_1.weight",
            "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev(ctx, a):
    return ctx.to_device(a) if a is not None else None


@functools.lru_cache(maxsize=None)
def _pattern(n, degs=(0, 1, 3, 4, 5, 40), seed=0):
    """A non-symmetric pattern of n rows whose degrees cycle through ``degs`` (capped at n), sorted columns, with stored
    self-loops where the draw gives them.  Returns read-only (rowptr, colidx)."""
    rng = np.random.default_rng(seed + n)
    cols = [np.sort(rng.choice(n, min(degs[i % len(degs)], n), replace=False)) for i in range(n)]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    colidx = np.concatenate(cols).astype(np.int32)
    rowptr.setflags(write=False); colidx.setflags(write=False)
    return rowptr, colidx


def _csr(ctx, rowptr, colidx):
    from gcnx.device import DeviceCSR
    return DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, np.array([0, len(rowptr) - 1], np.int32), symmetric=False)


def _edge_ops(n, nnz, f, d, seed, bias=True):
    """x [n, f], e [nnz, d], w_e [d, f], b_e [f] or None (float32)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, f), dtype=np.float32)
    e = rng.uniform(0, 1, (nnz, d)).astype(np.float32)
    w_e = (rng.standard_normal((d, f)) / np.sqrt(d)).astype(np.float32)
    b_e = (0.3 * rng.standard_normal(f)).astype(np.float32) if bias else None
    return x, e, w_e, b_e


def _mlp(rng, k0, k1, k2):
    mk = lambda fi, fo: (rng.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32)
    return mk(k0, k1), rng.standard_normal(k1).astype(np.float32), mk(k1, k2), rng.standard_normal(k2).astype(np.float32)


def _eps_dev(ctx, eps):
    return None if eps is None else ctx.to_device(np.full(1, eps, np.float32))


def _ref_fwd(rowptr, colidx, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b):
    """(out, T, U, message mask) in float64 on the contract's side of every message kink."""
    mask = ER.contract_mask(colidx, x, e, w_e.T, b_e)
    out, t, u, _, _ = ER.gine_conv_fwd(rowptr, colidx, x, e, 0.0 if eps is None else np.float32(eps), w_e.T, b_e, w_a.T, b_a, w_b.T, b_b,
                                       msg_mask=mask)
    return out, t, u, mask


def _run_conv(ctx, a, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b, keep=True):
    """gcnx_gine_conv with every operand that carries rows inside a sentinel frame (x a column slice of a wider array; room for a
    whole tile behind the last row of every output).  Returns (out, t, u) as host arrays (t, u None without keep)."""
    from gcnx import device as D
    n, k0 = x.shape
    k1, k2 = w_a.shape[1], w_b.shape[1]
    fx, fe = Frame(ctx, n, k0, 2 * k0, 4, data=x), Frame(ctx, e.shape[0], e.shape[1], e.shape[1] + 3, 1, data=e)
    fo = Frame(ctx, n, k2, k2 + 8, 8, tail=33 * (k2 + 8))
    ft, fu = Frame(ctx, n, k0, k0 + 4, 12, tail=33 * (k0 + 4)), Frame(ctx, n, k1, k1 + 12, 4, tail=33 * (k1 + 12))
    assert fx.aligned() and fo.aligned() and ft.aligned() and fu.aligned()
    assert D.gine_conv_ok(ctx, n, k0, k1, k2, fx.view.ld, e.shape[1])
    D.gine_conv(ctx, a, fx.view, _eps_dev(ctx, eps), fe.view, ctx.to_device(w_e), _dev(ctx, b_e), ctx.to_device(w_a), _dev(ctx, b_a),
                ctx.to_device(w_b), _dev(ctx, b_b), fo.view, t=ft.view if keep else None, u=fu.view if keep else None)
    fx.untouched("x"); fe.untouched("e")
    if not keep:
        ft.untouched("t = NULL"); fu.untouched("u = NULL")
        return fo.numpy(), None, None
    return fo.numpy(), ft.numpy(), fu.numpy()                            # (numpy() asserts that nothing outside the view was written)


def _aggregate(ctx, a, x, e, eps, w_e, b_e, ldx=None, ldo=None, lead=0):
    from gcnx import device as D
    n, f = x.shape
    fx, fo = Frame(ctx, n, f, ldx or f, lead, data=x), Frame(ctx, n, f, ldo or f, lead)
    D.gine_aggregate(ctx, a, fx.view, _eps_dev(ctx, eps), ctx.to_device(e), ctx.to_device(w_e), _dev(ctx, b_e), fo.view)
    fx.untouched("x")
    return fo.numpy()


def _bwd(ctx, a, x, e, eps, w_e, b_e, dt, lead=0, pad=0):
    """(dw_e, db_e, dx) of gcnx_gine_bwd_edges / gcnx_gine_bwd_nodes; the gradient outputs start as NaN (written, not accumulated),
    dx sits in a frame; bwd_edges runs twice and must leave the same bits."""
    from gcnx import device as D
    n, f = x.shape
    d = e.shape[1]
    fx, fdt, fdx = Frame(ctx, n, f, f + pad, lead, data=x), Frame(ctx, n, f, f + pad, lead, data=dt), Frame(ctx, n, f, f + pad, lead)
    de, dwe, dbe = ctx.to_device(e), ctx.to_device(w_e), _dev(ctx, b_e)
    scratch = ctx.empty(max(D.gine_bwd_scratch_floats(ctx, n, f, d), 4))
    got = []
    for _ in range(2):
        g_w, g_b = ctx.to_device(np.full((d, f), np.nan, np.float32)), ctx.to_device(np.full(f, np.nan, np.float32))
        D.gine_bwd_edges(ctx, a, fx.view, de, dwe, dbe, fdt.view, g_w, g_b, scratch)
        got.append((g_w.numpy(), g_b.numpy()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    D.gine_bwd_nodes(ctx, a, fx.view, _eps_dev(ctx, eps), de, dwe, dbe, fdt.view, fdx.view)
    fx.untouched("x"); fdt.untouched("dt")
    return got[0][0], got[0][1], fdx.numpy()


def _ref_bwd(rowptr, colidx, x, e, eps, w_e, b_e, dt):
    mask = ER.contract_mask(colidx, x, e, w_e.T, b_e)
    dx, _, dlw, dlb = ER.gine_edge_bwd(rowptr, colidx, x, e, 0.0 if eps is None else np.float32(eps), mask, dt)
    return dlw.T, dlb, dx


# ---- 1. the one launch against float64 -------------------------------------------------------------------------------------
CASES = [(16, 64, 64, 2, None, True), (32, 48, 112, 1, -0.3, False), (64, 64, 64, 2, -0.3, True), (128, 128, 128, 8, None, True),
         (128, 16, 32, 2, -0.3, False), (16, 128, 16, 8, -0.3, True), (64, 32, 48, 1, None, False)]


@pytest.mark.parametrize("k0,k1,k2,d,eps,bias", CASES)
def test_gine_conv_against_float64(ctx, k0, k1, k2, d, eps, bias):
    rowptr, colidx = _pattern(70)
    assert set(np.diff(rowptr)) == {0, 1, 3, 4, 5, 40}
    a = _csr(ctx, rowptr, colidx)
    x, e, w_e, b_e = _edge_ops(70, len(colidx), k0, d, 1000 * k0 + 10 * k1 + d, bias)
    w_a, b_a, w_b, b_b = _mlp(np.random.default_rng(k0 + k1 + k2), k0, k1, k2)
    out, t, u = _run_conv(ctx, a, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b)
    r_out, r_t, r_u, mask = _ref_fwd(rowptr, colidx, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b)
    assert mask.any() and not mask.all()
    e_out, e_t, e_u = rel_err(out, r_out), rel_err(t, r_t), rel_err(u, r_u)
    print(f"gine_conv k=({k0},{k1},{k2}) D={d} eps={eps} bias={bias}: rel_err out {e_out:.2e} t {e_t:.2e} u {e_u:.2e}")
    assert e_out < TIGHT and e_t < TIGHT and e_u < TIGHT and (u >= 0).all()
    empty = np.diff(rowptr) == 0
    scale = np.float32(1.0) + (np.float32(eps) if eps is not None else np.float32(0.0))
    assert np.array_equal(_bits(t[empty]), _bits(scale * x[empty]))      # rows without entries: T = (1 + eps) x exactly
    # no atomics: a second call leaves the same bits; t = u = NULL gives the same out and writes neither
    out2, t2, u2 = _run_conv(ctx, a, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b)
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(t2), _bits(t)) and np.array_equal(_bits(u2), _bits(u))
    out3, _, _ = _run_conv(ctx, a, x, e, eps, w_e, b_e, w_a, b_a, w_b, b_b, keep=False)
    assert np.array_equal(_bits(out3), _bits(out))
    # T is gcnx_gine_aggregate's float4 T, bit for bit
    t6 = _aggregate(ctx, a, x, e, eps, w_e, b_e, ldx=k0 + 4, ldo=k0 + 8, lead=4)
    assert np.array_equal(_bits(t6), _bits(t))
    # without the MLP's biases
    out5, _, u5 = _run_conv(ctx, a, x, e, eps, w_e, b_e, w_a, None, w_b, None)
    r_out5, _, r_u5, _ = _ref_fwd(rowptr, colidx, x, e, eps, w_e, b_e, w_a, None, w_b, None)
    assert rel_err(out5, r_out5) < TIGHT and rel_err(u5, r_u5) < TIGHT


@pytest.mark.parametrize("n", [1, 31, 32, 33, 70])
def test_gine_conv_tile_edges(ctx, n):
    rowptr, colidx = _pattern(n, degs=(1, 0, 3, 4, 5, 40))
    a = _csr(ctx, rowptr, colidx)
    x, e, w_e, b_e = _edge_ops(n, len(colidx), 32, 2, 77 + n)
    w_a, b_a, w_b, b_b = _mlp(np.random.default_rng(n), 32, 48, 16)
    out, t, u = _run_conv(ctx, a, x, e, -0.3, w_e, b_e, w_a, b_a, w_b, b_b)      # (the frames catch rows at or past n)
    r_out, r_t, r_u, _ = _ref_fwd(rowptr, colidx, x, e, -0.3, w_e, b_e, w_a, b_a, w_b, b_b)
    assert rel_err(out, r_out) < TIGHT and rel_err(t, r_t) < TIGHT and rel_err(u, r_u) < TIGHT
    dt = np.random.default_rng(n + 1).standard_normal((n, 32)).astype(np.float32)
    g_w, g_b, dx = _bwd(ctx, a, x, e, -0.3, w_e, b_e, dt, lead=4, pad=4)
    r_w, r_b, r_dx = _ref_bwd(rowptr, colidx, x, e, -0.3, w_e, b_e, dt)
    assert rel_err(g_w, r_w) < TIGHT and rel_err(g_b, r_b) < TIGHT and rel_err(dx, r_dx) < TIGHT


# ---- 2. a row longer than the staged entries -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_row():
    """1 200 rows; row 0 holds 1 100 entries (past the 1 024 a tile stages), the others 0 .. 6; column 3 is listed by most rows."""
    rng = np.random.default_rng(5)
    n = 1200
    cols = [np.sort(rng.choice(n, 1100, replace=False))]
    for i in range(1, n):
        c = set(rng.choice(n, i % 7, replace=False).tolist())
        if i % 3:
            c.add(3)
        cols.append(np.sort(np.fromiter(c, np.int64)))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    return rowptr, np.concatenate(cols).astype(np.int32)


def test_gine_one_row_beyond_the_staged_entries(ctx):
    rowptr, colidx = _long_row()
    n, k0 = 1200, 64
    assert rowptr[1] == 1100 and rowptr[32] - rowptr[0] > 1024
    a = _csr(ctx, rowptr, colidx)
    x, e, w_e, b_e = _edge_ops(n, len(colidx), k0, 2, 9)
    w_a, b_a, w_b, b_b = _mlp(np.random.default_rng(3), k0, 32, 48)
    out, t, u = _run_conv(ctx, a, x, e, -0.3, w_e, b_e, w_a, b_a, w_b, b_b)
    r_out, r_t, r_u, _ = _ref_fwd(rowptr, colidx, x, e, -0.3, w_e, b_e, w_a, b_a, w_b, b_b)
    e_out, e_t, e_u = rel_err(out, r_out), rel_err(t, r_t), rel_err(u, r_u)
    print(f"gine_conv long row: rel_err out {e_out:.2e} t {e_t:.2e} u {e_u:.2e}")
    assert e_out < TIGHT and e_t < TIGHT and e_u < TIGHT
    assert rel_err(t[:32], r_t[:32]) < TIGHT                              # the tile that runs past its staged entries, on its own scale
    assert np.array_equal(_bits(_aggregate(ctx, a, x, e, -0.3, w_e, b_e)), _bits(t))
    dt = np.random.default_rng(4).standard_normal((n, k0)).astype(np.float32)
    g_w, g_b, dx = _bwd(ctx, a, x, e, -0.3, w_e, b_e, dt)
    r_w, r_b, r_dx = _ref_bwd(rowptr, colidx, x, e, -0.3, w_e, b_e, dt)
    print(f"gine bwd long row: dw_e {rel_err(g_w, r_w):.2e} db_e {rel_err(g_b, r_b):.2e} dx {rel_err(dx, r_dx):.2e}")
    assert rel_err(g_w, r_w) < TIGHT and rel_err(g_b, r_b) < TIGHT and rel_err(dx, r_dx) < TIGHT


# ---- 3. any width: scalar lanes and float4 lanes of the three any-width kernels ------------------------------------------
@pytest.mark.parametrize("f,d,bias", [(5, 2, True), (18, 8, True), (20, 1, False), (16, 2, True), (64, 8, False)])
def test_gine_any_width_kernels(ctx, f, d, bias):
    rowptr, colidx = _pattern(70)
    a = _csr(ctx, rowptr, colidx)
    x, e, w_e, b_e = _edge_ops(70, len(colidx), f, d, 31 * f + d, bias)
    dt = np.random.default_rng(f).standard_normal((70, f)).astype(np.float32)
    mask = ER.contract_mask(colidx, x, e, w_e.T, b_e)
    for eps in (None, -0.3):
        want, _ = ER.gine_aggregate(rowptr, colidx, x, e, 0.0 if eps is None else np.float32(eps), w_e.T, b_e, msg_mask=mask)
        r_w, r_b, r_dx = _ref_bwd(rowptr, colidx, x, e, eps, w_e, b_e, dt)
        # contiguous; an odd start and odd leading dimensions (scalar lanes whatever f is)
        for lead, pad in ((0, 0), (1, 3)):
            got = _aggregate(ctx, a, x, e, eps, w_e, b_e, ldx=f + pad, ldo=f + pad, lead=lead)
            g_w, g_b, dx = _bwd(ctx, a, x, e, eps, w_e, b_e, dt, lead=lead, pad=pad)
            errs = (rel_err(got, want), rel_err(g_w, r_w), rel_err(g_b, r_b), rel_err(dx, r_dx))
            print(f"gine any width f={f} D={d} eps={eps} lead={lead}: T {errs[0]:.2e} dw_e {errs[1]:.2e} db_e {errs[2]:.2e} dx {errs[3]:.2e}")
            assert max(errs) < TIGHT, errs


def test_gine_bwd_nodes_needs_the_permutation_on_a_symmetric_pattern(ctx):
    """A symmetric pattern whose two directions of an edge carry different features: dx read through perm_t matches the oracle."""
    hb = _tiny_host(6, 16, seed=3)
    rowptr, colidx = hb.rowptr, hb.colidx
    a = _csr(ctx, rowptr, colidx)
    x, e, w_e, b_e = _edge_ops(hb.n, len(colidx), 16, 2, 12)
    dt = np.random.default_rng(2).standard_normal((hb.n, 16)).astype(np.float32)
    g_w, g_b, dx = _bwd(ctx, a, x, e, None, w_e, b_e, dt)
    r_w, r_b, r_dx = _ref_bwd(rowptr, colidx, x, e, None, w_e, b_e, dt)
    assert rel_err(g_w, r_w) < TIGHT and rel_err(g_b, r_b) < TIGHT and rel_err(dx, r_dx) < TIGHT
    rp, ci, pm = (v.numpy() for v in a.transpose_perm())
    assert np.array_equal(rp, rowptr) and np.array_equal(ci[:len(colidx)], colidx) and not np.array_equal(pm[:len(colidx)], np.arange(len(colidx)))


# ---- 4. padding slots and exact kinks ----------------------------------------------------------------------------------------
def test_gine_padding_slots_add_nothing(ctx):
    """b_e large and positive, every row with a number of entries that is no multiple of 4: a gather that adds relu(0 + v) for
    the slots past a row's end is off by 50 per slot."""
    rowptr, colidx = _pattern(45, degs=(1, 2, 3, 5, 6, 7, 0))
    assert not any(dg % 4 == 0 and dg for dg in np.diff(rowptr))
    a = _csr(ctx, rowptr, colidx)
    for k0, d in ((16, 2), (128, 8)):
        x, e, w_e, _ = _edge_ops(45, len(colidx), k0, d, 5 + k0)
        b_e = np.full(k0, 50.0, np.float32)
        w_a, b_a, w_b, b_b = _mlp(np.random.default_rng(1), k0, 32, 16)
        out, t, u = _run_conv(ctx, a, x, e, None, w_e, b_e, w_a, b_a, w_b, b_b)
        r_out, r_t, r_u, mask = _ref_fwd(rowptr, colidx, x, e, None, w_e, b_e, w_a, b_a, w_b, b_b)
        assert mask.all() and rel_err(t, r_t) < TIGHT and rel_err(out, r_out) < TIGHT and rel_err(u, r_u) < TIGHT
        assert np.array_equal(_bits(t[6]), _bits(x[6]))                 # a row without entries gets no bias at all
        assert np.array_equal(_bits(_aggregate(ctx, a, x, e, None, w_e, b_e)), _bits(t))


@pytest.mark.parametrize("k0,d", [(16, 1), (32, 2), (128, 8)])
def test_gine_messages_have_the_contracts_bits(ctx, k0, d):
    """Rows that hold zeros and list one source: their T is relu(m) itself, and m must be the contract's float32 value bit for
    bit (every product and sum rounded on its own, in the stated order: a fused multiply-add gives other bits) -- from the one
    launch and from both lane forms of gcnx_gine_aggregate."""
    n = 64
    rng = np.random.default_rng(k0 + d)
    colidx = rng.integers(32, n, n).astype(np.int32)                       # row i lists source colidx[i] in 32 .. 63
    rowptr = np.arange(n + 1, dtype=np.int32)
    x, e, w_e, b_e = _edge_ops(n, n, k0, d, 3 * k0 + d)
    x[:32] = 0
    a = _csr(ctx, rowptr, colidx)
    m = ER.contract_m(colidx, x, e, w_e.T, b_e)
    want = np.where(m > 0, m, np.float32(0))[:32]
    assert (want > 0).any() and (want == 0).any()
    exact = x.astype(np.float64)[colidx] + (e.astype(np.float64) @ w_e.astype(np.float64) + b_e)
    assert d == 1 or np.any(m != exact.astype(np.float32))                 # (the order of the roundings is visible in these inputs)
    w_a, b_a, w_b, b_b = _mlp(rng, k0, 16, 16)
    _, t, _ = _run_conv(ctx, a, x, e, None, w_e, b_e, w_a, b_a, w_b, b_b)
    assert np.array_equal(_bits(t[:32]), _bits(want))
    assert np.array_equal(_bits(_aggregate(ctx, a, x, e, None, w_e, b_e)[:32]), _bits(want))
    assert np.array_equal(_bits(_aggregate(ctx, a, x, e, None, w_e, b_e, ldx=k0 + 1, ldo=k0 + 3, lead=1)[:32]), _bits(want))


def test_gine_exact_kinks_land_on_the_same_side_in_all_three_kernels(ctx):
    """e = 0 and b_e[c] = -x[5, c]: every message from source 5 is m == 0 exactly (the zero side, gradient 0); source 6 sits one
    ulp above it in every channel (passes, message = that ulp), source 7 one ulp below (blocked).  Rows 0 / 1 / 2 hold zeros and
    list only source 5 / 6 / 7: their T is the message itself."""
    k0, n = 32, 40
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n, k0), dtype=np.float32)
    x[6], x[7] = np.nextafter(x[5], np.float32(np.inf)), np.nextafter(x[5], np.float32(-np.inf))
    x[:3] = 0
    cols = [[5], [6], [7]] + [sorted({5, 6, 7, int(i)} | set(rng.choice(n, 3).tolist())) for i in range(3, n)]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    colidx = np.concatenate(cols).astype(np.int32)
    a = _csr(ctx, rowptr, colidx)
    e = np.zeros((len(colidx), 2), np.float32)
    w_e = rng.standard_normal((2, k0)).astype(np.float32)
    b_e = -x[5]
    m = ER.contract_m(colidx, x, e, w_e.T, b_e)
    mask = m > 0
    assert (m[colidx == 5] == 0).all() and mask[colidx == 6].all() and not mask[colidx == 7].any() and not mask[colidx == 5].any()
    w_a, b_a, w_b, b_b = _mlp(rng, k0, 32, 16)
    out, t, u = _run_conv(ctx, a, x, e, None, w_e, b_e, w_a, b_a, w_b, b_b)
    r_out, r_t, _, mk = _ref_fwd(rowptr, colidx, x, e, None, w_e, b_e, w_a, b_a, w_b, b_b)
    assert np.array_equal(mk, mask) and rel_err(t, r_t) < TIGHT and rel_err(out, r_out) < TIGHT
    ulp = x[6] - x[5]
    assert (ulp > 0).all() and not t[0].any() and np.array_equal(_bits(t[1]), _bits(ulp)) and not t[2].any()    # the messages themselves
    t_agg = _aggregate(ctx, a, x, e, None, w_e, b_e)
    assert np.array_equal(_bits(t_agg), _bits(t))
    t_sc = _aggregate(ctx, a, x, e, None, w_e, b_e, ldx=k0 + 1, ldo=k0 + 1, lead=1)                              # scalar lanes
    assert not t_sc[0].any() and np.array_equal(_bits(t_sc[1]), _bits(ulp)) and not t_sc[2].any()
    dt = (1.0 + rng.uniform(0, 1, (n, k0))).astype(np.float32)            # all positive: a wrong side moves every sum by >= 1
    for lead, pad in ((0, 0), (1, 1)):
        g_w, g_b, dx = _bwd(ctx, a, x, e, None, w_e, b_e, dt, lead=lead, pad=pad)
        r_w, r_b, r_dx = _ref_bwd(rowptr, colidx, x, e, None, w_e, b_e, dt)
        assert rel_err(g_b, r_b) < TIGHT and rel_err(dx, r_dx) < TIGHT and not g_w.any() and not r_w.any()     # e = 0: dW_e = 0
        assert np.array_equal(_bits(dx[5]), _bits(dt[5])) and np.array_equal(_bits(dx[7]), _bits(dt[7]))       # blocked: (1 + 0) dT alone
        assert (dx[6] > dt[6] + n - 3).all()                                                            # passes from every row that lists it


# ---- 5. the error contract -------------------------------------------------------------------------------------------------
def test_gine_refusals_launch_and_write_nothing(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    rowptr, colidx = _pattern(70)
    a = _csr(ctx, rowptr, colidx)
    n, nnz = 70, len(colidx)
    e, w_a, w_b = ctx.zeros((nnz, 2)), ctx.zeros((16, 64)), ctx.zeros((64, 64))

    def conv(x, w_e, out, t, u, w_a=w_a, w_b=w_b, e=e):
        D.gine_conv(ctx, a, x, None, e, w_e, None, w_a, None, w_b, None, out, t=t, u=u)

    def refused(code, **kw):
        fr = {k: Frame(ctx, n, f, f, 0) for k, f in (("out", 64), ("t", 16), ("u", 64))}
        args = dict(x=ctx.zeros((n, 16)), w_e=ctx.zeros((2, 16)), out=fr["out"].view, t=fr["t"].view, u=fr["u"].view)
        args.update(kw)
        with pytest.raises(_lib.GcnxError) as err:
            conv(**args)
        assert err.value.code == code, (kw.keys(), err.value.code)
        for k in fr:
            fr[k].untouched(k)

    # UNSUPPORTED: shapes gcnx_gine_conv_ok refuses, a misaligned pointer, a leading dimension that is no multiple of 4 floats
    assert not D.gine_conv_ok(ctx, n, 96, 64, 64, edge_dim=2) and not D.gine_conv_ok(ctx, n, 16, 64, 64, 18, 2)
    assert not D.gine_conv_ok(ctx, n, 16, 64, 64, edge_dim=9)
    refused(_lib.ERR_UNSUPPORTED, x=ctx.zeros((n, 96)), w_e=ctx.zeros((2, 96)), w_a=ctx.zeros((96, 64)), t=None)
    refused(_lib.ERR_UNSUPPORTED, e=ctx.zeros((nnz, 9)), w_e=ctx.zeros((9, 16)))
    wide = ctx.zeros((n, 18))
    refused(_lib.ERR_UNSUPPORTED, x=DeviceArray(ctx, wide.ptr, (n, 16), np.float32, ld=18, base=wide))          # ldx % 4 != 0
    off = Frame(ctx, n, 16, 16, 1)
    assert off.view.ptr % 16 == 4
    refused(_lib.ERR_UNSUPPORTED, x=off.view)
    woff = Frame(ctx, 2, 16, 16, 1)
    refused(_lib.ERR_UNSUPPORTED, w_e=woff.view)
    for which, f in (("out", 64), ("t", 16), ("u", 64)):
        bad = Frame(ctx, n, f, f + 2, 0)
        refused(_lib.ERR_UNSUPPORTED, **{which: bad.view})
        bad.untouched(which)
        bad = Frame(ctx, n, f, f, 1)
        refused(_lib.ERR_UNSUPPORTED, **{which: bad.view})
        bad.untouched(which)
    # INVALID: aliasing
    xa = ctx.zeros((n, 16))
    refused(1, x=xa, t=xa)
    # raw calls: n == 0 succeeds and writes nothing; negative sizes and NULL mandatory pointers are invalid
    x, w_e, out = ctx.zeros((4, 16)), ctx.zeros((2, 16)), Frame(ctx, 4, 64, 64, 0)
    call = lambda **kw: ctx.lib.gcnx_gine_conv(ctx.h, a.rowptr.ptr, a.colidx.ptr, kw.get("x", x.ptr), 16, kw.get("n", 4), 16, None,
                                               kw.get("e", e.ptr), kw.get("lde", 2), kw.get("d", 2), kw.get("w_e", w_e.ptr), None,
                                               kw.get("w_a", w_a.ptr), None, 64, kw.get("w_b", w_b.ptr), None, 64, None, 0, None, 0,
                                               out.view.ptr, 64)
    assert call(n=0) == _lib.OK
    for bad in (dict(n=-1), dict(d=-1), dict(x=None), dict(e=None), dict(w_e=None), dict(w_a=None), dict(w_b=None), dict(lde=1)):
        assert call(**bad) == 1, bad                                       # GCNX_ERR_INVALID
    assert call(d=0) == _lib.ERR_UNSUPPORTED and call(d=9) == _lib.ERR_UNSUPPORTED
    out.untouched("refused calls and n = 0 write nothing")
    # the any-width calls: aliasing, NULL, negative sizes, edge_dim outside 1 .. 8 are invalid; n == 0 succeeds
    xn, dtn, dxn = ctx.zeros((n, 16)), ctx.zeros((n, 16)), Frame(ctx, n, 16, 16, 0)
    scratch = ctx.zeros(max(D.gine_bwd_scratch_floats(ctx, n, 16, 2), 4))
    for fn in (lambda: D.gine_aggregate(ctx, a, xn, None, e, w_e, None, xn),
               lambda: D.gine_bwd_nodes(ctx, a, xn, None, e, w_e, None, dtn, dtn),
               lambda: D.gine_bwd_nodes(ctx, a, xn, None, e, w_e, None, dtn, xn)):
        with pytest.raises(_lib.GcnxError) as err:
            fn()
        assert err.value.code == 1
    rp, ci, pm = a.transpose_perm()
    agg = lambda **kw: ctx.lib.gcnx_gine_aggregate(ctx.h, a.rowptr.ptr, a.colidx.ptr, kw.get("x", xn.ptr), 16, None, kw.get("e", e.ptr), 2,
                                                   kw.get("d", 2), w_e.ptr, None, dxn.view.ptr, 16, kw.get("n", n), kw.get("f", 16))
    nodes = lambda **kw: ctx.lib.gcnx_gine_bwd_nodes(ctx.h, rp.ptr, ci.ptr, kw.get("pm", pm.ptr), xn.ptr, 16, None, e.ptr, 2, kw.get("d", 2),
                                                     w_e.ptr, None, dtn.ptr, 16, dxn.view.ptr, 16, kw.get("n", n), kw.get("f", 16))
    g_w, g_b = Frame(ctx, 2, 16, 16, 0), Frame(ctx, 1, 16, 16, 0)
    edges = lambda **kw: ctx.lib.gcnx_gine_bwd_edges(ctx.h, a.rowptr.ptr, a.colidx.ptr, kw.get("x", xn.ptr), 16, e.ptr, 2, kw.get("d", 2),
                                                     w_e.ptr, None, dtn.ptr, 16, kw.get("n", n), kw.get("f", 16), kw.get("g_w", g_w.view.ptr),
                                                     g_b.view.ptr, scratch.ptr)
    for fn in (agg, nodes, edges):
        for bad in (dict(n=-1), dict(f=0), dict(d=0), dict(d=9)):
            assert fn(**bad) == 1, bad
    assert agg(x=None) == 1 and agg(e=None) == 1 and nodes(pm=None) == 1 and edges(x=None) == 1 and edges(g_w=None) == 1
    assert agg(n=0) == _lib.OK and nodes(n=0) == _lib.OK
    dxn.untouched("refused calls and n = 0 write nothing"); g_w.untouched("dw_e"); g_b.untouched("db_e")
    assert edges(n=0) == _lib.OK                                              # n == 0: the two gradients are written as zeros
    assert not g_w.numpy().any() and not g_b.numpy().any()


# ---- 6. the layer -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mlp_hidden", [32, 48])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("train_eps", [False, True])
def test_gineconv_layer_forward_and_backward(ctx, train_eps, fused, mlp_hidden):
    from gcnx.layers import GINEConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb.rowptr, hb.colidx)
    e = np.random.default_rng(6).uniform(0, 1, (len(hb.colidx), 2)).astype(np.float32)
    lay = GINEConv(64, 2, mlp_hidden=mlp_hidden, eps=-0.3, train_eps=train_eps, fused=fused, seed=3)
    x, de = ctx.to_device(hb.x), ctx.to_device(e)
    y = lay([x, GINEConv.preprocess(a), de])
    p = {k: v.numpy().astype(np.float64) for k, v in lay.params.items()}
    assert list(p) == (["eps"] if train_eps else []) + ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "lin.weight", "lin.bias"]
    assert all(v.ptr % 16 == 0 for v in lay.params.values())
    assert lay._one_launch(x, mlp_hidden, 64, y) == fused
    eps = np.float32(-0.3)
    w_a, w_b, lw, lb = p["nn.0.weight"].T, p["nn.2.weight"].T, p["lin.weight"].T, p["lin.bias"]
    mm = ER.contract_mask(hb.colidx, hb.x, e, lay.params["lin.weight"].numpy().T, lay.params["lin.bias"].numpy())
    r_y, r_t, r_u, _, _ = ER.gine_conv_fwd(hb.rowptr, hb.colidx, hb.x, e, eps, lw, lb, w_a, p["nn.0.bias"], w_b, p["nn.2.bias"], msg_mask=mm)
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = np.random.default_rng(9).standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    relu = lay._saved[4].numpy() > 0                                      # the device's side of the inner ReLU
    r_dx, r_deps, r_dwa, r_dba, r_dwb, r_dbb, r_dlw, r_dlb = ER.gine_conv_bwd(hb.rowptr, hb.colidx, hb.x, e, eps, r_t, r_u, mm, relu,
                                                                              w_a, w_b, dy)
    g = {k: v.numpy() for k, v in lay.grads.items()}
    errs = {"dx": rel_err(dx.numpy(), r_dx), "nn.0.weight": rel_err(g["nn.0.weight"], r_dwa.T), "nn.0.bias": rel_err(g["nn.0.bias"], r_dba),
            "nn.2.weight": rel_err(g["nn.2.weight"], r_dwb.T), "nn.2.bias": rel_err(g["nn.2.bias"], r_dbb),
            "lin.weight": rel_err(g["lin.weight"], r_dlw.T), "lin.bias": rel_err(g["lin.bias"], r_dlb)}
    if train_eps:
        errs["eps"] = abs(float(g["eps"][0]) - float(r_deps[0])) / abs(float(r_deps[0]))
    print(f"GINEConv layer mlp_hidden={mlp_hidden} fused={fused} train_eps={train_eps}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) < TIGHT, errs
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    g2 = {k: v.numpy() for k, v in lay.grads.items()}
    assert all(np.array_equal(_bits(g2[k]), _bits(g[k])) for k in g)      # need_dx=False leaves the same gradients
    with pytest.raises(ValueError):
        lay([x, a])
    with pytest.raises(ValueError):
        lay([x, a, ctx.zeros((len(hb.colidx), 3))])


# ---- 7. gcnx.GINE: a full step on either route against the oracle -------------------------------------------------------------
def _features(nnz, d, seed):
    return np.random.default_rng(seed).uniform(0, 1, (nnz, d)).astype(np.float32)


def _device_batch(ctx, hb, e):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), e=ctx.to_device(e))


def _sides(m, hb, e, pre=None, pre_lin=None, relu=True):
    """The sides of every kink of the last call: the PReLU sides and the inner ReLU masks are the device's; the message masks are
    the contract's, restated in float32 from the operands the device read (x / the device's y1, e, lin as the step began)."""
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    lin = pre_lin or {k: m.p[k].numpy() for k in ("we1", "bl1", "we2", "bl2")}
    s = {}
    if m.norm == "batch":
        s.update({f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
                  for i in (1, 2)})
    if relu:
        s.update(relu1=b["u1"].numpy() > 0, relu2=b["u2"].numpy() > 0)
    s["msg1"] = ER.contract_mask(hb.colidx, hb.x, e, lin["we1"].T, lin["bl1"])
    s["msg2"] = ER.contract_mask(hb.colidx, b["y1"].numpy(), e, lin["we2"].T, lin["bl2"])
    return s


def _cmp_grads(got, ref, tol, what):
    worst = 0.0
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN.get(k, k)], np.float64))))
        diff = float(np.max(np.abs(g - r)))
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)      # (a gradient that is exactly zero on both sides)
        worst = max(worst, err)
        assert err <= tol, (what, k, err)
    return worst


def _oracle(m, hb, e, p, sides):
    arg = m._bufs["arg"].numpy().astype(np.int64) if m.readout == "max" else None
    return ER.model(hb.x, hb.rowptr, hb.colidx, e, hb.graph_ptr, p, hb.y, masks=sides, argmax=arg, readout=m.readout, norm=m.norm)


def _check_step(m, batch, hb, e, p, tol, what):
    m.loss_and_grads(batch)
    r = _oracle(m, hb, e, p, _sides(m, hb, e))
    e_out = rel_err(m._bufs["out"].numpy(), r["out"])
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol and la[1] == r["hits"], (la, r["loss"], r["hits"])
    got = m.gradients()
    assert list(got) == [k for k, _, _ in m.TORCH_KEYS] and (("conv1.eps" in got) == ("conv2.eps" in got) == m.train_eps)
    worst = _cmp_grads(got, r["grads"], tol, what)
    print(f"GINE step {what}: logits {e_out:.2e} loss {rel_err(la[0], r['loss']):.2e} worst gradient {worst:.2e}")
    return r


@pytest.mark.parametrize("f_in,hidden", [(16, 64), (5, 32)])
@pytest.mark.parametrize("train_eps", [False, True])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_gine_step_against_oracle(ctx, monkeypatch, fused, train_eps, f_in, hidden):
    import gcnx
    from gcnx import device as D
    hb = _tiny_host(6, f_in, seed=4)
    e = _features(hb.nnz, 2, 5)
    batch = _device_batch(ctx, hb, e)
    monkeypatch.setenv("GCNX_GINE_FUSED", fused)
    m = gcnx.GINE(ctx, hidden_channels=hidden, edge_dim=2, train_eps=train_eps, seed=0)
    assert m._fused == (fused == "1") and m.uses_edge_features
    p = {k: v.astype(np.float32) for k, v in ER.init_params(f_in, hidden, 2, seed=7, eps=(-0.3, 0.2)).items()}
    m.load_state_dict(p)
    sd = m.state_dict()
    assert list(sd) == list(ER.KEYS) and all(np.array_equal(_bits(sd[k]), _bits(p[k])) for k in p)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    what = f"F={f_in} H={hidden} fused={fused} train_eps={train_eps}"
    _check_step(m, batch, hb, e, p, 1e-4, what)
    b = m._bufs
    assert m._one_launch(batch.x, hidden, hidden, b["z1"], b["t1"], b["u1"]) == (fused == "1" and f_in == 16)    # F = 5: composed
    assert m._one_launch(b["y1"], hidden, hidden, b["z2"], b["t2"], b["u2"]) == (fused == "1")
    assert not D.gine_conv_ok(ctx, hb.n, 5, hidden, hidden, 8, 2)
    # five SGD steps, each oracle step on the kink sides of that step (taken with the step's own weights)
    ph = {k: v.astype(np.float64) for k, v in p.items()}
    for _ in range(5):
        pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
        pre_lin = {k: m.p[k].numpy() for k in ("we1", "bl1", "we2", "bl2")}
        m.train_step(batch, lr=0.02)
        r = _oracle(m, hb, e, ph, _sides(m, hb, e, pre, pre_lin))
        grads = {k: (r["grads"][k] if train_eps or k not in ER.EPS_KEYS else 0.0 * r["grads"][k]) for k in ph}   # a fixed eps stays
        ph = ER.sgd(ph, grads, 0.02)
    sd = m.state_dict()
    assert list(sd) == list(ER.KEYS)
    worst = 0.0
    for k in ER.KEYS:
        worst = max(worst, rel_err(sd[k], ph[k].reshape(sd[k].shape)))
        assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{what} after 5 steps {k}")
    print(f"GINE {what}: worst weight after 5 SGD steps {worst:.2e}")
    if train_eps:
        assert sd["conv1.eps"][0] != np.float32(-0.3) and sd["conv2.eps"][0] != np.float32(0.2)
    else:
        assert sd["conv1.eps"][0] == np.float32(-0.3) and sd["conv2.eps"][0] == np.float32(0.2)


@pytest.mark.parametrize("kw", [dict(readout="attention"), dict(norm="graph"), dict(readout="attention", norm="graph")])
def test_gine_step_with_the_scaffolds_readout_and_norm(ctx, kw):
    import gcnx
    hb = _tiny_host(6, 16, seed=4)
    e = _features(hb.nnz, 2, 5)
    m = gcnx.GINE(ctx, hidden_channels=32, edge_dim=2, train_eps=True, seed=0, **kw)
    p = {k: v.astype(np.float32) for k, v in ER.init_params(16, 32, 2, seed=7, eps=(-0.3, 0.2), **kw).items()}
    m.load_state_dict(p)
    assert list(m.state_dict()) == list(ER.keys(**kw))
    batch = _device_batch(ctx, hb, e)
    if m.norm == "batch":
        _check_step(m, batch, hb, e, p, 1e-4, str(kw))
        return
    # GraphNorm·PReLU: the PReLU sides are the signs of y1 / y2 of a forward of its own (the max readout's backward overwrites y2)
    m(batch)
    pos = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
    m.loss_and_grads(batch)
    sides = _sides(m, hb, e)
    sides.update(pos)
    r = _oracle(m, hb, e, p, sides)
    assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, f"{kw} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < 1e-4 and la[1] == r["hits"], (la, r["loss"], r["hits"])
    worst = _cmp_grads(m.gradients(), r["grads"], 1e-4, str(kw))
    print(f"GINE step {kw}: worst gradient {worst:.2e}")


def test_gine_one_clipped_adam_step_matches_the_restatement(ctx):
    import gcnx
    from test_gpu_optim import _assert_adam, _assert_norm
    hb = _tiny_host(6, 16, seed=4)
    batch = _device_batch(ctx, hb, _features(hb.nnz, 2, 5))
    m = gcnx.GINE(ctx, hidden_channels=32, edge_dim=2, train_eps=True, seed=0)
    m.load_state_dict({k: v.astype(np.float32) for k, v in ER.init_params(16, 32, 2, seed=7).items()})
    opt = gcnx.Adam(clipnorm=1.0)
    m.set_optimizer(opt)
    n, lr = m.n_params, 1e-2
    p0, m0, v0 = m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy()
    m.train_step(batch, None, lr=lr)
    g = m.flat_g.numpy()[:n]
    norm = opt.last_grad_norm()
    _assert_norm(norm, g, min(256, -(-n // 256)), "GINE Adam step")
    _assert_adam(m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy(), p0, g, m0, v0, 1, lr, norm, "GINE Adam step",
                 beta1=opt.beta1, beta2=opt.beta2, eps=opt.eps, weight_decay=opt.weight_decay, clipnorm=opt.clipnorm)
    # SGD with momentum runs too
    m.set_optimizer(gcnx.SGD(momentum=0.9))
    assert np.all(np.isfinite(m.train_step(batch, None, lr=lr)))


def test_gine_batch_sources_give_the_same_bits_and_the_logits_read_e(ctx):
    """The same step from a host batch (x, a, e, i), a DeviceBatch that carries e and a DeviceDisjointLoader(DeviceDataset(
    edge_features=True)) batch: the same loss, hits and gradients bit for bit (the loader's batch brings its own transposed
    pattern and permutation).  The logits move with e and with lin.weight."""
    import gcnx
    from gcnx import Graph, ListDataset, synth
    from gcnx.device import Segments
    from gcnx.models import DeviceBatch
    raw = synth.tiny_graphs(6, 16, seed=3)
    graphs = []
    for k, (x, a, y) in enumerate(raw):
        a = a.tocsr()
        a.sort_indices()
        graphs.append(Graph(x=x, a=a, y=y, e=_features(a.nnz, 2, 100 + k)))
    ds = ListDataset(graphs)
    dev = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, ds, edge_features=True), batch_size=6, epochs=1, shuffle=False)
    host = gcnx.DisjointLoader(ds, batch_size=6, epochs=1, shuffle=False)
    m = gcnx.GINE(ctx, hidden_channels=64, edge_dim=2, train_eps=True, seed=2)
    (inputs, target), (db, none) = next(iter(host)), next(iter(dev))
    assert none is None and len(inputs) == 4
    m.loss_and_grads(inputs, target)
    hbatch = m._last_batch
    la_h, g_h, out_h = m.loss_acc.numpy(), m.gradients(), m._bufs["out"].numpy()
    assert hbatch.a.nnz == db.a.nnz and np.array_equal(hbatch.a.colidx.numpy()[:db.a.nnz], db.a.colidx.numpy()[:db.a.nnz])
    assert np.array_equal(_bits(hbatch.e.numpy()), _bits(db.e.numpy()))
    preset = [v.ptr for v in db.a.transpose_perm()]
    m.loss_and_grads(db)
    assert [v.ptr for v in m._op(db)[1].transpose_perm()] == preset      # the loader's transposed pattern is used
    la_d, g_d = m.loss_acc.numpy(), m.gradients()
    gp = np.concatenate([[0], np.cumsum(np.bincount(np.asarray(inputs[3])))]).astype(np.int32)
    mine = DeviceBatch(ctx, ctx.to_device(hbatch.x.numpy()), hbatch.a, Segments(ctx, gp), ctx.to_device(hbatch.y.numpy()),
                       e=ctx.to_device(hbatch.e.numpy()))
    m.loss_and_grads(mine)
    la_m, g_m = m.loss_acc.numpy(), m.gradients()
    for la, g in ((la_d, g_d), (la_m, g_m)):
        assert np.array_equal(_bits(la), _bits(la_h))
        assert all(np.array_equal(_bits(g[k]), _bits(g_h[k])) for k in g_h)
    assert max(np.max(np.abs(g_h[f"conv{k}.lin.weight"])) for k in (1, 2)) > 0
    # the logits read e and lin.weight
    x, a, e, i = inputs
    assert np.array_equal(_bits(m(inputs)), _bits(out_h))
    assert not np.allclose(m((x, a, 0.5 * np.asarray(e), i)), out_h, rtol=1e-3, atol=1e-3)
    sd = m.state_dict()
    sd["conv1.lin.weight"] = 2.0 * sd["conv1.lin.weight"]
    m.load_state_dict(sd)
    assert not np.allclose(m(inputs), out_h, rtol=1e-3, atol=1e-3)
    with pytest.raises(ValueError):
        m.loss_and_grads(inputs[:2] + inputs[3:], target)                 # (x, a, i) for a model that reads e
    with pytest.raises(ValueError):
        m((x, a, np.zeros((np.asarray(e).shape[0], 3), np.float32), i))   # another edge_dim


def test_fit_and_evaluate_run_the_gine_model_from_device_batches(ctx):
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(8, 16, seed=3)
    mk = lambda part: ListDataset([Graph(x=x, a=a.tocsr(), y=y, e=_features(a.tocsr().nnz, 2, 7)) for x, a, y in part])
    tr, te = gcnx.DeviceDataset(ctx, mk(raw[:5]), edge_features=True), gcnx.DeviceDataset(ctx, mk(raw[5:]), edge_features=True)
    m = gcnx.GINE(ctx, hidden_channels=32, edge_dim=2, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=1, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=1, schedule=lambda it: 0.01, verbose=False,
                   optimizer=gcnx.Adam())
    assert len(out["history"]) == 1 and np.all(np.isfinite(out["history"][0]))
    (loss, acc), preds = gcnx.models.evaluate(m, gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False))
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and len(preds) == 1

"""GPU tests of gcnx.Explainer and csrc/explain.hip: the sampled dense-dense product and the mask kernels in
sentinel frames against float64, the saturated mask, step parity against tests/explain_ref.py on the device's kink sides, the
frozen model, and the objective going down."""
import numpy as np
import pytest

from conftest import assert_close
import attn_pool_ref as AR
import explain_ref as X
import gcn_bn_ref as R
import graph_norm_ref as GN
from gpu_frames import Frame, bits, same

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FAST = (16, 32, 64, 128)
WORST = {}                                       # what -> the worst error / bound ratio seen (printed by the last test of a group)


def _worst(what, value):
    WORST[what] = max(WORST.get(what, 0.0), float(value))


def _csr(ctx, rowptr, colidx, vals=None):
    from gcnx.device import DeviceCSR
    n, nnz = len(rowptr) - 1, len(colidx)
    rp = ctx.to_device(np.asarray(rowptr, np.int32))
    ci = ctx.to_device(np.asarray(colidx, np.int32)) if nnz else ctx.zeros(4, np.int32)
    v = None if vals is None else ctx.to_device(np.asarray(vals, np.float32)) if nnz else ctx.zeros(4)
    return DeviceCSR(ctx, n, nnz, rp, ci, v, symmetric=False)


# ---- 1. gcnx_sddmm_csr ---------------------------------------------------------------------------------------------------------
def _pattern(shape):
    """(rowptr, colidx) of the two test patterns.  70: two full 32-row tiles and a 6-row tail, degrees 0 .. 12.  1200: row 40
    holds 1100 entries (its tile passes the 1024 staged ones), rows of 0 and 1 entries around it, an empty last row."""
    rng = np.random.default_rng(shape)
    n = shape
    deg = rng.integers(0, 13, n)
    if n == 1200:
        deg[40], deg[41], deg[42], deg[-1] = 1100, 0, 1, 0
    deg[3], deg[4] = 0, 1
    cols = [np.sort(rng.choice(n, d, replace=False)) for d in deg]
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), np.concatenate(cols).astype(np.int32)


@pytest.mark.parametrize("f", [1, 5, 16, 20, 32, 64, 128, 256])
@pytest.mark.parametrize("shape", [70, 1200])
def test_sddmm_in_frames(ctx, shape, f):
    from gcnx import device as D
    rowptr, colidx = _pattern(shape)
    n, nnz = shape, len(colidx)
    assert nnz > 0 and (shape != 1200 or rowptr[64] - rowptr[32] > 1024)
    a = _csr(ctx, rowptr, colidx)
    rng = np.random.default_rng(1000 * shape + f)
    l, r = rng.normal(size=(n, f)).astype(np.float32), rng.normal(size=(n, f)).astype(np.float32)
    scale, prev = rng.normal(size=nnz).astype(np.float32), rng.normal(size=nnz).astype(np.float32)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    l64, r64 = l.astype(np.float64)[rows], r.astype(np.float64)[colidx]
    dot, mag = np.einsum("ek,ek->e", l64, r64), np.einsum("ek,ek->e", np.abs(l64), np.abs(r64))
    for layout in ("aligned", "odd"):
        ld, leads = (f, (0, 0, 0)) if layout == "aligned" else (f + 3, (3, 5, 1))
        fl, fr = Frame(ctx, n, f, ld, leads[0], l), Frame(ctx, n, f, ld, leads[1], r)
        fs = Frame(ctx, 1, nnz, nnz, leads[2], scale)
        if layout == "aligned" and f in FAST:
            assert fl.aligned() and fr.aligned()             # the tile kernel's operands
        for use_scale in (False, True):
            for acc in (False, True):
                what = f"sddmm n={shape} f={f} {layout} scale={use_scale} acc={acc}"
                out = Frame(ctx, 1, nnz, nnz, leads[2], prev)
                D.sddmm(ctx, a, fl.view, fr.view, out.view, fs.view if use_scale else None, accumulate=acc)
                got = out.numpy().reshape(-1).astype(np.float64)
                s64 = scale.astype(np.float64) if use_scale else 1.0
                p64 = prev.astype(np.float64) if acc else 0.0
                bound = (f + 3) * U * (np.abs(s64) * mag + np.abs(p64))
                err = np.abs(got - (s64 * dot + p64))
                assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))
                _worst("sddmm err / bound", np.max(err / np.maximum(bound, 1e-300)))
                if not acc:                                  # the same call leaves the same bits
                    again = Frame(ctx, 1, nnz, nnz, leads[2], prev)
                    D.sddmm(ctx, a, fl.view, fr.view, again.view, fs.view if use_scale else None)
                    assert same(again.numpy(), out.numpy()), what
        fl.untouched(f"{layout} L")
        fr.untouched(f"{layout} R")
        fs.untouched(f"{layout} scale")


def test_sddmm_empty_and_refusals(ctx):
    from gcnx import _lib, device as D
    l, r = Frame(ctx, 8, 16, 16, 0, np.ones((8, 16))), Frame(ctx, 8, 16, 16, 0, np.ones((8, 16)))
    out = Frame(ctx, 1, 8, 8, 1)
    D.sddmm(ctx, _csr(ctx, np.zeros(9, np.int32), []), l.view, r.view, out.view)               # nnz == 0
    out.untouched("nnz == 0")
    e = Frame(ctx, 0, 16, 16, 0)
    D.sddmm(ctx, _csr(ctx, np.zeros(1, np.int32), []), e.view, e.view, out.view)               # n == 0
    out.untouched("n == 0")
    a = _csr(ctx, np.arange(9, dtype=np.int32), np.arange(8)[::-1].copy())
    lib = ctx.lib
    for lp, rp, op in ((None, r.view.ptr, out.view.ptr), (l.view.ptr, None, out.view.ptr), (l.view.ptr, r.view.ptr, None)):
        rc = lib.gcnx_sddmm_csr(ctx.h, a.rowptr.ptr, a.colidx.ptr, 8, 8, lp, 16, rp, 16, 16, None, op, 0)
        assert rc != _lib.OK
    out.untouched("refused")
    D.sddmm(ctx, a, l.view, r.view, out.view)
    out.check(np.full(8, 16.0, np.float32), "ones")
    print("worst:", WORST)


# ---- 2. the mask kernels -------------------------------------------------------------------------------------------------------
def _mask_pattern(kind):
    """(A^ scipy CSR with every diagonal entry, rows, off): the small batch of the step tests, or 3000 rows of ~25 entries
    (more entries than one pass of the 256 workgroups covers, so the grid-stride loop runs)."""
    if kind == "small":
        x, a, gp, _ = X.make_batch((12, 19, 10, 25), 4, seed=1)
        return X.operator(a, x.shape[0])
    import scipy.sparse as sp
    rng = np.random.default_rng(7)
    n = 3000
    d = sp.random(n, n, density=25 / n, random_state=rng, format="csr")
    return X.operator(sp.csr_matrix(d + d.T + sp.identity(n)), n)


@pytest.mark.parametrize("kind", ["small", "large"])
@pytest.mark.parametrize("span", [8.0, 40.0])
def test_edge_mask_kernels_in_frames(ctx, kind, span):
    from gcnx import device as D
    A, rows, off = _mask_pattern(kind)
    n, nnz = A.shape[0], A.nnz
    assert kind == "small" or nnz > 256 * 256
    rng = np.random.default_rng(nnz)
    logits = (rng.uniform(-span, span, nnz) if span == 8.0 else rng.choice([-span, span], nnz)).astype(np.float32)
    a32, dv = A.data.astype(np.float32), rng.normal(size=nnz).astype(np.float32)
    a = _csr(ctx, A.indptr, A.indices, a32)
    pm = a.transpose_perm()[2]
    perm = pm.numpy()[:nnz]
    fa, fm, fdv = (Frame(ctx, 1, nnz, nnz, lead, d) for lead, d in ((0, a32), (1, logits), (3, dv)))
    a.vals = fa.view
    v, vt, dm = Frame(ctx, 1, nnz, nnz, 1), Frame(ctx, 1, nnz, nnz, 2), Frame(ctx, 1, nnz, nnz, 3)
    terms, scratch = Frame(ctx, 1, 2, 2, 1), ctx.empty(D.mask_scratch_floats(ctx))
    D.edge_mask_fwd(ctx, a, fm.view, v.view, pm, vt.view)
    c_size, c_ent = 0.005, 1.0 / max(int(off.sum()), 1)
    D.edge_mask_bwd(ctx, a, fm.view, fdv.view, dm.view, terms.view, scratch, c_size, c_ent)
    got_v, got_vt, got_dm, got_t = (fr.numpy().reshape(-1) for fr in (v, vt, dm, terms))
    for fr in (fa, fm, fdv):
        fr.untouched("mask operand")
    s = X.sigmoid(logits)
    assert np.array_equal(bits(got_v[~off]), bits(a32[~off]))                                   # the diagonal passes through
    assert np.array_equal(bits(got_vt), bits(got_v[perm]))
    assert not got_dm[~off].any()                                                                  # exactly 0 on the diagonal
    assert all(np.all(np.isfinite(g)) for g in (got_v, got_vt, got_dm, got_t))
    if span == 40.0:
        return                                               # saturated in fp32: finite outputs, a clean diagonal
    ref_v = a32.astype(np.float64) * np.where(off, s, 1.0)
    ref_dm = np.where(off, (dv.astype(np.float64) * a32 + c_size + c_ent * X.dent(s)) * s * (1 - s), 0.0)
    ref_t = np.array([s[off].sum(), X.ent(s[off]).sum()])
    assert_close(got_v, ref_v, 1e-5, f"edge_mask_fwd {kind}")
    assert_close(got_dm, ref_dm, 1e-5, f"edge_mask_bwd dlogits {kind}")
    assert np.all(np.abs(got_t - ref_t) <= 1e-5 * np.abs(ref_t)), (got_t, ref_t)
    _worst("edge mask rel", max(np.max(np.abs(got_v - ref_v)) / np.max(np.abs(ref_v)), np.max(np.abs(got_dm - ref_dm)) / np.max(np.abs(ref_dm)),
                                np.max(np.abs(got_t - ref_t) / np.abs(ref_t))))
    again = Frame(ctx, 1, 2, 2, 1)
    D.edge_mask_bwd(ctx, a, fm.view, fdv.view, dm.view, again.view, scratch, c_size, c_ent)
    assert same(again.numpy(), terms.numpy())                                                    # a fixed order of summation


@pytest.mark.parametrize("n,f", [(70, 5), (3000, 16), (20000, 3)])
@pytest.mark.parametrize("form", ["common", "rows"])
@pytest.mark.parametrize("span", [8.0, 40.0])
def test_feat_mask_kernels_in_frames(ctx, n, f, form, span):
    from gcnx import device as D
    rng = np.random.default_rng(n + f)
    shape = (1, f) if form == "common" else (n, f)
    logits = (rng.uniform(-span, span, shape) if span == 8.0 else rng.choice([-span, span], shape)).astype(np.float32)
    x, dxm = rng.normal(size=(n, f)).astype(np.float32), rng.normal(size=(n, f)).astype(np.float32)
    fx, fd = Frame(ctx, n, f, f + 3, 1, x), Frame(ctx, n, f, f + 3, 5, dxm)
    fm = Frame(ctx, shape[0], f, f, 0, logits)
    out, dm, terms = Frame(ctx, n, f, f + 1, 3), Frame(ctx, shape[0], f, f, 2), Frame(ctx, 1, 2, 2, 1)
    scratch = ctx.empty(D.mask_scratch_floats(ctx, n, f, form == "rows"))
    D.feat_mask_fwd(ctx, fx.view, fm.view, out.view)
    c_size, c_ent = 1.0 / logits.size, 0.1 / logits.size
    D.feat_mask_bwd(ctx, fd.view, fx.view, fm.view, dm.view, terms.view, scratch, c_size, c_ent)
    got_o, got_dm, got_t = out.numpy(), dm.numpy(), terms.numpy().reshape(-1)
    for fr in (fx, fd, fm):
        fr.untouched("mask operand")
    assert all(np.all(np.isfinite(g)) for g in (got_o, got_dm, got_t))
    if span == 40.0:
        return
    s = X.sigmoid(logits)
    data = dxm.astype(np.float64) * x
    ref_dm = ((data.sum(0, keepdims=True) if form == "common" else data) + c_size + c_ent * X.dent(s)) * s * (1 - s)
    ref_t = np.array([s.sum(), X.ent(s).sum()])
    assert_close(got_o, x.astype(np.float64) * s, 1e-5, f"feat_mask_fwd {form}")
    assert_close(got_dm, ref_dm, 1e-5, f"feat_mask_bwd {form}")
    assert np.all(np.abs(got_t - ref_t) <= 1e-5 * np.abs(ref_t)), (got_t, ref_t)
    _worst("feat mask rel", max(np.max(np.abs(got_dm - ref_dm)) / np.max(np.abs(ref_dm)), np.max(np.abs(got_t - ref_t) / np.abs(ref_t))))


# ---- the model-level tests -----------------------------------------------------------------------------------------------------
def _params(f, h, seed, norm="batch", readout="max"):
    if norm == "graph":
        p = GN.init_params(f, h, seed, readout=readout)
    else:
        p = AR.init_params(f, h, seed) if readout == "attention" else R.init_params(f, h, seed)
    return {k: np.asarray(v, np.float32) for k, v in p.items()}


def _model(ctx, f, h, p, norm="batch", readout="max"):
    import gcnx
    m = gcnx.GCN(ctx, hidden_channels=h, seed=0, norm=norm, readout=readout)
    m.build(f)
    m.load_state_dict(p)
    return m


def _batch(ctx, x, a, gp, y=None):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    csr = DeviceCSR.from_host_csr(ctx, a.indptr.astype(np.int32), a.indices.astype(np.int32), None, gp)
    return DeviceBatch(ctx, ctx.to_device(x), csr, Segments(ctx, gp), ctx.to_device(np.asarray(y, np.float32)) if y is not None else None)


# ---- 3. a saturated mask is no mask --------------------------------------------------------------------------------------------
def test_saturated_mask_is_no_mask(ctx):
    import gcnx
    x, a, gp, y = X.make_batch((14, 22, 30, 17), 16, seed=2)
    m = _model(ctx, 16, 64, _params(16, 64, 3))
    batch = _batch(ctx, x, a, gp, y)
    m.loss_and_grads(batch)
    want = m._bufs["out"].numpy()
    ex = gcnx.Explainer(m, explanation_type="phenomenon").begin(batch)
    try:
        ex.set_logits(edge=np.full(a.nnz, 40.0, np.float32))
        ex.step()
        assert same(m._bufs["out"].numpy(), want)            # rcp(1 + exp(-40)) is exactly 1 and A^ * 1 is A^
    finally:
        ex.end()


# ---- 4. step parity ----------------------------------------------------------------------------------------------------------------
# (f_in, hidden, norm, readout, node_mask, edge_mask, directed, explanation_type)
CASES = {
    "symmetric-16-64": (16, 64, "batch", "max", None, True, False, "model"),
    "off-widths-5-20": (5, 20, "batch", "max", "common_attributes", True, False, "phenomenon"),
    "hidden-256": (16, 256, "batch", "max", None, True, False, "model"),
    "directed": (16, 64, "batch", "max", None, True, True, "phenomenon"),
    "graph-norm": (16, 64, "graph", "max", None, True, False, "model"),
    "attention": (16, 64, "batch", "attention", None, True, False, "model"),
    "node-common": (16, 64, "batch", "max", "common_attributes", True, False, "model"),
    "node-attributes": (16, 32, "batch", "max", "attributes", True, False, "phenomenon"),
    "node-only": (16, 64, "batch", "max", "attributes", False, False, "model"),
}
SIZES = (14, 22, 40, 17)                         # four graphs of 10 .. 40 nodes; node 13 is isolated (explain_ref.make_batch)


def _sides(m):
    """The device's kink sides of the forward it just ran, as explain_ref.model takes them."""
    b, p = m._bufs, m.p
    if m.norm == "graph":
        masks = {"m1": b["y1"].numpy() > 0, "m2": b["y2"].numpy() > 0}
    else:
        masks = {f"m{k}": R.device_prelu_sides(b[f"z{k}"].numpy(), b[f"m{k}"].numpy(), b[f"i{k}"].numpy(), p[f"g{k}"].numpy(),
                                                p[f"be{k}"].numpy()) for k in (1, 2)}
    return {"masks": masks, "argmax": b["arg"].numpy().astype(np.int64) if m.readout == "max" else None}


def _rule(got, ref, what):
    """The whole-step rule: 1e-4 of the tensor's largest reference magnitude (conftest.assert_close)."""
    assert_close(got, ref, 1e-4, what)
    ref = np.asarray(ref, np.float64)
    _worst("step rel", np.max(np.abs(np.asarray(got, np.float64) - ref)) / max(np.max(np.abs(ref)), 1e-30))


@pytest.mark.parametrize("case", list(CASES))
def test_step_parity(ctx, case):
    import gcnx
    f, h, norm, readout, node, edge, directed, kind = CASES[case]
    x, a, gp, y = X.make_batch(SIZES, f, seed=len(case), directed=directed)
    n = x.shape[0]
    A, rows, off = X.operator(a, n)
    assert directed == ((A != A.T).nnz != 0) and A[13].nnz == 1
    p = _params(f, h, 21, norm, readout)
    m = _model(ctx, f, h, p, norm, readout)
    ex = gcnx.Explainer(m, node_mask=node, edge_mask=edge, explanation_type=kind, seed=4).begin(_batch(ctx, x, a, gp, y))
    try:
        t = ex._s["target"]
        if kind == "phenomenon":
            assert np.array_equal(t, y)
        lg = ex.logits()
        e0, n0 = X.initial_logits(n, A.nnz, None if node is None else lg["node"].shape, seed=4, edge=edge)
        assert (lg["edge"] is None) == (not edge) and (not edge or np.array_equal(lg["edge"], e0.astype(np.float32)))
        assert (lg["node"] is None) == (node is None) and (node is None or np.array_equal(lg["node"], n0.astype(np.float32)))
        if edge:                                 # m_ij != m_ji on the symmetric pattern: a backward that reuses A^_m as its transpose fails
            ex.set_logits(edge=np.random.default_rng(9).normal(0, 1.5, A.nnz))
        state = None
        for step in range(5):
            lg = ex.logits()
            out = ex.forward()
            sides = _sides(m)
            r = X.model(x, a, gp, p, t, lg["edge"], lg["node"], norm=norm, readout=readout, **sides)
            _rule(out, r["out"], f"{case} step {step} logits")
            ex.step()
            obj, g = ex.objective(), ex.gradients()
            for k in X.TERMS:
                assert abs(obj[k] - r["terms"][k]) <= 1e-4 * abs(r["terms"][k]), (case, step, k, obj[k], r["terms"][k])
                _worst("step term rel", abs(obj[k] - r["terms"][k]) / max(abs(r["terms"][k]), 1e-30))
            if edge:
                _rule(g["edge"], r["d_edge"], f"{case} step {step} d_edge")
                assert not g["edge"][~off].any()
            if node is not None:
                _rule(g["node"], r["d_node"], f"{case} step {step} d_node")
            state = state or X.adam_init(lg["edge"], lg["node"])
            want = X.adam_step([lg["edge"], lg["node"]], [r["d_edge"], r["d_node"]], state, lr=0.01)
            after = ex.logits()
            if edge:
                _rule(after["edge"], want[0], f"{case} step {step} edge logits")
            if node is not None:
                _rule(after["node"], want[1], f"{case} step {step} node logits")
        assert ex.history().shape == (5, 5)
    finally:
        ex.end()
    print("worst:", WORST)


def test_step_cases_cover_both_conv_routes(ctx):
    from gcnx import device as D
    n = sum(SIZES)
    routes = set()
    for f, h, *_ in CASES.values():
        routes |= {bool(D.gcn_conv_fused_ok(ctx, n, f, h, f)), bool(D.gcn_conv_fused_ok(ctx, n, h, h, h))}
    assert routes == {True, False}                           # the one-launch (A^ x) W and the composed GEMM + SpMM


# ---- 5. the model is frozen ------------------------------------------------------------------------------------------------------
def _snapshot(m, opt, batch):
    return {"p": m.flat_p.numpy(), "m": opt.flat("m").numpy(), "v": opt.flat("v").numpy(), "t": opt.t.numpy(), "out": m(batch)}


def _same_snapshot(a, b):
    assert np.array_equal(a["t"], b["t"])
    for k in ("p", "m", "v", "out"):
        assert same(a[k], b[k]), k


def test_model_is_frozen(ctx):
    import gcnx
    from gcnx.models import DeviceBatch
    x, a, gp, y = X.make_batch(SIZES, 16, seed=6)
    m = _model(ctx, 16, 64, _params(16, 64, 5))
    opt = gcnx.Adam()
    m.set_optimizer(opt)
    batch = _batch(ctx, x, a, gp, y)
    m.train_step(batch, lr=0.01)                             # the optimizer's state is no longer zero
    before = _snapshot(m, opt, batch)
    assert before["m"].any() and before["v"].any()
    cache = m._op_cache
    expl = gcnx.Explainer(m, epochs=5, node_mask="common_attributes")(batch)
    assert m._op_cache is cache
    _same_snapshot(before, _snapshot(m, opt, batch))
    n_off = a.nnz - x.shape[0]
    assert expl.edge_mask.shape == (n_off,) and expl.edge_index.shape == (2, n_off) and expl.graph_of_edge.shape == (n_off,)
    assert expl.node_mask.shape == (1, 16) and expl.history.shape == (5, 5) and expl.target.shape == (4,)
    assert np.all((expl.edge_mask > 0) & (expl.edge_mask < 1)) and np.all(np.isfinite(expl.history))
    ei, em = expl.top_edges(3, graph=2)
    assert em.shape == (3,) and np.all(np.diff(em) <= 0) and np.all((ei >= gp[2]) & (ei < gp[3]))
    # a step that raises midway (the masks are formed, then the model refuses a batch of the wrong width), then end()
    ex = gcnx.Explainer(m, epochs=5).begin(batch)
    ex.step()
    ex._s["mbatch"] = DeviceBatch(ctx, ctx.zeros((x.shape[0], 7)), batch.a, batch.seg, ex._s["y"])
    with pytest.raises(ValueError):
        ex.step()
    ex.end()
    ex.end()
    assert m._op_cache is cache
    _same_snapshot(before, _snapshot(m, opt, batch))
    with pytest.raises(ValueError):                          # a batch of one graph: as training
        gcnx.Explainer(m).begin(_batch(ctx, x[:14], a[:14, :14], gp[:2], y[:1]))
    assert m._op_cache is cache


# ---- 6. it optimises ---------------------------------------------------------------------------------------------------------------
def test_objective_goes_down(ctx):
    """The run tests/test_explain_host.py checks on the restatement (there: down by more than 1 % in 30 steps, every step)."""
    import gcnx
    x, a, gp, p = X.opt_case()
    c = X.OPT_CASE
    m = _model(ctx, c["f"], c["h"], {k: np.asarray(v, np.float32) for k, v in p.items()})
    expl = gcnx.Explainer(m, epochs=30, seed=c["seed"])((x, a, np.repeat(np.arange(len(gp) - 1), np.diff(gp))))
    h = expl.history
    assert h.shape == (30, 5) and h[-1].sum() < h[0].sum(), (h[0].sum(), h[-1].sum())

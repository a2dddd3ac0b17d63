"""GPU tests of gcnx.PDN and csrc/pdn.hip: the operator and its backward in sentinel frames against float64
(tests/pdn_ref.py), saturated gates against gcnx.GCN, step parity on the device's kink sides, the device loader and the gates
read back."""
import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import pdn_ref as PR
from gpu_frames import Frame, bits, same
from test_gpu_gcn_bn import UNDER_BN

pytestmark = pytest.mark.gpu

WORST = {}                                       # what -> the worst error / tolerance ratio seen


def _worst(what, value):
    WORST[what] = max(WORST.get(what, 0.0), float(value))


def _csr(ctx, rowptr, colidx):
    from gcnx.device import DeviceCSR
    n, nnz = len(rowptr) - 1, len(colidx)
    return DeviceCSR(ctx, n, nnz, ctx.to_device(np.asarray(rowptr, np.int32)), ctx.to_device(np.asarray(colidx, np.int32)), None,
                     symmetric=False)


def _as(frame, shape):
    """The frame's (contiguous) view under another shape."""
    from gcnx.device import DeviceArray
    return DeviceArray(frame.ctx, frame.view.ptr, shape, np.float32, base=frame.buf)


class _Mlp:
    """The four tensors of a gate MLP in frames, stored as the library reads them: W1 [D, He], b1 [He], w2 [He], b2 [1]."""

    def __init__(self, ctx, c, b2=None, w2=None):
        he, d = c["w1"].shape
        w2 = c["w2"] if w2 is None else w2
        self.frames = [Frame(ctx, 1, d * he, d * he, 3, c["w1"].T), Frame(ctx, 1, he, he, 1, c["b1"]), Frame(ctx, 1, he, he, 2, w2),
                       Frame(ctx, 1, 1, 1, 5, c["b2"] if b2 is None else b2)]
        self.views = (_as(self.frames[0], (d, he)), _as(self.frames[1], (he,)), _as(self.frames[2], (he,)), _as(self.frames[3], (1,)))

    def untouched(self):
        for f in self.frames:
            f.untouched("gate MLP")


def _layouts(c):
    d = c["e"].shape[1]
    return (("aligned", d, 0), ("odd", d + 3, 3))


def _ratio(got, ref, tol):
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref))) / (tol * max(float(np.max(np.abs(ref))), 1e-30))


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,d,he", PR.operator_cases())
def test_operator_forward_in_frames(ctx, shape, d, he):
    from gcnx import device as D
    c = PR.operator_case(shape, d, he)
    n, nnz = c["n"], c["nnz"]
    a = _csr(ctx, c["rowptr"], c["colidx"])
    pm = a.transpose_perm()[2]
    perm = pm.numpy()[:nnz]
    assert np.array_equal(perm, PR.transpose_perm(c["rowptr"], c["colidx"])[2])
    empty = np.diff(c["rowptr"]) == 0
    mlp = _Mlp(ctx, c)
    for layout, lde, lead in _layouts(c):
        fe = Frame(ctx, nnz, d, lde, lead, c["e"])
        for use_unit in (False, True):
            unit = ctx.to_device(c["unit"].astype(np.uint8)) if use_unit else None
            ref = PR.operator(c["rowptr"], c["colidx"], c["e"], c["w1"], c["b1"], c["w2"], c["b2"], unit=c["unit"] if use_unit else None)
            for use_perm in (False, True):
                what = f"pdn_operator n={shape} D={d} He={he} {layout} unit={use_unit} perm={use_perm}"
                outs = []
                for _ in range(2):                           # a second call leaves the same bits
                    w, r, v, vt = Frame(ctx, 1, nnz, nnz, 1), Frame(ctx, 1, n, n, 2), Frame(ctx, 1, nnz, nnz, 3), Frame(ctx, 1, nnz, nnz, 1)
                    D.pdn_operator(ctx, a, fe.view, *mlp.views, _as(w, (nnz,)), _as(r, (n,)), _as(v, (nnz,)), unit=unit,
                                   perm_t=pm if use_perm else None, vals_t_out=_as(vt, (nnz,)) if use_perm else None)
                    outs.append([fr.numpy().reshape(-1) for fr in (w, r, v)] + [vt])
                (gw, gr, gv, fvt), again = outs
                assert all(same(x, y) for x, y in zip(again[:3], (gw, gr, gv))), what
                if use_perm:
                    assert np.array_equal(bits(fvt.numpy().reshape(-1)), bits(gv[perm])), what
                    assert same(again[3].numpy(), fvt.numpy())
                else:
                    fvt.untouched(what)
                for name, got, want in (("w", gw, ref["w"]), ("r", gr, ref["r"]), ("v", gv, ref["v"])):
                    assert_close(got, want, 1e-5, f"{what} {name}")
                    _worst("operator forward err / tol", _ratio(got, want, 1e-5))
                assert not gr[empty].any() and empty.any(), what                       # an empty row: r == 0
                if use_unit:
                    assert np.array_equal(bits(gw[c["unit"]]), bits(np.ones(int(c["unit"].sum()), np.float32))), what
            if unit is not None:
                assert np.array_equal(unit.numpy(), c["unit"].astype(np.uint8))
        fe.untouched(f"{layout} e")
    mlp.untouched()
    print("worst:", WORST)


@pytest.mark.parametrize("shape,d,he", [(70, 2, 16), (1200, 8, 64)])
def test_operator_saturated_logits_stay_finite(ctx, shape, d, he):
    from gcnx import device as D
    c = PR.operator_case(shape, d, he)
    n, nnz = c["n"], c["nnz"]
    a = _csr(ctx, c["rowptr"], c["colidx"])
    rp_t, ci_t, pm = a.transpose_perm()
    e, g = ctx.to_device(c["e"]), ctx.to_device(c["g"])
    scratch = ctx.empty(D.pdn_bwd_scratch_floats(ctx, n, nnz, d, he))
    for sign in (40.0, -40.0):
        mlp = _Mlp(ctx, c, b2=np.array([sign], np.float32), w2=np.zeros(he, np.float32))     # every logit is exactly +-40
        w, r, v, vt = (Frame(ctx, 1, k, k, 1) for k in (nnz, n, nnz, nnz))
        D.pdn_operator(ctx, a, e, *mlp.views, _as(w, (nnz,)), _as(r, (n,)), _as(v, (nnz,)), perm_t=pm, vals_t_out=_as(vt, (nnz,)))
        got = [fr.numpy().reshape(-1) for fr in (w, r, v, vt)]
        assert all(np.all(np.isfinite(x)) for x in got), sign
        if sign > 0:
            assert np.array_equal(bits(got[0]), bits(np.ones(nnz, np.float32)))         # w == 1 exactly
            ref = PR.operator(c["rowptr"], c["colidx"], c["e"], c["w1"], c["b1"], np.zeros(he), [sign])
            assert_close(got[2], ref["v"], 1e-5, "saturated v")
        grads = [Frame(ctx, 1, k, k, 1) for k in (d * he, he, he, 1)]
        D.pdn_operator_bwd(ctx, a, e, *mlp.views, _as(w, (nnz,)), _as(r, (n,)), g, _as(grads[0], (d, he)), _as(grads[1], (he,)),
                           _as(grads[2], (he,)), _as(grads[3], (1,)), scratch)
        assert all(np.all(np.isfinite(fr.numpy())) for fr in grads), sign


# ---- 2. its backward ---------------------------------------------------------------------------------------------------------------
def _bwd_case(ctx, c, g, lde, lead, use_unit, what):
    """One gcnx_pdn_operator_bwd in frames on w, r of the float64 forward (rounded to float32): every gradient within 1e-5 of
    the condition of its sum; the worst ratio."""
    from gcnx import device as D
    n, nnz = c["n"], c["nnz"]
    he, d = c["w1"].shape
    a = _csr(ctx, c["rowptr"], c["colidx"])
    a.transpose_perm()
    op = PR.operator(c["rowptr"], c["colidx"], c["e"], c["w1"], c["b1"], c["w2"], c["b2"], unit=c["unit"] if use_unit else None)
    ref, cond, _, _ = PR.operator_bwd(op, c["w2"], g)
    mlp = _Mlp(ctx, c)
    fe, fw, fr, fg = Frame(ctx, nnz, d, lde, lead, c["e"]), Frame(ctx, 1, nnz, nnz, 1, op["w"]), Frame(ctx, 1, n, n, 3, op["r"]), \
        Frame(ctx, 1, nnz, nnz, 2, g)
    unit = ctx.to_device(c["unit"].astype(np.uint8)) if use_unit else None
    scratch = ctx.empty(D.pdn_bwd_scratch_floats(ctx, n, nnz, d, he))
    outs = []
    for _ in range(2):
        grads = [Frame(ctx, 1, k, k, lead_) for k, lead_ in ((d * he, 1), (he, 2), (he, 3), (1, 1))]
        D.pdn_operator_bwd(ctx, a, fe.view, *mlp.views, _as(fw, (nnz,)), _as(fr, (n,)), _as(fg, (nnz,)), _as(grads[0], (d, he)),
                           _as(grads[1], (he,)), _as(grads[2], (he,)), _as(grads[3], (1,)), scratch, unit=unit)
        outs.append([fr_.numpy().reshape(-1) for fr_ in grads])
    assert all(same(x, y) for x, y in zip(*outs)), what      # a fixed order of summation
    for f in (fe, fw, fr, fg):
        f.untouched(what)
    mlp.untouched()
    worst = 0.0
    got = dict(zip(("w1", "b1", "w2", "b2"), outs[0]))
    for k in got:
        want = ref[k].T.reshape(-1) if k == "w1" else ref[k].reshape(-1)             # the library stores W1 [D, He]
        bound = 1e-5 * (cond[k].T.reshape(-1) if k == "w1" else cond[k].reshape(-1))
        err = np.abs(got[k].astype(np.float64) - want)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.all(err <= bound), (what, k, ratio)
        worst = max(worst, ratio)
    return worst, ref


@pytest.mark.parametrize("shape,d,he", PR.operator_cases())
def test_operator_backward_in_frames(ctx, shape, d, he):
    c = PR.operator_case(shape, d, he)
    for layout, lde, lead in _layouts(c):
        for use_unit in (False, True):
            worst, ref = _bwd_case(ctx, c, c["g"], lde, lead, use_unit, f"pdn_operator_bwd n={shape} D={d} He={he} {layout} unit={use_unit}")
            _worst("operator backward err / tol", worst)
            assert all(np.abs(v).max() > 0 for v in ref.values())
    print("worst:", WORST)


def test_operator_backward_walks_the_transposed_pattern(ctx):
    """G non-zero on ONE off-diagonal entry (i <- j) whose reverse is not stored: the column walk must find it in row j of the
    transposed pattern.  A walk that takes the forward pattern for its own transpose gives another q_j, far outside the bound."""
    c = PR.operator_case(70, 2, 16)
    rows, cols = PR.rows_of(c["rowptr"]), c["colidx"].astype(np.int64)
    deg = np.diff(c["rowptr"])
    pairs = set(zip(rows.tolist(), cols.tolist()))
    e0 = next(k for k, (i, j) in enumerate(zip(rows, cols)) if i != j and (j, i) not in pairs and deg[i] > 2 and deg[j] > 2)
    g = np.zeros(c["nnz"], np.float32)
    g[e0] = 1.0
    op = PR.operator(c["rowptr"], cols, c["e"], c["w1"], c["b1"], c["w2"], c["b2"])
    ref, cond, _, _ = PR.operator_bwd(op, c["w2"], g)
    c_e = g.astype(np.float64) * op["w"]
    walk = np.bincount(rows, c_e * op["r"][cols], minlength=c["n"])
    q_ok = walk + np.bincount(cols, c_e * op["r"][rows], minlength=c["n"])
    q_bad = 2 * walk                                         # the second walk over the forward pattern's own rows
    assert np.abs(q_bad - q_ok).max() > 0.1 * np.abs(q_ok).max() and np.abs(ref["w1"]).max() > 0 and cond["b2"][0] > 0
    worst, _ = _bwd_case(ctx, c, g, 2, 0, False, "one off-diagonal entry")
    _worst("operator backward, one entry, err / tol", worst)
    print("worst:", WORST)


# ---- the model-level tests -----------------------------------------------------------------------------------------------------
def _device_batch(ctx, x, a, e, gp, y=None):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    csr = DeviceCSR.from_host_csr(ctx, a.indptr.astype(np.int32), a.indices.astype(np.int32), None, gp)
    return DeviceBatch(ctx, ctx.to_device(x), csr, Segments(ctx, gp), ctx.to_device(np.asarray(y, np.float32)) if y is not None else None,
                       e=ctx.to_device(e))


# ---- 3. saturated gates give the reference's model ---------------------------------------------------------------------------------
def test_saturated_gates_give_gcn(ctx):
    import gcnx
    x, a, e, gp, y = PR.make_batch(PR.SIZES, 16, 2, seed=2)
    p = {k: np.asarray(v, np.float32) for k, v in PR.init_params(16, 64, 2, 16, seed=3).items()}
    for k in (1, 2):
        p[f"conv{k}.mlp.2.weight"] = np.zeros((1, 16), np.float32)
        p[f"conv{k}.mlp.2.bias"] = np.array([40.0], np.float32)
    gcn = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    gcn.build(16)
    gcn.load_state_dict({k: v for k, v in p.items() if k not in PR.GATE_KEYS})
    pdn = gcnx.PDN(ctx, hidden_channels=64, edge_dim=2, edge_hidden=16, seed=0)
    pdn.load_state_dict(p)
    batch = _device_batch(ctx, x, a, e, gp, y)
    want, got = gcn(batch), pdn(batch)
    # w == 1 exactly: the weighted normalisation is gcn_norm of the unweighted pattern; the two kernels may round deg^-1/2
    # differently, the restatement below is the float64 value of both
    top = float(np.max(np.abs(want)))
    assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-6 * top, (np.max(np.abs(got - want)), top)
    assert all(np.array_equal(bits(w), bits(np.ones(a.nnz, np.float32))) for w in pdn.edge_weights(batch))
    ref_pdn = PR.model(x, a.indptr, a.indices, e, gp, p)["out"]
    ref_gcn = R.model(x, a, gp, {k: v for k, v in p.items() if k not in PR.GATE_KEYS})["out"]
    assert np.max(np.abs(ref_pdn - ref_gcn)) <= 1e-12 * top
    _worst("saturated PDN vs GCN / (1e-6 top)", np.max(np.abs(got.astype(np.float64) - want)) / (1e-6 * top))
    print("worst:", WORST)


# ---- 4. step parity ----------------------------------------------------------------------------------------------------------------
def _sides(m, e_used, p, pos=None):
    """The device's kink sides of the step it just ran, at the parameters p it ran with."""
    b = m._bufs
    s = dict(pos or {})
    if m.norm == "batch":
        s.update({f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), p[f"batch_norm_{i}.weight"],
                                                p[f"batch_norm_{i}.bias"]) for i in (1, 2)})
    for i in (1, 2):
        s[f"gate{i}"] = PR.gate_sides(e_used, p[f"conv{i}.mlp.0.weight"], p[f"conv{i}.mlp.0.bias"])
    return s


def _cmp_grads(got, ref, tol, what):
    """The family's step rule: 1e-4 of the tensor's largest reference magnitude (an analytically zero gradient: of the weight
    gradient test_gpu_gcn_bn.UNDER_BN names)."""
    for k in got:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN.get(k, k)], np.float64))))
        err = float(np.max(np.abs(g - r)))
        assert err <= tol * scale, (what, k, err, scale)     # (scale == 0: a gradient that is exactly zero on both sides)
        _worst("step gradient err / tol", err / (tol * scale) if scale > 0 else 0.0)


@pytest.mark.parametrize("case", list(PR.STEP_CASES))
def test_step_parity(ctx, case):
    import gcnx
    f, h, d, he, norm, readout, directed, loops, route = PR.STEP_CASES[case]
    x, a, e, gp, y, p0 = PR.step_case(case)
    rp, ci, e2, unit = PR.with_unit_self_loops(a.indptr, a.indices, e)
    m = gcnx.PDN(ctx, hidden_channels=h, edge_dim=d, edge_hidden=he, seed=0, norm=norm, readout=readout)
    m.load_state_dict(p0)
    assert list(m.state_dict()) == list(PR.keys(readout, norm))
    ids = np.repeat(np.arange(len(gp) - 1), np.diff(gp))
    inputs = _device_batch(ctx, x, a, e, gp, y) if route == "device" else (x, a, e, ids)
    lr = 0.05
    for step in range(3):
        p = m.state_dict()                                   # the device's current parameters
        pos = None
        if norm == "graph":                                  # the PReLU sides: the signs of y1 / y2 of a forward of its own
            m(inputs)
            pos = {f"m{k}": m._bufs[f"y{k}"].numpy() > 0 for k in (1, 2)}
        m.loss_and_grads(inputs, None if route == "device" else y)
        batch = m._last_batch
        if route == "host":
            assert batch.a.nnz == len(ci) and np.array_equal(batch.a.colidx.numpy()[:len(ci)], ci)
            assert unit.any() and np.array_equal(batch.unit.numpy(), unit.astype(np.uint8)) and np.array_equal(batch.e.numpy(), e2)
        else:
            assert batch.unit is None and not unit.any()
        arg = m._bufs["arg"].numpy().astype(np.int64) if readout == "max" else None
        r = PR.model(x, rp, ci, e2, gp, p, y, masks=_sides(m, e2, p, pos), argmax=arg, readout=readout, norm=norm, unit=unit)
        what = f"{case} step {step}"
        assert_close(m._bufs["out"].numpy(), r["out"], 1e-4, f"{what} logits")
        la = m.loss_acc.numpy()
        assert rel_err(la[0], r["loss"]) < 1e-4 and la[1] == r["hits"], (what, la, r["loss"], r["hits"])
        _worst("step loss err / tol", rel_err(la[0], r["loss"]) / 1e-4)
        got = m.gradients()
        assert list(got) == list(PR.keys(readout, norm))
        _cmp_grads(got, r["grads"], 1e-4, what)
        assert all(np.abs(got[k]).max() > 0 for k in PR.GATE_KEYS), what
        m._apply_sgd(lr)
        after = m.state_dict()
        assert any(not np.array_equal(after[k], p[k]) for k in PR.GATE_KEYS)
    print("worst:", WORST)


def test_step_cases_cover_both_conv_routes(ctx):
    from gcnx import device as D
    n = sum(PR.SIZES)
    routes = set()
    for f, h, *_ in PR.STEP_CASES.values():
        routes |= {bool(D.gcn_conv_fused_ok(ctx, n, f, h, f)), bool(D.gcn_conv_fused_ok(ctx, n, h, h, h))}
    assert routes == {True, False}                           # the one-launch (A^ x) W and the composed GEMM + SpMM


def test_pdnconv_layer_runs_the_same_sequence(ctx):
    """gcnx.PDNConv on a host matrix with missing loops: output, dx and every gradient against the restatement."""
    from gcnx.layers import PDNConv
    x, a, e, gp, _ = PR.make_batch(PR.SIZES, 16, 2, seed=5, loops="some")
    lay = PDNConv(32, edge_dim=2, hidden_channels=8, seed=1)
    a2, e2, unit = lay.preprocess(a, e)
    rp, ci, e_ref, un = PR.with_unit_self_loops(a.indptr, a.indices, e)
    assert np.array_equal(a2.indices, ci) and np.array_equal(e2, e_ref) and np.array_equal(unit.astype(bool), un)
    out = lay([ctx.to_device(x), _csr(ctx, a2.indptr, a2.indices), ctx.to_device(e2), ctx.to_device(unit)])
    sd = {k: v.numpy() for k, v in lay.params.items()}
    rng = np.random.default_rng(0)
    for k in ("bias", "mlp.0.bias", "mlp.2.bias"):           # biases away from their zero start
        sd[k] = rng.uniform(-0.5, 0.5, sd[k].shape).astype(np.float32)
        lay.params[k].copy_from_host(sd[k])
    out = lay([ctx.to_device(x), _csr(ctx, a2.indptr, a2.indices), ctx.to_device(e2), ctx.to_device(unit)])
    import scipy.sparse as sp
    op = PR.operator(rp, ci, e_ref, sd["mlp.0.weight"].T, sd["mlp.0.bias"], sd["mlp.2.weight"].T, sd["mlp.2.bias"], unit=un,
                     relu_mask=PR.gate_sides(e_ref, sd["mlp.0.weight"].T, sd["mlp.0.bias"]))
    A = sp.csr_matrix((op["v"], ci, rp), shape=(x.shape[0],) * 2)
    hw = x.astype(np.float64) @ sd["lin.weight"]
    assert_close(out.numpy(), A @ hw + sd["bias"], 1e-5, "PDNConv out")
    assert_close(lay.edge_weights(), op["w"], 1e-5, "PDNConv gates")
    dy = rng.normal(size=out.shape).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy))
    t = A.T @ dy.astype(np.float64)
    gg, _, _, _ = PR.operator_bwd(op, sd["mlp.2.weight"].T, np.einsum("ek,ek->e", dy.astype(np.float64)[op["rows"]], hw[ci]))
    want = {"bias": dy.sum(0, dtype=np.float64), "lin.weight": x.astype(np.float64).T @ t, "mlp.0.weight": gg["w1"].T, "mlp.0.bias": gg["b1"],
            "mlp.2.weight": gg["w2"].T, "mlp.2.bias": gg["b2"]}
    assert_close(dx.numpy(), t @ sd["lin.weight"].astype(np.float64).T, 1e-4, "PDNConv dx")
    for k, v in want.items():
        assert_close(lay.grads[k].numpy(), v, 1e-4, f"PDNConv d {k}")


# ---- 5. the device loader and the gates read back --------------------------------------------------------------------------------
def _graphs(seed=3, count=6):
    import scipy.sparse as sp
    from gcnx import Graph, synth
    graphs = []
    for k, (x, a, y) in enumerate(synth.tiny_graphs(count, 16, seed=seed)):
        a = sp.csr_matrix(a.tocsr() + sp.identity(a.shape[0]))               # every loop stored, as the reference's graphs
        a.data[:] = 1.0
        a.sort_indices()
        graphs.append(Graph(x=x, a=a, y=y, e=np.random.default_rng(100 + k).uniform(0, 1, (a.nnz, 2)).astype(np.float32)))
    return graphs


def test_loader_batches_give_the_same_bits_and_the_gates_read_back(ctx):
    import gcnx
    from gcnx import ListDataset
    ds = ListDataset(_graphs())
    dev = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, ds, edge_features=True), batch_size=6, epochs=1, shuffle=False)
    host = gcnx.DisjointLoader(ds, batch_size=6, epochs=1, shuffle=False)
    m = gcnx.PDN(ctx, hidden_channels=64, edge_dim=2, edge_hidden=16, seed=2)
    (inputs, target), (db, none) = next(iter(host)), next(iter(dev))
    assert none is None and len(inputs) == 4
    m.loss_and_grads(inputs, target)
    hbatch = m._last_batch
    la_h, g_h = m.loss_acc.numpy(), m.gradients()
    nnz = db.a.nnz
    assert hbatch.unit is None and hbatch.a.nnz == nnz and np.array_equal(hbatch.a.colidx.numpy()[:nnz], db.a.colidx.numpy()[:nnz])
    assert np.array_equal(bits(hbatch.e.numpy()), bits(db.e.numpy()))
    preset = [v.ptr for v in db.a.transpose_perm()]
    m.loss_and_grads(db)
    assert [v.ptr for v in m._op(db)[1].transpose_perm()] == preset      # the loader's transposed pattern is used
    la_d, g_d = m.loss_acc.numpy(), m.gradients()
    assert np.array_equal(bits(la_d), bits(la_h)) and all(np.array_equal(bits(g_d[k]), bits(g_h[k])) for k in g_h)
    assert all(np.abs(g_h[k]).max() > 0 for k in PR.GATE_KEYS)
    # the gates, before normalisation, in the batch's CSR order
    w1, w2 = m.edge_weights(db)
    p = m.state_dict()
    rp, ci, e = db.a.rowptr.numpy(), db.a.colidx.numpy()[:nnz], db.e.numpy()
    for k, w in ((1, w1), (2, w2)):
        ref = PR.operator(rp, ci, e, p[f"conv{k}.mlp.0.weight"], p[f"conv{k}.mlp.0.bias"], p[f"conv{k}.mlp.2.weight"], p[f"conv{k}.mlp.2.bias"])
        assert w.shape == (nnz,) and w.dtype == np.float32
        assert_close(w, ref["w"], 1e-5, f"edge_weights conv{k}")
        _worst("edge_weights err / tol", _ratio(w, ref["w"], 1e-5))
    from gcnx.explain import edge_layout
    off, edge_index, graph = edge_layout(rp, ci, db.seg.host)
    assert w1[off].shape == (edge_index.shape[1],) == graph.shape
    print("worst:", WORST)


def test_fit_runs_two_epochs_with_adam(ctx):
    import gcnx
    from gcnx import ListDataset
    g = _graphs(seed=4, count=8)
    tr, te = gcnx.DeviceDataset(ctx, ListDataset(g[:5]), edge_features=True), gcnx.DeviceDataset(ctx, ListDataset(g[5:]), edge_features=True)
    m = gcnx.PDN(ctx, hidden_channels=32, edge_dim=2, edge_hidden=8, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=2, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=2, schedule=lambda it: 0.01, verbose=False,
                   optimizer=gcnx.Adam())
    assert len(out["history"]) == 2 and np.all(np.isfinite(out["history"]))
    sd = m.state_dict()
    assert all(np.all(np.isfinite(v)) for v in sd.values()) and sd["conv1.mlp.2.bias"][0] != 0.0     # the gates trained

"""Every route a gcnx.GCN training step can take, against the float64 oracle tests/gcn_bn_ref.py evaluated on the device's
side of every kink: conv1 / conv2 fused or GEMM + SpMM (and with them both branches of GCN._backward), batches with and
without an SpMM plan (tile kernels, hub rows, column blocks), hidden widths off the 64-column grid, directed graphs
(A^ != A^T), empty graphs, streamed batches of changing shape -- and the kernel-level edges of the head and the fused
BN·PReLU·max-pool pair (strided operands, empty graphs, widths that fill no tile, saturated logits).

Every model case asserts the route it claims, so that a later change of a threshold cannot quietly turn it into a
duplicate of another case."""
import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
from test_gpu_gcn_bn import HEAD_KEYS, UNDER_BN, _bn_inputs, _cmp_grads, _device_batch, _device_sides, _scipy_adj, _tiny_host

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FC0DEAD], np.uint32).view(np.float32)[0]     # a NaN with a payload: read by mistake, it propagates


# ---- batches --------------------------------------------------------------------------------------------------------------
def _ecoli(n_graphs, f):
    from gcnx import synth
    return synth.ecoli_batch(n_graphs=n_graphs, f=f)


def _power_law(f):
    from gcnx import synth
    return synth.power_law_batch(n_graphs=3, graph_size=8192, f=f)


def _directed_host(n_graphs, f, seed):
    """Random DIRECTED graphs of 5-30 nodes (every diagonal stored), one disjoint batch."""
    import scipy.sparse as sp
    from gcnx import synth
    rng = np.random.default_rng(seed)
    sizes = rng.integers(5, 31, n_graphs)
    blocks = []
    for s in sizes:
        m = rng.random((s, s)) < 0.2
        np.fill_diagonal(m, True)
        blocks.append(sp.csr_matrix(m.astype(np.float64)))
    a = sp.block_diag(blocks, format="csr")
    a.sort_indices()
    pat = a != 0
    assert (pat != pat.T).nnz > 0
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    x = rng.standard_normal((int(gp[-1]), f)).astype(np.float32)
    y = np.eye(2, dtype=np.float32)[rng.integers(0, 2, n_graphs)]
    return synth.HostBatch(x, a.indptr.astype(np.int32), a.indices.astype(np.int32), None, gp, y)


def _with_empty_graphs(hb, seed):
    """hb with zero-row graphs inserted first, twice in a row in the middle, and last (labels of both kinds)."""
    from gcnx import synth
    sizes = list(np.diff(hb.graph_ptr))
    k = len(sizes) // 2
    sizes = [0] + sizes[:k] + [0, 0] + sizes[k:] + [0]
    rng = np.random.default_rng(seed)
    ey = np.eye(2, dtype=np.float32)[rng.integers(0, 2, 4)]
    y = np.concatenate([ey[:1], hb.y[:k], ey[1:3], hb.y[k:], ey[3:]]).astype(np.float32)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return synth.HostBatch(hb.x, hb.rowptr, hb.colidx, None, gp, y)


# case: (host batch, f_in, hidden, route).  Route keys: plan (SpMM plan on A^ and A^T), c1 / s2 (conv1 / conv2 in the
# one-launch fused form), cb (column-block graphs), hub (rows above the hub threshold), directed, empty, sgd (run the
# three-step trajectory)
CASES = {
    "ref": (lambda: _tiny_host(50, 16, seed=11), 16, 64, dict(plan=False, c1=False, s2=True)),
    "fused_conv1": (lambda: _tiny_host(24, 32, seed=12), 32, 64, dict(plan=False, c1=True, s2=True)),
    "h48": (lambda: _tiny_host(20, 16, seed=13), 16, 48, dict(plan=False, c1=False, s2=False, sgd=True)),
    "h100": (lambda: _tiny_host(20, 16, seed=14), 16, 100, dict(plan=False, c1=False, s2=False, sgd=True)),
    "h256": (lambda: _tiny_host(20, 16, seed=15), 16, 256, dict(plan=False, c1=False, s2=False)),
    "plan_h64": (lambda: _tiny_host(136, 16, seed=16), 16, 64, dict(plan=True, c1=False, s2=False, sgd=True)),
    "plan_h128": (lambda: _ecoli(136, 16), 16, 128, dict(plan=True, c1=False, s2=False)),
    "large_graphs": (lambda: _power_law(16), 16, 128, dict(plan=True, c1=False, s2=False, cb=True, hub=True, b3=True)),
    "directed_h64": (lambda: _directed_host(20, 16, seed=17), 16, 64, dict(plan=False, c1=False, s2=True, directed=True, sgd=True)),
    "directed_h48": (lambda: _directed_host(20, 16, seed=18), 16, 48, dict(plan=False, c1=False, s2=False, directed=True, sgd=True)),
    "directed_plan_h64": (lambda: _directed_host(136, 16, seed=19), 16, 64,
                          dict(plan=True, c1=False, s2=False, directed=True, sgd=True)),
    "directed_plan_h48": (lambda: _directed_host(136, 16, seed=20), 16, 48,
                          dict(plan=True, c1=False, s2=False, directed=True, sgd=True)),
    "empty": (lambda: _with_empty_graphs(_tiny_host(12, 16, seed=21), 1), 16, 64, dict(plan=False, c1=False, s2=True, empty=True)),
    "empty_plan": (lambda: _with_empty_graphs(_tiny_host(132, 16, seed=22), 2), 16, 64,
                   dict(plan=True, c1=False, s2=False, empty=True)),
}


def _gcn(ctx, f, h, p, knob="1", monkeypatch=None):
    import gcnx
    if monkeypatch is not None:
        monkeypatch.setenv("GCNX_BN_POOL", knob)
    m = gcnx.GCN(ctx, hidden_channels=h, seed=0)
    m.build(f)
    m.load_state_dict(p)
    assert m._bn_pool == (knob == "1")
    return m


def _assert_route(ctx, m, batch, hb, h, route):
    from gcnx import device as D
    a_hat, a_t = m._op(batch)
    assert (a_hat.plan is not None) == route["plan"] and (a_t.plan is not None) == route["plan"]
    assert m._bufs["s2_ok"] == route["s2"]
    c1 = a_hat.plan is None and batch.x.contiguous and D.gcn_conv_fused_ok(ctx, batch.n, batch.f, h, batch.x.ld)
    assert c1 == route["c1"]
    assert (a_hat.max_block_rows >= 4096 and h % 64 == 0 and h >= 128) == route.get("cb", False)
    assert (int(np.diff(hb.rowptr).max()) > 256) == route.get("hub", False)            # spmm.hip kHubDeg
    if route.get("directed"):
        assert not a_hat.symmetric and a_t is not a_hat
    else:
        assert a_hat.symmetric and a_t is a_hat
    assert batch.seg.has_empty == route.get("empty", False)


def _assert_hits(got, r, y):
    """Hits equal, except graphs whose reference logit is within 1e-6 max|logit| of 0 (either side is then right)."""
    z = np.asarray(r["out"], np.float64).ravel()
    amb = np.abs(z) <= 1e-6 * np.max(np.abs(z))
    sure = int(np.sum(((z > 0) == (R.targets(y) > 0.5))[~amb]))
    assert sure <= got <= sure + int(amb.sum()), (got, sure, int(amb.sum()))


def _assert_pool(m, hb, r, what):
    """Argmax validity (the argmax row lies inside its graph and is a column maximum of the fp64 activation to 1e-5), the
    pooled values against the oracle's own maxima, and empty graphs pooled to exactly 0."""
    arg, pooled, y2, gp = m._bufs["arg"].numpy(), m._bufs["pooled"].numpy(), r["y2"], hb.graph_ptr
    cols = np.arange(y2.shape[1])
    scale = float(np.max(np.abs(y2)))
    ref = np.zeros(pooled.shape)
    for g in range(len(gp) - 1):
        lo, hi = int(gp[g]), int(gp[g + 1])
        if hi == lo:
            assert np.all(pooled[g].view(np.uint32) == 0), (what, g)
            continue
        a = arg[g].astype(np.int64)
        assert np.all((a >= lo) & (a < hi)), (what, g)
        ref[g] = y2[lo:hi].max(0)
        assert np.all(y2[a, cols] >= ref[g] - 1e-5 * scale), (what, g)
    assert_close(pooled, ref, 1e-4, f"{what} pooled")


def _step_and_check(m, batch, hb, p, tol, what, pooled_slack=False):
    """One loss_and_grads against R.model on the device's kink sides and argmax, and the head's own arithmetic against
    R.head evaluated on the device's pooled rows.  pooled_slack: the end-to-end head gradients may differ from R.model by
    what the fp32 pooled rows alone move the fp64 head (R.head on the device's rows against R.head on the exact ones) on
    top of tol -- see test_gcn_route_against_oracle."""
    m.loss_and_grads(batch)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = R.model(hb.x, _scipy_adj(hb), hb.graph_ptr, p, hb.y, masks=_device_sides(m), argmax=arg)
    assert_close(m._bufs["out"].numpy(), r["out"], tol, f"{what} logits")
    la = m.loss_acc.numpy()
    assert rel_err(la[0], r["loss"]) < tol, (what, la, r["loss"])
    _assert_hits(la[1], r, hb.y)
    grads = m.gradients()
    rh = R.head(m._bufs["pooled"].numpy().astype(np.float64), p, hb.y)
    assert_close(m._bufs["dpooled"].numpy(), rh["dP"], tol, f"{what} dpooled at the device's pooled rows")
    _cmp_grads(grads, rh["grads"], tol, f"{what} head at the device's pooled rows")
    if not pooled_slack:
        _cmp_grads(grads, r["grads"], tol, what)
        return r
    _cmp_grads(grads, r["grads"], tol, what, [k for k in R.KEYS if k not in rh["grads"]])
    for k in rh["grads"]:
        ref = np.asarray(r["grads"][k], np.float64).reshape(grads[k].shape)
        slack = float(np.max(np.abs(rh["grads"][k].reshape(ref.shape) - ref)))
        scale = float(np.max(np.abs(np.asarray(r["grads"][UNDER_BN.get(k, k)], np.float64))))
        err = float(np.max(np.abs(grads[k] - ref)))
        assert err <= tol * scale + slack, (what, k, err, tol * scale, slack)
    return r


@pytest.mark.parametrize("case", list(CASES))
def test_gcn_route_against_oracle(ctx, case, monkeypatch):
    """One step against R.model at 1e-4, the route, argmax validity, GCNX_BN_POOL=0 against =1, the forward-only calls and
    (route "sgd") a three-step SGD trajectory.

    large_graphs has B = 3: BatchNorm3 and BatchNorm4 normalise three rows, the column maxima of three 8192-row graphs,
    which lie close together, so the head amplifies the fp32 rounding of the pooled rows themselves (two GCNConvs with
    4096-entry hub rows and a BatchNorm over 24 576 rows before them): measured 1.05e-4 on linear_1.weight end to end.
    There the head's arithmetic is held to 1e-4 against R.head on the device's own pooled rows (as in every case), and the
    end-to-end head gradients may differ from R.model by 1e-4 plus what the pooled rows' rounding alone moves the fp64
    head."""
    build, f, h, route = CASES[case]
    hb = build()
    assert hb.f == f
    batch = _device_batch(ctx, hb)
    p = {k: v.astype(np.float32) for k, v in R.init_params(f, h, seed=len(case)).items()}
    m = _gcn(ctx, f, h, p, "1", monkeypatch)
    r = _step_and_check(m, batch, hb, p, 1e-4, case, pooled_slack=route.get("b3", False))
    _assert_route(ctx, m, batch, hb, h, route)
    _assert_pool(m, hb, r, case)
    fused = (m._bufs["out"].numpy(), m.loss_acc.numpy(), m._bufs["pooled"].numpy(), m._bufs["arg"].numpy(), m.gradients())

    # GCNX_BN_POOL=0 (bn_act + segment_pool and their backward): the same forward bits, gradients to 1e-5
    m0 = _gcn(ctx, f, h, p, "0", monkeypatch)
    m0.loss_and_grads(batch)
    assert m0._bufs["s2_ok"] == route["s2"]
    for got, ref in zip((m0._bufs["out"].numpy(), m0.loss_acc.numpy(), m0._bufs["pooled"].numpy(), m0._bufs["arg"].numpy()), fused):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), case
    g0 = m0.gradients()
    for k in HEAD_KEYS.values():                         # the head runs on the same bits before either pool backward
        assert np.array_equal(g0[k].view(np.uint32), fused[4][k].view(np.uint32)), (case, k)
    assert_close(m0._bufs["dz2"].numpy(), m._bufs["dz2"].numpy(), 1e-5, f"{case} knob dz2")
    _cmp_grads(g0, fused[4], 1e-5, f"{case} knob", [k for k in R.KEYS if k != "prelu_1.weight"])
    # prelu_1.weight is one sum over N x H terms dy1 * min(zb1, 0) that cancel: its two fp32 evaluations are compared
    # relative to sum |terms| (measured at empty_plan: 6.1e-5 of the value -1.5e-4, both within 1e-4 of the oracle)
    b_ = m._bufs
    zb1 = ((b_["z1"].numpy().astype(np.float64) - b_["m1"].numpy()) * (m.p["g1"].numpy() * b_["i1"].numpy()).astype(np.float64)
           + m.p["be1"].numpy())
    terms = float(np.sum(np.abs(b_["dy1"].numpy() * np.minimum(zb1, 0.0))))
    assert abs(float(g0["prelu_1.weight"][0]) - float(fused[4]["prelu_1.weight"][0])) <= 1e-5 * terms, case
    _cmp_grads(g0, r["grads"], 1e-4, f"{case} knob against the oracle", [k for k in R.KEYS if k not in HEAD_KEYS.values()])

    # forward-only calls: the raw (x, a, i) surface and evaluate_batch
    from gcnx.device import Segments
    a = _scipy_adj(hb)
    ids = Segments(ctx, hb.graph_ptr) if route.get("empty") else hb.ids()     # (ids alone drop a trailing empty graph)
    logits = m((hb.x, a, ids))
    rf = R.model(hb.x, a, hb.graph_ptr, p, masks=_device_sides(m), argmax=m._bufs["arg"].numpy().astype(np.int64))
    assert_close(logits, rf["out"], 1e-4, f"{case} forward")
    if not route.get("empty"):
        coo = a.tocoo()
        assert np.array_equal(m.forward(hb.x, np.stack([coo.col, coo.row]), ids), logits)
    loss, acc, probs = m.evaluate_batch(batch, None)
    assert rel_err(loss, r["loss"]) < 1e-4, (case, loss, r["loss"])
    _assert_hits(round(acc * hb.n_graphs), r, hb.y)
    assert_close(probs, r["probs"], 1e-4, f"{case} evaluate probs")

    if route.get("sgd"):
        # three SGD steps at the reference's learning rate, each oracle step on that step's device kink sides
        ph = {k: v.astype(np.float64) for k, v in p.items()}
        for _ in range(3):
            pre = {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}     # the kink sides of the weights of this step
            m.train_step(batch, lr=0.02)
            b_ = m._bufs
            sides = {"m1": R.device_prelu_sides(b_["z1"].numpy(), b_["m1"].numpy(), b_["i1"].numpy(), pre["g1"], pre["be1"]),
                     "m2": R.device_prelu_sides(b_["z2"].numpy(), b_["m2"].numpy(), b_["i2"].numpy(), pre["g2"], pre["be2"])}
            rs = R.model(hb.x, a, hb.graph_ptr, ph, hb.y, masks=sides, argmax=b_["arg"].numpy().astype(np.int64))
            ph = R.sgd(ph, rs["grads"], 0.02)
        sd = m.state_dict()
        for k in R.KEYS:
            assert_close(sd[k], ph[k].reshape(sd[k].shape), 1e-4, f"{case} after 3 steps {k}")


# ---- streamed batches of changing shape ---------------------------------------------------------------------------------
def test_gcn_streamed_batches_of_changing_shape(ctx):
    """A streamed epoch: a plan batch, a short batch, a batch of the same N and one graph fewer, the first batch again.
    _ensure keys its buffers on (N, B), _op caches per batch.uid and the _Capacity views grow but never shrink: every
    step must give the bits of a fresh model loaded with the same weights."""
    import gcnx
    from gcnx import synth
    big = _tiny_host(136, 16, seed=30)
    small = _tiny_host(9, 16, seed=31)
    gp = np.delete(small.graph_ptr, 4)                      # graphs 3 and 4 as one: same N, B - 1, still block-diagonal
    merged = synth.HostBatch(small.x, small.rowptr, small.colidx, None, gp, np.delete(small.y, 4, axis=0))
    batches = [_device_batch(ctx, hb) for hb in (big, small, merged)]
    order = [0, 1, 2, 0]
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, 64, seed=5).items()}
    m = gcnx.GCN(ctx, hidden_channels=64, seed=0)
    m.load_state_dict(p)
    for step, bi in enumerate(order):
        batch = batches[bi]
        fresh = gcnx.GCN(ctx, hidden_channels=64, seed=1)
        fresh.load_state_dict(m.state_dict())
        fresh.loss_and_grads(batch)
        m.train_step(batch, lr=0.02)
        assert m._bufs["key"] == (batch.n, batch.n_graphs)
        assert (m._op(batch)[0].plan is not None) == (bi == 0)
        assert np.array_equal(m._bufs["out"].numpy().view(np.uint32), fresh._bufs["out"].numpy().view(np.uint32)), step
        assert np.array_equal(m.loss_acc.numpy().view(np.uint32), fresh.loss_acc.numpy().view(np.uint32)), step
        gm, gf = m.gradients(), fresh.gradients()
        for k in R.KEYS:
            assert np.array_equal(gm[k].view(np.uint32), gf[k].view(np.uint32)), (step, k)
    assert batches[1].n == batches[2].n and batches[1].n_graphs == batches[2].n_graphs + 1


# ---- kernel edges: gcnx_bn_prelu_bce_head --------------------------------------------------------------------------------
def _wide(ctx, host, c0, extra):
    """host [r, c] inside a wider device buffer [r, c + extra] filled with SENTINEL: (buffer, column view, host image)."""
    r, c = host.shape
    img = np.full((r, c + extra), SENTINEL, np.float32)
    img[:, c0:c0 + c] = host
    buf = ctx.to_device(img)
    return buf, buf.cols(c0, c0 + c), img


def _outside(img, c0, c):
    return np.concatenate([img[:, :c0], img[:, c0 + c:]], axis=1).view(np.uint32)


def _head_views(ctx, P, p, y):
    """The head with pooled and dpooled as column views of wider, sentinel-filled buffers (ld > H)."""
    from gcnx import device as D
    B, H = P.shape
    dp = {k: ctx.to_device(np.asarray(p[t], np.float32)) for k, t in HEAD_KEYS.items()}
    dg = {k: ctx.zeros(v.shape) for k, v in dp.items()}
    pbuf, pview, pimg = _wide(ctx, P, 1, 3)
    dbuf, dview, dimg = _wide(ctx, np.zeros((B, H), np.float32), 2, 5)
    assert pview.ld == H + 3 and dview.ld == H + 5
    out, probs, la = ctx.empty((B, 1)), ctx.empty((B, 1)), ctx.zeros(2)
    scratch = ctx.empty(D.bce_head_scratch_floats(ctx, B, H))
    args = D.bce_head_args(pview, dp, scratch, out, probs, y=ctx.to_device(np.asarray(y, np.float32)), loss_acc=la, denom=B,
                           g=dg, dpooled=dview)
    D.bn_prelu_bce_head(ctx, args)
    assert np.array_equal(pbuf.numpy().view(np.uint32), pimg.view(np.uint32))           # the input buffer is untouched
    assert np.array_equal(_outside(dbuf.numpy(), 2, H), _outside(dimg, 2, H))            # nothing written outside the view
    return out.numpy(), probs.numpy(), la.numpy(), dview.numpy(), {HEAD_KEYS[k]: v.numpy() for k, v in dg.items()}


def _check_head(got, r, y, what):
    out, probs, la, dP, g = got
    assert_close(out, r["out"], 1e-4, f"{what} out")
    assert_close(probs, r["probs"], 1e-4, f"{what} probs")
    assert rel_err(la[0], r["loss"]) < 1e-4, (what, la[0], r["loss"])
    _assert_hits(la[1], r, y)
    assert_close(dP, r["dP"], 1e-4, f"{what} dP")
    if dP.shape[1] > 1:
        _cmp_grads(g, r["grads"], 1e-4, what)
        return
    # H = 1: each Linear feeds a one-column BatchNorm, so its input lies in span{1, xhat} of that BatchNorm and the weight
    # gradient is analytically zero up to the eps term (the BN backward output is orthogonal to both); the two weights and
    # biases are compared relative to the same BatchNorm's weight gradient, as UNDER_BN does
    for lin, bn in (("linear_1", "batch_norm_3"), ("linear_2", "batch_norm_4")):
        scale = float(np.max(np.abs(r["grads"][f"{bn}.weight"])))
        for k in (f"{lin}.weight", f"{lin}.bias"):
            err = float(np.max(np.abs(g[k] - np.asarray(r["grads"][k]).reshape(g[k].shape))))
            assert err <= 1e-4 * scale, (what, k, err, scale)
    _cmp_grads(g, r["grads"], 1e-4, what, [k for k in r["grads"] if not k.startswith("linear_")])


@pytest.mark.parametrize("B", [257, 4096])
@pytest.mark.parametrize("H", [1, 5, 48, 100, 200, 255])
def test_bce_head_widths_and_column_views(ctx, B, H):
    rng = np.random.default_rng(B * 7 + H)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=B + H).items()}
    P = rng.normal(size=(B, H)).astype(np.float32)
    y = np.eye(2)[rng.integers(0, 2, B)]
    got = _head_views(ctx, P, p, y)
    _check_head(got, R.head(P.astype(np.float64), p, y), y, f"head B={B} H={H}")


def test_bce_head_saturated_logits(ctx):
    """|out| of about 100 (BN4's gamma and beta large): sigmoid saturates to 0 / 1 in fp32, the loss of a wrong graph is
    |out| itself.  Loss and gradients stay finite and match the oracle."""
    B, H = 64, 32
    rng = np.random.default_rng(3)
    p = {k: v.astype(np.float32) for k, v in R.init_params(16, H, seed=4).items()}
    p["batch_norm_4.weight"] = np.array([70.0], np.float32)
    p["batch_norm_4.bias"] = np.array([30.0], np.float32)
    p["prelu_4.weight"] = np.array([0.9], np.float32)
    P = rng.normal(size=(B, H)).astype(np.float32)
    y = np.eye(2)[rng.integers(0, 2, B)]
    r = R.head(P.astype(np.float64), p, y)
    assert np.max(np.abs(r["out"])) > 90
    got = _head_views(ctx, P, p, y)
    assert all(np.all(np.isfinite(v)) for v in got[:4]) and all(np.all(np.isfinite(v)) for v in got[4].values())
    _check_head(got, r, y, "head saturated")


# ---- kernel edges: gcnx_bn_act_pool(_bwd) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 3, 48, 100, 200])
def test_bn_act_pool_views_and_empty_graphs(ctx, f):
    """z as a column view whose base is not 16-byte aligned (start column 1), pooled / dpooled / dz as views too; graphs
    of 0 rows first, in the middle (two in a row) and last, and of 1 row.  Forward bit-identical to gcnx_bn_act +
    gcnx_segment_pool(max), backward against their backward and the oracle; nothing written outside the views."""
    from gcnx import device as D
    from gcnx.device import Segments
    sizes = [0, 1, 37, 0, 0, 300, 1, 64, 1, 0]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, B = int(gp[-1]), len(sizes)
    z, gamma, beta, alpha, dz, mean, inv = _bn_inputs(ctx, n, f, seed=f + 100)
    z[gp[5] + 7:gp[5] + 12] = z[gp[5] + 3]                 # exact ties inside one graph: the first row must win
    dz.copy_from_host(z)
    D.bn_moments(ctx, dz, None, mean, inv, eps=D.TORCH_BN_EPS)
    seg = Segments(ctx, gp)
    g, b, a = ctx.to_device(gamma), ctx.to_device(beta), ctx.to_device(alpha)
    zbuf, zv, zimg = _wide(ctx, z, 1, 3)
    assert zv.ptr % 16 != 0 and zv.ld == f + 3
    pbuf, pv, pimg = _wide(ctx, np.zeros((B, f), np.float32), 1, 2)
    arg = ctx.empty((B, f), np.int32)
    D.bn_act_pool(ctx, seg, zv, mean, inv, g, b, pv, arg, alpha=a)
    y, pooled2, arg2 = ctx.empty((n, f)), ctx.empty((B, f)), ctx.empty((B, f), np.int32)
    D.bn_act(ctx, dz, mean, inv, g, b, y, act="prelu_shared", alpha=a)
    D.segment_pool(ctx, seg, y, pooled2, "max", arg2)
    pooled = pv.numpy()
    assert np.array_equal(pooled.view(np.uint32), pooled2.numpy().view(np.uint32))
    assert np.array_equal(arg.numpy(), arg2.numpy())
    empty = np.diff(gp) == 0
    assert np.all(pooled[empty].view(np.uint32) == 0)
    assert np.all(arg.numpy()[empty] == gp[:-1][empty, None])
    assert np.array_equal(_outside(pbuf.numpy(), 1, f), _outside(pimg, 1, f))
    # the oracle's pooled maxima
    pos = R.device_prelu_sides(z, mean.numpy(), inv.numpy(), gamma, beta)
    zb, _ = R.bn_fwd(z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    y64, _ = R.prelu_fwd(zb, float(alpha[0]), pos)
    ref = np.stack([y64[gp[i]:gp[i + 1]].max(0) if not empty[i] else np.zeros(f) for i in range(B)])
    assert_close(pooled, ref, 1e-5, f"bn_act_pool f={f}")

    # backward through views
    dp = np.random.default_rng(f).normal(size=(B, f)).astype(np.float32)
    dpbuf, dpv, dpimg = _wide(ctx, dp, 2, 4)
    dzbuf, dzv, dzimg = _wide(ctx, np.zeros((n, f), np.float32), 1, 3)
    out = {k: ctx.zeros(s) for k, s in (("dg", f), ("db", f), ("da", 1))}
    D.bn_act_pool_bwd(ctx, seg, dpv, arg, zv, mean, inv, g, b, dzv, alpha=a, dgamma=out["dg"], dbeta=out["db"], dalpha=out["da"])
    assert np.array_equal(dpbuf.numpy().view(np.uint32), dpimg.view(np.uint32))
    assert np.array_equal(zbuf.numpy().view(np.uint32), zimg.view(np.uint32))
    assert np.array_equal(_outside(dzbuf.numpy(), 1, f), _outside(dzimg, 1, f))
    got = {"dz": dzv.numpy(), "dg": out["dg"].numpy(), "db": out["db"].numpy(), "da": out["da"].numpy()}
    dy = ctx.empty((n, f))
    D.segment_pool_bwd(ctx, seg, ctx.to_device(dp), dy, "max", arg2)
    ref = {k: ctx.zeros(s) for k, s in (("dz", (n, f)), ("dg", f), ("db", f), ("da", 1))}
    D.bn_act_bwd(ctx, dy, dz, mean, inv, g, b, ref["dz"], ctx.empty(3 * f), act="prelu_shared", alpha=a, dgamma=ref["dg"],
                 dbeta=ref["db"], dalpha=ref["da"])
    orc = R.bn_act_pool_bwd(dp.astype(np.float64), arg.numpy(), z, gamma.astype(np.float64), beta.astype(np.float64), alpha, gp, pos)
    for k, o in zip(("dz", "dg", "db", "da"), orc):
        assert_close(got[k], ref[k].numpy(), 1e-5, f"bn_act_pool_bwd {k} vs unfused f={f}")
        assert_close(got[k], o, 1e-4, f"bn_act_pool_bwd {k} vs oracle f={f}")

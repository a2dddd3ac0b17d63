"""GPU tests of TransformerConv: the kernels of csrc/transformer.hip (gcnx_transformer_aggregate, gcnx_transformer_beta_bwd,
gcnx_transformer_bwd_targets, gcnx_transformer_bwd_sources), the layer gcnx.TransformerConv and the model gcnx.Transformer -- each
against the float64 oracle tests/transformer_ref.py.  Softmax, dot and sigmoid have no kink: only the model's PReLU / pool sides
are taken from the device.  Bound: test_gpu_gat.TIGHT = 2e-5 (max-norm relative against float64) for every kernel output, the
layer, a whole step of the model; the two loader routes agree bit for bit."""
import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import transformer_ref as TR
from gpu_frames import SENTINEL, Frame
from test_gpu_gat import TIGHT, UNDER_BN, _bits, _csr, _ecoli3, _edge_case_csr, _frame_check
from test_gpu_gatv2 import _one_long_row
from test_gpu_gcn_bn import _tiny_host

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16), (1, 64), (4, 16), (8, 16), (2, 32), (1, 128), (4, 32)]
EDGE_DIMS = [0, 1, 2, 8]


def _operands(n, nnz, heads, c, d, seed, x=None, q_scale=1.0, k_shift=None):
    """P = Q | K | V | S (unit scale: scores ~ N(0, 1), the softmax neither flat nor saturated; x: given Q block), e in (0, 1) as
    dca / proximity are, W_e ~ N(0, 1) / 2, w_beta ~ N(0, 1) / sqrt(HC), dout.  k_shift: K is first rounded to multiples of 2^-16,
    so that K + k_shift is exact in float32 and the shifted and the unshifted operands describe the same attention."""
    rng = np.random.default_rng(seed)
    hc = heads * c
    p = rng.standard_normal((n, 4 * hc)).astype(np.float32)
    if x is not None:
        p[:, :hc] = x
    p[:, :hc] *= np.float32(q_scale)
    if k_shift is not None:
        p[:, hc:2 * hc] = np.round(p[:, hc:2 * hc] * 65536.0) / 65536.0 + np.float32(k_shift)
    e = rng.uniform(0, 1, (nnz, d)).astype(np.float32) if d else None
    w_e = (rng.standard_normal((d, hc)) / 2).astype(np.float32) if d else None
    w_beta = (rng.standard_normal(3 * hc) / np.sqrt(hc)).astype(np.float32)
    dout = rng.standard_normal((n, hc)).astype(np.float32)
    return dict(p=p, e=e, w_e=w_e, w_beta=w_beta, dout=dout)


class _Dev:
    """The device side of one layer evaluation: operands uploaded once (or given as device views), every kernel callable."""

    def __init__(self, ctx, a, ops, heads):
        up = lambda t: t if t is None or hasattr(t, "ptr") else ctx.to_device(t)
        self.ctx, self.a, self.heads = ctx, a, heads
        self.p, self.e, self.w_e, self.w_beta, self.dout = (up(ops[k]) for k in ("p", "e", "w_e", "w_beta", "dout"))
        self.n, self.hc = self.p.shape[0], self.dout.shape[1]
        self.c = self.hc // heads
        self.d = 0 if self.e is None else self.e.shape[1]
        self.skip = self.p.cols(3 * self.hc, 4 * self.hc)

    def aggregate(self, alpha=True, o_pre=True, root=True, beta=False, out=None, o=None):
        from gcnx import device as D
        ctx = self.ctx
        self.out = out if out is not None else ctx.empty((self.n, self.hc))
        self.alpha = ctx.zeros((self.a.nnz, self.heads)) if alpha else None
        self.o = (o if o is not None else ctx.empty((self.n, self.hc))) if o_pre else None
        D.transformer_aggregate(ctx, self.a, self.p, self.out, self.heads, e=self.e, w_e=self.w_e, skip=self.skip if root else None,
                                w_beta=self.w_beta if beta else None, alpha=self.alpha, o_pre=self.o)
        return self.out.numpy(), (self.alpha.numpy() if alpha else None), (self.o.numpy() if o_pre else None)

    def _scratch(self, beta):
        from gcnx import device as D
        return self.ctx.empty(max(D.transformer_bwd_scratch_floats(self.ctx, self.n, self.heads, self.c, self.d, beta), 1))

    def beta_bwd(self, d_o=None, d_s=None):
        from gcnx import device as D
        ctx = self.ctx
        self.d_o = d_o if d_o is not None else ctx.empty((self.n, self.hc))
        self.d_s = d_s if d_s is not None else ctx.empty((self.n, self.hc))
        self.dwb = ctx.empty(3 * self.hc)
        D.transformer_beta_bwd(ctx, self.dout, self.o, self.skip, self.w_beta, self.d_o, self.d_s, self.dwb, self._scratch(True))
        return self.d_o.numpy(), self.d_s.numpy(), self.dwb.numpy()

    def bwd_targets(self, d_o=None, dq=None, ds=None):
        from gcnx import device as D
        ctx = self.ctx
        self.d_o_used = d_o if d_o is not None else self.dout
        self.dscore = ctx.zeros((self.a.nnz, self.heads))
        self.dq = dq if dq is not None else ctx.empty((self.n, self.hc))
        self.dwe = ctx.empty((self.d, self.hc)) if self.d else None
        D.transformer_bwd_targets(ctx, self.a, self.p, self.alpha, self.d_o_used, self.o, self.dscore, self.dq, self.heads, self._scratch(False),
                                  ds=ds, e=self.e, w_e=self.w_e, dw_e=self.dwe)
        return self.dscore.numpy(), self.dq.numpy(), (self.dwe.numpy() if self.d else None)

    def bwd_sources(self, dkv=None):
        from gcnx import device as D
        self.dkv = dkv if dkv is not None else self.ctx.empty((self.n, 2 * self.hc))
        D.transformer_bwd_sources(self.ctx, self.a, self.p, self.alpha, self.dscore, self.d_o_used, self.dkv, self.heads)
        return self.dkv.numpy()


def _oracle(rowptr, colidx, ops, heads, root=True, beta=False):
    hc = ops["dout"].shape[1]
    p = np.asarray(ops["p"], np.float64)
    out, cache = TR.conv_fwd(rowptr, colidx, p, heads, hc // heads, ops["e"], ops["w_e"], p[:, 3 * hc:4 * hc] if root else None,
                             ops["w_beta"] if beta else None)
    cache["grads"] = TR.conv_bwd(cache, ops["dout"])
    return out, cache


WORST = {}


def _check_all(ctx, a, rowptr, colidx, ops, heads, what, root=True, beta=False, tol=TIGHT, cancelling=False):
    """Every kernel on one input against the oracle; returns the device object with the host copies (errors printed first).
    cancelling: dQ[i] = s sum_j dscore_ij k_ij is measured against the largest sum of the MAGNITUDES of its terms instead of the
    largest result -- for inputs on which every key carries one large common vector, whose part of dQ is analytically ZERO (a
    softmax's score gradients sum to zero over its row).  The rounding error of an fp32 sum is bounded by eps times the sum of
    its terms' magnitudes, whatever cancels; relative to a result that has lost its leading part no bound can hold."""
    d = _Dev(ctx, a, ops, heads)
    out, alpha, o = d.aggregate(root=root, beta=beta)
    r_out, k = _oracle(rowptr, colidx, ops, heads, root, beta)
    g = k["grads"]
    errs = {"out": rel_err(out, r_out), "alpha": rel_err(alpha, k["alpha"]), "o_pre": rel_err(o, k["O"])}
    host = dict(out=out, alpha=alpha, o=o)
    d_o = None
    if beta:
        dO, dS, dwb = d.beta_bwd()
        errs.update(dO=rel_err(dO, g["dO"]), dS=rel_err(dS, g["dS"]), dw_beta=rel_err(dwb, g["dw_beta"]))
        host.update(dO=dO, dS=dS, dwb=dwb)
        d_o = d.d_o
    ds = ctx.empty((d.n, d.hc)) if root and not beta else None
    dscore, dq, dwe = d.bwd_targets(d_o=d_o, ds=ds)
    dkv = d.bwd_sources()
    if ds is not None:
        assert np.array_equal(_bits(ds.numpy()), _bits(ops["dout"])), "dS is the copy of dO"
    errs.update(dscore=rel_err(dscore, g["dscore"]), dQ=rel_err(dq, g["dQ"]), dKV=rel_err(dkv, np.hstack([g["dK"], g["dV"]])))
    if d.d:
        errs["dw_e"] = rel_err(dwe, g["dWe"])
    if cancelling:
        n, hc = d.n, d.hc
        row = np.repeat(np.arange(n), np.diff(np.asarray(rowptr, np.int64)))
        terms = np.zeros((n, hc))
        np.add.at(terms, row, k["s"] * np.abs(np.repeat(g["dscore"], d.c, axis=1) * k["kk"]))
        errs["dQ"] = float(np.max(np.abs(dq - g["dQ"]))) / float(terms.max())
    print(f"transformer {what} heads={heads} c={d.c} edge_dim={d.d} root={root} beta={beta}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    for key, v in errs.items():
        WORST[key] = max(WORST.get(key, 0.0), v)
    print("transformer worst so far: " + " ".join(f"{key} {v:.2e}" for key, v in WORST.items()))
    assert all(np.isfinite(t).all() for t in (out, alpha, o, dscore, dq, dkv))
    for key, v in errs.items():
        assert v < tol, (what, key, v)
    host.update(dscore=dscore, dq=dq, dwe=dwe, dkv=dkv, ref=k, r_out=r_out)
    d.host = host
    return d


# ---- 1. the kernels against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("heads,c", SHAPES)
def test_transformer_kernels_against_float64(ctx, heads, c, edge_dim):
    from gcnx import device as D
    hb = _ecoli3(heads * c)
    a = _csr(ctx, hb)
    assert D.transformer_conv_ok(ctx, hb.n, heads, c, ldp=4 * heads * c, edge_dim=edge_dim) and hb.n % 32 != 0
    ops = _operands(hb.n, hb.nnz, heads, c, edge_dim, 1000 * edge_dim + 100 * heads + c, x=hb.x)
    d = _check_all(ctx, a, hb.rowptr, hb.colidx, ops, heads, "ecoli-3")
    h = d.host
    sums = np.add.reduceat(h["alpha"].astype(np.float64), hb.rowptr[:-1].astype(np.int64))
    assert np.diff(hb.rowptr).min() > 0 and np.max(np.abs(sums - 1.0)) < 1e-6, np.max(np.abs(sums - 1.0))
    # no atomics: a second call of each leaves the same bits
    second = d.aggregate() + d.bwd_targets() + (d.bwd_sources(),)
    first = tuple(h[k] for k in ("out", "alpha", "o", "dscore", "dq", "dwe", "dkv"))
    for k, (x, y) in enumerate(zip(first, second)):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), k
    # alpha = NULL and o_pre = NULL give the same out bits; skip = NULL gives out == o_pre bit for bit
    out3, alpha3, o3 = d.aggregate(alpha=False, o_pre=False)
    assert alpha3 is None and o3 is None and np.array_equal(_bits(out3), _bits(h["out"]))
    out4, _, o4 = d.aggregate(root=False)
    assert np.array_equal(_bits(out4), _bits(o4)) and np.array_equal(_bits(o4), _bits(h["o"]))
    # the beta gate and its backward on the same operands
    db = _check_all(ctx, a, hb.rowptr, hb.colidx, ops, heads, "ecoli-3", beta=True)
    assert np.array_equal(_bits(db.host["alpha"]), _bits(h["alpha"])) and np.array_equal(_bits(db.host["o"]), _bits(h["o"]))
    again = db.beta_bwd()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(again, (db.host["dO"], db.host["dS"], db.host["dwb"])))


# ---- 2. the smallest shapes that can still go wrong -----------------------------------------------------------------------------
@pytest.mark.parametrize("heads,c,edge_dim", [(4, 8, 2), (1, 16, 0), (1, 128, 2)])
def test_transformer_kernels_degenerate_inputs(ctx, heads, c, edge_dim):
    """Rows without entries, a directed pattern (the transposed pattern differs), fewer rows than a tile, a row with only its
    loop, a row whose only entry is in no row.  (1, 128): the 16-row workgroups."""
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _edge_case_csr()
    n, hc = 56, heads * c
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp, symmetric=False)
    assert not a.symmetric and not np.diff(rowptr)[[4, 20]].any()
    ops = _operands(n, len(colidx), heads, c, edge_dim, 7 + heads)
    h = _check_all(ctx, a, rowptr, colidx, ops, heads, "56 rows").host
    assert not h["o"][[4, 20]].any() and not h["dq"][[4, 20]].any()                           # no entries: O = 0 exactly
    assert np.array_equal(_bits(h["out"][[4, 20]]), _bits(ops["p"][[4, 20], 3 * hc:]))       # ... and out = S, bit for bit
    hb_ = _check_all(ctx, a, rowptr, colidx, ops, heads, "56 rows", beta=True).host         # with beta: the oracle at TIGHT
    assert not hb_["o"][[4, 20]].any()
    hn = _check_all(ctx, a, rowptr, colidx, ops, heads, "56 rows", root=False).host
    assert not hn["out"][[4, 20]].any()
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    nnz5 = int(rowptr[5])
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:nnz5], None, gp[:4].copy(), symmetric=False)
    ops5 = _operands(5, nnz5, heads, c, edge_dim, 32)
    _check_all(ctx, a5, rowptr[:6], colidx[:nnz5], ops5, heads, "5 rows")
    _check_all(ctx, a5, rowptr[:6], colidx[:nnz5], ops5, heads, "5 rows", beta=True)
    # one row with only its self-loop: alpha == 1 exactly, O == V[0] + T.  T is a chain of edge_dim FMAs and O one more add: at
    # most 3 roundings of half a unit each on magnitudes below M = |V| + sum_d |e_d W_e[d]|, so |O - (V + T)| <= 3 * 2^-24 * M;
    # without edge features O is V[0], bit for bit.
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), None, one, symmetric=True)
    ops1 = _operands(1, 1, heads, c, edge_dim, 33)
    d1 = _check_all(ctx, a1, one, np.zeros(1, np.int32), ops1, heads, "1 row, self-loop")
    assert np.array_equal(d1.host["alpha"], np.ones((1, heads), np.float32))
    v = ops1["p"][:, 2 * hc:3 * hc].astype(np.float64)
    if edge_dim:
        t = ops1["e"].astype(np.float64) @ ops1["w_e"].astype(np.float64)
        m = np.abs(v) + np.abs(ops1["e"].astype(np.float64)) @ np.abs(ops1["w_e"].astype(np.float64))
        assert np.all(np.abs(d1.host["o"] - (v + t)) <= 3 * 2.0 ** -24 * m)
    else:
        assert np.array_equal(_bits(d1.host["o"]), _bits(ops1["p"][:, 2 * hc:3 * hc]))
    # one row without any entry (the stored entry is in no row)
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), None, one, symmetric=True)
    d0 = _Dev(ctx, a0, ops1, heads)
    out0, _, o0 = d0.aggregate()
    assert np.array_equal(_bits(out0), _bits(ops1["p"][:, 3 * hc:])) and not o0.any()
    _, dq0, dwe0 = d0.bwd_targets()                                      # (no transposed pattern of a CSR whose entry is in no row)
    assert not dq0.any() and (dwe0 is None or not dwe0.any())


# ---- 3. a row beyond the staged entries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,edge_dim", [(1, 2), (4, 0)])
def test_transformer_kernels_one_row_beyond_the_staged_entries(ctx, heads, edge_dim):
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _one_long_row()
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp)
    assert a.symmetric
    _check_all(ctx, a, rowptr, colidx, _operands(1300, len(colidx), heads, 64 // heads, edge_dim, 11 + heads), heads, "long row")


# ---- 4. n = 0 -------------------------------------------------------------------------------------------------------------------
def test_transformer_no_rows(ctx):
    """n = 0 succeeds and writes nothing."""
    from gcnx import _lib
    lib = ctx.lib
    out, kv, al, wb, big = Frame(ctx, 4, 16, 16, 0), Frame(ctx, 4, 32, 32, 0), Frame(ctx, 16, 1, 1, 0), Frame(ctx, 1, 48, 48, 0), ctx.zeros(64)
    x, w = ctx.zeros((4, 64)), ctx.zeros(48)
    rp = ctx.to_device(np.zeros(1, np.int32))
    rcs = (lib.gcnx_transformer_aggregate(ctx.h, rp.ptr, rp.ptr, x.ptr, 64, 0, 1, 16, None, 0, 0, None, x.ptr + 192, 64, w.ptr, out.view.ptr,
                                          16, al.view.ptr, None, 0),
           lib.gcnx_transformer_beta_bwd(ctx.h, x.ptr, 64, x.ptr, 64, x.ptr, 64, w.ptr, 0, 16, out.view.ptr, 16, kv.view.ptr, 32, wb.view.ptr,
                                         big.ptr),
           lib.gcnx_transformer_bwd_targets(ctx.h, rp.ptr, rp.ptr, x.ptr, 64, 0, 1, 16, None, 0, 0, None, al.view.ptr, x.ptr, 64, x.ptr, 64,
                                            al.view.ptr, out.view.ptr, 16, kv.view.ptr, 32, None, big.ptr),
           lib.gcnx_transformer_bwd_sources(ctx.h, rp.ptr, rp.ptr, rp.ptr, x.ptr, 64, 0, 1, 16, al.view.ptr, al.view.ptr, x.ptr, 64,
                                            kv.view.ptr, 32))
    assert rcs == (_lib.OK,) * 4
    for fr in (out, kv, al, wb):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "n = 0 writes nothing")
    assert not big.numpy().any()


# ---- 5. strided operands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [False, True])
def test_transformer_strided_operands(ctx, beta):
    """ldp > 4 HC, a strided e, strided out / o_pre / d_out, and dQ | dK | dV | dS written as columns of ONE wider array."""
    from gcnx import device as D
    heads, c, ed = 4, 8, 2
    hc = heads * c
    hb = _ecoli3(hc)
    a = _csr(ctx, hb)
    ops = _operands(hb.n, hb.nnz, heads, c, ed, 51, x=hb.x)
    fp = Frame(ctx, hb.n, 4 * hc, 4 * hc + 8, 4, data=ops["p"])
    fe = Frame(ctx, hb.nnz, ed, ed + 3, 1, data=ops["e"])               # (e is read with scalar loads: no alignment rule)
    f_out, f_o = Frame(ctx, hb.n, hc, hc + 8, 8), Frame(ctx, hb.n, hc, hc + 4, 12)
    f_do = Frame(ctx, hb.n, hc, hc + 4, 4, data=ops["dout"])
    f_dp = Frame(ctx, hb.n, 4 * hc, 4 * hc + 4, 4)
    f_go = Frame(ctx, hb.n, hc, hc + 12, 4)
    assert all(f.aligned() for f in (fp, f_out, f_o, f_do, f_dp, f_go)) and D.transformer_conv_ok(ctx, hb.n, heads, c, fp.view.ld, ed)
    d = _Dev(ctx, a, dict(ops, p=fp.view, e=fe.view, dout=f_do.view), heads)
    d.aggregate(out=f_out.view, o=f_o.view, beta=beta)
    r_out, k = _oracle(hb.rowptr, hb.colidx, ops, heads, True, beta)
    g = k["grads"]
    dS = f_dp.view.cols(3 * hc, 4 * hc)
    if beta:
        d.beta_bwd(d_o=f_go.view, d_s=dS)
        d.bwd_targets(d_o=f_go.view, dq=f_dp.view.cols(0, hc))
        assert rel_err(d.dwb.numpy(), g["dw_beta"]) < TIGHT
        _frame_check(f_go, g["dO"], TIGHT, "dO")
    else:
        d.bwd_targets(dq=f_dp.view.cols(0, hc), ds=dS)
        f_go.check(np.full((hb.n, hc), SENTINEL), "unused")
    d.bwd_sources(dkv=f_dp.view.cols(hc, 3 * hc))
    assert rel_err(d.alpha.numpy(), k["alpha"]) < TIGHT and rel_err(d.dscore.numpy(), g["dscore"]) < TIGHT
    assert rel_err(d.dwe.numpy(), g["dWe"]) < TIGHT
    _frame_check(f_out, r_out, TIGHT, "out")
    _frame_check(f_o, k["O"], TIGHT, "o_pre")
    _frame_check(f_dp, np.hstack([g["dQ"], g["dK"], g["dV"], g["dS"]]), TIGHT, "dQ | dK | dV | dS")
    fp.check(ops["p"], "p is not written")
    fe.check(ops["e"], "e is not written")
    f_do.check(ops["dout"], "d_out is not written")


# ---- 6. the range of the exponential ----------------------------------------------------------------------------------------
Q_SCALE = 16.0       # float64 oracle on the E. coli-shaped batch, heads 4, c 16, edge_dim 2: median row maximum of alpha 0.935 at 8,
                     # 0.985 at 12, 0.9967 at 16, 0.9998 at 24
K_SHIFT = 28.0       # ... largest |score| 79 at a shift of 20 (exp finite in fp32), 117 at 30; 28 gives about 110


def test_transformer_scaled_queries_give_near_one_hot_rows(ctx):
    hb = _ecoli3(64)
    ops = _operands(hb.n, hb.nnz, 4, 16, 2, 41, q_scale=Q_SCALE)
    _, k = _oracle(hb.rowptr, hb.colidx, ops, 4)
    top = np.maximum.reduceat(k["alpha"], hb.rowptr[:-1].astype(np.int64))
    assert np.median(top) > 0.99, np.median(top)                          # near one-hot (asserted on the oracle)
    _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, 4, f"Q x {Q_SCALE:.0f}")
    _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, 4, f"Q x {Q_SCALE:.0f}", beta=True)


@pytest.mark.parametrize("shift", [K_SHIFT, -K_SHIFT])
def test_transformer_shifted_keys_stay_finite(ctx, shift):
    """K shifted by +-28 in every channel: the scores of row i move by s <Q[i], shift>, by hundreds over the batch.  The running
    maximum is subtracted before each exponential, so nothing overflows (asserted below for fp32: what a kernel without the
    subtraction would sum) and no row divides 0 by 0; a common shift of a row's scores changes no alpha, so out still matches
    the oracle of the UNSHIFTED operands.  dQ = s sum_j dscore_ij (K[j] + shift + T_ij) is a cancelling sum (_check_all)."""
    hb = _ecoli3(64)
    ops = _operands(hb.n, hb.nnz, 4, 16, 2, 43, k_shift=shift)
    base = _operands(hb.n, hb.nnz, 4, 16, 2, 43, k_shift=0.0)
    assert np.array_equal(ops["p"][:, 64:128] - np.float32(shift), base["p"][:, 64:128])     # the shift is exact in float32
    for beta in (False, True):
        d = _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, 4, f"K {shift:+.0f}", beta=beta, cancelling=True)
        top = np.abs(d.host["ref"]["score"]).max()
        assert top > 100.0, top
        with np.errstate(over="ignore"):
            assert np.exp(np.float32(top)) == np.inf
        r0, _ = _oracle(hb.rowptr, hb.colidx, base, 4, True, beta)
        err = rel_err(d.host["out"], r0)
        print(f"transformer K {shift:+.0f} beta={beta}: out against the unshifted oracle {err:.2e}")
        assert err < TIGHT, err


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_transformer_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb = _ecoli3(16)
    a = _csr(ctx, hb)
    n, nnz = hb.n, a.nnz

    def refused(p, heads, c, ed=0, bad=None):
        """Every call with the operand ``p`` (and, bad = (name, frame view): that operand replaced) is refused, nothing written."""
        hc = heads * c
        w_e, e = (ctx.zeros((ed, hc)) if ed else None), (ctx.zeros((nnz, ed)) if ed else None)
        out, o, dq, d_o, d_s = (Frame(ctx, n, hc, hc, 0) for _ in range(5))
        dkv = Frame(ctx, n, 2 * hc, 2 * hc, 0)
        alpha, ds = Frame(ctx, nnz, heads, heads, 0), Frame(ctx, nnz, heads, heads, 0)
        dwb, dwe = Frame(ctx, 1, 3 * hc, 3 * hc, 0), (Frame(ctx, ed, hc, hc, 0) if ed else None)
        dense, wb = ctx.zeros((n, hc)), ctx.zeros(3 * hc)
        scratch = ctx.zeros(16 * n * max(ed, 3))
        v = dict(out=out.view, o=o.view, dq=dq.view, dkv=dkv.view, dout=dense, d_o=d_o.view, d_s=d_s.view)
        calls = ["agg", "beta", "tgt", "src"]
        if bad is not None:
            v[bad[0]] = bad[1]
            calls = {"out": ["agg"], "o": ["agg", "beta", "tgt"], "dq": ["tgt"], "dkv": ["src"], "dout": ["beta", "tgt", "src"],
                     "d_o": ["beta"], "d_s": ["beta"]}[bad[0]]
        skip = p.cols(3 * hc, 4 * hc) if p.shape[1] >= 4 * hc else dense
        fns = dict(agg=lambda: D.transformer_aggregate(ctx, a, p, v["out"], heads, e=e, w_e=w_e, skip=skip, w_beta=wb, alpha=alpha.view,
                                                       o_pre=v["o"]),
                   beta=lambda: D.transformer_beta_bwd(ctx, v["dout"], v["o"], dense, wb, v["d_o"], v["d_s"],
                                                       DeviceArray(ctx, dwb.view.ptr, (3 * hc,), np.float32, base=dwb.buf), scratch),
                   tgt=lambda: D.transformer_bwd_targets(ctx, a, p, alpha.view, v["dout"], v["o"], ds.view, v["dq"], heads, scratch, e=e, w_e=w_e,
                                                         dw_e=dwe.view if ed else None),
                   src=lambda: D.transformer_bwd_sources(ctx, a, p, alpha.view, ds.view, v["dout"], v["dkv"], heads))
        for name in calls:
            if name == "beta" and bad is None and hc in (16, 32, 64, 128):
                continue                                                    # (the row-wise pass has no p: a servable hc is served)
            if name == "src" and ed > 8:
                continue                                                    # (the source pass reads no edge features: it is served)
            with pytest.raises(_lib.GcnxError) as err:
                fns[name]()
            assert err.value.code == _lib.ERR_UNSUPPORTED, name
        for fr in (out, o, dq, d_o, d_s, dkv, alpha, ds, dwb) + ((dwe,) if ed else ()):
            fr.check(np.full((fr.n, fr.f), SENTINEL), "a refused call writes nothing")

    # every rule of conv_ok
    for heads, c in ((3, 16), (1, 96), (8, 32), (8, 2)):
        assert not D.transformer_conv_ok(ctx, n, heads, c)
        refused(ctx.zeros((n, 4 * heads * c)), heads, c)
    assert not D.transformer_conv_ok(ctx, n, 1, 16, edge_dim=9)
    refused(ctx.zeros((n, 64)), 1, 16, ed=9)
    assert not D.transformer_conv_ok(ctx, n, 1, 16, ldp=44)
    narrow = ctx.zeros((n, 64))
    refused(DeviceArray(ctx, narrow.ptr, (n, 48), np.float32, ld=44, base=narrow), 1, 16)        # ldp < 3 HC
    wide = ctx.zeros((n, 66))
    assert not D.transformer_conv_ok(ctx, n, 1, 16, ldp=66)
    refused(DeviceArray(ctx, wide.ptr, (n, 64), np.float32, ld=66, base=wide), 1, 16)            # ldp % 4 != 0
    assert not ctx.lib.gcnx_transformer_conv_ok(2 ** 24, 1, 16, 64, 0)                          # n * ldp * 4 reaches 2^32
    # misaligned pointers and bad leading dimensions of the other float4 operands
    off = Frame(ctx, n, 64, 64, 1)                                                              # one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4 and D.transformer_conv_ok(ctx, n, 1, 16, ldp=64)
    refused(off.view, 1, 16)
    good = ctx.zeros((n, 64))
    for name, width in (("out", 16), ("o", 16), ("dq", 16), ("dkv", 32), ("dout", 16), ("d_o", 16), ("d_s", 16)):
        fr = Frame(ctx, n, width, width, 1)                                                     # off a 16-byte boundary
        refused(good, 1, 16, bad=(name, fr.view))
        fr.check(np.full((n, width), SENTINEL), "a refused call writes nothing")
        fr = Frame(ctx, n, width, width + 2, 0)                                                 # a leading dimension that is no multiple of 4
        refused(good, 1, 16, bad=(name, fr.view))
        fr.check(np.full((n, width), SENTINEL), "a refused call writes nothing")
    # negative sizes and NULL mandatory pointers: invalid arguments; e = NULL with edge_dim > 0 and w_beta without skip too
    lib = ctx.lib
    x, w, out = ctx.zeros((4, 64)), ctx.zeros(48), Frame(ctx, 4, 16, 16, 0)
    kv, al, big, we = Frame(ctx, 4, 32, 32, 0), Frame(ctx, 16, 1, 1, 0), ctx.zeros(256), ctx.zeros((2, 16))
    rp, ci = a.rowptr.ptr, a.colidx.ptr

    def call(which, nn, xp, ed=0, ep=None, skip=x.ptr + 192):
        """The return codes of the named calls (only calls that must be refused are made: the operands are 4 rows wide)."""
        fns = dict(
            agg=lambda: lib.gcnx_transformer_aggregate(ctx.h, rp, ci, xp, 64, nn, 1, 16, ep, ed, ed, we.ptr, skip, 64, w.ptr, out.view.ptr, 16,
                                                       al.view.ptr, None, 0),
            tgt=lambda: lib.gcnx_transformer_bwd_targets(ctx.h, rp, ci, xp, 64, nn, 1, 16, ep, ed, ed, we.ptr, al.view.ptr, x.ptr, 64, x.ptr, 64,
                                                         al.view.ptr, out.view.ptr, 16, None, 0, big.ptr, big.ptr),
            src=lambda: lib.gcnx_transformer_bwd_sources(ctx.h, rp, ci, ci, xp, 64, nn, 1, 16, al.view.ptr, al.view.ptr, x.ptr, 64,
                                                         kv.view.ptr, 32),
            beta=lambda: lib.gcnx_transformer_beta_bwd(ctx.h, xp, 64, x.ptr, 64, x.ptr, 64, w.ptr, nn, 16, out.view.ptr, 16, kv.view.ptr, 32,
                                                       big.ptr, big.ptr))
        return tuple(fns[k]() for k in which)

    every = ("agg", "tgt", "src", "beta")
    assert call(every, -1, x.ptr) == (1,) * 4                                                   # GCNX_ERR_INVALID
    assert call(every, 4, None) == (1,) * 4
    assert call(("agg", "tgt"), 4, x.ptr, ed=2, ep=None) == (1,) * 2
    assert call(("agg",), 4, x.ptr, skip=None) == (1,)                                          # w_beta without skip
    for fr in (out, al):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "invalid calls write nothing")
    assert not big.numpy().any()


# ---- 8. the layer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("edge_dim", [None, 2])
def test_transformerconv_layer_forward_and_backward(ctx, edge_dim, beta):
    from gcnx.layers import TransformerConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    lay = TransformerConv(16, heads=4, edge_dim=edge_dim, beta=beta, seed=3)
    pre = TransformerConv.preprocess(a)
    assert pre.vals is None and pre.nnz == a.nnz
    lay.build(ctx, 16)
    names = list(TR.conv_keys(edge_dim, beta, True))
    assert list(lay.params) == names == list(lay.grads)
    assert lay.lin_weight.shape == (16, 256) and lay.lin_bias.shape == (256,) and all(v.ptr % 16 == 0 for v in lay.params.values())
    assert lay.params["lin_query.weight"].ptr == lay.lin_weight.ptr and lay.params["lin_key.weight"].ptr == lay.lin_weight.ptr + 4 * 64
    assert lay.params["lin_skip.weight"].ptr == lay.lin_weight.ptr + 4 * 192 and lay.params["lin_key.weight"].ld == 256       # views of ONE tensor
    assert lay.params["lin_value.bias"].ptr == lay.lin_bias.ptr + 4 * 128
    rng = np.random.default_rng(1)
    sd0 = lay.state_dict()
    assert sd0["lin_key.weight"].shape == (64, 16) and sd0["lin_skip.bias"].shape == (64,)
    assert (not edge_dim or sd0["lin_edge.weight"].shape == (64, 2)) and (not beta or sd0["lin_beta.weight"].shape == (1, 192))
    sd = {k: (rng.standard_normal(v.shape) * (0.3 if k.endswith("bias") else 1.0 / np.sqrt(v.shape[-1]))).astype(np.float32) for k, v in sd0.items()}
    lay.load_state_dict(sd)
    back = lay.state_dict()
    assert list(back) == names and all(np.array_equal(_bits(back[k]), _bits(sd[k])) for k in sd)
    assert np.array_equal(sd["lin_key.weight"].T, lay.params["lin_key.weight"].numpy())
    p = {f"conv1.{k}": v.astype(np.float64) for k, v in sd.items()}
    W, b, We, wb = TR.split(p, 1)
    x = ctx.to_device(hb.x)
    e_host = rng.uniform(0, 1, (hb.nnz, 2)).astype(np.float32) if edge_dim else None
    e = ctx.to_device(e_host) if edge_dim else None
    y = lay([x, pre, e] if edge_dim else [x, pre])
    r_y, k = TR.layer_fwd(hb.rowptr, hb.colidx, hb.x, W, b, We, wb, 4, 64, e_host)
    assert rel_err(lay._saved[3].numpy(), k["P"]) < TIGHT                  # ONE gcnx_gemm, stacked bias
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = rng.standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    ref = TR.join(TR.layer_bwd(k, dy), 1, 64)
    got = lay.gradients()
    assert list(got) == names
    errs = {"dx": rel_err(dx.numpy(), k["dP"] @ k["W"].T)}
    for key in names:
        r = ref["conv1." + key]
        scale = np.max(np.abs(ref["conv1.lin_key.weight"])) if key == "lin_key.bias" else None      # analytically zero
        errs[key] = float(np.max(np.abs(got[key] - r)) / scale) if scale else rel_err(got[key], r)
    print(f"transformer layer edge_dim={edge_dim} beta={beta}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert max(errs.values()) < TIGHT, errs
    before = {key: v.numpy() for key, v in lay.grads.items()}
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    assert all(np.array_equal(_bits(before[key]), _bits(lay.grads[key].numpy())) for key in before)     # the same gradients without dx
    with pytest.raises(ValueError):
        lay([x, pre] if edge_dim else [x, pre, ctx.zeros((hb.nnz, 2))])  # e missing with edge_dim / given without
    if edge_dim:
        with pytest.raises(ValueError):
            lay([x, pre, ctx.zeros((hb.nnz, 3))])                        # a wrong width
    nob = TransformerConv(16, heads=4, edge_dim=edge_dim, beta=beta, use_bias=False, seed=3)
    nob.build(ctx, 16)
    assert nob.lin_bias is None and not any(k.endswith(".bias") for k in nob.params)
    y2 = nob([x, pre, e] if edge_dim else [x, pre])
    q = {f"conv1.{k}": v.astype(np.float64) for k, v in nob.state_dict().items()}
    for s in TR.BLOCKS:
        q[f"conv1.{s}.bias"] = np.zeros(64)
    r2, _ = TR.layer_fwd(hb.rowptr, hb.colidx, hb.x, *TR.split(q, 1), 4, 64, e_host)
    assert rel_err(y2.numpy(), r2) < TIGHT
    nob.backward(ctx.to_device(dy), need_dx=False)


# ---- 9. gcnx.Transformer: a full step against the oracle ---------------------------------------------------------------------
def _sides(m, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    return {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
            for i in (1, 2)}


def _under(beta, every_row_has_an_entry):
    """Gradients that are analytically zero, measured relative to their weight's gradient (test_gpu_gat.UNDER_BN): lin_key.bias
    always (a common shift of all keys cancels in the softmax); in front of BatchNorm and without the beta gate a constant
    added to every row of the output cancels: lin_skip.bias, and lin_value.bias when every row has an entry (alpha sums to 1)."""
    t = {k: v for k, v in UNDER_BN.items() if not k.startswith("conv")}
    for c in ("conv1", "conv2"):
        t[f"{c}.lin_key.bias"] = f"{c}.lin_key.weight"
        if not beta:
            t[f"{c}.lin_skip.bias"] = f"{c}.lin_skip.weight"
            if every_row_has_an_entry:
                t[f"{c}.lin_value.bias"] = f"{c}.lin_value.weight"
    return t


def _cmp_grads(got, ref, tol, what, under):
    """Every gradient block against the oracle; returns "worst error (its key)" (all errors are printed before any assertion)."""
    errs = {}
    for k in ref:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[under.get(k, k)], np.float64))))
        diff = float(np.max(np.abs(g - r)))
        errs[k] = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)  # (a gradient that is exactly zero on both sides)
    print(f"transformer step {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol, (what, k, v)
    worst = max(errs, key=errs.get)
    return f"{errs[worst]:.2e} ({worst})"


def _device_batch(ctx, hb, e):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), e=None if e is None else ctx.to_device(e))


def _features(nnz, d, seed):
    return np.random.default_rng(seed).uniform(0, 1, (nnz, d)).astype(np.float32)


@pytest.mark.parametrize("heads,edge_dim,beta", [(1, None, False), (1, 2, False), (4, None, False), (4, 2, False), (4, 2, True)])
def test_transformer_step_against_oracle(ctx, heads, edge_dim, beta):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    e = _features(hb.nnz, 2, 5) if edge_dim else None
    batch = _device_batch(ctx, hb, e)
    m = gcnx.Transformer(ctx, hidden_channels=64, heads=heads, edge_dim=edge_dim, beta=beta, seed=0)
    assert m.uses_edge_features is bool(edge_dim)
    p = {k: v.astype(np.float32) for k, v in TR.init_params(16, 64, edge_dim, beta, True, seed=7).items()}
    m.load_state_dict(p)
    sd = m.state_dict()
    assert list(sd) == list(TR.keys(edge_dim, beta, True)) and all(np.array_equal(_bits(sd[k]), _bits(p[k])) for k in p)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    what = f"heads={heads} edge_dim={edge_dim} beta={beta}"
    m.loss_and_grads(batch)
    for k in ("p1", "p2", "dp", "o1", "o2", "alpha1", "alpha2", "dscore", "scratch"):
        assert k in m._bufs, k
    assert m._bufs["alpha1"].shape == (hb.nnz, heads) and m._bufs["p1"].shape == (hb.n, 256)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = TR.model(hb.x, hb.rowptr, hb.colidx, e, hb.graph_ptr, p, heads=heads, y=hb.y, masks=_sides(m), argmax=arg)
    la = m.loss_acc.numpy()
    e_out, e_loss = rel_err(m._bufs["out"].numpy(), r["out"]), rel_err(la[0], r["loss"])
    print(f"transformer step {what}: logits {e_out:.2e} loss {e_loss:.2e}")
    assert_close(m._bufs["out"].numpy(), r["out"], TIGHT, f"{what} logits")
    assert e_loss < TIGHT and la[1] == r["hits"], (la, r["loss"], r["hits"])
    grads = m.gradients()
    assert list(grads) == list(TR.keys(edge_dim, beta, True))
    under = _under(beta, bool(np.diff(hb.rowptr).min() > 0))
    print(f"transformer step {what}: worst gradient {_cmp_grads(grads, r['grads'], TIGHT, what, under)}")
    # three steps with gcnx.Adam run and lower the loss
    m.set_optimizer(gcnx.Adam())
    losses = [m.train_step(batch, lr=0.01)[0] for _ in range(3)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_transformer_one_clipped_adam_step_matches_the_restatement(ctx):
    """One Adam(clipnorm=1) step through set_optimizer: the device's parameters and state against optim_ref applied to that
    step's device gradients (the bounds of test_gpu_optim)."""
    import gcnx
    from test_gpu_optim import _assert_adam, _assert_norm
    hb = _tiny_host(16, 16, seed=4)
    batch = _device_batch(ctx, hb, _features(hb.nnz, 2, 5))
    m = gcnx.Transformer(ctx, hidden_channels=64, heads=4, edge_dim=2, beta=True, seed=0)
    m.load_state_dict({k: v.astype(np.float32) for k, v in TR.init_params(16, 64, 2, True, True, seed=7).items()})
    opt = gcnx.Adam(clipnorm=1.0)
    m.set_optimizer(opt)
    n, lr = m.n_params, 1e-2
    p0, m0, v0 = m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy()
    assert not m0.any() and not v0.any()
    m.train_step(batch, None, lr=lr)
    g = m.flat_g.numpy()[:n]
    norm = opt.last_grad_norm()
    _assert_norm(norm, g, min(256, -(-n // 256)), "transformer Adam step")
    _assert_adam(m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy(), p0, g, m0, v0, 1, lr, norm, "transformer Adam step",
                 beta1=opt.beta1, beta2=opt.beta2, eps=opt.eps, weight_decay=opt.weight_decay, clipnorm=opt.clipnorm)


def test_transformer_host_and_device_loader_routes_agree(ctx):
    """The same model fed (a) DisjointLoader batches (host route: pattern and e as stored) and (b) DeviceDisjointLoader batches
    of DeviceDataset(edge_features=True) over the same graphs in the same order: the same loss and gradients, bit for bit (the
    same kernels on the same operands, no atomics).  On route (b) the transposed pattern is the loader's preset: no host sort."""
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(12, 16, seed=3)
    graphs = []
    for k, (x, a, y) in enumerate(raw):
        a = a.tocsr()
        a.sort_indices()
        graphs.append(Graph(x=x, a=a, y=y, e=_features(a.nnz, 2, 100 + k)))
    ds = ListDataset(graphs)
    dsd = gcnx.DeviceDataset(ctx, ds, edge_features=True)
    dev = gcnx.DeviceDisjointLoader(dsd, batch_size=4, epochs=1, shuffle=True, seed=8)
    host = gcnx.DisjointLoader(ds, batch_size=4, epochs=1, shuffle=True, seed=8)
    m = gcnx.Transformer(ctx, hidden_channels=64, heads=4, edge_dim=2, beta=True, seed=2)
    seen = 0
    for (inputs, target), (db, none) in zip(host, dev):
        assert none is None and len(inputs) == 4
        m.loss_and_grads(inputs, target)
        hbatch = m._last_batch
        la_h, g_h = m.loss_acc.numpy(), m.gradients()
        assert hbatch.a.nnz == db.a.nnz and np.array_equal(hbatch.a.colidx.numpy()[:db.a.nnz], db.a.colidx.numpy()[:db.a.nnz])
        assert np.array_equal(_bits(hbatch.e.numpy()), _bits(db.e.numpy()))                         # e as stored on both routes
        preset = [v.ptr for v in db.a.transpose_perm()]
        assert preset == [dev._bufs.rowptr_t.ptr, dev._bufs.colidx_t.ptr, dev._bufs.perm_t.ptr]
        m.loss_and_grads(db)
        assert [v.ptr for v in m._op(db)[1].transpose_perm()] == preset                             # the preset views are used
        la_d, g_d = m.loss_acc.numpy(), m.gradients()
        assert np.array_equal(_bits(la_d), _bits(la_h))
        assert list(g_d) == list(g_h) and all(np.array_equal(_bits(g_d[k]), _bits(g_h[k])) for k in g_h)
        seen += 1
    assert seen == 3
    with pytest.raises(ValueError):
        m.loss_and_grads(inputs[:2] + inputs[3:], target)                 # (x, a, i) for a model that reads e


def test_fit_runs_the_transformer_model_from_device_batches(ctx):
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    mk = lambda part: ListDataset([Graph(x=x, a=a.tocsr(), y=y, e=_features(a.tocsr().nnz, 2, 7)) for x, a, y in part])
    tr, te = gcnx.DeviceDataset(ctx, mk(raw[:10]), edge_features=True), gcnx.DeviceDataset(ctx, mk(raw[10:]), edge_features=True)
    m = gcnx.Transformer(ctx, heads=4, edge_dim=2, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=6, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=6, schedule=lambda it: 0.01, verbose=False,
                   optimizer=gcnx.Adam())
    hist = out["history"]
    assert len(hist) == 6 and all(np.all(np.isfinite(h)) for h in hist)
    print("transformer fit: train loss per epoch " + " ".join(f"{h[0]:.4f}" for h in hist))
    assert hist[-1][0] < hist[0][0], (hist[0], hist[-1])                  # the loss falls

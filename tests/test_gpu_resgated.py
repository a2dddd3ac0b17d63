"""GPU tests of ResGatedGraphConv: the kernels of csrc/resgated.hip (gcnx_resgated_aggregate, gcnx_resgated_bwd_targets,
gcnx_resgated_bwd_sources), the layer gcnx.ResGatedGraphConv and the model gcnx.ResGated -- each against the float64 oracle
tests/resgated_ref.py.  The sigmoid has no kink, so the convolutions need no side masks; the model's PReLU sides and max-pool
winners are the device's (gcn_bn_ref).  Bound: test_gpu_gat.TIGHT = 2e-5 (max-norm relative against float64) for every kernel
output, the layer, a whole step of the model and the two loader routes."""
import functools

import numpy as np
import pytest

from conftest import assert_close, rel_err
import gcn_bn_ref as R
import resgated_ref as RG
from gpu_frames import SENTINEL, Frame
from test_gpu_gat import TIGHT, UNDER_BN, _bits, _csr, _ecoli3, _edge_case_csr, _frame_check
from test_gpu_gcn_bn import _tiny_host

pytestmark = pytest.mark.gpu

WIDTHS = [16, 32, 64, 128]
EDGE_DIMS = [0, 1, 2, 8]
ERR_INVALID = 1                     # GCNX_ERR_INVALID (include/gcnx.h)
# gradients that are analytically zero (a shift in front of a BatchNorm): compared relative to the weight gradient named here
UNDER_BN_RG = {"conv1.bias": "conv1.lin_value.weight", "conv2.bias": "conv2.lin_value.weight", "linear_1.bias": "linear_1.weight",
               "linear_2.bias": "linear_2.weight", "batch_norm_2.bias": "batch_norm_2.weight"}
assert set(UNDER_BN_RG) == set(UNDER_BN)


def _operands(n, nnz, h, d, seed, shift=0.0):
    """P = K | Q | V | S at unit scale (K + Q ~ N(0, 2): the gates neither flat nor saturated; shift: added to K), a bias, e in
    (0, 1) as dca / proximity are, W_e ~ N(0, 1) / 2, dout."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 4 * h)).astype(np.float32)
    p[:, :h] += np.float32(shift)
    bias = rng.standard_normal(h).astype(np.float32)
    e = rng.uniform(0, 1, (nnz, d)).astype(np.float32) if d else None
    w_e = (rng.standard_normal((d, 3 * h)) / 2).astype(np.float32) if d else None
    dout = rng.standard_normal((n, h)).astype(np.float32)
    return dict(p=p, bias=bias, e=e, w_e=w_e, dout=dout)


class _Dev:
    """The device side of one layer evaluation: operands uploaded once (or given as device views), every kernel callable."""

    def __init__(self, ctx, a, ops):
        up = lambda t: t if t is None or hasattr(t, "ptr") else ctx.to_device(t)
        self.ctx, self.a = ctx, a
        self.p, self.bias, self.e, self.w_e, self.dout = (up(ops[k]) for k in ("p", "bias", "e", "w_e", "dout"))
        self.n, self.h = self.dout.shape
        self.d = 0 if self.e is None else self.e.shape[1]

    def _skip(self):
        return self.p.cols(3 * self.h, 4 * self.h)

    def aggregate(self, skip=True, bias=True, out=None):
        from gcnx import device as D
        self.out = out if out is not None else self.ctx.empty((self.n, self.h))
        D.resgated_aggregate(self.ctx, self.a, self.p, self.out, e=self.e, w_e=self.w_e, skip=self._skip() if skip else None,
                             bias=self.bias if bias else None)
        return self.out.numpy()

    def bwd_targets(self, dk=None, ds=None, with_ds=True):
        from gcnx import device as D
        ctx = self.ctx
        self.dk = dk if dk is not None else ctx.empty((self.n, self.h))
        self.ds = (ds if ds is not None else ctx.empty((self.n, self.h))) if with_ds else None
        self.dwe = ctx.empty((self.d, 3 * self.h)) if self.d else None
        scratch = ctx.empty(max(D.resgated_bwd_scratch_floats(ctx, self.n, self.h, self.d), 1))
        D.resgated_bwd_targets(ctx, self.a, self.p, self.dout, self.dk, scratch, ds=self.ds, e=self.e, w_e=self.w_e, dw_e=self.dwe)
        return self.dk.numpy(), (self.ds.numpy() if with_ds else None), (self.dwe.numpy() if self.d else None)

    def bwd_sources(self, dqv=None):
        from gcnx import device as D
        self.dqv = dqv if dqv is not None else self.ctx.empty((self.n, 2 * self.h))
        D.resgated_bwd_sources(self.ctx, self.a, self.p, self.dout, self.dqv, e=self.e, w_e=self.w_e)
        return self.dqv.numpy()


def _oracle(rowptr, colidx, ops, skip=True, bias=True):
    h = ops["dout"].shape[1]
    out, cache = RG.conv_fwd(rowptr, colidx, ops["p"], h, ops["e"], ops["w_e"], ops["p"][:, 3 * h:4 * h] if skip else None,
                             ops["bias"] if bias else None)
    cache["grads"] = RG.conv_bwd(cache, ops["dout"])
    return out, cache


def _check_all(ctx, a, rowptr, colidx, ops, what, tol=TIGHT, saturated=None):
    """Every kernel on one input against the oracle; returns the device object with the host copies (errors printed first).
    saturated: "one" / "zero" -- every gate at 1 / 0 in float32: g (1 - g) is exactly 0 there while float64 keeps ~1e-87, so dK,
    dQ and the gate blocks of dw_e are asserted to be (next to) zero instead of measured relative to a reference of that size."""
    d = _Dev(ctx, a, ops)
    out = d.aggregate()
    dk, ds, dwe = d.bwd_targets()
    dqv = d.bwd_sources()
    r_out, k = _oracle(rowptr, colidx, ops)
    g, h = k["grads"], d.h
    assert all(np.isfinite(t).all() for t in (out, dk, ds, dqv)) and (dwe is None or np.isfinite(dwe).all())
    assert np.array_equal(_bits(ds), _bits(ops["dout"]))                       # dS is a copy
    errs = {"out": rel_err(out, r_out), "dV": rel_err(dqv[:, h:], g["dV"])}
    if saturated is None:
        errs.update(dK=rel_err(dk, g["dK"]), dQ=rel_err(dqv[:, :h], g["dQ"]))
        if d.d:
            errs["dw_e"] = rel_err(dwe, g["dWe"])
    else:
        assert np.max(np.abs(dk)) < 1e-30 and np.max(np.abs(dqv[:, :h])) < 1e-30 and np.max(np.abs(g["dK"])) < 1e-30
        if d.d:
            assert np.max(np.abs(dwe[:, :2 * h])) < 1e-30
            errs["dw_ve"] = rel_err(dwe[:, 2 * h:], g["dWe"][:, 2 * h:]) if saturated == "one" else float(np.max(np.abs(dwe[:, 2 * h:])))
    if d.d:
        assert np.array_equal(_bits(dwe[:, :h]), _bits(dwe[:, h:2 * h]))      # dW_ke and dW_qe: the same numbers
    print(f"resgated {what} h={h} edge_dim={d.d}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    for key, v in errs.items():
        assert v < tol, (what, key, v)
    d.host = dict(out=out, dk=dk, ds=ds, dwe=dwe, dqv=dqv, ref=k, r_out=r_out)
    return d


# ---- 1. the kernels against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dim", EDGE_DIMS)
@pytest.mark.parametrize("h", WIDTHS)
def test_resgated_kernels_against_float64(ctx, h, edge_dim):
    from gcnx import device as D
    hb = _ecoli3(h)
    a = _csr(ctx, hb)
    assert D.resgated_conv_ok(ctx, hb.n, h, 4 * h, edge_dim) and hb.n % 32 != 0
    ops = _operands(hb.n, hb.nnz, h, edge_dim, 1000 * edge_dim + h)
    d = _check_all(ctx, a, hb.rowptr, hb.colidx, ops, "ecoli-3")
    hh = d.host
    gates = hh["ref"]["g"]
    assert 0.2 < (gates > 0.5).mean() < 0.8 and gates.min() < 0.1 and gates.max() > 0.9     # the whole range of the sigmoid is exercised
    # no atomics: a second call of each leaves the same bits
    second = (d.aggregate(),) + d.bwd_targets() + (d.bwd_sources(),)
    first = tuple(hh[k] for k in ("out", "dk", "ds", "dwe", "dqv"))
    for k, (x, y) in enumerate(zip(first, second)):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), k
    # without skip, without bias, without either, without ds
    for skip, bias in ((False, True), (True, False), (False, False)):
        got = d.aggregate(skip=skip, bias=bias)
        want, _ = _oracle(hb.rowptr, hb.colidx, ops, skip, bias)
        assert rel_err(got, want) < TIGHT, (skip, bias, rel_err(got, want))
    dk2, ds2, dwe2 = d.bwd_targets(with_ds=False)
    assert ds2 is None and np.array_equal(_bits(dk2), _bits(hh["dk"])) and (dwe2 is None or np.array_equal(_bits(dwe2), _bits(hh["dwe"])))


# ---- 2. the smallest shapes that can still go wrong -----------------------------------------------------------------------------
@pytest.mark.parametrize("h,edge_dim", [(32, 2), (16, 0), (128, 2)])
def test_resgated_kernels_degenerate_inputs(ctx, h, edge_dim):
    """Rows without entries, a directed pattern (the transposed pattern differs), fewer rows than a tile, a row with only its
    loop, a row whose only entry is in no row, duplicate entries.  h = 128: the 16-row workgroups."""
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _edge_case_csr()
    n = 56
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp, symmetric=False)
    assert not a.symmetric
    ops = _operands(n, len(colidx), h, edge_dim, 7 + h)
    d = _check_all(ctx, a, rowptr, colidx, ops, "56 rows")
    hh = d.host
    assert np.array_equal(_bits(hh["out"][[4, 20]]), _bits(ops["p"][[4, 20], 3 * h:] + ops["bias"]))   # no entries: S + bias
    assert not hh["dk"][[4, 20]].any()
    # fewer rows than a tile
    assert list(gp[:4]) == [0, 1, 4, 5]
    nnz5 = int(rowptr[5])
    a5 = DeviceCSR.from_host_csr(ctx, rowptr[:6], colidx[:nnz5], None, gp[:4].copy(), symmetric=False)
    _check_all(ctx, a5, rowptr[:6], colidx[:nnz5], _operands(5, nnz5, h, edge_dim, 32), "5 rows")
    # one row with only its self-loop
    one = np.array([0, 1], np.int32)
    a1 = DeviceCSR.from_host_csr(ctx, one, np.zeros(1, np.int32), None, one, symmetric=True)
    ops1 = _operands(1, 1, h, edge_dim, 33)
    _check_all(ctx, a1, one, np.zeros(1, np.int32), ops1, "1 row, self-loop")
    # one row without any entry (the stored entry is in no row)
    a0 = DeviceCSR.from_host_csr(ctx, np.zeros(2, np.int32), np.zeros(1, np.int32), None, one, symmetric=True)
    d0 = _Dev(ctx, a0, ops1)
    assert np.array_equal(_bits(d0.aggregate()), _bits(ops1["p"][:, 3 * h:] + ops1["bias"]))
    dk0, ds0, dwe0 = d0.bwd_targets()                                    # (no transposed pattern of a CSR whose entry is in no row)
    assert not dk0.any() and np.array_equal(_bits(ds0), _bits(ops1["dout"])) and (dwe0 is None or not dwe0.any())
    # duplicate entries: every stored entry is a message of its own (with its own edge features)
    rp3, ci3 = np.array([0, 3, 4, 6], np.int32), np.array([1, 1, 2, 0, 2, 2], np.int32)
    a3 = DeviceCSR.from_host_csr(ctx, rp3, ci3, None, np.array([0, 3], np.int32), symmetric=False)
    _check_all(ctx, a3, rp3, ci3, _operands(3, 6, h, edge_dim, 34), "duplicates")


@functools.lru_cache(maxsize=None)
def _one_long_row():
    """One graph of 4 300 rows (not a multiple of 32): every loop, a ring, and row 7 <-> columns 0 .. 4 199 -- a single row of
    more than four times the 1 024 entries a tile stages in LDS, in the forward CSR and, the pattern being symmetric, in the
    transposed one."""
    import scipy.sparse as sp
    n = 4300
    i = np.arange(n)
    hub = np.arange(4200)
    rows = np.concatenate([i, i, (i + 1) % n, np.full(hub.size, 7), hub])
    cols = np.concatenate([i, (i + 1) % n, i, hub, np.full(hub.size, 7)])
    a = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    deg = np.diff(a.indptr)
    assert deg[7] >= 4097 and np.sum(deg > 1024) == 1 and n % 32 != 0
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), np.array([0, n], np.int32)


@pytest.mark.parametrize("h,edge_dim", [(64, 2), (128, 0)])
def test_resgated_kernels_one_row_beyond_the_staged_entries(ctx, h, edge_dim):
    from gcnx.device import DeviceCSR
    rowptr, colidx, gp = _one_long_row()
    a = DeviceCSR.from_host_csr(ctx, rowptr, colidx, None, gp)
    assert a.symmetric
    _check_all(ctx, a, rowptr, colidx, _operands(4300, len(colidx), h, edge_dim, 11 + h), "long row")


def test_resgated_no_rows(ctx):
    """n = 0 succeeds and writes nothing."""
    from gcnx import _lib
    lib = ctx.lib
    out, wide, big = Frame(ctx, 4, 16, 16, 0), Frame(ctx, 4, 32, 32, 0), ctx.zeros(64)
    p = ctx.zeros((4, 64))
    rp = ctx.to_device(np.zeros(1, np.int32))
    rcs = (lib.gcnx_resgated_aggregate(ctx.h, rp.ptr, rp.ptr, p.ptr, 64, 0, 16, None, 0, 0, None, None, 0, None, out.view.ptr, 16),
           lib.gcnx_resgated_bwd_targets(ctx.h, rp.ptr, rp.ptr, p.ptr, 64, 0, 16, None, 0, 0, None, p.ptr, 64, out.view.ptr, 16, None, 0, None,
                                         big.ptr),
           lib.gcnx_resgated_bwd_sources(ctx.h, rp.ptr, rp.ptr, rp.ptr, p.ptr, 64, 0, 16, None, 0, 0, None, p.ptr, 64, wide.view.ptr, 32))
    assert rcs == (_lib.OK,) * 3
    for fr in (out, wide):
        fr.check(np.full((fr.n, fr.f), SENTINEL), "n = 0 writes nothing")
    assert not big.numpy().any()


def test_resgated_strided_operands(ctx):
    """ldp > 4 h, a strided e, strided out / d_out, and dK | dQ | dV | dS written as the column blocks of ONE wider array."""
    from gcnx import device as D
    h, ed = 32, 2
    hb = _ecoli3(h)
    a = _csr(ctx, hb)
    ops = _operands(hb.n, hb.nnz, h, ed, 51)
    fp = Frame(ctx, hb.n, 4 * h, 4 * h + 8, 4, data=ops["p"])
    fe = Frame(ctx, hb.nnz, ed, ed + 3, 1, data=ops["e"])               # (e is read with scalar loads: no alignment rule)
    f_out = Frame(ctx, hb.n, h, h + 8, 8)
    f_do = Frame(ctx, hb.n, h, h + 4, 4, data=ops["dout"])
    f_dp = Frame(ctx, hb.n, 4 * h, 4 * h + 4, 4)
    assert all(f.aligned() for f in (fp, f_out, f_do, f_dp)) and D.resgated_conv_ok(ctx, hb.n, h, fp.view.ld, ed)
    d = _Dev(ctx, a, dict(ops, p=fp.view, e=fe.view, dout=f_do.view))
    d.aggregate(out=f_out.view)
    d.bwd_targets(dk=f_dp.view.cols(0, h), ds=f_dp.view.cols(3 * h, 4 * h))
    d.bwd_sources(dqv=f_dp.view.cols(h, 3 * h))
    r_out, k = _oracle(hb.rowptr, hb.colidx, ops)
    g = k["grads"]
    assert rel_err(d.dwe.numpy(), g["dWe"]) < TIGHT
    _frame_check(f_out, r_out, TIGHT, "out")
    _frame_check(f_dp, np.hstack([g["dK"], g["dQ"], g["dV"], g["dS"]]), TIGHT, "dK | dQ | dV | dS")
    fp.check(ops["p"], "p is not written")
    fe.check(ops["e"], "e is not written")
    f_do.check(ops["dout"], "d_out is not written")


# ---- 3. the range of the exponential ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [200.0, -200.0])
def test_resgated_shifted_keys_saturate_without_nan(ctx, shift):
    """K shifted by +-200: every a moves by hundreds, exp(-a) overflows to inf (a << 0) or underflows to 0 (a >> 0).  Gate ~ 1:
    out = S + bias + sum m; gate ~ 0: out = S + bias, dV = 0; dK, dQ ~ 0 on both sides; nothing is inf or NaN."""
    hb = _ecoli3(64)
    ops = _operands(hb.n, hb.nnz, 64, 2, 43, shift=shift)
    d = _check_all(ctx, _csr(ctx, hb), hb.rowptr, hb.colidx, ops, f"K {shift:+.0f}", saturated="one" if shift > 0 else "zero")
    hh, k = d.host, d.host["ref"]
    assert np.min(np.abs(k["a"])) > 150                                   # every gate is saturated
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(np.max(np.abs(k["a"])))) == np.inf       # what a kernel that multiplied by exp(-a) would hold
    s_b = ops["p"][:, 192:].astype(np.float64) + ops["bias"]
    if shift > 0:
        sum_m = np.zeros((hb.n, 64))
        np.add.at(sum_m, k["row"], k["m"])
        assert rel_err(hh["out"], s_b + sum_m) < TIGHT
    else:
        assert np.array_equal(_bits(hh["out"]), _bits((ops["p"][:, 192:] + ops["bias"]).astype(np.float32)))
        assert not hh["dqv"][:, 64:].any()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_resgated_refusals(ctx):
    from gcnx import _lib, device as D
    from gcnx.device import DeviceArray
    hb = _ecoli3(16)
    a = _csr(ctx, hb)
    a.transpose_perm()
    n, nnz = hb.n, a.nnz
    lib = ctx.lib
    rp, ci = a.rowptr.ptr, a.colidx.ptr
    rt, ct, pt = (v.ptr for v in a.transpose_perm())

    def refused(h, ed=0, p=None, ldp=None, out_lead=0, bias_off=0, ldo=None, e_null=False, we_null=False, nn=None, p_null=False,
                dwe_null=False, calls=(0, 1, 2)):
        """The calls named (0 aggregate, 1 bwd_targets, 2 bwd_sources) with one thing wrong: returns their codes after checking
        that no output frame was written."""
        hw = max(h, 4)
        p = p if p is not None else ctx.zeros((n, 4 * hw))
        ldp = ldp if ldp is not None else p.ld
        e, w_e = (ctx.zeros((nnz, ed)), ctx.zeros((ed, 3 * hw))) if ed > 0 else (None, None)
        out, dk, ds = (Frame(ctx, n, hw, hw, out_lead) for _ in range(3))
        dqv, dwe = Frame(ctx, n, 2 * hw, 2 * hw, out_lead), Frame(ctx, max(ed, 1), 3 * hw, 3 * hw, 0)
        bias, dense = ctx.zeros(hw + 4), ctx.zeros((n, hw))
        scratch = Frame(ctx, 1, 64 * 1024, 64 * 1024, 0)
        ldo = ldo if ldo is not None else hw
        nn = n if nn is None else nn
        pp = None if p_null else p.ptr
        ep, wp = (None if e_null or ed <= 0 else e.ptr), (None if we_null or ed <= 0 else w_e.ptr)
        dwp = None if dwe_null or ed <= 0 else dwe.view.ptr
        lde = max(ed, 0)
        fns = (lambda: lib.gcnx_resgated_aggregate(ctx.h, rp, ci, pp, ldp, nn, h, ep, lde, ed, wp, None, 0, bias.ptr + 4 * bias_off,
                                                   out.view.ptr, ldo),
               lambda: lib.gcnx_resgated_bwd_targets(ctx.h, rp, ci, pp, ldp, nn, h, ep, lde, ed, wp, dense.ptr, hw, dk.view.ptr, ldo,
                                                     ds.view.ptr, ldo, dwp, scratch.view.ptr),
               lambda: lib.gcnx_resgated_bwd_sources(ctx.h, rt, ct, pt, pp, ldp, nn, h, ep, lde, ed, wp, dense.ptr, hw, dqv.view.ptr,
                                                     2 * hw + (ldo - hw)))
        rcs = tuple(fns[i]() for i in calls)
        for fr in (out, dk, ds, dqv, dwe, scratch):
            fr.check(np.full((fr.n, fr.f), SENTINEL), "a refused call writes nothing")
        return rcs

    U, I = _lib.ERR_UNSUPPORTED, ERR_INVALID
    for h in (0, 8, 48, 96, 256):                                           # widths without a kernel
        assert not D.resgated_conv_ok(ctx, n, h, 4 * max(h, 4)) and refused(h) == (U,) * 3, h
    assert not D.resgated_conv_ok(ctx, n, 16, 64, 9) and refused(16, ed=9) == (U,) * 3
    wide = ctx.zeros((n, 66))
    assert not D.resgated_conv_ok(ctx, n, 16, 66)
    assert refused(16, p=DeviceArray(ctx, wide.ptr, (n, 64), np.float32, ld=66, base=wide)) == (U,) * 3        # ldp % 4 != 0
    assert not D.resgated_conv_ok(ctx, n, 16, 44) and refused(16, ldp=44) == (U,) * 3                          # ldp < 3 h
    assert not D.resgated_conv_ok(ctx, n, 16, 2 ** 20) and refused(16, ldp=2 ** 20) == (U,) * 3                # n * ldp * 4 >= 2^32
    off = Frame(ctx, n, 64, 64, 1)                                          # one float off a 16-byte boundary
    assert off.view.ptr % 16 == 4 and D.resgated_conv_ok(ctx, n, 16, 64)
    assert refused(16, p=off.view) == (U,) * 3
    assert refused(16, out_lead=1) == (U,) * 3                              # out / dk / ds / dqv off the boundary
    assert refused(16, bias_off=1, calls=(0,)) == (U,)                      # bias off the boundary (the forward's operand)
    assert refused(16, ldo=18) == (U,) * 3                                  # ldo / ldg % 4 != 0
    # negative sizes and NULL mandatory pointers: invalid arguments; e / w_e / dw_e = NULL with edge_dim > 0 too
    assert refused(16, nn=-1) == (I,) * 3
    assert refused(-16) == (I,) * 3
    assert refused(16, ed=-1) == (I,) * 3
    assert refused(16, p_null=True) == (I,) * 3
    assert refused(16, ed=2, e_null=True) == (I,) * 3
    assert refused(16, ed=2, we_null=True) == (I,) * 3
    assert refused(16, ed=2, dwe_null=True, calls=(1,)) == (I,)
    # and the wrappers raise what the library answers
    with pytest.raises(_lib.GcnxError) as err:
        D.resgated_aggregate(ctx, a, off.view, ctx.zeros((n, 16)))
    assert err.value.code == U


# ---- 5. the layer ---------------------------------------------------------------------------------------------------------
def _layer_params(p, k=1):
    c = f"conv{k}."
    return {key[len(c):]: v for key, v in p.items() if key.startswith(c)}


@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("edge_dim", [None, 2])
def test_resgatedgraphconv_layer_forward_and_backward(ctx, edge_dim, root_weight):
    from gcnx.layers import ResGatedGraphConv
    hb = _tiny_host(16, 16)
    a = _csr(ctx, hb)
    d = edge_dim or 0
    lay = ResGatedGraphConv(64, edge_dim=edge_dim, root_weight=root_weight, seed=3)
    pre = ResGatedGraphConv.preprocess(a)
    assert pre.vals is None and pre.nnz == a.nnz
    lay.build(ctx, 16)
    w = 256 if root_weight else 192
    assert list(lay.params) == ["bias", "weight", "lin_bias"] + (["edge_weight"] if d else []) == list(lay.grads)
    assert lay.params["weight"].shape == (16, w) and lay.params["lin_bias"].shape == (192,) and all(v.ptr % 16 == 0 for v in lay.params.values())
    assert not d or lay.params["edge_weight"].shape == (d, 192)
    sd0 = lay.state_dict()
    assert list(sd0) == [n for n, _, _ in lay._param_spec(16)] and sd0["lin_key.weight"].shape == (64, 16 + d)
    assert not sd0["bias"].any() and 0 < np.max(np.abs(sd0["lin_query.weight"])) <= 1 / np.sqrt(16 + d)
    p = {k: v.astype(np.float32) for k, v in _layer_params(RG.init_params(16, 64, edge_dim, root_weight, seed=5)).items()}
    lay.load_state_dict(p)
    back = lay.state_dict()
    assert list(back) == list(p) and all(np.array_equal(_bits(back[k]), _bits(p[k])) for k in p)      # split and joined again
    W, b, We, bias, _ = RG.split({"conv1." + k: v for k, v in p.items()}, 1, edge_dim)
    x = ctx.to_device(hb.x)
    rng = np.random.default_rng(1)
    e_host = rng.uniform(0, 1, (hb.nnz, 2)).astype(np.float32) if d else None
    e = ctx.to_device(e_host) if d else None
    y = lay([x, pre, e] if d else [x, pre])
    r_y, k = RG.layer_fwd(hb.rowptr, hb.colidx, hb.x, W, b, We, bias, e_host)
    assert rel_err(lay._saved[3].numpy(), k["P"]) < TIGHT                 # ONE gcnx_gemm: stacked weight, stacked bias, S without one
    assert rel_err(y.numpy(), r_y) < TIGHT
    dy = rng.standard_normal((hb.n, 64)).astype(np.float32)
    dx = lay.backward(ctx.to_device(dy), need_dx=True)
    r = RG.layer_bwd(k, dy)
    want = _layer_params(RG.join(r, 1, edge_dim))
    got = lay.gradients()
    assert list(got) == list(p)
    errs = {"dx": rel_err(dx.numpy(), r["x"])}
    errs.update({key: rel_err(got[key], want[key]) for key in want})
    print(f"resgated layer edge_dim={edge_dim} root_weight={root_weight}: " + " ".join(f"{key} {v:.2e}" for key, v in errs.items()))
    assert max(errs.values()) < TIGHT, errs
    if d:
        assert np.array_equal(_bits(got["lin_key.weight"][:, 16:]), _bits(got["lin_query.weight"][:, 16:]))   # dW_ke == dW_qe
    before = {key: v.numpy() for key, v in lay.grads.items()}
    assert lay.backward(ctx.to_device(dy), need_dx=False) is None
    assert all(np.array_equal(_bits(before[key]), _bits(lay.grads[key].numpy())) for key in before)     # the same gradients without dx
    with pytest.raises(ValueError):
        lay([x, pre] if d else [x, pre, ctx.zeros((hb.nnz, 2))])         # e missing with edge_dim / given without
    if d:
        with pytest.raises(ValueError):
            lay([x, pre, ctx.zeros((hb.nnz, 3))])                        # a wrong width


# ---- 6. gcnx.ResGated: a full step against the oracle -----------------------------------------------------------------------
def _sides(m, pre=None):
    b = m._bufs
    pre = pre or {k: m.p[k].numpy() for k in ("g1", "be1", "g2", "be2")}
    return {f"m{i}": R.device_prelu_sides(b[f"z{i}"].numpy(), b[f"m{i}"].numpy(), b[f"i{i}"].numpy(), pre[f"g{i}"], pre[f"be{i}"])
            for i in (1, 2)}


def _cmp_grads(got, ref, tol, what):
    worst = 0.0
    for k in ref:
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64).reshape(np.shape(got[k]))
        scale = float(np.max(np.abs(np.asarray(ref[UNDER_BN_RG.get(k, k)], np.float64))))
        diff = float(np.max(np.abs(g - r)))
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)      # (a gradient that is exactly zero on both sides)
        worst = max(worst, err)
        assert err <= tol, (what, k, err)
    return worst


def _device_batch(ctx, hb, e):
    from gcnx.device import DeviceCSR, Segments
    from gcnx.models import DeviceBatch
    a = DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, None, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y), e=None if e is None else ctx.to_device(e))


def _features(nnz, d, seed):
    return np.random.default_rng(seed).uniform(0, 1, (nnz, d)).astype(np.float32)


@pytest.mark.parametrize("edge_dim,root_weight", [(None, True), (2, True), (2, False)])
def test_resgated_step_against_oracle(ctx, edge_dim, root_weight):
    import gcnx
    hb = _tiny_host(16, 16, seed=4)
    e = _features(hb.nnz, 2, 5) if edge_dim else None
    batch = _device_batch(ctx, hb, e)
    m = gcnx.ResGated(ctx, hidden_channels=64, edge_dim=edge_dim, root_weight=root_weight, seed=0)
    assert m.uses_edge_features is bool(edge_dim)
    p = {k: v.astype(np.float32) for k, v in RG.init_params(16, 64, edge_dim, root_weight, seed=7).items()}
    m.load_state_dict(p)
    sd = m.state_dict()
    assert list(sd) == list(RG.keys(root_weight)) and all(np.array_equal(_bits(sd[k]), _bits(p[k])) for k in p)
    assert all(m.p[k].ptr % 16 == 0 for k in m.PARAM_ORDER)
    what = f"edge_dim={edge_dim} root_weight={root_weight}"
    m.loss_and_grads(batch)
    w = 256 if root_weight else 192
    for k in ("p1", "p2", "dp", "scratch"):
        assert k in m._bufs, k
    assert m._bufs["p1"].shape == (hb.n, w) and m._bufs["dp"].shape == (hb.n, w)
    arg = m._bufs["arg"].numpy().astype(np.int64)
    r = RG.model(hb.x, hb.rowptr, hb.colidx, e, hb.graph_ptr, p, hb.y, masks=_sides(m), argmax=arg, edge_dim=edge_dim)
    la = m.loss_acc.numpy()
    e_out, e_loss = rel_err(m._bufs["out"].numpy(), r["out"]), rel_err(la[0], r["loss"])
    print(f"resgated step {what}: logits {e_out:.2e} loss {e_loss:.2e}")
    assert_close(m._bufs["out"].numpy(), r["out"], TIGHT, f"{what} logits")
    assert e_loss < TIGHT and la[1] == r["hits"], (la, r["loss"], r["hits"])
    grads = m.gradients()
    assert list(grads) == list(RG.keys(root_weight))
    print(f"resgated step {what}: worst gradient {_cmp_grads(grads, r['grads'], TIGHT, what):.2e}")
    if edge_dim:
        for k in (1, 2):
            f = 16 if k == 1 else 64
            assert np.array_equal(_bits(grads[f"conv{k}.lin_key.weight"][:, f:]), _bits(grads[f"conv{k}.lin_query.weight"][:, f:]))
    if root_weight:
        assert not any(m.p[f"lz{k}"].numpy().any() or m.g[f"lz{k}"].numpy().any() for k in (1, 2))     # the S block has no bias
    # three steps with gcnx.Adam run and lower the loss
    m.set_optimizer(gcnx.Adam())
    losses = [m.train_step(batch, lr=0.01)[0] for _ in range(3)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert not root_weight or not any(m.p[f"lz{k}"].numpy().any() for k in (1, 2))


def test_resgated_one_clipped_adam_step_matches_the_restatement(ctx):
    """One Adam(clipnorm=1) step through set_optimizer: the device's parameters and state against optim_ref applied to that
    step's device gradients (the bounds of test_gpu_optim)."""
    import gcnx
    from test_gpu_optim import _assert_adam, _assert_norm
    hb = _tiny_host(16, 16, seed=4)
    batch = _device_batch(ctx, hb, _features(hb.nnz, 2, 5))
    m = gcnx.ResGated(ctx, hidden_channels=64, edge_dim=2, seed=0)
    m.load_state_dict({k: v.astype(np.float32) for k, v in RG.init_params(16, 64, 2, True, seed=7).items()})
    opt = gcnx.Adam(clipnorm=1.0)
    m.set_optimizer(opt)
    n, lr = m.n_params, 1e-2
    p0, m0, v0 = m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy()
    assert not m0.any() and not v0.any()
    m.train_step(batch, None, lr=lr)
    g = m.flat_g.numpy()[:n]
    norm = opt.last_grad_norm()
    _assert_norm(norm, g, min(256, -(-n // 256)), "resgated Adam step")
    _assert_adam(m.flat_p.numpy(), opt.flat("m").numpy(), opt.flat("v").numpy(), p0, g, m0, v0, 1, lr, norm, "resgated Adam step",
                 beta1=opt.beta1, beta2=opt.beta2, eps=opt.eps, weight_decay=opt.weight_decay, clipnorm=opt.clipnorm)
    assert not any(m.p[f"lz{k}"].numpy().any() for k in (1, 2))           # zero gradient: the update leaves the S block's bias at zero


def test_resgated_host_and_device_loader_routes_agree(ctx):
    """The same model fed (a) DisjointLoader batches (host route: pattern and e as stored) and (b) DeviceDisjointLoader batches
    of DeviceDataset(edge_features=True) over the same graphs in the same order: the same loss and gradients to TIGHT.  On
    route (b) the transposed pattern is the loader's preset: no host sort."""
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
    m = gcnx.ResGated(ctx, hidden_channels=64, edge_dim=2, seed=2)
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
        assert rel_err(la_d[0], la_h[0]) < TIGHT and la_d[1] == la_h[1]
        worst = _cmp_grads(g_d, g_h, TIGHT, "device loader vs host loader")
        print(f"resgated loader routes batch {seen}: loss {rel_err(la_d[0], la_h[0]):.2e} worst gradient {worst:.2e}")
        seen += 1
    assert seen == 3
    with pytest.raises(ValueError):
        m.loss_and_grads(inputs[:2] + inputs[3:], target)                 # (x, a, i) for a model that reads e


def test_fit_runs_the_resgated_model_from_device_batches(ctx):
    import gcnx
    from gcnx import Graph, ListDataset, synth
    raw = synth.tiny_graphs(16, 16, seed=3)
    mk = lambda part: ListDataset([Graph(x=x, a=a.tocsr(), y=y, e=_features(a.tocsr().nnz, 2, 7)) for x, a, y in part])
    tr, te = gcnx.DeviceDataset(ctx, mk(raw[:10]), edge_features=True), gcnx.DeviceDataset(ctx, mk(raw[10:]), edge_features=True)
    m = gcnx.ResGated(ctx, edge_dim=2, seed=0)
    out = gcnx.fit(m, gcnx.DeviceDisjointLoader(tr, batch_size=5, epochs=6, shuffle=True, seed=1),
                   gcnx.DeviceDisjointLoader(te, batch_size=3, shuffle=False), epochs=6, schedule=lambda it: 0.01, verbose=False,
                   optimizer=gcnx.Adam())
    hist = out["history"]
    assert len(hist) == 6 and all(np.all(np.isfinite(h)) for h in hist)
    print("resgated fit: train loss per epoch " + " ".join(f"{h[0]:.4f}" for h in hist))
    assert hist[-1][0] < hist[0][0], (hist[0], hist[-1])                  # the loss falls

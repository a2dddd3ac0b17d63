"""Every launch route of the dense weight GEMMs (csrc/gemm.hip, gemm_stream.hip, gemm_panel.hip) bit for bit inside sentinel
frames: the case table of tests/gemm_route_cases.py (pinned on the host by tests/test_gemm_route_cases_host.py) run on the
device.

For every case:
  * before the call, the restated dispatch predicate is asserted on the case's own shape, the frames' real pointers and
    ctx.info()["cus"]: on any chip the case reaches the kernel it names or fails loudly;
  * each written frame holds the float32 (uint16 for bf16 rows) bit patterns of the EXACT result -- small-integer operands,
    every partial sum below 2^24, so no tolerance applies to any route, split or summation order;
  * everything outside each written view is still the sentinel (tail of n * (ld - f) + 64 elements: a store that took f for
    the row stride, or a float4 across the edge of a ragged tile, lands in sentinels);
  * every input frame is untouched;
  * where an entry point answers GCNX_ERR_UNSUPPORTED, that answer is asserted, with nothing written and ctx's last error
    unchanged.
One Gaussian case per route (aligned layout) is held to float64 at the project's bars (TIGHT, the bf16 bar against
bf16-rounded operands, TOL) through conftest.assert_close: these exercise the `lo` planes of bf16x3."""
import contextlib

import numpy as np
import pytest

import gemm_route_cases as G
from conftest import assert_close
from gpu_frames import Frame

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5                     # GCNX_ERR_UNSUPPORTED


@contextlib.contextmanager
def _knob(ctx, value):
    """gemm_stream for the length of one case; always back to its default (1)."""
    try:
        ctx.set_tuning("gemm_stream", value)
        yield
    finally:
        ctx.set_tuning("gemm_stream", 1)


def _frame(ctx, n, f, op, data=None, dtype=np.float32):
    fr = Frame(ctx, n, f, op.ld, op.lead, data, tail=n * (op.ld - f) + 64, dtype=dtype)
    assert (fr.view.ptr % 16 == 0) == G.al16(op) and fr.view.ld == op.ld           # the pointer the predicate was asked about
    return fr


def _arg(fr):
    return fr.row(0) if fr is not None else None


def _err(ctx):
    return ctx.lib.gcnx_last_error(ctx.h)


class _Call:
    """The frames of one call: inputs are checked untouched, outputs against the case's exact results."""

    def __init__(self, ctx, case, gauss):
        self.ctx, self.case, self.gauss, self.ins, self.outs = ctx, case, gauss, {}, {}
        self.ops = case.ops()

    def inp(self, name, n, f, data, op=None, dtype=np.float32):
        self.ins[name] = _frame(self.ctx, n, f, op or self.ops[name], data, dtype)
        return self.ins[name]

    def out(self, name, n, f, op=None, data=None, dtype=np.float32):
        self.outs[name] = _frame(self.ctx, n, f, op or self.ops[name], data, dtype)
        return self.outs[name]

    def check(self, want):
        assert set(want) == set(self.outs), (set(want), set(self.outs))
        for name, fr in self.outs.items():
            what = f"gemm route {self.case.entry} {self.case.route} {self.case.n}x{self.case.fi}x{self.case.fo} {self.case.prec} {name}"
            if self.gauss:
                assert_close(fr.numpy(), np.asarray(want[name], np.float64).reshape(fr.n, fr.f), G.GAUSS_TOL[self.case.prec], what)
            else:
                fr.check(want[name], (self.case.id, name))
        self.inputs_untouched()

    def inputs_untouched(self):
        for name, fr in self.ins.items():
            fr.untouched((self.case.id, name))

    def nothing_written(self, err_before):
        for name, fr in list(self.ins.items()) + list(self.outs.items()):
            fr.untouched((self.case.id, name, "written by a refused call"))
        assert _err(self.ctx) == err_before, "a refusal is an answer: the last error stays what it was"


# ------------------------------------------------------------------------------------------------ the entry points
def _run_gemm(ctx, c, k):
    from gcnx import device as D
    d, o = c.data(), c.opt
    x, w, out = k.inp("x", c.n, c.fi, d.x), k.inp("w", c.fi, c.fo, d.w), k.out("out", c.n, c.fo)
    bias = k.inp("bias", 1, c.fo, d.bias) if o.get("bias") else None
    alpha = k.inp("alpha", 1, c.fo, d.alpha, c.op("alpha", c.fo)) if o.get("act") == "prelu" else None
    D.gemm(ctx, x.view, w.view, _arg(bias), out.view, act=o.get("act"), prec=c.prec, alpha=_arg(alpha))
    k.check(c.expected())


def _run_dx(ctx, c, k):
    from gcnx import device as D
    d, o = c.data(), c.opt
    dh, w = k.inp("dh", c.n, c.fo, d.dh), k.inp("w", c.fi, c.fo, d.w)
    dx = k.out("dx", c.n, c.fi, data=d.base if o.get("accumulate") else None)
    y = k.inp("y", c.n, c.fi, d.y) if o.get("mask") else None
    db = k.out("db", 1, c.fi) if c.want_db() else None
    D.gemm_dx(ctx, dh.view, w.view, dx.view, prec=c.prec, accumulate=bool(o.get("accumulate")), y_mask=y.view if y else None, db=_arg(db))
    k.check(c.expected())


def _run_dw(ctx, c, k):
    from gcnx import device as D
    d = c.data()
    x, dh, dw = k.inp("x", c.n, c.fi, d.x), k.inp("dh", c.n, c.fo, d.dh), k.out("dw", c.fi, c.fo)
    D.gemm_dw(ctx, x.view, dh.view, dw.view, prec=c.prec)
    k.check(c.expected())


def _run_dense_bwd(ctx, c, k):
    from gcnx import device as D
    d, o = c.data(), c.opt
    x, dh, w = k.inp("x", c.n, c.fi, d.x), k.inp("dh", c.n, c.fo, d.dh), k.inp("w", c.fi, c.fo, d.w)
    y = k.inp("y", c.n, c.fi, d.y) if o.get("mask") else None
    dx, dw = k.out("dx", c.n, c.fi), k.out("dw", c.fi, c.fo)
    db = k.out("db", 1, c.fi) if c.want_db() else None
    D.dense_bwd(ctx, x.view, dh.view, w.view, dx.view, dw.view, prec=c.prec, y_mask=y.view if y else None, db_prev=_arg(db))
    k.check(c.expected())


def _run_dense_bwd_deferred(ctx, c, k):
    """dw and db are views into a flat gradient buffer; the pending record is finished by gcnx_gemm_dw_sgd, which forms the same
    X^T dH once more as the step's last gradient and applies params -= lr * grads (lr = 1/2: exact on integers)."""
    from gcnx import device as D
    d, o, lr = c.data(), c.opt, 0.5
    x, dh, w = k.inp("x", c.n, c.fi, d.x), k.inp("dh", c.n, c.fo, d.dh), k.inp("w", c.fi, c.fo, d.w)
    y = k.inp("y", c.n, c.fi, d.y) if o.get("mask") else None
    dx = k.out("dx", c.n, c.fi)
    total = c.fi * c.fo
    o_dw = 5 if c.layout("dw") == "off4" else 4
    o_db = (o_dw + total + 7) // 4 * 4
    o_last = o_db + c.fi + 4
    size = o_last + total + 4
    g0 = np.arange(size, dtype=np.float32) % 7 - 3                   # what the gaps hold: integers the update must still apply
    p0 = (np.arange(size, dtype=np.float32) % 5 - 2)
    grads = Frame(ctx, 1, size, size, 4, g0, tail=64)
    params = Frame(ctx, 1, size, size, 8, p0, tail=64)
    gv, pv = grads.row(0), params.row(0)
    dw, last = gv.flat(o_dw, total, (c.fi, c.fo)), gv.flat(o_last, total, (c.fi, c.fo))
    db = gv.flat(o_db, c.fi) if c.want_db() else None
    assert (dw.ptr % 16 == 0) == (c.layout("dw") != "off4") and (db is None or db.ptr % 16 == 0)
    scratch = ctx.empty(max(D.dense_bwd_scratch_floats(ctx, c.n, c.fi, c.fo), 4))
    pend = D.dense_bwd_deferred(ctx, x.view, dh.view, w.view, dx.view, dw, scratch, prec=c.prec, y_mask=y.view if y else None, db_prev=db)
    fused = c.route.startswith("duo")
    assert bool(pend.colpart) == (fused and c.want_db()) and bool(pend.slabs) == (c.route == "duo/splitk")
    D.gemm_dw_sgd(ctx, x.view, dh.view, last, pv, gv, lr, prec=c.prec, pending=pend)
    want = c.expected()
    k.check({"dx": want["dx"]})
    g = g0.copy()
    g[o_dw:o_dw + total] = want["dw"].ravel()
    g[o_last:o_last + total] = want["dw"].ravel()
    if c.want_db():
        g[o_db:o_db + c.fi] = want["db"]
    if k.gauss:
        assert_close(grads.numpy(), g, G.GAUSS_TOL[c.prec], f"gemm route {c.entry} {c.route} grads")
        return
    grads.check(g, (c.id, "grads"))
    params.check(p0 - np.float32(lr) * g, (c.id, "params"))


def _bits_frame(ctx, n, prec):
    """The image buffer.  include/gcnx.h reserves 64 bytes per row; the kernel writes 32 bytes per row and column half: the
    one-plane bf16 form has one half (32 bytes x n, the sentinels behind them must survive), bf16x3 two (all 64 bytes x n)."""
    words = 8 * n * (2 if prec == "bf16x3" else 1)
    fr = Frame(ctx, 1, words, words, 4, tail=16 * n - words + 64, dtype=np.int32)
    from gcnx.device import DeviceArray
    return fr, DeviceArray(ctx, fr.view.ptr, (16 * n,), np.int32, base=fr.buf)


def _run_bits_pair(ctx, c, k):
    """gcnx_gemm_relu_bits, then gcnx_gemm_dx_bits on its image: dX2 = dH2 W2^T * [out > 0] and db2, exactly.  The image is
    private to the pair: not decoded, only its frame is held."""
    from gcnx import device as D, _lib as L
    d, n = c.data(), c.n
    fwd_ok, bwd_ok = [r == "stream" for r in c.route.split("/")]
    x, w, bias, out = k.inp("x", n, c.fi, d.x), k.inp("w", c.fi, c.fo, d.w), k.inp("bias", 1, c.fo, d.bias), k.out("out", n, c.fo)
    bits, bits_arr = _bits_frame(ctx, n, c.prec)
    err = _err(ctx)
    assert D.gemm_relu_bits(ctx, x.view, w.view, _arg(bias), out.view, bits_arr, prec=c.prec) == fwd_ok
    want = c.expected()
    if fwd_ok:
        k.check({"out": want["out"]})
        bits.numpy()                                               # (asserts the sentinels around the image)
    else:
        k.nothing_written(err)
        bits.untouched((c.id, "bits"))
        al = G.Case("bits_pair", "", n, c.fi, c.fo, c.prec if c.prec != "f32" else "bf16", act="relu", bias=1)
        if G.relu_bits_ok(1, n, c.fi, c.fo, al.prec, al.ops()["x"], al.ops()["out"]):        # an image from an aligned forward
            ka = _Call(ctx, al, False)
            with _knob(ctx, 1):
                assert D.gemm_relu_bits(ctx, ka.inp("x", n, c.fi, d.x).view, ka.inp("w", c.fi, c.fo, d.w).view,
                                        _arg(ka.inp("bias", 1, c.fo, d.bias)), ka.out("out", n, c.fo).view, bits_arr, prec=al.prec)
            ctx.set_tuning("gemm_stream", c.knob)
    image_before = bits.buf.numpy()
    k2 = _Call(ctx, c, False)
    dh = k2.inp("dh", n, 256, d.dh2, G.place(256, c.layout("dh"), 1))
    w2 = k2.inp("w", c.fo, 256, d.w2)
    dx = k2.out("dx", n, 256, G.place(256, c.layout("dx"), 3))
    db = k2.out("db", 1, 256) if c.want_db() else None
    err = _err(ctx)
    rc = ctx.lib.gcnx_gemm_dx_bits(ctx.h, dh.view.ptr, dh.view.ld, w2.view.ptr, dx.view.ptr, dx.view.ld, n, 256, 256, L.PRECS[c.prec],
                                   bits.view.ptr, _arg(db).ptr if db else None)
    if bwd_ok:
        ctx._ck(rc)
        k2.check({kk: v for kk, v in want.items() if kk in ("dx", "db")})
    else:
        assert rc == UNSUPPORTED
        k2.nothing_written(err)
    assert np.array_equal(bits.buf.numpy(), image_before), "gcnx_gemm_dx_bits wrote its image"


def _run_pair16(ctx, c, k):
    """The same pair on the bf16-stored kernels: gcnx_gemm_fwd_bf16 writes the image of its (fp32 or bf16) ReLU rows,
    gcnx_gemm_dx_bf16 masks dX2 = dH2 W2^T with it and sums db2."""
    from gcnx import device as D
    d, n = c.data(), c.n
    odt = np.uint16 if c.opt.get("out16") else np.float32
    x, w, bias = k.inp("x", n, c.fi, _u16(d.x), dtype=np.uint16), k.inp("w", c.fi, c.fo, d.w), k.inp("bias", 1, c.fo, d.bias)
    out = k.out("out", n, c.fo, dtype=odt)
    bits, bits_arr = _bits_frame(ctx, n, "bf16")
    assert D.gemm_fwd_bf16(ctx, x.view, w.view, _arg(bias), out.view, act="relu", bits=bits_arr)
    want = c.expected()
    k.check({"out": want["out"]})
    image = bits.numpy()                                            # (asserts the sentinels behind 32 bytes x n)
    k2 = _Call(ctx, c, False)
    dh = k2.inp("dh", n, 256, _u16(d.dh2), G.place(256, c.layout("dh"), 1, 2), dtype=np.uint16)
    w2 = k2.inp("w", c.fo, 256, d.w2)
    dx = k2.out("dx", n, 256, G.place(256, c.layout("dx"), 3, np.dtype(odt).itemsize), dtype=odt)
    db = k2.out("db", 1, 256)
    assert D.gemm_dx_bf16(ctx, dh.view, w2.view, dx.view, mask_bits=bits_arr, db=_arg(db))
    k2.check({"dx": want["dx"], "db": want["db"]})
    assert np.array_equal(bits.numpy(), image)


def _u16(a):
    return G.bf16_bits(a)


def _run_16(ctx, c, k):
    """The bf16-stored streaming kernels: uint16 operand rows, fp32 or uint16 result rows; with the caller's weight image
    (gcnx_gemm_stream_images) and without, bit-identical."""
    from gcnx import device as D
    d, o, e = c.data(), c.opt, c.entry
    odt = np.uint16 if o.get("out16") else np.float32
    served = c.route == "stream16"
    err = _err(ctx)
    if e == "dw16":
        x, dh, dw = k.inp("x", c.n, c.fi, _u16(d.x), dtype=np.uint16), k.inp("dh", c.n, c.fo, _u16(d.dh), dtype=np.uint16), k.out("dw", c.fi, c.fo)
        assert D.gemm_dw_bf16(ctx, x.view, dh.view, dw.view) == served
        return k.check(c.expected()) if served else k.nothing_written(err)
    w = k.inp("w", c.fi, c.fo, d.w, G.place_flat(c.fo, "cont", 0))
    store = ctx.empty(65536, np.uint16)
    if e == "fwd16":
        a, out = k.inp("x", c.n, c.fi, _u16(d.x), dtype=np.uint16), k.out("out", c.n, c.fo, dtype=odt)
        bias = k.inp("bias", 1, c.fo, d.bias)
        call = lambda wimg: D.gemm_fwd_bf16(ctx, a.view, w.view, _arg(bias), out.view, act=o.get("act"), wimg=wimg)
    else:
        a, out = k.inp("dh", c.n, c.fo, _u16(d.dh), dtype=np.uint16), k.out("dx", c.n, c.fi, dtype=odt)
        db = k.out("db", 1, c.fi) if c.want_db() else None
        call = lambda wimg: D.gemm_dx_bf16(ctx, a.view, w.view, out.view, db=_arg(db), wimg=wimg)
    assert call(None) == served
    if not served:
        return k.nothing_written(err)
    k.check(c.expected())
    first = out.buf.numpy()
    img = D.stream_images(ctx, [(w.view, e == "fwd16")], store)[0]
    assert call(img)
    k.check(c.expected())
    assert np.array_equal(out.buf.numpy(), first)


def _run_wimage(ctx, c, k):
    from gcnx import device as D
    d, o = c.data(), c.opt
    tr = bool(o.get("transpose"))
    wdev = ctx.to_device(d.w)
    img = ctx.empty(max(D.wimage_elems(ctx, c.fi, c.fo, tr, c.prec), 8), np.uint16)
    D.wimage_prepare(ctx, [(wdev, img, tr, c.prec)])
    if tr:
        a, out = k.inp("dh", c.n, c.fo, d.dh), k.out("dx", c.n, c.fi, data=d.base if o.get("accumulate") else None)
    else:
        a, out = k.inp("x", c.n, c.fi, d.x), k.out("out", c.n, c.fo)
    bias = k.inp("bias", 1, c.fo, d.bias) if o.get("bias") else None
    nparts = D.gemm_wimage_parts(ctx, c.n) if o.get("bn") else 0
    parts = Frame(ctx, 1, 3 * nparts * c.fo, 3 * nparts * c.fo, 4, tail=3 * c.fo + 64) if nparts else None
    err = _err(ctx)
    got = D.gemm_wimage(ctx, a.view, img, c.fi, c.fo, out.view, transpose=tr, bias=_arg(bias), prec=c.prec, accumulate=bool(o.get("accumulate")),
                        bn_parts=_arg(parts))
    if c.route == "unsupported":
        assert got is None
        return k.nothing_written(err)
    assert got == nparts
    k.check(c.expected())
    assert np.array_equal(wdev.numpy(), d.w)
    if parts is not None:
        _check_bn_parts(c, parts.numpy().reshape(nparts, 3, c.fo), np.asarray(c.expected()["out"], np.float64))


def _check_bn_parts(c, parts, out):
    """bn_parts [nparts][3][fo] = (rows, mean, M2) per column and workgroup (include/gcnx.h): the row counts add up to n
    exactly; combined by Chan's formula in float64 they are the moments of the (exact) rows written, at TIGHT -- the parts
    are formed in fp32 whatever the precision of the product."""
    rows, mean, m2 = (parts[:, i].astype(np.float64) for i in range(3))
    assert np.array_equal(rows.sum(axis=0), np.full(c.fo, float(c.n))) and (rows >= 0).all()
    mean = np.where(rows > 0, mean, 0.0)
    tot = (rows * mean).sum(axis=0) / c.n
    var = (np.where(rows > 0, m2, 0.0).sum(axis=0) + (rows * (mean - tot) ** 2).sum(axis=0)) / c.n
    what = f"gemm route wimage bn_parts {c.n}x{c.fi}x{c.fo} {c.prec}"
    assert_close(tot, out.mean(axis=0), G.GAUSS_TOL["f32"], what + " mean")
    assert_close(var, out.var(axis=0), G.GAUSS_TOL["f32"], what + " variance")


RUN = {"gemm": _run_gemm, "dx": _run_dx, "dw": _run_dw, "dense_bwd": _run_dense_bwd, "dense_bwd_deferred": _run_dense_bwd_deferred,
       "bits_pair": _run_bits_pair, "pair16": _run_pair16, "fwd16": _run_16, "dx16": _run_16, "dw16": _run_16, "wimage": _run_wimage}


def _run(ctx, case, gauss=False):
    cus = ctx.info()["cus"]
    assert case.predicted(cus) == case.route, ("the dispatch, restated, does not send this case to its route on this chip", cus, case.predicted(cus))
    if not gauss:
        out, db = case.bounds()
        assert out < G.EXACT and db < G.EXACT
    with _knob(ctx, case.knob):
        RUN[case.entry](ctx, case, _Call(ctx, case, gauss))


def _select(entries, tall=None):
    sel = [c for c in G.CASES if c.entry in entries and (tall is None or (c.n >= G.TALL - 1) == tall)]
    return dict(argvalues=sel, ids=[c.id for c in sel])


@pytest.mark.parametrize("case", **_select(("gemm",), tall=False))
def test_gemm(ctx, case):
    """gcnx_gemm: gemm_f32_kernel<true, false> at every n-, K- and column-edge with va, vb and vec_c each broken alone, the
    row-tile kernel and each of its refusals, wprep_kernel + gemm_bf16_kernel<0> at both precisions."""
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("dx",), tall=False))
def test_gemm_dx(ctx, case):
    """gcnx_gemm_dx: the row-tile kernel (mask, accumulate, db through the partial rows) and its refusals, gemm_f32_kernel
    <true, true> with db fused or through gcnx_colsum, y_mask with +0.0 / -0.0 / negative entries, n = 0, the bf16 tiles."""
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("dw",), tall=False))
def test_gemm_dw(ctx, case):
    """gcnx_gemm_dw: gemm_f32_kernel<false, false> unsplit and split-K, gemm_bf16_kernel<1>, gcnx_gemm_dw_panels and its refusals."""
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("dense_bwd", "dense_bwd_deferred")))
def test_dense_bwd(ctx, case):
    """gcnx_dense_bwd / _deferred: the duo kernel, each clause of `fused` broken alone, the pending record through gcnx_gemm_dw_sgd."""
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("gemm", "dx", "dw"), tall=True))
def test_streaming_kernels(ctx, case):
    """gcnx_gemm_stream_nn through gcnx_gemm / gcnx_gemm_dx, the tall streamed dW, and each refusal onto the tile kernels."""
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("bits_pair",)))
def test_relu_bits_pair(ctx, case):
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("fwd16", "dx16", "dw16", "pair16")))
def test_bf16_stored_streaming_kernels(ctx, case):
    _run(ctx, case)


@pytest.mark.parametrize("case", **_select(("wimage",)))
def test_gemm_wimage(ctx, case):
    _run(ctx, case)


@pytest.mark.parametrize("case", G.gaussian_cases(), ids=lambda c: c.id)
def test_gaussian(ctx, case):
    """One Gaussian case per route against float64 at TIGHT (f32), 2e-5 against bf16-rounded operands (bf16), TOL (bf16x3)."""
    _run(ctx, case, gauss=True)

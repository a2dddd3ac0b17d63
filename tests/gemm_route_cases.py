"""The dense weight GEMMs (csrc/gemm.hip, gemm_stream.hip, gemm_panel.hip) route by route: the case table, the seeded
small-integer operands, the exact references and a Python restatement of every dispatch predicate.  No GPU import:
tests/test_gemm_route_cases_host.py pins the table on the host, tests/test_gpu_gemm_routes.py runs it on the device.

Why bit-exact: with integers in [-3, 3] every product and every partial sum of every route is an integer below 2^24, so the
f32 MFMA chains, the bf16 planes (the integers are bf16 numbers, the `lo` planes of bf16x3 are zero), a PReLU with a
power-of-two slope, the column sums and the split-K slabs are all exact in any order: each route must produce the float32
bit patterns of the exact product.  The condition -- for every output element the sum of the ABSOLUTE values of its terms
stays below 2^24 -- is a property of the operands alone (abs_bound below).

Layouts of a matrix operand, as (ld, lead) inside a flat sentinel buffer (tests/gpu_frames.py):
  cont   a fresh allocation (ld = f, lead = 0)
  al     a column slice: ld > f, ld % 4 == 0, lead % 4 == 0, a different ld for every operand slot of the call
  up     the pointer one float off a 16-byte boundary (lead % 4 == 1), ld % 4 == 0
  uld    ld % 4 == 1, pointer aligned
  ld8    (bf16-stored rows only) ld % 8 == 4: passes an fp32-style `ld % 4` check, fails gcnx_gemm_stream_bf16's `lda % 8`
Vectors (bias, alpha, db) and w / dw have no leading dimension: `al` (16-byte aligned inside the buffer) or `off4` (4 bytes off).
"""
from collections import namedtuple

import numpy as np

EXACT = float(1 << 24)
TALL = 32 * 1024                     # the streaming kernels' smallest batch (gemm_stream.hip: m >= 32 * 1024)
BM = BN = 64                         # gemm.hip: the f32 tile
BK = 32
HM = HN = 128                        # gemm.hip: the bf16 tile
HK = 32
K_MIN_SLICE_STEPS = 10               # gemm.hip: kMinSliceSteps


# ------------------------------------------------------------------------------------------------ layouts
Op = namedtuple("Op", "ld lead item")          # an operand as the dispatch sees it: leading dimension, offset, element bytes


def place(f, layout, slot, item=4):
    """(ld, lead) of an [n, f] operand in `layout`; `slot` (0, 1, 2 ...) makes every operand's ld and lead differ."""
    per16 = 16 // item
    fr = -(-f // per16) * per16
    if layout == "cont":
        return Op(f, 0, item)
    ld, lead = fr + per16 * (2 + slot), per16 * (1 + slot)
    if layout == "al":
        return Op(ld, lead, item)
    if layout == "up":
        return Op(ld, lead + 4 // item, item)            # 4 bytes off
    if layout == "uld":
        assert item == 4
        return Op(ld + 1, lead, item)
    if layout == "ld8":
        assert item == 2
        return Op(ld + 4, lead, item)
    raise KeyError(layout)


def place_flat(f, layout, slot):
    """A contiguous vector / weight matrix (row length f) inside a flat buffer: aligned, or 4 bytes off."""
    return Op(f, {"cont": 0, "al": 4 * (1 + slot), "off4": 4 * (1 + slot) + 1}[layout], 4)


def al16(op):
    """gcnx_aligned16 of the operand's pointer (the buffer itself is at least 16-byte aligned)."""
    return op is None or op.lead * op.item % 16 == 0


def vec_ok(op):
    """`gcnx_aligned16(p) && ld % 4 == 0`: va / vb / vec_c of gemm.hip."""
    return al16(op) and op.ld % 4 == 0


# ------------------------------------------------------------------------------------------------ dispatch, restated
def cdiv(a, b):
    return -(-a // b)


def split_rows(want, n, kstep, min_steps):
    """gcnx_split_rows (common.h) -> (nsplit, kchunk)."""
    ksteps = cdiv(n, kstep)
    nsplit = min(int(want), ksteps // min_steps)
    nsplit = max(nsplit, 1)
    kchunk = cdiv(ksteps, nsplit) * kstep
    return cdiv(n, kchunk), kchunk


def splitk_fill(cus, tiles):
    """splitk_fill (gemm.hip)."""
    return (4 * cus + tiles - 1) // tiles


def dw_tiles(fi, fo):
    """dw_tiles (gemm.hip)."""
    return cdiv(fi, BM) * cdiv(fo, BN)


def fits_buffer(rows, ld, item):
    """gcnx_fits_buffer (common.h)."""
    return rows * ld * item < 0xFFFFFF00


def rowtile_ok(knob, m, k, nc, a):
    """rowtile_ok (gemm.hip)."""
    return bool(knob and m >= 2048 and k in (16, 32, 64, 128, 256) and 192 <= nc <= 256 and nc % 16 == 0 and vec_ok(a))


def stream_nn(knob, m, K, ncol, a, c, mask=None, accumulate=False, colsum=None, bits=False):
    """gcnx_gemm_stream_nn (gemm_stream.hip): True when it launches, False for GCNX_ERR_UNSUPPORTED."""
    if bits and (ncol != 256 or not fits_buffer(m, 64, 1)):
        return False
    if accumulate or not knob:
        return False
    shape_ok = (K == 256 and ncol % 4 == 0 and 64 <= ncol <= 256 and m >= TALL and vec_ok(a) and vec_ok(c) and
                fits_buffer(m, a.ld, 4) and fits_buffer(m, c.ld, 4) and (mask is None or (vec_ok(mask) and fits_buffer(m, mask.ld, 4))))
    if not shape_ok:
        return False
    return colsum is None or (ncol % 4 == 0 and al16(colsum))


def bf16_nn(knob, m, K, ncol, a, c, vec_c, mask=None, accumulate=False, colsum=None):
    """launch_bf16_nn (gemm.hip) -> (kernel, colsum_done).  ep.colpart is never set by its callers."""
    if vec_c:
        if stream_nn(knob, m, K, ncol, a, c, mask, accumulate, colsum):
            return "stream", colsum is not None
        if colsum is not None and stream_nn(knob, m, K, ncol, a, c, mask, accumulate, None):
            return "stream", False                                   # the second attempt, without the sums
    return "bf16_tile", False


def route_gemm(cus, knob, n, fi, fo, prec, x, out):
    """gcnx_gemm."""
    vec_c = vec_ok(out)
    if prec != "f32":
        return bf16_nn(knob, n, fi, fo, x, out, vec_c)[0]
    return "rowtile" if rowtile_ok(knob, n, fi, fo, x) else "tile_f32"


def route_dx(cus, knob, n, fi, fo, prec, dh, dx, y=None, db=None, accumulate=False, want_db=False):
    """gcnx_gemm_dx -> "kernel" or "kernel+how db is formed"."""
    if n == 0 or fi == 0:
        return "memset" if (want_db and fi > 0) else "nothing"
    vec_c = vec_ok(dx) and (y is None or vec_ok(y))
    if prec != "f32":
        kern, done = bf16_nn(knob, n, fo, fi, dh, dx, vec_c, y, accumulate, db if want_db else None)
        return kern + ("" if not want_db else "+sums" if done else "+colsum")
    if rowtile_ok(knob, n, fo, fi, dh) and (not want_db or al16(db)):
        return "rowtile" + ("+partials" if want_db else "")
    if not want_db:
        return "tile_f32"
    return "tile_f32+fused_db" if (vec_c and fi % BN == 0) else "tile_f32+colsum"


def dw_stream_operands_ok(x, dh, n):
    """dw_stream_operands_ok (gemm_stream.hip)."""
    per16 = 16 // x.item
    return x.ld % per16 == 0 and dh.ld % per16 == 0 and al16(x) and al16(dh) and fits_buffer(n, x.ld, x.item) and fits_buffer(n, dh.ld, dh.item)


def route_dw(cus, knob, n, fi, fo, prec, x, dh, dw):
    """gcnx_gemm_dw (with gcnx_gemm_dw_stream / gcnx_gemm_dw_panels of gemm_stream.hip) -> "kernel/1" (no split) or
    "kernel/splitk"."""
    if n == 0:
        return "memset"
    if prec != "f32":
        if fi == 256 and fo == 256 and n >= TALL and knob and dw_stream_operands_ok(x, dh, n):
            return "stream_tall"
        if n < TALL or fi != 256:
            if knob and fo == 256 and fi % 256 == 0 and 256 <= fi <= 2048 and n >= 2048 and dw_stream_operands_ok(x, dh, n) and al16(dw):
                return "panels"
        ns = split_rows(splitk_fill(cus, cdiv(fi, HM) * cdiv(fo, HN)), n, HK, 1)[0]
        return "bf16_tile/" + ("1" if ns == 1 else "splitk")
    ns = split_rows(splitk_fill(cus, dw_tiles(fi, fo)), n, BK, K_MIN_SLICE_STEPS)[0]
    return "tile_f32/" + ("1" if ns == 1 else "splitk")


def dense_bwd_split(cus, n, fi, fo):
    """dense_bwd_split (gemm.hip) -> nsplit."""
    n_dx = cdiv(n, BM) * (fi // BN)
    slots = 4 * cus
    spare = slots - n_dx % slots
    if spare < slots // 4:
        spare += slots
    return split_rows(spare // dw_tiles(fi, fo), n, BK, K_MIN_SLICE_STEPS)[0]


def route_dense_bwd(cus, knob, n, fi, fo, prec, dx, y=None, db=None):
    """dense_bwd_impl's `fused` (gemm.hip): the duo kernel, or the two separate calls."""
    gy = cdiv(n, BM)
    fused = (prec == "f32" and n > 0 and fi > 0 and fo > 0 and fi % BN == 0 and vec_ok(dx) and (y is None or vec_ok(y)) and fo % 4 == 0 and
             (db is None or (al16(db) and 2 * gy <= 4096)) and gy * (fi // BN) < (1 << 30))
    if not fused:
        return "two_calls"
    return "duo/" + ("1" if dense_bwd_split(cus, n, fi, fo) == 1 else "splitk")


def relu_bits_ok(knob, n, fi, fo, prec, x, out):
    """gcnx_gemm_relu_bits: True when the streaming kernel runs, False for GCNX_ERR_UNSUPPORTED."""
    if prec == "f32" or fo != 256 or not vec_ok(out):
        return False
    return stream_nn(knob, n, fi, fo, x, out, bits=True)


def dx_bits_ok(knob, n, fi, fo, prec, dh, dx, db=None):
    """gcnx_gemm_dx_bits."""
    if prec == "f32" or fi != 256 or not vec_ok(dx) or not al16(db):
        return False
    return stream_nn(knob, n, fo, fi, dh, dx, colsum=db, bits=True)


def stream_bf16_ok(knob, m, K, ncol, a16, c, c_item, colsum=None):
    """gcnx_gemm_stream_bf16 (gemm_stream.hip)."""
    if not knob or K != 256 or ncol != 256 or m < TALL:
        return False
    if a16.ld % 8 or c.ld % 4 or not al16(a16) or not al16(c) or not fits_buffer(m, a16.ld, 2) or not fits_buffer(m, c.ld, c_item):
        return False
    return al16(colsum)


def fwd_bf16_ok(knob, n, fi, fo, x16, out, bias=None):
    """gcnx_gemm_fwd_bf16."""
    if fi != 256 or fo != 256 or not al16(bias):
        return False
    return stream_bf16_ok(knob, n, fi, fo, x16, out, out.item)


def dx_bf16_ok(knob, n, fi, fo, dh16, dx, db=None):
    """gcnx_gemm_dx_bf16."""
    if fi != 256 or fo != 256:
        return False
    return stream_bf16_ok(knob, n, fo, fi, dh16, dx, dx.item, db)


def dw_bf16_ok(knob, n, fi, fo, x16, dh16, dw):
    """gcnx_gemm_dw_bf16 (with gcnx_gemm_dw_stream16)."""
    if fi != 256 or fo != 256 or n < TALL or not knob or not al16(dw):
        return False
    return dw_stream_operands_ok(x16, dh16, n)


def wimage_ok(n, fi, fo, transpose, x):
    """gcnx_gemm_wimage (gemm_panel.hip); the image itself is a fresh allocation."""
    K, nc = (fo, fi) if transpose else (fi, fo)
    return nc % 16 == 0 and K % 4 == 0 and vec_ok(x) and fits_buffer(n, x.ld, 4)


# ------------------------------------------------------------------------------------------------ operands and references
def bf16_round(x):
    """Round-to-nearest-even fp32 -> bf16 -> fp32 (the rounding of _bf16_round in tests/test_gpu_kernels.py)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_bits(x):
    """The same rounding as uint16 patterns (a bf16 result row)."""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def bf16_ties(z):
    """How many elements of z lie exactly half way between two bf16 numbers (the low 16 bits are 0x8000)."""
    return int(((np.ascontiguousarray(z, np.float32).view(np.uint32) & 0xFFFF) == 0x8000).sum())


def ints(rng, shape, lim=3, keep=1.0):
    """Integers in [-lim, lim] as float32; keep < 1: that share survives, the rest are zeros."""
    a = rng.integers(-lim, lim + 1, size=shape).astype(np.float32)
    if keep < 1.0:
        a *= rng.random(shape) < keep
    return a + np.float32(0)                                        # (no -0.0 from the multiplication)


def zero_grid(x, w, bias):
    """Exact zeros in x w + bias at every shape: rows i % 4 == 1 of x, columns j % 4 == 2 of w and every even entry of bias
    are zeroed, so (zero row or zero column) x (zero bias) is exactly 0 whatever K is."""
    x, w, bias = x.copy(), w.copy(), bias.copy()
    x[1::4] = 0
    w[:, 2::4] = 0
    bias[0::2] = 0
    return x, w, bias


def mask_source(rng, shape):
    """A saved activation for [y > 0]: positive, negative, +0.0 and -0.0 entries."""
    y = ints(rng, shape)
    flat = y.reshape(-1)
    z = np.flatnonzero(flat == 0)
    flat[z[::2]] = np.float32(-0.0)
    if flat.size >= 16:                                             # every kind is there whatever the draw
        flat[:4] = np.array([0.0, -0.0, -2.0, 1.0], np.float32)
    return y


def f64(a):
    return np.asarray(a, np.float64)


def forward_ref(x, w, bias=None, act=None, alpha=None):
    """(z, out): the float64 pre-activation and the exact float32 result of gcnx_gemm."""
    z = f64(x) @ f64(w)
    if bias is not None:
        z = z + f64(bias)
    out = z
    if act == "relu":
        out = np.maximum(z, 0.0)
    elif act == "prelu":
        out = np.where(z > 0, z, f64(alpha) * z)
    return z, out.astype(np.float32)


def dx_ref(dh, w, y=None, base=None):
    """dH W^T (* [y > 0]) (+ base) as float32, and its column sums."""
    d = f64(dh) @ f64(w).T
    if y is not None:
        d = np.where(np.asarray(y) > 0, d, 0.0)
    if base is not None:
        d = d + f64(base)
    return d.astype(np.float32), d.sum(axis=0).astype(np.float32)


def dw_ref(x, dh):
    return (f64(x).T @ f64(dh)).astype(np.float32)


def abs_bound(a, b):
    """max over the output elements of sum |terms| of a @ b, and the largest column sum of that (the bound of db)."""
    p = np.abs(f64(a)) @ np.abs(f64(b))
    return (float(p.max()), float(p.sum(axis=0).max())) if p.size else (0.0, 0.0)


# ------------------------------------------------------------------------------------------------ the case table
class Case:
    """One call: entry point, the route it must take at any CU count, shape, precision, layout per operand and options.
    lay: operand name -> layout (matrices default to "al", vectors and weights to "al"); opt: act / bias / mask /
    accumulate / db / knob (gemm_stream) / vals ("i3": [-3, 3], "i1": {-1, 0, 1} with a share of zeros) / deferred ..."""

    def __init__(self, entry, route, n, fi, fo, prec="f32", lay=None, **opt):
        self.entry, self.route, self.n, self.fi, self.fo, self.prec = entry, route, n, fi, fo, prec
        self.lay = dict(lay or {})
        self.opt = opt
        self.knob = opt.get("knob", 1)

    def layout(self, name):
        return self.lay.get(name, "al")

    @property
    def id(self):
        lay = ",".join(f"{k}={v}" for k, v in sorted(self.lay.items())) or "al"
        opt = ",".join(f"{k}={v}" for k, v in sorted(self.opt.items()))
        return f"{self.entry}-{self.route}-{self.n}x{self.fi}x{self.fo}-{self.prec}-{lay}" + (f"-{opt}" if opt else "")

    def __repr__(self):
        return self.id

    # operand slots: every operand of a call gets its own ld / lead
    SLOTS = {"x": 0, "dh": 1, "out": 2, "dx": 2, "y": 3, "w": 0, "dw": 1, "bias": 2, "alpha": 3, "db": 4}

    def op(self, name, f, item=4):
        if name in ("w", "dw", "bias", "alpha", "db"):
            return place_flat(f, self.layout(name), self.SLOTS[name])
        return place(f, self.layout(name), self.SLOTS[name], item)

    def want_db(self):
        return bool(self.opt.get("db"))

    def ops(self):
        """The operands the dispatch looks at, by name."""
        n, fi, fo, o = self.n, self.fi, self.fo, self.opt
        item_in = 2 if self.entry in ("fwd16", "dx16", "dw16", "pair16") else 4
        d = {"x": self.op("x", fi, item_in), "dh": self.op("dh", fo, item_in), "w": self.op("w", fo), "dw": self.op("dw", fo),
             "out": self.op("out", fo, 2 if o.get("out16") else 4), "dx": self.op("dx", fi, 2 if o.get("out16") else 4),
             "y": self.op("y", fi) if o.get("mask") else None, "db": self.op("db", fi) if self.want_db() else None,
             "bias": self.op("bias", fo) if o.get("bias") else None}
        return d

    def predicted(self, cus):
        """The route the restated dispatch gives at `cus` compute units."""
        n, fi, fo, p, k, o = self.n, self.fi, self.fo, self.prec, self.knob, self.ops()
        e = self.entry
        if e == "gemm":
            return route_gemm(cus, k, n, fi, fo, p, o["x"], o["out"])
        if e == "dx":
            return route_dx(cus, k, n, fi, fo, p, o["dh"], o["dx"], o["y"], o["db"], bool(self.opt.get("accumulate")), self.want_db())
        if e == "dw":
            return route_dw(cus, k, n, fi, fo, p, o["x"], o["dh"], o["dw"])
        if e in ("dense_bwd", "dense_bwd_deferred"):
            r = route_dense_bwd(cus, k, n, fi, fo, p, o["dx"], o["y"], o["db"])
            if r != "two_calls":
                return r
            return "two_calls:" + route_dx(cus, k, n, fi, fo, p, o["dh"], o["dx"], o["y"], o["db"], False, self.want_db()) + ":" + \
                route_dw(cus, k, n, fi, fo, p, o["x"], o["dh"], o["dw"])
        if e == "bits_pair":                                        # gcnx_gemm_relu_bits, then gcnx_gemm_dx_bits on its image
            fwd = relu_bits_ok(k, n, fi, fo, p, o["x"], o["out"])
            # the backward product of the pair is dH [n, fi'] W2^T with fi' = fo of the forward: a 256 x 256 second weight
            bwd = dx_bits_ok(k, n, 256, 256, p, place(256, self.layout("dh"), 1), place(256, self.layout("dx"), 3), o["db"] if self.want_db() else None)
            return ("stream" if fwd else "unsupported") + "/" + ("stream" if bwd else "unsupported")
        if e == "pair16":                                           # gcnx_gemm_fwd_bf16 (relu_bits), then gcnx_gemm_dx_bf16 (mask_bits)
            item = 2 if self.opt.get("out16") else 4
            fwd = fwd_bf16_ok(k, n, fi, fo, o["x"], o["out"], o["bias"])
            bwd = dx_bf16_ok(k, n, 256, 256, place(256, self.layout("dh"), 1, 2), place(256, self.layout("dx"), 3, item), o["db"])
            return ("stream16" if fwd else "unsupported") + "/" + ("stream16" if bwd else "unsupported")
        if e == "fwd16":
            return "stream16" if fwd_bf16_ok(k, n, fi, fo, o["x"], o["out"], o["bias"]) else "unsupported"
        if e == "dx16":
            return "stream16" if dx_bf16_ok(k, n, fi, fo, o["dh"], o["dx"], o["db"]) else "unsupported"
        if e == "dw16":
            return "stream16" if dw_bf16_ok(k, n, fi, fo, o["x"], o["dh"], o["dw"]) else "unsupported"
        if e == "wimage":
            tr = bool(self.opt.get("transpose"))
            return "panel" if wimage_ok(n, fi, fo, tr, o["dh"] if tr else o["x"]) else "unsupported"
        raise KeyError(e)

    def vals(self):
        return self.opt.get("vals", "i3")

    def data(self):
        """The host operands of the call and its exact results (Data), shared by every case of the same shape and values."""
        return data_of(self.n, self.fi, self.fo, self.vals(), self.prec if self.vals() == "gauss" else "")

    def expected(self):
        """What the call must leave in each frame it writes, by operand name: float32 arrays (uint16 patterns for bf16 result
        rows).  The pair's "dx" / "db" are those of gcnx_gemm_dx_bits on the image of its "out"."""
        d, o, e = self.data(), self.opt, self.entry
        tr, want = bool(o.get("transpose")), {}
        rows = bf16_bits if o.get("out16") else (lambda a: a)
        if e in ("gemm", "fwd16", "bits_pair", "pair16") or (e == "wimage" and not tr):
            want["out"] = rows(d.fwd(o.get("bias"), o.get("act"))[1])
        if e in ("dx", "dx16", "dense_bwd", "dense_bwd_deferred") or (e == "wimage" and tr):
            dx, db = d.dx(o.get("mask"), o.get("accumulate"))
            want["dx"] = rows(dx)
            if self.want_db():
                want["db"] = db
        if e in ("dw", "dw16", "dense_bwd", "dense_bwd_deferred"):
            want["dw"] = d.dw()
        if e in ("bits_pair", "pair16"):
            dx, db = d.dx2()
            want["dx"] = rows(dx)
            if self.want_db():
                want["db"] = db
        return want

    def bounds(self):
        """(largest sum of |terms| of any output element, largest such sum of any db element) over every product the case forms."""
        d, e, o = self.data(), self.entry, self.opt
        b = [(0.0, 0.0)]
        if e in ("gemm", "fwd16", "bits_pair", "pair16") or (e == "wimage" and not o.get("transpose")):
            p, _ = d.bound("fwd")
            b.append((p + (float(np.abs(d.bias).max()) if o.get("bias") else 0.0), 0.0))
        if e in ("dx", "dx16", "dense_bwd", "dense_bwd_deferred") or (e == "wimage" and o.get("transpose")):
            p, c = d.bound("dx")
            b.append((p + (3.0 if o.get("accumulate") else 0.0), c if self.want_db() else 0.0))
        if e in ("dw", "dw16", "dense_bwd", "dense_bwd_deferred"):
            b.append((d.bound("dw")[0], 0.0))
        if e in ("bits_pair", "pair16"):
            p, c = d.bound("dx2")
            b.append((p, c if self.want_db() else 0.0))
        return max(x[0] for x in b), max(x[1] for x in b)


class Data:
    """Operands and references of one (n, fi, fo, values): x [n, fi], dh [n, fo], w [fi, fo], bias / alpha [fo], y / base
    [n, fi] and, for the bit-image pair, w2 [fo, 256] / dh2 [n, 256].  Every operand has its own seeded stream and every
    reference is computed on first use, once.  Integer operands always carry zero_grid's zeros.  Gaussian operands at "bf16" are
    held to the product of their bf16-rounded values (the project's bf16 bar)."""

    def __init__(self, n, fi, fo, vals, prec):
        self.n, self.fi, self.fo, self.vals, self.prec = n, fi, fo, vals, prec
        self._memo = {}
        x, w, bias = self._draw(0, (n, fi)), self._draw(1, (fi, fo)), self._draw(2, (fo,), vec=True)
        if vals != "gauss":
            x, w, bias = zero_grid(x, w, bias)
        self.x, self.w, self.bias = x, w, bias
        self.alpha = np.array([0.25, 0.5, 2.0, 0.125], np.float32)[np.arange(fo) % 4]     # powers of two: one exact multiply

    def _draw(self, k, shape, vec=False):
        rng = np.random.default_rng([self.n, self.fi, self.fo, {"i3": 3, "i1": 1, "gauss": 7}[self.vals], k])
        if self.vals == "gauss":
            return rng.standard_normal(shape, dtype=np.float32)
        return ints(rng, shape) if (self.vals == "i3" or vec) else ints(rng, shape, 1, 0.5)

    def _get(self, name, make):
        if name not in self._memo:
            self._memo[name] = make()
        return self._memo[name]

    dh = property(lambda s: s._get("dh", lambda: s._draw(3, (s.n, s.fo))))
    base = property(lambda s: s._get("base", lambda: s._draw(5, (s.n, s.fi))))
    w2 = property(lambda s: s._get("w2", lambda: s._draw(6, (s.fo, 256))))
    dh2 = property(lambda s: s._get("dh2", lambda: s._draw(7, (s.n, 256))))

    @property
    def y(self):
        def make():
            rng = np.random.default_rng([self.n, self.fi, self.fo, 4])
            return rng.standard_normal((self.n, self.fi), dtype=np.float32) if self.vals == "gauss" else mask_source(rng, (self.n, self.fi))
        return self._get("y", make)

    def _r(self, a):
        return bf16_round(a) if (self.vals == "gauss" and self.prec == "bf16") else a

    def fwd(self, bias=False, act=None):
        """(z, out) of gcnx_gemm: float64 pre-activation, float32 result."""
        return self._get(("fwd", bool(bias), act), lambda: forward_ref(self._r(self.x), self._r(self.w), self.bias if bias else None, act, self.alpha))

    def dx(self, mask=False, accumulate=False):
        """(dX, db) of gcnx_gemm_dx."""
        return self._get(("dx", bool(mask), bool(accumulate)),
                         lambda: dx_ref(self._r(self.dh), self._r(self.w), self.y if mask else None, self.base if accumulate else None))

    def dw(self):
        return self._get("dw", lambda: dw_ref(self._r(self.x), self._r(self.dh)))

    def dx2(self, masked=True):
        """(dX2, db2) of the pair: dH2 W2^T * [relu(x w + bias) > 0]."""
        return self._get(("dx2", masked), lambda: dx_ref(self.dh2, self.w2, self.fwd(True, "relu")[1] if masked else None))

    def bound(self, which):
        a, b = {"fwd": lambda: (self.x, self.w), "dx": lambda: (self.dh, self.w.T), "dw": lambda: (self.x.T, self.dh),
                "dx2": lambda: (self.dh2, self.w2.T)}[which]()
        return self._get(("bound", which), lambda: abs_bound(a, b))


_DATA = {}
_BIG = 1 << 22            # operands of more than 4M elements: only the two latest such sets are kept


def data_of(n, fi, fo, vals, prec=""):
    key = (n, fi, fo, vals, prec)
    if key not in _DATA:
        if n * max(fi, fo) > _BIG:
            for k in [k for k in _DATA if k[0] * max(k[1], k[2]) > _BIG][:-1]:
                del _DATA[k]
        _DATA[key] = Data(n, fi, fo, vals, prec)
    _DATA[key] = _DATA.pop(key)                                     # (latest use last)
    return _DATA[key]


def C(*a, **k):
    return Case(*a, **k)


def _cases():
    t = []
    # ---- gcnx_gemm, f32, gemm_f32_kernel<true, false>: every n-, K- and column-edge with va, vb, vec_c each 0 and 1
    edge = [(1, 1, 2), (63, 31, 63), (64, 32, 64), (65, 33, 65), (129, 67, 130), (129, 64, 1), (1, 67, 130), (64, 1, 64), (65, 32, 2)]
    for n, fi, fo in edge:
        t.append(C("gemm", "tile_f32", n, fi, fo))                                              # va = vb = vec_c = 1 (fo % 4 == 0)
        t.append(C("gemm", "tile_f32", n, fi, fo, lay={"x": "up"}))                               # va alone
        t.append(C("gemm", "tile_f32", n, fi, fo, lay={"x": "uld"}))
        t.append(C("gemm", "tile_f32", n, fi, fo, lay={"w": "off4"}))                             # vb alone
        t.append(C("gemm", "tile_f32", n, fi, fo, lay={"out": "up"}))                             # vec_c alone
        t.append(C("gemm", "tile_f32", n, fi, fo, lay={"out": "uld"}))
    for n, fi, fo in [(63, 31, 63), (64, 32, 64), (129, 67, 130), (65, 33, 65), (1, 67, 130), (129, 64, 1)]:
        for act in ("relu", "prelu"):
            for lay in ({}, {"x": "cont", "out": "cont", "w": "cont", "bias": "cont", "alpha": "cont"}, {"out": "up"}, {"bias": "off4"}, {"alpha": "off4"}):
                if act == "relu" and "alpha" in lay and len(lay) == 1:
                    continue
                t.append(C("gemm", "tile_f32", n, fi, fo, lay=lay, act=act, bias=1))
    t.append(C("gemm", "tile_f32", 129, 67, 130, lay={"x": "cont", "out": "cont", "w": "cont"}))
    # ---- f32 row-tile kernel through gcnx_gemm (K = fi, columns = fo) and its refusals onto the tile kernel
    for n, k, nc in [(2048, 16, 192), (2049, 256, 256), (2049, 16, 256), (2048, 256, 192)]:
        t.append(C("gemm", "rowtile", n, k, nc, act="relu", bias=1))
        t.append(C("gemm", "rowtile", n, k, nc, lay={"out": "uld", "bias": "off4"}, act="prelu", bias=1))   # only A's alignment is consulted
    t.append(C("gemm", "rowtile", 2049, 64, 208))
    for lay, kw in [({"x": "uld"}, {}), ({"x": "up"}, {}), ({}, {"knob": 0})]:
        t.append(C("gemm", "tile_f32", 2049, 16, 192, lay=lay, act="relu", bias=1, **kw))
    t.append(C("gemm", "tile_f32", 2047, 16, 192, act="relu", bias=1))
    t.append(C("gemm", "tile_f32", 2048, 16, 176, act="relu", bias=1))
    t.append(C("gemm", "tile_f32", 2048, 16, 272, act="relu", bias=1))
    t.append(C("gemm", "tile_f32", 2048, 48, 192))                                                # K not in the list
    # ---- row-tile through gcnx_gemm_dx (K = fo, columns = fi): mask, accumulate, db through the partial rows
    for n, fi, fo in [(2048, 192, 16), (2049, 256, 256), (2049, 192, 256)]:
        t.append(C("dx", "rowtile+partials", n, fi, fo, mask=1, db=1))
        t.append(C("dx", "rowtile", n, fi, fo, accumulate=1))
        t.append(C("dx", "rowtile+partials", n, fi, fo, lay={"dx": "uld", "y": "up"}, mask=1, db=1))
    t.append(C("dx", "tile_f32+fused_db", 2049, 192, 16, lay={"db": "off4"}, mask=1, db=1))         # unaligned db alone (dX only)
    t.append(C("dx", "tile_f32+fused_db", 2049, 192, 16, lay={"dh": "uld"}, mask=1, db=1))
    t.append(C("dx", "tile_f32+fused_db", 2049, 192, 16, lay={"dh": "up"}, mask=1, db=1))
    t.append(C("dx", "tile_f32+fused_db", 2049, 192, 16, mask=1, db=1, knob=0))
    t.append(C("dx", "tile_f32+fused_db", 2047, 192, 16, mask=1, db=1))
    t.append(C("dx", "tile_f32+colsum", 2048, 176, 16, mask=1, db=1))
    t.append(C("dx", "tile_f32+colsum", 2048, 272, 16, mask=1, db=1))
    # ---- gcnx_gemm_dx, f32 tile kernel gemm_f32_kernel<true, true>: the two db forms, mask, accumulate, n = 0
    for n, fi, fo in [(65, 64, 33), (129, 128, 6), (1, 64, 67)]:
        t.append(C("dx", "tile_f32+fused_db", n, fi, fo, mask=1, db=1))
        t.append(C("dx", "tile_f32+fused_db", n, fi, fo, db=1))
        t.append(C("dx", "tile_f32+fused_db", n, fi, fo, lay={"dh": "up", "w": "off4", "db": "off4"}, mask=1, db=1))   # db's alignment is not consulted
        t.append(C("dx", "tile_f32+colsum", n, fi, fo, lay={"dx": "up"}, mask=1, db=1))
        t.append(C("dx", "tile_f32+colsum", n, fi, fo, lay={"dx": "uld"}, mask=1, db=1))
        t.append(C("dx", "tile_f32+colsum", n, fi, fo, lay={"y": "up"}, mask=1, db=1))
        t.append(C("dx", "tile_f32+colsum", n, fi, fo, lay={"y": "uld"}, mask=1, db=1))
    for n, fi, fo in [(63, 31, 63), (65, 65, 32), (129, 130, 67), (64, 1, 64), (1, 2, 1)]:
        m = int(n * fi >= 16)                                                                       # (a mask has four kinds of entries)
        t.append(C("dx", "tile_f32+colsum", n, fi, fo, mask=m, db=1))                               # ragged fi
        t.append(C("dx", "tile_f32", n, fi, fo, mask=m))
        t.append(C("dx", "tile_f32", n, fi, fo, accumulate=1))
        t.append(C("dx", "tile_f32", n, fi, fo, lay={"dx": "up"}, accumulate=1))
        t.append(C("dx", "tile_f32", n, fi, fo, lay={"dh": "uld", "dx": "cont"}))
    t.append(C("dx", "memset", 0, 64, 33, db=1))
    t.append(C("dx", "memset", 0, 31, 8, lay={"db": "off4"}, db=1))
    # ---- gcnx_gemm_dw, f32: nsplit 1 below 2 x 320 rows, > 1 from there; x / dh are va / vb of dw_job; dw aligned and 4 bytes off
    for n in (1, 33, 319, 640, 1000):
        r = "tile_f32/" + ("1" if n < 640 else "splitk")
        for fi, fo in [(64, 64), (67, 130), (33, 6), (65, 3)]:
            t.append(C("dw", r, n, fi, fo))
            t.append(C("dw", r, n, fi, fo, lay={"dw": "off4"}))
        t.append(C("dw", r, n, 67, 130, lay={"x": "up"}))
        t.append(C("dw", r, n, 67, 130, lay={"x": "uld"}))
        t.append(C("dw", r, n, 67, 130, lay={"dh": "up"}))
        t.append(C("dw", r, n, 67, 130, lay={"dh": "uld"}))
        t.append(C("dw", r, n, 64, 64, lay={"x": "cont", "dh": "cont", "dw": "cont"}))
    # ---- gcnx_dense_bwd / _deferred: the duo kernel (nsplit 1 and > 1) and each clause of `fused` broken alone
    for entry in ("dense_bwd", "dense_bwd_deferred"):
        for n, r in [(300, "duo/1"), (1000, "duo/splitk")]:
            t.append(C(entry, r, n, 64, 8, mask=1, db=1))
            t.append(C(entry, r, n, 128, 36, lay={"x": "uld", "dh": "up", "dw": "off4"}, mask=1, db=1))    # va / vb of both jobs: no clause of `fused`
            t.append(C(entry, r, n, 64, 8))
    dwr = {300: "tile_f32/1", 1000: "tile_f32/splitk"}
    for n in (300, 1000):
        t.append(C("dense_bwd", "two_calls:tile_f32+colsum:" + dwr[n], n, 65, 8, mask=1, db=1))              # ragged fi
        t.append(C("dense_bwd", "two_calls:tile_f32+fused_db:" + dwr[n], n, 64, 6, mask=1, db=1))            # fo % 4 != 0
        t.append(C("dense_bwd", "two_calls:tile_f32+colsum:" + dwr[n], n, 64, 8, lay={"dx": "up"}, mask=1, db=1))
        t.append(C("dense_bwd", "two_calls:tile_f32+colsum:" + dwr[n], n, 64, 8, lay={"dx": "uld"}, mask=1, db=1))
        t.append(C("dense_bwd", "two_calls:tile_f32+colsum:" + dwr[n], n, 64, 8, lay={"y": "up"}, mask=1, db=1))
        t.append(C("dense_bwd", "two_calls:tile_f32+colsum:" + dwr[n], n, 64, 8, lay={"y": "uld"}, mask=1, db=1))
        t.append(C("dense_bwd", "two_calls:tile_f32+fused_db:" + dwr[n], n, 64, 8, lay={"db": "off4"}, mask=1, db=1))
    t.append(C("dense_bwd_deferred", "two_calls:tile_f32+colsum:tile_f32/splitk", 1000, 65, 8, mask=1, db=1))
    # ---- bf16 / bf16x3 tile kernels: wprep_kernel + gemm_bf16_kernel<0> (X W, dH W^T), gemm_bf16_kernel<1> + split-K reduce (dW)
    for prec in ("bf16", "bf16x3"):
        for n, fi, fo in [(1, 1, 2), (63, 31, 63), (129, 67, 130), (128, 32, 128), (257, 33, 129), (65, 64, 1)]:
            t.append(C("gemm", "bf16_tile", n, fi, fo, prec))
            t.append(C("gemm", "bf16_tile", n, fi, fo, prec, lay={"x": "up", "out": "uld"}))
            if n > 1:
                t.append(C("gemm", "bf16_tile", n, fi, fo, prec, act="relu", bias=1))
                t.append(C("gemm", "bf16_tile", n, fi, fo, prec, lay={"x": "uld", "bias": "off4", "out": "up"}, act="prelu", bias=1))
            m = int(n * fi >= 16)
            t.append(C("dx", "bf16_tile+colsum", n, fi, fo, prec, mask=m, db=1))
            t.append(C("dx", "bf16_tile+colsum", n, fi, fo, prec, lay={"dh": "up", "dx": "uld", "y": "up", "db": "off4"}, mask=m, db=1))
            t.append(C("dx", "bf16_tile", n, fi, fo, prec, accumulate=1))
        for n in (1, 33, 1000):
            r = "bf16_tile/" + ("1" if n <= 32 else "splitk")
            for fi, fo in [(67, 130), (128, 128), (129, 6)]:
                t.append(C("dw", r, n, fi, fo, prec))
                t.append(C("dw", r, n, fi, fo, prec, lay={"x": "up", "dh": "uld", "dw": "off4"}))
        # ---- gcnx_gemm_dw_panels and its refusals onto gemm_bf16_kernel<1>
        for n, fi in [(2048, 256), (2049, 512), (2049, 256)]:
            t.append(C("dw", "panels", n, fi, 256, prec))
        t.append(C("dw", "panels", 2049, 256, 256, prec, lay={"x": "cont", "dh": "cont", "dw": "cont"}))
        t.append(C("dw", "bf16_tile/splitk", 2047, 256, 256, prec))
        for lay in ({"x": "up"}, {"x": "uld"}, {"dh": "up"}, {"dh": "uld"}, {"dw": "off4"}):
            t.append(C("dw", "bf16_tile/splitk", 2049, 256, 256, prec, lay=lay))
        t.append(C("dw", "bf16_tile/splitk", 2049, 256, 256, prec, knob=0))
    # ---- the streaming kernel gcnx_gemm_stream_nn through gcnx_gemm / gcnx_gemm_dx / the bit-image pair (tall: {-1, 0, 1})
    for prec in ("bf16", "bf16x3"):
        for n, nc in [(TALL, 64), (TALL + 1, 256), (TALL + 1, 192)]:
            t.append(C("gemm", "stream", n, 256, nc, prec, act="relu", bias=1, vals="i1"))
            t.append(C("dx", "stream+sums", n, nc, 256, prec, mask=1, db=1, vals="i1"))
        t.append(C("gemm", "stream", TALL + 1, 256, 256, prec, lay={"bias": "off4"}, act="relu", bias=1, vals="i1"))
        cont = {k: "cont" for k in ("x", "dh", "w", "out", "dx", "y", "bias", "db")}
        t.append(C("gemm", "stream", TALL + 1, 256, 256, prec, lay=cont, act="relu", bias=1, vals="i1"))
        t.append(C("dx", "stream+sums", TALL + 1, 256, 256, prec, lay=cont, mask=1, db=1, vals="i1"))
        t.append(C("gemm", "stream", TALL + 1, 256, 256, prec, lay={"alpha": "off4"}, act="prelu", bias=1, vals="i1"))
        t.append(C("gemm", "bf16_tile", TALL - 1, 256, 256, prec, act="relu", bias=1, vals="i1"))
        for lay, kw in [({"x": "up"}, {}), ({"x": "uld"}, {}), ({"out": "up"}, {}), ({"out": "uld"}, {}), ({}, {"knob": 0})]:
            t.append(C("gemm", "bf16_tile", TALL + 1, 256, 256, prec, lay=lay, act="relu", bias=1, vals="i1", **kw))
        t.append(C("dx", "stream+colsum", TALL + 1, 256, 256, prec, lay={"db": "off4"}, mask=1, db=1, vals="i1"))   # the retry without the sums
        t.append(C("dx", "bf16_tile", TALL + 1, 256, 256, prec, accumulate=1, vals="i1"))
        t.append(C("dx", "bf16_tile+colsum", TALL - 1, 256, 256, prec, mask=1, db=1, vals="i1"))
        for lay, kw in [({"dh": "up"}, {}), ({"dx": "up"}, {}), ({"y": "up"}, {}), ({"y": "uld"}, {}), ({}, {"knob": 0})]:
            t.append(C("dx", "bf16_tile+colsum", TALL + 1, 256, 256, prec, lay=lay, mask=1, db=1, vals="i1", **kw))
        t.append(C("dw", "stream_tall", TALL + 1, 256, 256, prec, vals="i1"))
        t.append(C("dw", "stream_tall", TALL + 1, 256, 256, prec, lay={"dw": "off4"}, vals="i1"))     # the narrow reduction kernel
        t.append(C("dw", "bf16_tile/splitk", TALL + 1, 256, 256, prec, lay={"x": "up"}, vals="i1"))
        t.append(C("dw", "bf16_tile/splitk", TALL + 1, 256, 256, prec, lay={"dh": "uld"}, vals="i1"))
        # the pair gcnx_gemm_relu_bits -> gcnx_gemm_dx_bits (the image is private to the pair: held through dX and db)
        for n in (TALL, TALL + 1):
            t.append(C("bits_pair", "stream/stream", n, 256, 256, prec, act="relu", bias=1, db=1, vals="i1"))
        t.append(C("bits_pair", "stream/stream", TALL + 1, 256, 256, prec, lay={"bias": "off4"}, act="relu", bias=1, vals="i1"))
        for lay in ({"out": "up"}, {"out": "uld"}, {"x": "up"}, {"x": "uld"}):
            t.append(C("bits_pair", "unsupported/stream", TALL + 1, 256, 256, prec, lay=lay, act="relu", bias=1, db=1, vals="i1"))
        for lay in ({"dx": "up"}, {"dx": "uld"}, {"dh": "up"}, {"db": "off4"}):
            t.append(C("bits_pair", "stream/unsupported", TALL + 1, 256, 256, prec, lay=lay, act="relu", bias=1, db=1, vals="i1"))
        t.append(C("bits_pair", "unsupported/unsupported", TALL + 1, 256, 256, prec, act="relu", bias=1, db=1, vals="i1", knob=0))
        t.append(C("bits_pair", "unsupported/unsupported", TALL - 1, 256, 256, prec, act="relu", bias=1, db=1, vals="i1"))
    t.append(C("bits_pair", "unsupported/unsupported", TALL + 1, 256, 256, "f32", act="relu", bias=1, db=1, vals="i1"))
    # ---- the bf16-stored streaming kernels (uint16 rows): fp32 and bf16 result rows, with and without the caller's image
    for n in (TALL, TALL + 1):
        for out16 in (0, 1):
            t.append(C("fwd16", "stream16", n, 256, 256, "bf16", act="relu", bias=1, out16=out16))
            t.append(C("dx16", "stream16", n, 256, 256, "bf16", out16=out16))                      # [-3, 3]: ties in the bf16 rows
            t.append(C("dx16", "stream16", n, 256, 256, "bf16", db=1, out16=out16, vals="i1"))       # |dX| <= 256: db of exact rows
        t.append(C("dw16", "stream16", n, 256, 256, "bf16"))
        t.append(C("dw16", "stream16", n, 256, 256, "bf16", lay={"x": "cont", "dh": "cont", "dw": "cont"}))
        t.append(C("fwd16", "stream16", n, 256, 256, "bf16", lay={"x": "cont", "out": "cont", "bias": "cont"}, act="relu", bias=1, out16=1))
        for out16 in (0, 1):                                          # the family's own bit image: forward -> masked dX and db
            t.append(C("pair16", "stream16/stream16", n, 256, 256, "bf16", act="relu", bias=1, db=1, out16=out16, vals="i1"))
    for out16 in (0, 1):
        for lay in ({"x": "ld8"}, {"x": "up"}, {"out": "up"}, {"bias": "off4"}):
            t.append(C("fwd16", "unsupported", TALL + 1, 256, 256, "bf16", lay=lay, act="relu", bias=1, out16=out16))
        for lay in ({"dh": "ld8"}, {"dh": "up"}, {"dx": "up"}, {"db": "off4"}):
            t.append(C("dx16", "unsupported", TALL + 1, 256, 256, "bf16", lay=lay, db=1, out16=out16, vals="i1"))
    t.append(C("fwd16", "unsupported", TALL + 1, 256, 256, "bf16", lay={"out": "uld"}, act="relu", bias=1, out16=0))
    t.append(C("fwd16", "unsupported", TALL - 1, 256, 256, "bf16", act="relu", bias=1, out16=1))
    t.append(C("fwd16", "unsupported", TALL + 1, 256, 256, "bf16", act="relu", bias=1, out16=1, knob=0))
    t.append(C("dx16", "unsupported", TALL - 1, 256, 256, "bf16", out16=1))
    for lay in ({"x": "ld8"}, {"dh": "ld8"}, {"x": "up"}, {"dh": "up"}, {"dw": "off4"}):
        t.append(C("dw16", "unsupported", TALL + 1, 256, 256, "bf16", lay=lay))
    t.append(C("dw16", "unsupported", TALL - 1, 256, 256, "bf16"))
    t.append(C("dw16", "unsupported", TALL + 1, 256, 256, "bf16", knob=0))
    # ---- gcnx_gemm_wimage (panel kernels): forward with bias, transposed, transposed with accumulate
    for prec in ("bf16", "bf16x3"):
        for n in (1, 33, 2049):
            t.append(C("wimage", "panel", n, 68, 48, prec, bias=1))                                 # K = 68, columns = 48
            t.append(C("wimage", "panel", n, 64, 36, prec, transpose=1))                            # K = 36, columns = 64
            t.append(C("wimage", "panel", n, 64, 36, prec, transpose=1, accumulate=1))
        for n, fi, fo in [(33, 68, 48), (2049, 68, 48), (2049, 260, 256)]:                          # bn_parts: one column panel
            t.append(C("wimage", "panel", n, fi, fo, prec, bias=1, bn=1))
        t.append(C("wimage", "panel", 2049, 260, 320, prec, bias=1))                                # two column panels, K past one K panel
        t.append(C("wimage", "panel", 33, 32, 512, prec, bias=1))                                   # the wide kernel (short K, > 256 columns)
        t.append(C("wimage", "unsupported", 33, 67, 48, prec, bias=1))                              # K % 4
        t.append(C("wimage", "unsupported", 33, 68, 40, prec, bias=1))                              # columns % 16
        t.append(C("wimage", "unsupported", 33, 68, 48, prec, lay={"x": "up"}, bias=1))
        t.append(C("wimage", "unsupported", 33, 68, 48, prec, lay={"x": "uld"}, bias=1))
    return t


CASES = _cases()


def gaussian_cases():
    """One Gaussian case per route in the aligned layout, against float64 at the project's bars: these exercise the `lo`
    planes of bf16x3, which the integers leave empty."""
    t = [C("gemm", "tile_f32", 129, 67, 130, act="prelu", bias=1, vals="gauss"),
         C("gemm", "rowtile", 2049, 256, 256, act="relu", bias=1, vals="gauss"),
         C("dx", "rowtile+partials", 2049, 256, 256, mask=1, db=1, vals="gauss"),
         C("dx", "tile_f32+fused_db", 129, 128, 67, mask=1, db=1, vals="gauss"),
         C("dx", "tile_f32+colsum", 129, 130, 67, mask=1, db=1, vals="gauss"),
         C("dw", "tile_f32/1", 319, 67, 130, vals="gauss"), C("dw", "tile_f32/splitk", 1000, 67, 130, vals="gauss"),
         C("dense_bwd", "duo/splitk", 1000, 128, 36, mask=1, db=1, vals="gauss")]
    for prec in ("bf16", "bf16x3"):
        t += [C("gemm", "bf16_tile", 257, 33, 129, prec, act="relu", bias=1, vals="gauss"),
              C("dx", "bf16_tile+colsum", 257, 33, 129, prec, mask=1, db=1, vals="gauss"),
              C("dw", "bf16_tile/splitk", 1000, 67, 130, prec, vals="gauss"),
              C("dw", "panels", 2049, 512, 256, prec, vals="gauss"),
              C("gemm", "stream", TALL + 1, 256, 256, prec, act="relu", bias=1, vals="gauss"),
              C("dx", "stream+sums", TALL + 1, 256, 256, prec, mask=1, db=1, vals="gauss"),
              C("dw", "stream_tall", TALL + 1, 256, 256, prec, vals="gauss"),
              C("wimage", "panel", 2049, 260, 320, prec, bias=1, vals="gauss")]
    t += [C("fwd16", "stream16", TALL + 1, 256, 256, "bf16", act="relu", bias=1, out16=0, vals="gauss"),
          C("dx16", "stream16", TALL + 1, 256, 256, "bf16", db=1, out16=0, vals="gauss"),
          C("dw16", "stream16", TALL + 1, 256, 256, "bf16", vals="gauss")]
    return t


GAUSS_TOL = {"f32": 2e-5, "bf16": 2e-5, "bf16x3": 1e-4}      # TIGHT, the bf16 bar against bf16-rounded operands, TOL

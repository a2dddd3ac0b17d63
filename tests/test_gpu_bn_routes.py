"""Every launch route of the plain BatchNorm entry points of csrc/bn.hip -- gcnx_bn_stats, gcnx_bn_finalize, gcnx_bn_moments,
gcnx_bn_act, gcnx_bn_act_bwd, gcnx_bn_act_bwd_stats, gcnx_bn_act_bwd_apply -- on strided views inside sentinel frames, against
tests/bn_ref.py.

A call picks its code path from the alignment of its operands, the width modulo 4, 64 and 256, the row count against 256 and
the row count against the chip's CU count.  CASES names, per shape, the path it is there for; every case asserts through
bn_ref.route(...) on its own shape that it reaches that path (shapes that depend on the chip are derived from
cus = ctx.info()["cus"]), so a later change of a threshold fails loudly instead of quietly doubling another case.

Each case runs in three layouts: (a) dense, (b) a view with an aligned base and ld = f + pad, ld % 4 == 0 (float4 loads with a
scalar 1-3 column tail when f % 4 != 0), (c) a view 1 or 3 elements into its buffer with an odd ld (everything scalar).  Outputs
live in frames of sentinels and must leave them intact; inputs must come back untouched; the in-place backward (dz over dy,
as the models call it) is checked as an output.  The three layouts must agree bit for bit in every output: neither the
arithmetic nor the summation order depends on the alignment.

Inputs are bn_ref.exact_data: every product and every partial column sum is exact in fp32, so the sums of gcnx_bn_stats (with
and without a shift), y of gcnx_bn_act, the three backward column sums with dbeta / dgamma / dalpha (the shared slope's single
value included) and the inference-mode dz must equal the float64 reference BIT FOR BIT -- a dropped, doubled or misplaced
row, a lost tail column or a chunk group that reads a chunk too many is a wrong integer.  mean / inv / the moving
statistics and the training-mode dz are rounded on the way: those meet float64 at TIGHT, and the identities the header
promises hold bit for bit in every layout: gcnx_bn_moments == stats + finalize taken twice, gcnx_bn_act_bwd == _stats +
_apply with count = n.  One Gaussian run per entry point (large mean for the moments, pre-activations on both sides of zero
for the backward) keeps the centred variance and the PReLU branches covered by numbers that do round.

What each case is there for (vec = layouts with aligned operands; the unaligned layout of every case is the scalar path):
  1x1, 7x3             small one-launch kernels; a lone scalar tail lane (1 and 3 columns); every chunk group but the first empty
  256x64               the top of the small range; one full fast tile
  7x66, 256x67         small kernels: a fast tile + a 2- / 3-column tail (float4 + tail in layout (b))
  1x256                one full apply tile, tail loop, a single row
  256x200              no full apply tile; three fast column-sum tiles + two generic float4 lanes
  7x260                a full apply tile + a partial one of one float4
  257x66, 257x256      two chunks: groups 2 and 3 empty
  513x67, 513x260,     three chunks: group 3 empty
  700x258, 700x3       ... 258: a partial apply tile with a 2-column tail
  1025x200, 1025x1     five chunks: per = 2, group 2 cut short by min(nchunks, .), group 3 empty
  1281x66              six chunks (cdiv(1281, 256) = 6, not 5): per = 2, group 3 empty, none cut short
  2049x64, 2049x67     nine chunks: per = 3, group 3 empty
  2305x200             ten chunks (cdiv(2305, 256) = 10, not 9): per = 3, no group empty, group 3 cut short to one chunk
  (step + 1)x256       step = 32 cus: the first two-row iteration that has a second row; the other threads take the tail loop
  (2 step)x260         an exact fit: the full tile never enters the tail loop; the partial tile does
  (2 step + 5)x256     the tail loop behind the two-row loop
  (3 step + 1)x260     two two-row iterations for row 0, one + a tail row for the rest; the partial tile next to it"""
from collections import namedtuple

import numpy as np
import pytest

import bn_ref as R
from conftest import rel_err
from gpu_frames import SENTINEL, Frame, same

pytestmark = pytest.mark.gpu

TIGHT = 2e-5                       # as tests/test_gpu_kernels.py holds these calls to
F32 = np.float32
MM0, MV0 = 0.5, 2.0                # the moving statistics before the update

# n: a row count, or (a, b) for a step + b rows with step = 32 cus (the rows one pass of the apply grid covers).
# small: nchunks == 1.  chunks: (nchunks, empty groups, short group) of the chunk reduction, None where it depends on the chip.
# lanes / loops / alanes: the column-sum lanes, the apply kernel's loops and its tail-loop lanes WITH aligned operands (without:
# "scalar", "tail", "scalar").
Case = namedtuple("Case", "n f act small chunks lanes loops exact_fit alanes")
_S, _F4, _T, _FAST = "scalar", "float4", "tail", "fast"


def _case(n, f, act, small, chunks, lanes, loops="tail", alanes=(_F4,), exact_fit=False):
    return Case(n, f, act, small, chunks, frozenset(lanes), loops, exact_fit, frozenset(alanes))


CASES = [
    _case(1, 1, None, True, (1, (1, 2, 3), None), [_T], alanes=[_T]),
    _case(7, 3, "relu", True, (1, (1, 2, 3), None), [_T], alanes=[_T]),
    _case(256, 64, "prelu", True, (1, (1, 2, 3), None), [_FAST]),
    _case(7, 66, "prelu_shared", True, (1, (1, 2, 3), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(256, 67, "prelu", True, (1, (1, 2, 3), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(1, 256, "prelu_shared", True, (1, (1, 2, 3), None), [_FAST]),
    _case(256, 200, "relu", True, (1, (1, 2, 3), None), [_FAST, _F4]),
    _case(7, 260, "prelu", True, (1, (1, 2, 3), None), [_FAST, _F4]),
    _case(257, 66, "prelu", False, (2, (2, 3), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(257, 256, None, False, (2, (2, 3), None), [_FAST]),
    _case(513, 67, "prelu_shared", False, (3, (3,), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(513, 260, "prelu_shared", False, (3, (3,), None), [_FAST, _F4]),
    _case(700, 258, "relu", False, (3, (3,), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(700, 3, "prelu", False, (3, (3,), None), [_T], alanes=[_T]),
    _case(1025, 200, "prelu", False, (5, (3,), 2), [_FAST, _F4]),
    _case(1025, 1, None, False, (5, (3,), 2), [_T], alanes=[_T]),
    _case(1281, 66, "prelu", False, (6, (3,), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(2049, 64, "prelu_shared", False, (9, (3,), None), [_FAST]),
    _case(2049, 67, "relu", False, (9, (3,), None), [_FAST, _T], alanes=[_F4, _T]),
    _case(2305, 200, None, False, (10, (), 3), [_FAST, _F4]),
    _case((1, 1), 256, "prelu", False, None, [_FAST], loops="two_row"),
    _case((2, 0), 260, "relu", False, None, [_FAST, _F4], loops="two_row,tail", exact_fit=True),
    _case((2, 5), 256, "prelu_shared", False, None, [_FAST], loops="two_row+tail"),
    _case((3, 1), 260, None, False, None, [_FAST, _F4], loops="two_row+tail,tail"),
]


def case_id(c):
    n = c.n if isinstance(c.n, int) else "%dstep+%d" % c.n
    return "%sx%d-%s" % (n, c.f, c.act or "none")


def rows(c, cus):
    return c.n if isinstance(c.n, int) else c.n[0] * 32 * cus + c.n[1]


def claim(c, kind, vec, cus):
    """The route of `kind` on this case's shape is the one the table names; returns the record."""
    n = rows(c, cus)
    r = R.route(kind, n, c.f, vec, cus)
    what = (case_id(c), kind, vec, cus, r)
    assert r["vec"] == vec, what
    if kind == "finalize":
        assert r["launch"] == "elementwise", what
        return r
    if r["lanes"] is not None:
        assert r["lanes"] == (c.lanes if vec else frozenset([_S])), what
    if kind in ("moments", "bn_act_bwd"):
        assert (r["launch"] == "small") == c.small, what
    if kind in ("stats", "bwd_stats"):
        assert r["launch"] == "chunked", what
    if r["launch"] == "chunked" and c.chunks is not None:
        assert (r["nchunks"], r["empty"], r["short"]) == c.chunks, what
    if r["launch"] == "small":
        assert r["apply"] is None and r["nchunks"] is None, what
    else:
        assert (r["apply"] is not None) == (kind in ("bn_act", "bn_act_bwd", "bwd_apply")), what
    if r["apply"] is not None:
        a = r["apply"]
        assert a["loops"] == (c.loops if vec else "tail"), what
        assert a["exact_fit"] == (vec and c.exact_fit), what
        assert a["lanes"] == (c.alanes if vec else frozenset([_S])), what
        if not isinstance(c.n, int):
            assert a["step"] == 32 * cus and n > a["step"], what
    return r


def layouts(f):
    """(name, ld, lead): (a) dense; (b) an aligned base and ld % 4 == 0 with padding; (c) 1 or 3 elements in, an odd ld."""
    return [("dense", f, 0), ("aligned view", (f + 3) // 4 * 4 + 8, 4), ("unaligned view", (f | 1) + 2, 1 if f % 2 else 3)]


def _vector(ctx, size, data=None, lead=3):
    """A contiguous [size] device vector inside a frame (lead = 3: nothing here may assume an aligned vector)."""
    return Frame(ctx, 1, size, size, lead, None if data is None else np.asarray(data, F32))


def _f32(a):
    return np.asarray(a, np.float64).astype(F32)


def _params(ctx, d, act):
    dev = {k: ctx.to_device(d[k]) for k in ("mean", "inv", "gamma", "beta", "shift")}
    al = R.alpha_of(d, act)
    dev["alpha"] = None if al is None else ctx.to_device(al)
    return dev


def _same_across(outs):
    names = [k for k in outs[0] if k != "layout"]
    for o in outs[1:]:
        for k in names:
            assert same(np.asarray(o[k]), np.asarray(outs[0][k])), (k, o["layout"], "differs from", outs[0]["layout"])


# ------------------------------------------------------------------------------------------- forward
def _forward(ctx, c, n, d, p, layout, cus):
    from gcnx import device as D
    name, ld, lead = layout
    f = c.f
    zf = Frame(ctx, n, f, ld, lead, d["z"])
    vec = zf.aligned()
    assert vec == (name == "aligned view" or (name == "dense" and f % 4 == 0))
    for kind in ("stats", "finalize", "moments", "bn_act"):
        claim(c, kind, vec, cus)
    out = {"layout": name}
    s = _vector(ctx, 2 * f)
    D.bn_stats(ctx, zf.view, s.row(0))
    out["sums"] = s.numpy()[0]
    s = _vector(ctx, 2 * f)
    D.bn_stats(ctx, zf.view, s.row(0), shift=p["shift"])
    out["sums_shift"] = s.numpy()[0]
    # moments in one call, then as the pairs the header says it equals; the second finalize has mean aliasing shift
    one = [_vector(ctx, f), _vector(ctx, f), _vector(ctx, f, np.full(f, MM0)), _vector(ctx, f, np.full(f, MV0))]
    D.bn_moments(ctx, zf.view, None, *[v.row(0) for v in one])
    two = [_vector(ctx, f), _vector(ctx, f), _vector(ctx, f, np.full(f, MM0)), _vector(ctx, f, np.full(f, MV0))]
    m2, i2, mm2, mv2 = [v.row(0) for v in two]
    s = _vector(ctx, 2 * f)
    D.bn_stats(ctx, zf.view, s.row(0))
    D.bn_finalize(ctx, s.row(0), n, m2, i2)
    D.bn_stats(ctx, zf.view, s.row(0), shift=m2)
    D.bn_finalize(ctx, s.row(0), n, m2, i2, mm2, mv2, shift=m2)
    s.numpy()
    for k, a, b in zip(("mean", "inv", "moving_mean", "moving_var"), one, two):
        out[k] = a.numpy()[0]
        assert same(out[k], b.numpy()[0]), (name, k, "gcnx_bn_moments != stats + finalize twice")
    y = Frame(ctx, n, f, ld, lead)
    assert y.aligned() == vec
    D.bn_act(ctx, zf.view, p["mean"], p["inv"], p["gamma"], p["beta"], y.view, act=c.act, alpha=p["alpha"])
    out["y"] = y.numpy()
    zf.untouched(name)
    return out


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forward_routes(ctx, c):
    """gcnx_bn_stats (with and without a shift), gcnx_bn_moments and its stats + finalize pairs, gcnx_bn_act."""
    cus = ctx.info()["cus"]
    n, f = rows(c, cus), c.f
    d = R.exact_data(n, f, 1000 + CASES.index(c))
    assert 16 * n * 8 < 2 ** 24                                   # |z - shift| <= 4: every partial sum is exact
    p = _params(ctx, d, c.act)
    outs = [_forward(ctx, c, n, d, p, layout, cus) for layout in layouts(f)]
    _same_across(outs)
    o = outs[0]
    assert same(o["sums"], _f32(R.stats(d["z"]).ravel())), "sums"
    assert same(o["sums_shift"], _f32(R.stats(d["z"], d["shift"]).ravel())), "sums with a shift"
    assert same(o["y"], _f32(R.bn_act(d["z"], d["mean"], d["inv"], d["gamma"], d["beta"], c.act, R.alpha_of(d, c.act)))), "y"
    want = R.moments(d["z"], np.full(f, MM0), np.full(f, MV0))
    for k, w in zip(("mean", "inv", "moving_mean", "moving_var"), want):
        assert rel_err(o[k], w) < TIGHT, k


# ------------------------------------------------------------------------------------------- backward
def _backward(ctx, c, n, d, p, layout, training, cus):
    from gcnx import device as D
    name, ld, lead = layout
    f, act = c.f, c.act
    zf = Frame(ctx, n, f, ld, lead, d["z"])
    vec = zf.aligned()
    for kind in ("bn_act_bwd", "bwd_stats", "bwd_apply"):
        claim(c, kind, vec, cus)
    na = {"prelu": f, "prelu_shared": 1}.get(act)
    runs = []
    for one_call in (True, False):
        in_place = one_call == training                            # the one call in place when training, the halves otherwise
        src = Frame(ctx, n, f, ld, lead, d["dy"])
        dz = src if in_place else Frame(ctx, n, f, ld, lead)
        sums, dg, db = _vector(ctx, 3 * f), _vector(ctx, f), _vector(ctx, f)
        da = _vector(ctx, na) if na else None
        grads = dict(dgamma=dg.row(0), dbeta=db.row(0), dalpha=da.row(0) if da else None)
        args = (p["mean"], p["inv"], p["gamma"], p["beta"])
        if one_call:
            D.bn_act_bwd(ctx, src.view, zf.view, *args, dz.view, sums.row(0), act=act, alpha=p["alpha"], training=training, **grads)
        else:
            D.bn_act_bwd_stats(ctx, src.view, zf.view, *args, sums.row(0), act=act, alpha=p["alpha"], **grads)
            D.bn_act_bwd_apply(ctx, src.view, zf.view, *args, sums.row(0), n, dz.view, act=act, alpha=p["alpha"], training=training)
        r = {"layout": name, "dz": dz.numpy(), "sums": sums.numpy()[0], "dgamma": dg.numpy()[0], "dbeta": db.numpy()[0]}
        if da:
            r["dalpha"] = da.numpy()[0]
        if not in_place:
            src.untouched((name, "dy"))
        runs.append(r)
    zf.untouched((name, "z"))
    for k in runs[0]:
        if k != "layout":
            assert same(runs[0][k], runs[1][k]), (name, k, "gcnx_bn_act_bwd != _stats + _apply")
    return runs[0]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_backward_routes(ctx, c):
    """gcnx_bn_act_bwd and its halves gcnx_bn_act_bwd_stats + gcnx_bn_act_bwd_apply (count = n), one of the two in place."""
    cus = ctx.info()["cus"]
    n, f = rows(c, cus), c.f
    d = R.exact_data(n, f, 2000 + CASES.index(c))
    R.assert_exact(d, c.act)
    p = _params(ctx, d, c.act)
    for training in (True, False):
        outs = [_backward(ctx, c, n, d, p, layout, training, cus) for layout in layouts(f)]
        _same_across(outs)
        o = outs[0]
        w = R.bn_act_bwd(d["dy"], d["z"], d["mean"], d["inv"], d["gamma"], d["beta"], c.act, R.alpha_of(d, c.act), training)
        assert same(o["sums"], _f32(w["sums"].ravel())), "the three column sums"
        assert same(o["dbeta"], _f32(w["dbeta"])) and same(o["dgamma"], _f32(w["dgamma"])), "dbeta / dgamma"
        if w["dalpha"] is not None:
            assert same(o["dalpha"], _f32(w["dalpha"])), "dalpha"
        if training:
            assert rel_err(o["dz"], w["dz"]) < TIGHT, "dz"
        else:
            assert R.is_f32(w["dz"]) and same(o["dz"], _f32(w["dz"])), "dz (inference)"


# ------------------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("f", [1, 3, 64, 67, 256, 260])
def test_finalize_modes(ctx, f):
    """gcnx_bn_finalize: training with and without the moving buffers, with mean aliasing shift (the same bits as without
    the alias), and inference (sums == NULL): mean is the moving mean, the moving buffers are left alone."""
    from gcnx import device as D
    n = 700
    d = R.exact_data(n, f, 3000 + f)
    sums = R.stats(d["z"], d["shift"])
    assert R.is_f32(sums)
    sd, shift = ctx.to_device(_f32(sums.ravel())), ctx.to_device(d["shift"])
    # no moving buffers, no shift
    mean, inv = _vector(ctx, f), _vector(ctx, f)
    D.bn_finalize(ctx, sd, n, mean.row(0), inv.row(0))
    w = R.finalize(sums, n)
    assert rel_err(mean.numpy()[0], w[0]) < TIGHT and rel_err(inv.numpy()[0], w[1]) < TIGHT
    # moving buffers and a shift; mean apart from shift, then aliasing it
    got = []
    for alias in (False, True):
        mean, inv = _vector(ctx, f, d["shift"]), _vector(ctx, f)
        mm, mv = _vector(ctx, f, np.full(f, MM0)), _vector(ctx, f, np.full(f, MV0))
        D.bn_finalize(ctx, sd, n, mean.row(0), inv.row(0), mm.row(0), mv.row(0), shift=mean.row(0) if alias else shift)
        got.append([v.numpy()[0] for v in (mean, inv, mm, mv)])
    w = R.finalize(sums, n, d["shift"], np.full(f, MM0), np.full(f, MV0))
    for k, a, b, ref in zip(("mean", "inv", "moving_mean", "moving_var"), got[0], got[1], w):
        assert same(a, b), (k, "mean aliasing shift changes the result")
        assert rel_err(a, ref) < TIGHT, k
    # inference
    rng = np.random.default_rng(f)
    mm0, mv0 = rng.standard_normal(f).astype(F32), (0.5 + rng.random(f)).astype(F32)
    mean, inv, mm, mv = _vector(ctx, f), _vector(ctx, f), _vector(ctx, f, mm0), _vector(ctx, f, mv0)
    D.bn_finalize(ctx, None, 0, mean.row(0), inv.row(0), mm.row(0), mv.row(0))
    w = R.finalize(None, 0, None, mm0, mv0)
    assert same(mean.numpy()[0], mm0) and rel_err(inv.numpy()[0], w[1]) < TIGHT
    mm.untouched("moving_mean")
    mv.untouched("moving_var")


# ------------------------------------------------------------------------------------------- Gaussian data
GAUSS_N, GAUSS_F = (200, 700), 67                                  # a small launch and three chunks; float4 lanes + a 3-column tail


def _aligned_view(ctx, data=None, shape=None):
    n, f = shape or data.shape
    name, ld, lead = layouts(f)[1]
    fr = Frame(ctx, n, f, ld, lead, data)
    assert fr.aligned()
    return fr


def test_gaussian_moments_against_float64(ctx):
    """A mean of 50 under a deviation of 3: the centred second pass matters.  gcnx_bn_stats, gcnx_bn_finalize, gcnx_bn_moments."""
    from gcnx import device as D
    f = GAUSS_F
    for n in GAUSS_N:
        rng = np.random.default_rng(4000 + n)
        z = (rng.standard_normal((n, f)) * 3 + 50).astype(F32)
        shift = np.round(z.mean(0)).astype(F32)
        zf = _aligned_view(ctx, z)
        for sh in (None, shift):
            s = _vector(ctx, 2 * f)
            D.bn_stats(ctx, zf.view, s.row(0), shift=None if sh is None else ctx.to_device(sh))
            got, want = s.numpy()[0].reshape(2, f), R.stats(z, sh)
            assert rel_err(got[0], want[0]) < TIGHT and rel_err(got[1], want[1]) < TIGHT, (n, sh is None)
        mean, inv, mm, mv = _vector(ctx, f), _vector(ctx, f), _vector(ctx, f, np.full(f, MM0)), _vector(ctx, f, np.full(f, MV0))
        D.bn_finalize(ctx, s.row(0), n, mean.row(0), inv.row(0), mm.row(0), mv.row(0), shift=ctx.to_device(shift))
        for k, v, w in zip("mean inv moving_mean moving_var".split(), (mean, inv, mm, mv),
                           R.finalize(R.stats(z, shift), n, shift, np.full(f, MM0), np.full(f, MV0))):
            assert rel_err(v.numpy()[0], w) < TIGHT, ("finalize", n, k)
        mean, inv, mm, mv = _vector(ctx, f), _vector(ctx, f), _vector(ctx, f, np.full(f, MM0)), _vector(ctx, f, np.full(f, MV0))
        D.bn_moments(ctx, zf.view, None, mean.row(0), inv.row(0), mm.row(0), mv.row(0))
        for k, v, w in zip("mean inv moving_mean moving_var".split(), (mean, inv, mm, mv), R.moments(z, np.full(f, MM0), np.full(f, MV0))):
            assert rel_err(v.numpy()[0], w) < TIGHT, ("moments", n, k)
        zf.untouched()


def _gauss_bn(n, f, seed):
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((n, f)) * 2 + 1).astype(F32)
    dy = rng.standard_normal((n, f)).astype(F32)
    z64 = z.astype(np.float64)
    d = {"z": z, "dy": dy, "mean": z64.mean(0).astype(F32), "inv": (1.0 / np.sqrt(z64.var(0) + R.EPS)).astype(F32),
         "gamma": ((1 + 0.2 * rng.standard_normal(f)) * rng.choice([-1, 1], f)).astype(F32),
         "beta": (0.3 * rng.standard_normal(f)).astype(F32), "alpha": (0.05 + 0.4 * rng.random(f)).astype(F32),
         "shift": np.zeros(f, F32)}
    d["alpha_shared"] = d["alpha"][:1].copy()
    return d


@pytest.mark.parametrize("act", R.ACTS, ids=lambda a: a or "none")
def test_gaussian_bn_act_and_backward_against_float64(ctx, act):
    """Pre-activations on both sides of zero, gamma of either sign: gcnx_bn_act, gcnx_bn_act_bwd and its halves in both modes.
    The reference takes the PReLU / ReLU side of each element as the device decides it (bn_ref.device_sides)."""
    from gcnx import device as D
    f = GAUSS_F
    for n in GAUSS_N:
        d = _gauss_bn(n, f, 5000 + n)
        p = _params(ctx, d, act)
        al = R.alpha_of(d, act)
        args = (p["mean"], p["inv"], p["gamma"], p["beta"])
        host = (d["mean"], d["inv"], d["gamma"], d["beta"])
        zf, dyf = _aligned_view(ctx, d["z"]), _aligned_view(ctx, d["dy"])
        y = _aligned_view(ctx, shape=(n, f))
        D.bn_act(ctx, zf.view, *args, y.view, act=act, alpha=p["alpha"])
        assert rel_err(y.numpy(), R.bn_act(d["z"], *host, act, al)) < TIGHT, (n, "y")
        pos = R.device_sides(d["z"], *host)
        na = {"prelu": f, "prelu_shared": 1}.get(act)
        for training in (True, False):
            w = R.bn_act_bwd(d["dy"], d["z"], *host, act, al, training, pos=pos)
            for one_call in (True, False):
                dz, sums, dg, db = _aligned_view(ctx, shape=(n, f)), _vector(ctx, 3 * f), _vector(ctx, f), _vector(ctx, f)
                da = _vector(ctx, na) if na else None
                grads = dict(dgamma=dg.row(0), dbeta=db.row(0), dalpha=da.row(0) if da else None)
                if one_call:
                    D.bn_act_bwd(ctx, dyf.view, zf.view, *args, dz.view, sums.row(0), act=act, alpha=p["alpha"], training=training, **grads)
                else:
                    D.bn_act_bwd_stats(ctx, dyf.view, zf.view, *args, sums.row(0), act=act, alpha=p["alpha"], **grads)
                    D.bn_act_bwd_apply(ctx, dyf.view, zf.view, *args, sums.row(0), n, dz.view, act=act, alpha=p["alpha"], training=training)
                what = (n, training, one_call)
                assert rel_err(dz.numpy(), w["dz"]) < TIGHT, what
                assert rel_err(dg.numpy()[0], w["dgamma"]) < TIGHT and rel_err(db.numpy()[0], w["dbeta"]) < TIGHT, what
                if da:
                    assert rel_err(da.numpy()[0], w["dalpha"]) < TIGHT, what
        zf.untouched()
        dyf.untouched()


# ------------------------------------------------------------------------------------------- zero sizes and refusals
def test_no_rows_zeroes_sums_and_gradients(ctx):
    """n == 0: gcnx_bn_stats zeroes sums[2f]; gcnx_bn_act_bwd_stats (and the one call) zero sums[3f] and the three gradients --
    dalpha[1] alone for the shared slope; gcnx_bn_act and gcnx_bn_act_bwd_apply write nothing."""
    from gcnx import device as D
    f = 5
    d = R.exact_data(1, f, 6000)
    empty = ctx.empty((0, f))
    s = _vector(ctx, 2 * f)
    D.bn_stats(ctx, empty, s.row(0))
    s.check(np.zeros(2 * f))
    for act in R.ACTS:
        p = _params(ctx, d, act)
        args = (p["mean"], p["inv"], p["gamma"], p["beta"])
        na = {"prelu": f, "prelu_shared": 1}.get(act)
        for one_call in (False, True):
            sums, dg, db = _vector(ctx, 3 * f), _vector(ctx, f), _vector(ctx, f)
            da = _vector(ctx, na) if na else None
            grads = dict(dgamma=dg.row(0), dbeta=db.row(0), dalpha=da.row(0) if da else None)
            if one_call:
                D.bn_act_bwd(ctx, empty, empty, *args, empty, sums.row(0), act=act, alpha=p["alpha"], **grads)
            else:
                D.bn_act_bwd_stats(ctx, empty, empty, *args, sums.row(0), act=act, alpha=p["alpha"], **grads)
            sums.check(np.zeros(3 * f), act)
            dg.check(np.zeros(f), act)
            db.check(np.zeros(f), act)
            if da:
                da.check(np.zeros(na), act)
        guard = _vector(ctx, 4)
        D.bn_act(ctx, empty, *args, empty, act=act, alpha=p["alpha"])
        D.bn_act_bwd_apply(ctx, empty, empty, *args, guard.row(0), 1, empty, act=act, alpha=p["alpha"])
        guard.untouched()


def test_no_columns_is_a_no_op(ctx):
    """f == 0 for every entry point: success, nothing written (the outputs keep their sentinels)."""
    from gcnx import device as D
    n = 5
    e2, e1 = ctx.empty((n, 0)), ctx.empty(0)
    guard = _vector(ctx, 8)
    g = guard.row(0)
    assert e2.shape == (n, 0) and e1.size == 0
    D.bn_stats(ctx, e2, g)
    D.bn_stats(ctx, e2, g, shift=e1)
    D.bn_finalize(ctx, g, n, e1, e1, e1, e1)
    D.bn_moments(ctx, e2, None, e1, e1)
    for act in R.ACTS:
        al = g if act in ("prelu", "prelu_shared") else None
        D.bn_act(ctx, e2, e1, e1, e1, e1, e2, act=act, alpha=al)
        D.bn_act_bwd(ctx, e2, e2, e1, e1, e1, e1, e2, g, act=act, alpha=al, dgamma=e1, dbeta=e1, dalpha=g if al is not None else None)
        D.bn_act_bwd_stats(ctx, e2, e2, e1, e1, e1, e1, g, act=act, alpha=al, dgamma=e1, dbeta=e1, dalpha=g if al is not None else None)
        D.bn_act_bwd_apply(ctx, e2, e2, e1, e1, e1, e1, g, n, e2, act=act, alpha=al)
    guard.untouched()


def test_refusals_leave_the_context_usable(ctx):
    """ld < f, a PReLU without alpha, count <= 0 and one moving buffer without the other come back as GCNX_ERR_INVALID with their
    message and launch nothing; a good call after each gives the right bits."""
    from gcnx import _lib
    from gcnx import device as D
    from gcnx.device import DeviceArray
    n, f = 7, 6
    d = R.exact_data(n, f, 7000)
    p = _params(ctx, d, "prelu")
    args = (p["mean"], p["inv"], p["gamma"], p["beta"])
    want_y = _f32(R.bn_act(d["z"], d["mean"], d["inv"], d["gamma"], d["beta"], "prelu", d["alpha"]))
    zf, dyf = Frame(ctx, n, f, f + 2, 1, d["z"]), Frame(ctx, n, f, f + 2, 1, d["dy"])
    out = Frame(ctx, n, f, f + 2, 1)
    narrow = lambda fr: DeviceArray(ctx, fr.view.ptr, (n, f), F32, ld=f - 1, base=fr.buf)       # ld < f
    vecs = [_vector(ctx, 3 * f) for _ in range(5)]
    s, v1, v2, v3, v4 = [v.row(0) for v in vecs]
    half = lambda a: a.flat(0, f)
    pre = dict(act="prelu", alpha=None)
    refused = [
        ("bad z / ldz", lambda: D.bn_stats(ctx, narrow(zf), s)),
        ("bad ldz", lambda: D.bn_moments(ctx, narrow(zf), None, half(v1), half(v2))),
        ("leading dimension too small", lambda: D.bn_act(ctx, narrow(zf), *args, out.view)),
        ("leading dimension too small", lambda: D.bn_act(ctx, zf.view, *args, narrow(out))),
        ("leading dimension too small", lambda: D.bn_act_bwd(ctx, narrow(dyf), zf.view, *args, out.view, s)),
        ("leading dimension too small", lambda: D.bn_act_bwd_stats(ctx, dyf.view, narrow(zf), *args, s)),
        ("leading dimension too small", lambda: D.bn_act_bwd_apply(ctx, dyf.view, zf.view, *args, s, n, narrow(out))),
        ("PReLU needs alpha", lambda: D.bn_act(ctx, zf.view, *args, out.view, **pre)),
        ("PReLU needs alpha", lambda: D.bn_act_bwd(ctx, dyf.view, zf.view, *args, out.view, s, **pre)),
        ("PReLU needs alpha", lambda: D.bn_act_bwd_stats(ctx, dyf.view, zf.view, *args, s, **pre)),
        ("PReLU needs alpha", lambda: D.bn_act_bwd_apply(ctx, dyf.view, zf.view, *args, s, n, out.view, **pre)),
        ("PReLU needs alpha", lambda: D.bn_act(ctx, zf.view, *args, out.view, act="prelu_shared", alpha=None)),
        ("count must be positive", lambda: D.bn_finalize(ctx, s, 0, half(v1), half(v2))),
        ("count must be positive", lambda: D.bn_finalize(ctx, s, -3, half(v1), half(v2))),
        ("count must be positive", lambda: D.bn_act_bwd_apply(ctx, dyf.view, zf.view, *args, s, 0, out.view)),
        ("pass both moving buffers or none", lambda: D.bn_finalize(ctx, s, n, half(v1), half(v2), half(v3), None)),
        ("pass both moving buffers or none", lambda: D.bn_finalize(ctx, s, n, half(v1), half(v2), None, half(v4))),
        ("pass both moving buffers or none", lambda: D.bn_moments(ctx, zf.view, None, half(v1), half(v2), half(v3), None)),
        ("pass both moving buffers or none", lambda: D.bn_moments(ctx, zf.view, None, half(v1), half(v2), None, half(v4))),
    ]
    for message, call in refused:
        with pytest.raises(_lib.GcnxError, match=message) as e:
            call()
        assert e.value.code == 1, message                             # GCNX_ERR_INVALID
        out.untouched(message)
        for v in vecs:
            v.untouched(message)
        y = Frame(ctx, n, f, f + 2, 1)
        D.bn_act(ctx, zf.view, *args, y.view, act="prelu", alpha=p["alpha"])
        y.check(want_y, ("after", message))
    zf.untouched()
    dyf.untouched()


# ------------------------------------------------------------------------------------------- the pooled backward on an empty shard
@pytest.mark.parametrize("act", ["prelu", "prelu_shared", "relu"])
def test_pool_bwd_without_rows_zeroes_the_parameter_gradients(ctx, act):
    """gcnx_bn_act_pool_bwd with n == 0 (every graph of the shard empty) and f > 0 zeroes dgamma, dbeta and dalpha ([f] for
    PRELU, [1] for PRELU_SHARED), as its split form gcnx_bn_act_pool_bwd_stats and gcnx_bn_act_bwd_stats do: a data-parallel
    rank with an empty shard must not add stale parameter gradients."""
    from gcnx import device as D
    from gcnx.device import Segments
    f, b = 5, 3
    d = R.exact_data(1, f, 8000)
    p = _params(ctx, d, act)
    seg = Segments(ctx, np.zeros(b + 1, np.int64))
    empty = ctx.empty((0, f))
    dp, arg = ctx.to_device(np.ones((b, f), F32)), ctx.to_device(np.zeros((b, f), np.int32))
    na = {"prelu": f, "prelu_shared": 1}.get(act)
    args = (p["mean"], p["inv"], p["gamma"], p["beta"])
    for split in (False, True):
        dg, db = _vector(ctx, f), _vector(ctx, f)
        da = _vector(ctx, na) if na else None
        assert dg.numpy()[0][0] == SENTINEL
        grads = dict(dgamma=dg.row(0), dbeta=db.row(0), dalpha=da.row(0) if da else None)
        if split:
            sums = _vector(ctx, 3 * f)
            D.bn_act_pool_bwd_stats(ctx, seg, dp, arg, empty, *args, sums.row(0), act=act, alpha=p["alpha"], **grads)
            sums.check(np.zeros(3 * f), (act, "sums"))
        else:
            D.bn_act_pool_bwd(ctx, seg, dp, arg, empty, *args, empty, act=act, alpha=p["alpha"], **grads)
        dg.check(np.zeros(f), (act, split, "dgamma"))
        db.check(np.zeros(f), (act, split, "dbeta"))
        if da:
            da.check(np.zeros(na), (act, split, "dalpha"))

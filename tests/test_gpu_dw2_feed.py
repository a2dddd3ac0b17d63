"""dw_tile_interior (csrc/gemm.hip), the tile body the dW1 + dW2 launch runs on its interior tiles, against gemm_f32_tile,
which GCNX_DW2_FEED=0 restores: one context each, every result compared as uint32, and dW1 / dW2 against the fp64 product at
TIGHT.

The new body serves the full 64 x 64 tiles of aligned operands over slices of whole K steps (32 rows); everything else
stays on the old one.  The plan is the library's documented rule (csrc/common.h gcnx_split_rows with slices of at least
10 steps, ~4 workgroups per CU wanted) and each case asserts the slice depths it relies on:
  n =   640   two slices of 10 steps: an even trip count
  n =   704   two of 11: odd -- the double-buffered images end on the other parity
  n = 1 000   slices of 11, 11 and 9.25 steps: the ragged last slice runs the old body in the same launch
  n = 3 552   ten slices of 11 steps and one of a single whole step (the prologue's second load group has no step 1 to
              fetch).  n = 736, the first guess, gives two slices of 12 and 11 steps under this rule; 3 552 is the
              smallest n whose last slice is one whole step.
(fi, fo) of the two products come in mixed pairs from {64, 128}^2, so one launch has tile grids of 1, 2 and 4 tiles.
Operands are strided views inside sentinel frames; the gradient buffer is a frame of its own."""
import os

import numpy as np
import pytest

from conftest import rel_err
from gpu_frames import SENTINEL, Frame, bits

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
LR = np.float32(2.0 ** -6)          # a power of two: lr * g is exact, p - lr * g is one rounding with or without an fma
H, C, B = 128, 2, 4                 # the head's shape in the merged launch (two classes, config 2's hidden width)
PAIRS = [((64, 64), (128, 64)), ((64, 128), (128, 128)), ((128, 128), (64, 64)), ((128, 64), (64, 128))]
STEPS = {640: [10, 10], 704: [11, 11], 1000: [11, 11, 9.25], 3552: [11] * 10 + [1]}
_inputs = {}


@pytest.fixture(scope="module")
def both():
    """(context with the new body, context with GCNX_DW2_FEED=0): the knob is read when a context is created."""
    import gcnx
    old = os.environ.pop("GCNX_DW2_FEED", None)
    try:
        on = gcnx.Context(0)
        os.environ["GCNX_DW2_FEED"] = "0"
        off = gcnx.Context(0)
    finally:
        os.environ.pop("GCNX_DW2_FEED", None)
        if old is not None:
            os.environ["GCNX_DW2_FEED"] = old
    yield on, off
    off.close()
    on.close()


def slice_steps(cus, tiles, n):
    """The split-K plan of gcnx_gemm_dw2 as documented: depth of every slice in K steps of 32 rows."""
    want = (4 * cus + tiles - 1) // tiles
    ksteps = (n + 31) // 32
    nsplit = max(1, min(want, ksteps // 10))
    kchunk = (ksteps + nsplit - 1) // nsplit * 32
    return [min(kchunk, n - k0) / 32 for k0 in range(0, n, kchunk)]


def inputs(n, pair):
    """Gaussian operands of both products and the fp64 products; the head's operands.  Computed once, never written."""
    key = (n, pair)
    if key not in _inputs:
        rng = np.random.default_rng(n + 7 * pair[0][0] + 3 * pair[1][1])
        (fia, foa), (fib, fob) = pair
        d = {"xa": rng.standard_normal((n, fia), dtype=np.float32), "dha": rng.standard_normal((n, foa), dtype=np.float32),
             "xb": rng.standard_normal((n, fib), dtype=np.float32), "dhb": rng.standard_normal((n, fob), dtype=np.float32)}
        d["dwa"] = d["xa"].astype(np.float64).T @ d["dha"].astype(np.float64)
        d["dwb"] = d["xb"].astype(np.float64).T @ d["dhb"].astype(np.float64)
        d["pool_sum"] = rng.standard_normal((B, H), dtype=np.float32)
        d["pool_cnt"] = rng.integers(0, n // B, (B, H)).astype(np.float32)
        d["w3"] = (rng.standard_normal((H, C)) / np.sqrt(H)).astype(np.float32)
        d["b3"] = rng.standard_normal(C).astype(np.float32)
        d["y"] = np.eye(C, dtype=np.float32)[rng.integers(0, C, B)]
        _inputs[key] = d
    return _inputs[key]


def run(ctx, n, pair, leaf, with_params, lead=None, pad=None):
    """One gcnx_gemm_dw2 call on framed operands; every output as a host array.  lead / pad: per operand, floats in front
    of the view (4: 16-byte aligned) and floats between its rows."""
    from gcnx import device as D
    from gcnx.device import Segments
    d = inputs(n, pair)
    (fia, foa), (fib, fob) = pair
    lead = dict({"xa": 4, "dha": 8, "xb": 12, "dhb": 4}, **(lead or {}))
    pad = dict({"xa": 4, "dha": 8, "xb": 0, "dhb": 12}, **(pad or {}))
    fr = {k: Frame(ctx, n, d[k].shape[1], d[k].shape[1] + pad[k], lead[k], d[k]) for k in ("xa", "dha", "xb", "dhb")}
    # gradient frame: pad | dW1 | gap | dW2 | gap | dW3 | db3 | gap | db2 | pad
    off, where = 0, {}
    for name, k in (("pad0", 8), ("dwa", fia * foa), ("gap0", 20), ("dwb", fib * fob), ("gap1", 12), ("dw3", H * C), ("db3", C), ("gap2", 6),
                    ("db2", H), ("pad1", 12)):
        where[name] = (off, k)
        off += k
    grads = ctx.to_device(np.full(off, SENTINEL, np.float32))
    p0 = np.linspace(-1, 1, off, dtype=np.float32)
    params = ctx.to_device(p0) if with_params else None
    gv = lambda name, shape: grads.flat(where[name][0], where[name][1], shape)
    out = {}
    ha = None
    if leaf:
        gp = np.linspace(0, n, B + 1).astype(np.int32)
        seg = Segments(ctx, gp)
        tp, tc = ctx.zeros((D.pool_tile_rows(n, B), H)), ctx.zeros((D.pool_tile_rows(n, B), H))
        head = {"probs": ctx.zeros((B, C)), "la": ctx.zeros(2), "pooled": ctx.zeros((B, H)), "dp": ctx.zeros((B, H))}
        keep = [seg, tp, tc, ctx.to_device(d["pool_sum"]), ctx.to_device(d["pool_cnt"]), ctx.to_device(d["w3"]), ctx.to_device(d["b3"]),
                ctx.to_device(d["y"])]
        ha = D.head_args(seg, tp, tc, keep[3], keep[4], keep[5], keep[6], keep[7], float(B + 1), head["probs"], head["la"],
                         gv("dw3", (H, C)), gv("db3", (C,)), gv("db2", (H,)), head["pooled"], head["dp"])
    D.gemm_dw2(ctx, fr["xa"].view, fr["dha"].view, gv("dwa", (fia, foa)), fr["xb"].view, fr["dhb"].view, gv("dwb", (fib, fob)),
               params=params, grads=grads, lr=float(LR), leaf=ha)
    g = grads.numpy()
    written = np.zeros(off, bool)
    for name in ("dwa", "dwb") + (("dw3", "db3", "db2") if leaf else ()):
        o, k = where[name]
        out[name] = g[o:o + k].copy()
        written[o:o + k] = True
    assert (g[~written] == SENTINEL).all(), "written outside the gradients"
    for k in fr:                                         # the operands and their frames are as they were
        fr[k].check(d[k], k)
    if leaf:
        out.update({k: v.numpy().copy() for k, v in head.items()})
    if with_params:
        out["params"] = params.numpy().copy()
        assert np.array_equal(bits(out["params"]), bits(p0 - LR * g))
    return out


def compare(both, n, pair, leaf, with_params, **kw):
    on, off = both
    d = inputs(n, pair)
    a, b = run(on, n, pair, leaf, with_params, **kw), run(off, n, pair, leaf, with_params, **kw)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), (k, n, pair, leaf, with_params)
    for k in ("dwa", "dwb"):
        err = rel_err(a[k].reshape(d[k].shape), d[k])
        print(f"n = {n} {pair} {k}: rel err against fp64 {err:.2e}")
        assert err < TIGHT, (k, err)
    if leaf:
        assert np.isfinite(a["la"]).all() and a["dw3"].any() and a["probs"].any()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%dx%d+%dx%d" % (p[0] + p[1]))
@pytest.mark.parametrize("n", sorted(STEPS))
def test_interior_body_equals_gemm_f32_tile_bit_for_bit(both, n, pair):
    tiles = sum(-(-fi // 64) * -(-fo // 64) for fi, fo in pair)
    assert slice_steps(both[0].info()["cus"], tiles, n) == STEPS[n]
    for leaf in (False, True):
        for with_params in (False, True):
            compare(both, n, pair, leaf, with_params)


@pytest.mark.parametrize("what", ["one float off 16-byte alignment", "ld % 4 != 0"])
def test_unaligned_operands_stay_on_the_old_body_and_agree(both, what):
    """Product a's x one float off alignment (its tiles take gemm_f32_tile's guarded loads, product b's the new body), or
    product b's dH with an odd row stride."""
    n, pair = 704, ((128, 128), (128, 128))
    assert slice_steps(both[0].info()["cus"], 8, n) == STEPS[n]
    kw = dict(lead={"xa": 5}) if what.startswith("one float") else dict(pad={"dhb": 5})
    compare(both, n, pair, True, True, **kw)
    compare(both, n, pair, False, False, **kw)


def test_captured_step_replays_the_same_bits(both):
    """GCN2's captured step on a three-graph E. coli-shaped batch (eager warm-up, capture + launch, two replays): loss,
    gradients and weights equal those of the context with the old loop, bit for bit."""
    import gcnx
    from gcnx import synth
    from gcnx.models import DeviceBatch, GCN2
    hb = synth.ecoli_batch(3, 128, seed=4)
    hb.vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    assert len(slice_steps(both[0].info()["cus"], 8, hb.n)) > 1       # the split route, not the separate calls
    res = []
    for ctx in both:
        a = gcnx.DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, hb.vals, hb.graph_ptr)
        batch = DeviceBatch(ctx, ctx.to_device(hb.x), a, gcnx.Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y, np.float32))
        m = GCN2(ctx, 2, hidden=128, seed=5, use_graph=True)
        steps = [m.train_step(batch, None, lr=float(LR)) for _ in range(4)]
        assert m.use_graph and any(not isinstance(g, str) for g in m._graphs.values())    # a graph was captured and replayed
        res.append((steps, m.gradients(), m.get_weights()))
    (s_on, g_on, w_on), (s_off, g_off, w_off) = res
    assert s_on == s_off and all(np.isfinite(l) for l, _ in s_on)
    for k in g_on:
        assert np.array_equal(bits(g_on[k]), bits(g_off[k])), k
    for x, y in zip(w_on, w_off):
        assert np.array_equal(bits(x), bits(y))

"""gcnx_gemm_dw2_graph (csrc/gemm.hip): dW2 = sum_g dP_g * (S2_g^T mask_g) from per-graph mask products on the bf16 MFMA with
the exact three-way split of S2, through the C ABI against float64 NumPy, and GCN2 with the route on against the route off.

Shapes are the smallest at which the kernel can go wrong (slices of at most KCHUNK = 352 rows, K steps of 32):
  one_row        one graph of one row, 64 x 64
  ragged_step    one graph of 33 rows: a second K step that holds a single row
  three_graphs   31 / 32 / 33 rows: graph boundaries inside one 64-row span, three slices
  past_slice     353 rows: one row past a full slice
  four_tiles     352 / 353 / 705 rows, 128 x 128: all four output tiles, six slices, both roles (dW1 tiles, C tiles) with four tiles each
  narrow         fi = 64, fo = 128 over 353 / 33 rows
Every case runs with an all-zero, an all-one and a random mask, SUM and AVG, gradients only (params == NULL) and with the SGD
step, twice (bitwise equal); S2 has one column whose entries span 2^-20 .. 2^20; operands are strided views inside sentinel
frames.

Tolerance: on the same operands the max-abs deviation from the float64 product relative to max|dW2| is measured for the
present route (gcnx_gemm_dw2 on the fp32 dZ2) and for the new one; the new one must stay within the fused tests' 2e-5 and
within twice the present route's figure (both are accumulation rounding of the same length)."""
import os

import numpy as np
import pytest

from conftest import rel_err
from gpu_frames import SENTINEL, Frame, bits

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
KCHUNK = 352
LR = np.float32(2.0 ** -6)
CASES = {"one_row": ([1], 64, 64), "ragged_step": ([33], 64, 64), "three_graphs": ([31, 32, 33], 64, 64),
         "past_slice": ([353], 64, 64), "four_tiles": ([352, 353, 705], 128, 128), "narrow": ([353, 33], 64, 128)}
MASKS = ("zero", "one", "random")
BYTE_SENTINEL = np.uint8(0xA5)          # nonzero: a mask byte read outside the view would count as a 1
_inputs = {}


@pytest.fixture(scope="module")
def both():
    """(context with the route on, context with GCNX_DW2_GRAPH=0): the knob is read when a context is created."""
    import gcnx
    old = os.environ.pop("GCNX_DW2_GRAPH", None)
    try:
        on = gcnx.Context(0)
        os.environ["GCNX_DW2_GRAPH"] = "0"
        off = gcnx.Context(0)
    finally:
        os.environ.pop("GCNX_DW2_GRAPH", None)
        if old is not None:
            os.environ["GCNX_DW2_GRAPH"] = old
    yield on, off
    off.close()
    on.close()


def inputs(case, mask, mode):
    """Operands and float64 results of one case; computed once, never written."""
    key = (case, mask, mode)
    if key not in _inputs:
        sizes, fi, fo = CASES[case]
        n, b = sum(sizes), len(sizes)
        rng = np.random.default_rng(1000 * sorted(CASES).index(case) + 10 * MASKS.index(mask) + (mode == "avg"))
        gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        ids = np.repeat(np.arange(b), sizes)
        s2 = rng.standard_normal((n, fi), dtype=np.float32)
        s2[:, 3] *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)          # one column spanning 2^-20 .. 2^20
        m8 = {"zero": np.zeros((n, fo), np.uint8), "one": np.ones((n, fo), np.uint8),
              "random": (rng.random((n, fo)) < 0.5).astype(np.uint8)}[mask]
        dp = rng.standard_normal((b, fo), dtype=np.float32)
        scale = dp if mode == "sum" else dp * (np.float32(1.0) / np.asarray(sizes, np.float32))[:, None]      # fp32, as the backward
        dz2 = (m8 * scale[ids]).astype(np.float32)                                # exact: a 0/1 factor
        fa = fi                                                                   # the dW1 product of the same launch
        xa, dha = rng.standard_normal((n, fa), dtype=np.float32), rng.standard_normal((n, fa), dtype=np.float32)
        _inputs[key] = {"gp": gp, "s2": s2, "m8": m8, "dp": dp, "dz2": dz2, "xa": xa, "dha": dha,
                        "dwa": xa.astype(np.float64).T @ dha.astype(np.float64),
                        "dwb": s2.astype(np.float64).T @ dz2.astype(np.float64)}
    return _inputs[key]


class ByteFrame:
    """Frame for uint8 rows (tests/gpu_frames.Frame holds 2- and 4-byte elements)."""

    def __init__(self, ctx, data, ld, lead, tail=9):
        from gcnx.device import DeviceArray
        n, f = data.shape
        host = np.full(lead + n * ld + tail, BYTE_SENTINEL, np.uint8)
        host[lead:lead + n * ld].reshape(n, ld)[:, :f] = data
        self._initial = host
        self.buf = ctx.to_device(host)
        self.view = DeviceArray(ctx, self.buf.ptr + lead, (n, f), np.uint8, ld=ld, base=self.buf)

    def untouched(self):
        assert np.array_equal(self.buf.numpy(), self._initial), "the mask frame was written"


def grad_frame(ctx, ta, tb, with_params):
    """pad | dW1 | gap | dW2 | pad in one flat sentinel buffer; the parameters beside it."""
    where, off = {}, 0
    for name, k in (("pad0", 8), ("dwa", ta), ("gap", 20), ("dwb", tb), ("pad1", 12)):
        where[name] = (off, k)
        off += k
    grads = ctx.to_device(np.full(off, SENTINEL, np.float32))
    p0 = np.linspace(-1, 1, off, dtype=np.float32)
    return where, grads, p0, (ctx.to_device(p0) if with_params else None)


def read_grads(where, grads, p0, params):
    g = grads.numpy()
    written = np.zeros(g.size, bool)
    out = {}
    for name in ("dwa", "dwb"):
        o, k = where[name]
        out[name] = g[o:o + k].copy()
        written[o:o + k] = True
    assert (g[~written] == SENTINEL).all(), "written outside the gradients"
    if params is not None:
        assert np.array_equal(bits(params.numpy()), bits(p0 - LR * g))
    return out


def run_new(ctx, d, fi, fo, mode, with_params, s2=None, n=None, plan_gp=None):
    """One gcnx_gemm_dw2_graph call on framed operands.  s2 / n / plan_gp: the ragged-edge case (rows behind the planned ones)."""
    from gcnx import device as D
    s2 = d["s2"] if s2 is None else s2
    n = s2.shape[0] if n is None else n
    gp = d["gp"] if plan_gp is None else plan_gp
    fa = d["xa"].shape[1]
    fr = {"xa": Frame(ctx, n, fa, fa + 4, 4, d["xa"][:n]), "dha": Frame(ctx, n, fa, fa + 8, 8, d["dha"][:n]),
          "s2": Frame(ctx, n, fi, fi + 8, 12, s2[:n]), "dp": Frame(ctx, d["dp"].shape[0], fo, fo + 3, 5, d["dp"])}
    m8 = ByteFrame(ctx, d["m8"][:n], fo + 16, 7)
    host_plan = D.dw2_slice_plan(gp, KCHUNK)
    plan = (ctx.to_device(host_plan, np.int32), len(host_plan), KCHUNK)
    where, grads, p0, params = grad_frame(ctx, fa * fa, fi * fo, with_params)
    gv = lambda name, shape: grads.flat(where[name][0], where[name][1], shape)
    assert D.gemm_dw2_graph(ctx, fr["xa"].view, fr["dha"].view, gv("dwa", (fa, fa)), fr["s2"].view, m8.view, gv("dwb", (fi, fo)), plan,
                            fr["dp"].view, mode=mode, params=params, grads=grads, lr=float(LR))
    out = read_grads(where, grads, p0, params)
    for k in fr:
        fr[k].untouched(k)
    m8.untouched()
    return out


def run_present(ctx, d, fi, fo):
    """The present route on the same operands: gcnx_gemm_dw2 with dZ2 as an fp32 matrix."""
    from gcnx import device as D
    n, fa = d["xa"].shape
    where, grads, p0, _ = grad_frame(ctx, fa * fa, fi * fo, False)
    gv = lambda name, shape: grads.flat(where[name][0], where[name][1], shape)
    D.gemm_dw2(ctx, ctx.to_device(d["xa"]), ctx.to_device(d["dha"]), gv("dwa", (fa, fa)), ctx.to_device(d["s2"]), ctx.to_device(d["dz2"]),
               gv("dwb", (fi, fo)), grads=grads)
    return read_grads(where, grads, p0, None)


def dev(got, want):
    """max |got - want| / max |want| (0 for an all-zero product)."""
    top = float(np.max(np.abs(want)))
    return float(np.max(np.abs(got.astype(np.float64).reshape(want.shape) - want))) / top if top else float(np.max(np.abs(got)))


@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_mask_products_against_float64(both, case, mask, mode):
    ctx = both[0]
    sizes, fi, fo = CASES[case]
    d = inputs(case, mask, mode)
    old = run_present(ctx, d, fi, fo)
    runs = [run_new(ctx, d, fi, fo, mode, with_params) for with_params in (False, True, False)]
    for r in runs[1:]:                                   # repeatable, and the SGD form folds the same gradients
        for k in ("dwa", "dwb"):
            assert np.array_equal(bits(r[k]), bits(runs[0][k])), (k, "not bitwise repeatable")
    if sum(sizes) <= KCHUNK:                             # one slice either way (beyond it the test's KCHUNK is not the library's own cut)
        assert np.array_equal(bits(runs[0]["dwa"]), bits(old["dwa"])), "dW1 is gcnx_gemm_dw2's, bit for bit"
    assert dev(runs[0]["dwa"], d["dwa"]) < TIGHT
    e_new, e_old = dev(runs[0]["dwb"], d["dwb"]), dev(old["dwb"], d["dwb"])
    print(f"{case} {mask} {mode}: dW2 deviation from float64, present route {e_old:.3e}, mask products {e_new:.3e}; "
          f"dW1 {dev(runs[0]['dwa'], d['dwa']):.3e}")
    assert e_new < TIGHT, (e_new, TIGHT)
    assert e_new <= 2.0 * e_old, (e_new, e_old)
    if mask == "zero":
        assert not runs[0]["dwb"].any()


def test_rows_of_the_next_graph_never_enter_a_product(both):
    """The planned graph has 33 rows: its second K step holds one row.  The 31 rows behind it -- the next graph's, not in the
    plan -- are NaN in one run and finite in the other: dW2 is the same bit for bit, so they were not multiplied, not even by 0."""
    ctx = both[0]
    d = inputs("three_graphs", "one", "sum")              # 96 rows; graph 0's plan only
    n = 64
    gp = np.array([0, 33], np.int32)
    s_nan = d["s2"].copy()
    s_nan[33:] = np.nan
    d1 = dict(d, dp=d["dp"][:1])
    a = run_new(ctx, d1, 64, 64, "sum", False, s2=d["s2"], n=n, plan_gp=gp)
    b = run_new(ctx, d1, 64, 64, "sum", False, s2=s_nan, n=n, plan_gp=gp)
    assert np.isfinite(b["dwb"]).all() and np.array_equal(bits(a["dwb"]), bits(b["dwb"]))
    want = d["s2"][:33].astype(np.float64).T @ (d["m8"][:33] * d["dp"][0]).astype(np.float64)
    assert dev(a["dwb"], want) < TIGHT


def test_refusals_launch_nothing(both):
    from gcnx import _lib as L
    from gcnx import device as D
    on, off = both
    d = inputs("three_graphs", "random", "sum")
    n = d["s2"].shape[0]
    plan_h = D.dw2_slice_plan(d["gp"], KCHUNK)

    def call(ctx, s2, m8, fi, fo, plan_h, mode="sum"):
        where, grads, p0, _ = grad_frame(ctx, 64 * 64, fi * fo, False)
        gv = lambda name, shape: grads.flat(where[name][0], where[name][1], shape)
        before = L.last_error(ctx.h)
        ok = D.gemm_dw2_graph(ctx, ctx.to_device(d["xa"]), ctx.to_device(d["dha"]), gv("dwa", (64, 64)), s2, m8, gv("dwb", (fi, fo)),
                              (ctx.to_device(plan_h, np.int32), len(plan_h), KCHUNK), ctx.to_device(np.zeros((3, fo), np.float32)), mode=mode,
                              grads=grads)
        assert (grads.numpy() == SENTINEL).all() and L.last_error(ctx.h) == before
        return ok

    s2, m8 = on.to_device(d["s2"]), on.to_device(d["m8"])
    wide = on.to_device(np.zeros((n, 96), np.float32))
    assert not call(on, wide, m8, 96, 64, plan_h)                                      # fi not in {64, 128}
    assert not call(on, s2, on.to_device(np.zeros((n, 96), np.uint8)), 64, 96, plan_h)  # fo no multiple of 64
    assert not call(on, s2, m8, 64, 64, plan_h, mode="max")
    many = D.dw2_slice_plan(np.arange(n + 1, dtype=np.int32), KCHUNK)                   # 96 one-row graphs: over the slice bound
    assert len(many) == n and not call(on, s2, m8, 64, 64, many)
    assert not call(off, off.to_device(d["s2"]), off.to_device(d["m8"]), 64, 64, plan_h)   # the knob
    assert D.gemm_dw2_graph_plan(off, type("S", (), {"host": d["gp"]})(), n, 64, 64, 64, 64) is None


# ---- GCN2 --------------------------------------------------------------------------------------------------------------

def small_batch(ctx, hb):
    import gcnx
    from gcnx.models import DeviceBatch
    a = gcnx.DeviceCSR.from_host_csr(ctx, hb.rowptr, hb.colidx, hb.vals, hb.graph_ptr)
    return DeviceBatch(ctx, ctx.to_device(hb.x), a, gcnx.Segments(ctx, hb.graph_ptr), ctx.to_device(hb.y, np.float32))


@pytest.fixture(scope="module")
def host_batch():
    """Three random graphs with self-loops, 31 + 35 + 37 = 103 rows, F = 128, GCN-normalised."""
    from gcnx import synth
    rng = np.random.default_rng(11)
    sizes = [31, 35, 37]
    n = sum(sizes)
    adj = np.zeros((n, n), bool)
    r0 = 0
    for k in sizes:
        upper = np.triu(rng.random((k, k)) < 0.15, 1)
        adj[r0:r0 + k, r0:r0 + k] = upper | upper.T | np.eye(k, dtype=bool)
        r0 += k
    rowptr = np.concatenate([[0], np.cumsum(adj.sum(1))]).astype(np.int32)
    colidx = np.nonzero(adj)[1].astype(np.int32)
    y = np.eye(2, dtype=np.float32)[[0, 1, 1]]
    hb = synth.HostBatch(rng.standard_normal((n, 128)).astype(np.float32), rowptr, colidx, None,
                         np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), y)
    hb.vals = synth.gcn_norm_host(hb.rowptr, hb.colidx)
    return hb


@pytest.mark.parametrize("pool", ["sum", "avg"])
def test_gcn2_step_with_the_route_on_and_off(both, host_batch, pool):
    from gcnx.models import GCN2
    res = []
    for ctx in both:
        m = GCN2(ctx, 2, hidden=128, seed=5, pool=pool)
        batch = small_batch(ctx, host_batch)
        loss = m.train_step(batch, None, lr=float(LR))
        res.append((loss, m.gradients(), m.dw2_plans_built, batch._route.get(("dw2_graph", id(m), batch.uid))))
    (l_on, g_on, built_on, plan_on), (l_off, g_off, _, plan_off) = res
    assert built_on == 1 and plan_on is not None and plan_off is None          # the route ran / did not run
    assert l_on == l_off
    for k in ("w1", "b1", "b2", "w3", "b3"):
        assert np.array_equal(bits(g_on[k]), bits(g_off[k])), (k, "only dW2 may change")
    e = rel_err(g_on["w2"], g_off["w2"])
    print(f"GCN2 {pool}: dW2 route on against off {e:.3e}")
    assert e < TIGHT


def test_gcn2_five_steps_against_the_c_oracle(both, host_batch):
    from gcnx.models import GCN2
    from oracle import c_oracle
    ctx = both[0]
    m = GCN2(ctx, 2, hidden=128, seed=5, use_graph=False)
    m.build(host_batch.f)
    flat = np.concatenate([w.ravel() for w in m.get_weights()]).astype(np.float32)
    cpu = c_oracle.Gcn2Cpu(host_batch, 128, 2, flat)
    batch = small_batch(ctx, host_batch)
    for _ in range(5):
        loss, _ = m.train_step(batch, None, lr=0.02)
        cl, _ = cpu.step(lr=0.02)
        assert abs(cl - loss) < 1e-4 * max(1.0, cl)
    assert batch._route.get(("dw2_graph", id(m), batch.uid)) is not None
    got = np.concatenate([w.ravel() for w in m.get_weights()])
    assert rel_err(got, cpu.params.astype(np.float64)) < 1e-4


def test_plan_is_kept_with_the_batch_and_rebuilt_after_invalidate(both, host_batch):
    from gcnx.models import GCN2
    ctx = both[0]
    m = GCN2(ctx, 2, hidden=128, seed=5)
    batch = small_batch(ctx, host_batch)
    m.train_step(batch, None, lr=0.02)
    first = batch._route[("dw2_graph", id(m), batch.uid)]
    m.train_step(batch, None, lr=0.02)
    assert m.dw2_plans_built == 1 and batch._route[("dw2_graph", id(m), batch.uid)] is first
    batch.invalidate()
    m.train_step(batch, None, lr=0.02)
    assert m.dw2_plans_built == 2 and batch._route[("dw2_graph", id(m), batch.uid)] is not first

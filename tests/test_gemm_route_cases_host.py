"""The case table of tests/gemm_route_cases.py, pinned without a GPU: for every case the operands keep every partial sum of
every summation order exact (sum of |terms| < 2^24), the restated dispatch sends the case to the route it names at 64, 256
and 304 compute units, and the expected outputs are not degenerate -- exact zeros where an activation, a mask or a bit image
is tested, both signs, round-to-even ties where bf16 result rows are written.  tests/test_gpu_gemm_routes.py runs the same
table on the device."""
import numpy as np
import pytest

import gemm_route_cases as G

CUS = (256, 64, 304)
IDS = [c.id for c in G.CASES]


def test_ids_are_unique_and_every_entry_point_is_there():
    assert len(set(IDS)) == len(IDS)
    assert {c.entry for c in G.CASES} == {"gemm", "dx", "dw", "dense_bwd", "dense_bwd_deferred", "bits_pair", "pair16", "fwd16", "dx16", "dw16", "wimage"}


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_route(case):
    """The restated predicate names the case's route at every CU count: the shapes do not depend on the chip."""
    for cus in CUS:
        assert case.predicted(cus) == case.route, (cus, case.predicted(cus))


@pytest.mark.parametrize("case", G.gaussian_cases(), ids=lambda c: c.id)
def test_gaussian_routes(case):
    for cus in CUS:
        assert case.predicted(cus) == case.route
    assert all(case.layout(k) == "al" for k in ("x", "dh", "w", "out", "dx", "y", "db", "dw", "bias"))


def _exact_range(case):
    """No partial sum of any order leaves the exact range: max over the outputs of sum |terms| < 2^24, db included."""
    out, db = case.bounds()
    assert out < G.EXACT and db < G.EXACT, (out, db)
    assert case.vals() in ("i3", "i1")
    d = case.data()
    for a in (d.x, d.dh, d.w, d.bias, d.base):
        assert np.array_equal(a, np.round(a)) and (np.abs(a) <= 3).all()
    assert set(np.unique(np.log2(d.alpha))) <= {-3.0, -2.0, -1.0, 1.0}           # powers of two


def _both_signs(a):
    a = np.asarray(a, np.float64)
    return a.size < 16 or ((a > 0).any() and (a < 0).any())


def _outputs_are_not_degenerate(case):
    """Exact zeros (at least 5 %) in front of every activation and in every mask source, +0.0, -0.0 and negative values in
    y_mask, both signs in every result of at least 16 elements (ReLU outputs: in the pre-activation), ties in bf16 rows."""
    d, o, e = case.data(), case.opt, case.entry
    want = case.expected()
    if e == "wimage" and case.route == "unsupported" or case.n == 0:
        return
    if "out" in want:
        z = d.fwd(o.get("bias"), o.get("act"))[0]
        assert _both_signs(z)
        if o.get("act"):
            assert z.size and (z == 0).mean() >= 0.05 and (z < 0).any(), (z == 0).mean()
        if e in ("bits_pair", "pair16"):
            out = d.fwd(True, "relu")[1]
            assert (out == 0).mean() >= 0.05 and (out > 0).mean() >= 0.05
    if o.get("mask"):
        y = d.y
        sign = np.signbit(y)
        assert (y == 0).mean() >= 0.05 and ((y == 0) & sign).any() and ((y == 0) & ~sign).any() and (y < 0).any() and (y > 0).any()
    if "dx" in want and not o.get("out16"):
        assert _both_signs(want["dx"])
        if "db" in want:
            assert _both_signs(want["db"])
    if "dw" in want:
        assert _both_signs(want["dw"])
    if e == "pair16":                                                # exact rows: the image and db are those of what is stored
        assert np.array_equal(G.bf16_round(d.fwd(True, "relu")[1]), d.fwd(True, "relu")[1]) and np.array_equal(G.bf16_round(d.dx2()[0]), d.dx2()[0])
        return
    if o.get("out16") and case.route != "unsupported" and not case.want_db():
        exact = d.fwd(o.get("bias"), o.get("act"))[1] if e == "fwd16" else d.dx(o.get("mask"))[0]
        ties = G.bf16_ties(exact)
        assert ties >= 1, "no round-to-even tie in the bf16 result rows"
        up = G.bf16_bits(exact)
        assert (up.astype(np.int64) << 16 != np.ascontiguousarray(exact).view(np.uint32)).sum() >= ties      # the ties are rounded
    if o.get("out16") and case.want_db():                            # db is that of rows that bf16 holds exactly
        assert np.array_equal(G.bf16_round(d.dx(o.get("mask"))[0]), d.dx(o.get("mask"))[0])


def test_ties_round_to_even():
    """bf16_bits on hand-made ties: 257 -> 256 (down to even), 259 -> 260 (up to even), -257 -> -256."""
    got = G.bf16_round(np.array([257.0, 259.0, -257.0, 258.0, 1.0], np.float32))
    assert got.tolist() == [256.0, 260.0, -256.0, 258.0, 1.0]
    assert G.bf16_ties(np.array([257.0, 259.0, 258.0, 3.0], np.float32)) == 2


def test_the_rounding_is_that_of_test_gpu_kernels():
    from test_gpu_kernels import _bf16_round
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 300, np.arange(-600, 600, dtype=np.float32)])
    assert G.bf16_ties(v) > 100 and np.array_equal(G.bf16_round(v).view(np.uint32), _bf16_round(v).view(np.uint32))


def _broken_alone(entry, route, name, layout, **opt):
    return [c for c in G.CASES if c.entry == entry and c.route == route and c.lay == {name: layout} and all(c.opt.get(k) == v for k, v in opt.items())]


def test_every_dispatch_flag_is_broken_alone():
    """Each flag of the dispatch has a case in which it alone is broken (one operand in one unaligned layout)."""
    for name, lays in (("x", ("up", "uld")), ("w", ("off4",)), ("out", ("up", "uld"))):             # va, vb, vec_c of gcnx_gemm
        for lay in lays:
            assert _broken_alone("gemm", "tile_f32", name, lay)
    for name, lays in (("dx", ("up", "uld")), ("y", ("up", "uld"))):                                    # vec_c -> fused_db of gcnx_gemm_dx
        for lay in lays:
            assert _broken_alone("dx", "tile_f32+colsum", name, lay)
    for name, lay in (("x", "up"), ("x", "uld")):                                                       # rowtile_ok
        assert [c for c in _broken_alone("gemm", "tile_f32", name, lay) if c.n == 2049]
    for name, lay in (("dh", "up"), ("dh", "uld"), ("db", "off4")):
        assert [c for c in _broken_alone("dx", "tile_f32+fused_db", name, lay) if c.n == 2049]
    for name, lay in (("dx", "up"), ("dx", "uld"), ("y", "up"), ("db", "off4")):                        # `fused` of dense_bwd_impl
        assert [c for c in G.CASES if c.entry == "dense_bwd" and c.route.startswith("two_calls") and c.lay == {name: lay}]
    for name, lays in (("x", ("up", "uld")), ("dh", ("up", "uld")), ("dw", ("off4",))):                 # dw_job / panels
        for lay in lays:
            assert [c for c in G.CASES if c.entry == "dw" and c.route.startswith("tile_f32") and c.lay == {name: lay}]
            assert [c for c in G.CASES if c.entry == "dw" and c.route == "bf16_tile/splitk" and c.lay == {name: lay} and c.n == 2049]
    for name, lay in (("x", "up"), ("x", "uld"), ("out", "up"), ("out", "uld")):                        # shape_ok of gcnx_gemm_stream_nn
        assert [c for c in _broken_alone("gemm", "bf16_tile", name, lay) if c.n > G.TALL]
    for name, lay in (("dh", "up"), ("dx", "up"), ("y", "up"), ("y", "uld")):
        assert [c for c in _broken_alone("dx", "bf16_tile+colsum", name, lay) if c.n > G.TALL]
    assert _broken_alone("dx", "stream+colsum", "db", "off4")                                           # launch_bf16_nn's second attempt
    for entry, name, lay in (("fwd16", "x", "ld8"), ("fwd16", "bias", "off4"), ("dx16", "dh", "ld8"), ("dx16", "db", "off4"),
                             ("dw16", "x", "ld8"), ("dw16", "dh", "ld8"), ("dw16", "dw", "off4")):      # lda % 8, bias / db, dw_stream_operands_ok
        assert _broken_alone(entry, "unsupported", name, lay)
    assert _broken_alone("bits_pair", "stream/unsupported", "db", "off4") and _broken_alone("bits_pair", "unsupported/stream", "out", "up")


def _mutants(case):
    """For the results of the case that an activation, a bias or a mask shapes: (name, exact result, the result of a subtly wrong
    kernel) -- `>=` for `>` in the mask or the bit image, the bias added behind the activation instead of in front of it."""
    d, o, e = case.data(), case.opt, case.entry
    if o.get("mask"):
        yield "mask >=", d.dx(True)[0], np.where(d.y >= 0, d.dx(False)[0], np.float32(0))
    if e in ("gemm", "fwd16", "wimage") and o.get("act") and o.get("bias") and d.bias.any():     # (fo = 1: the one bias is the zero)
        late = d.fwd(False, o["act"])[1] + d.bias
        yield "bias behind the activation", d.fwd(True, o["act"])[1], late
    if e in ("bits_pair", "pair16"):
        z = d.fwd(True, "relu")[0]
        yield "image >=", d.dx2()[0], np.where(z >= 0, d.dx2(masked=False)[0], np.float32(0))


def _exact_results_tell_subtly_wrong_kernels_apart(case):
    """What the bit comparison is for: in every case with a mask, an image or a biased activation, a kernel that read `>= 0`
    for `> 0`, or added the bias behind the activation, would leave other bits than the exact result (decided on the operands
    alone, here on the host: no wrong kernel is built or run)."""
    if case.route == "unsupported" or case.n == 0:
        return
    for name, exact, wrong in _mutants(case):
        assert exact.shape == wrong.shape and (exact != wrong).any(), name


# (cases that share operands next to each other: a 32 768-row set and its float64 products are formed once)
BY_DATA = sorted(G.CASES, key=lambda c: (c.n, c.fi, c.fo, c.vals()))


@pytest.mark.parametrize("case", BY_DATA, ids=lambda c: c.id)
def test_operands_and_exact_results(case):
    _exact_range(case)
    _outputs_are_not_degenerate(case)
    _exact_results_tell_subtly_wrong_kernels_apart(case)

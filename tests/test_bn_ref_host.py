"""tests/bn_ref.py checked on the host: its float64 references against the oracle's BatchNorm / activation functions, its route
model against the route every case of tests/test_gpu_bn_routes.py names, and its exact-data generator against the claim that
every result it is compared bit for bit on is an fp32 number."""
import numpy as np
import pytest

import bn_ref as R
from test_gpu_bn_routes import CASES, case_id, claim, layouts, rows

CUS = (256, 64)                    # the MI355X and a smaller chip: the shapes that depend on the CU count move with it


def O():
    from oracle import gcn_oracle
    return gcn_oracle


def _close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and float(np.max(np.abs(a - b), initial=0.0)) <= tol * max(1.0, float(np.max(np.abs(b), initial=0.0)))


@pytest.mark.parametrize("n,f", [(1, 3), (50, 7), (700, 67)])
def test_forward_references_agree_with_the_oracle(n, f):
    o = O()
    rng = np.random.default_rng(n + f)
    z = rng.standard_normal((n, f)) * 3 + 5
    gamma, beta, alpha = rng.standard_normal(f), rng.standard_normal(f), rng.random(f)
    mm, mv = rng.standard_normal(f), 0.5 + rng.random(f)
    shift = np.round(z.mean(0))
    # training: two-pass moments, and the one-pass form from (shifted) sums
    zb, cache, omm, omv = o.bn_fwd(z, gamma, beta, mm, mv, True)
    mean, inv, nmm, nmv = R.moments(z, mm, mv)
    assert _close(mean, z.mean(0)) and _close(inv, cache["inv"]) and _close(nmm, omm) and _close(nmv, omv)
    s = R.stats(z)
    zb1, c1, omm1, omv1 = o.bn_fwd(z, gamma, beta, mm, mv, True, sums=(s[0], s[1], n))
    for sh in (None, shift):
        m1, i1, nmm1, nmv1 = R.finalize(R.stats(z, sh), n, sh, mm, mv)
        assert _close(m1, mean) and _close(i1, c1["inv"], 1e-9) and _close(nmm1, omm1) and _close(nmv1, omv1, 1e-9)
    m0, i0, a, b = R.finalize(s, n)
    assert _close(m0, mean) and a is None and b is None
    # inference: the moving statistics, left alone
    zbi, ci, imm, imv = o.bn_fwd(z, gamma, beta, mm, mv, False)
    mi, ii, kmm, kmv = R.finalize(None, 0, None, mm, mv)
    assert np.array_equal(mi, mm) and _close(ii, ci["inv"]) and np.array_equal(kmm, imm) and np.array_equal(kmv, imv)
    # bn_act for the four activations
    assert _close(R.bn_act(z, mean, inv, gamma, beta), zb)
    assert _close(R.bn_act(z, mean, inv, gamma, beta, "relu"), o.act_fwd(zb, "relu"))
    assert _close(R.bn_act(z, mean, inv, gamma, beta, "prelu", alpha), o.act_fwd(zb, "prelu", alpha))
    assert _close(R.bn_act(z, mean, inv, gamma, beta, "prelu_shared", alpha[:1]), o.act_fwd(zb, "prelu", alpha[0]))
    assert _close(R.bn_act(z, mi, ii, gamma, beta, "relu"), o.act_fwd(zbi, "relu"))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act", R.ACTS, ids=lambda a: a or "none")
def test_backward_reference_agrees_with_the_oracle(act, training):
    o = O()
    n, f = 300, 11
    rng = np.random.default_rng(17)
    z, dy = rng.standard_normal((n, f)) * 2 + 1, rng.standard_normal((n, f))
    gamma, beta = rng.standard_normal(f), rng.standard_normal(f)
    alpha = {"prelu": rng.random(f), "prelu_shared": rng.random(1)}.get(act)
    mm, mv = rng.standard_normal(f), 0.5 + rng.random(f)
    zb, cache, _, _ = o.bn_fwd(z, gamma, beta, mm, mv, training)
    mean, inv = (z.mean(0), cache["inv"]) if training else (mm, cache["inv"])
    oact = "prelu" if act == "prelu_shared" else act
    oalpha = None if alpha is None else np.broadcast_to(alpha, (f,))
    dzb = o.act_bwd(dy, zb, oact, oalpha)
    dz, dgamma, dbeta = o.bn_bwd(dzb, cache, gamma)
    got = R.bn_act_bwd(dy, z, mean, inv, gamma, beta, act, alpha, training)
    assert _close(got["dz"], dz, 1e-9) and _close(got["dgamma"], dgamma, 1e-9) and _close(got["dbeta"], dbeta, 1e-9)
    assert np.array_equal(got["sums"][0], got["dbeta"]) and np.array_equal(got["sums"][1], got["dgamma"])
    term = (dy * np.minimum(zb, 0)).sum(0)
    if act == "prelu":
        assert _close(got["dalpha"], term, 1e-9) and np.array_equal(got["sums"][2], got["dalpha"])
    elif act == "prelu_shared":
        assert got["dalpha"].shape == (1,) and _close(got["dalpha"], [term.sum()], 1e-9)
    else:
        assert got["dalpha"] is None and not got["sums"][2].any()
    # the sync-BN halves: dz from reduced sums and a global count, as the oracle's `red`
    if training:
        red = got["sums"] * 3 + 1
        dz2, _, _ = o.bn_bwd(dzb, cache, gamma, red=(red[0], red[1], 4 * n))
        assert _close(R.bn_act_bwd(dy, z, mean, inv, gamma, beta, act, alpha, True, sums=red, count=4 * n)["dz"], dz2, 1e-9)
    # the device's sides are this reference's own wherever the pre-activation is not within rounding of zero
    pos = R.device_sides(z, mean, inv, gamma, beta)
    far = np.abs(zb) > 1e-4
    assert np.array_equal(pos[far], (zb > 0)[far])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_every_case_reaches_the_route_it_names(c):
    for cus in CUS:
        for vec in (True, False):
            for kind in R.KINDS:
                claim(c, kind, vec, cus)
        # layout (b) is aligned, layout (c) is not, the dense one is aligned iff f % 4 == 0
        (_, ld_a, lead_a), (_, ld_b, lead_b), (_, ld_c, lead_c) = layouts(c.f)
        assert ld_a == c.f and lead_a == 0
        assert ld_b % 4 == 0 and lead_b % 4 == 0 and ld_b > c.f
        assert ld_c % 2 == 1 and lead_c in (1, 3) and ld_c >= c.f


def test_the_table_covers_every_route():
    """Done-when of the routes file: small and chunked launches; fast, float4, tail and scalar lanes; the two-row loop in its
    three endings and the tail loop; every empty-group pattern of the chunk reduction -- each by at least one case, for every
    entry point the route applies to."""
    cus = 256
    seen = {k: {"launch": set(), "lanes": set(), "groups": set(), "loops": set(), "alanes": set()} for k in R.KINDS}
    for c in CASES:
        for kind in R.KINDS:
            for vec in (True, False):
                r = R.route(kind, rows(c, cus), c.f, vec, cus)
                s = seen[kind]
                s["launch"].add(r["launch"])
                s["lanes"] |= set(r["lanes"] or ())
                if r["launch"] == "chunked":
                    s["groups"].add((r["empty"], r["short"] is not None))
                if r["apply"]:
                    s["loops"].add(r["apply"]["loops"].split(",")[0] + ("=" if r["apply"]["exact_fit"] else ""))
                    s["alanes"] |= set(r["apply"]["lanes"])
    lanes = {"fast", "float4", "tail", "scalar"}
    groups = {((1, 2, 3), False), ((2, 3), False), ((3,), False), ((3,), True)}       # nchunks 1; 2; 3, 6, 9; 5
    loops = {"tail", "two_row", "two_row=", "two_row+tail"}
    assert seen["moments"]["launch"] == {"small", "chunked"} and seen["bn_act_bwd"]["launch"] == {"small", "chunked"}
    for kind in ("stats", "moments", "bn_act_bwd", "bwd_stats"):
        assert seen[kind]["lanes"] == lanes, kind
        assert groups <= seen[kind]["groups"] or kind in ("moments", "bn_act_bwd"), kind
        assert groups - {((1, 2, 3), False)} <= seen[kind]["groups"], kind            # one chunk is the small launch there
    for kind in ("bn_act", "bn_act_bwd", "bwd_apply"):
        assert seen[kind]["loops"] == loops, kind
        assert seen[kind]["alanes"] == {"float4", "tail", "scalar"}, kind
    nchunks = {R.route("stats", c.n, c.f, True, cus)["nchunks"] for c in CASES if isinstance(c.n, int)}
    assert {1, 2, 3, 5, 6, 9} <= nchunks
    assert {a for c in CASES for a in [c.act]} == set(R.ACTS)


def test_route_thresholds():
    """The rules themselves, at their edges."""
    cus = 256
    step = 32 * cus
    assert R.route("moments", 256, 64, True, cus)["launch"] == "small" and R.route("moments", 257, 64, True, cus)["launch"] == "chunked"
    assert R.route("stats", 256, 64, True, cus)["launch"] == "chunked"
    assert R.route("bn_act_bwd", 256, 64, True, cus)["apply"] is None and R.route("bn_act_bwd", 257, 64, True, cus)["apply"] is not None
    assert R.route("stats", 7, 64, True, cus)["lanes"] == {"fast"} and R.route("stats", 7, 63, True, cus)["lanes"] == {"float4", "tail"}
    assert R.route("stats", 7, 64, False, cus)["lanes"] == {"scalar"}
    assert R.route("stats", 7, 68, True, cus)["lanes"] == {"fast", "float4"}
    assert R.route("bn_act", step, 256, True, cus)["apply"]["loops"] == "tail"            # n > step is strict
    assert R.route("bn_act", step + 1, 256, True, cus)["apply"]["loops"] == "two_row"
    assert R.route("bn_act", step + 1, 255, True, cus)["apply"]["loops"] == "tail"        # no full tile
    assert R.route("bn_act", step + 1, 256, False, cus)["apply"]["loops"] == "tail"
    assert R.route("bn_act", 2 * step, 256, True, cus)["apply"]["exact_fit"] and not R.route("bn_act", 2 * step + 1, 256, True, cus)["apply"]["exact_fit"]
    assert R.route("bn_act", 4 * step, 256, True, cus)["apply"]["exact_fit"]
    assert R.route("bn_act", 100, 256, True, cus)["apply"]["step"] == 100 and R.route("bn_act", 101, 256, True, cus)["apply"]["step"] == 104
    for nchunks, want in ((1, (1, (1, 2, 3), None)), (2, (1, (2, 3), None)), (3, (1, (3,), None)), (4, (1, (), None)),
                          (5, (2, (3,), 2)), (6, (2, (3,), None)), (7, (2, (), 3)), (9, (3, (3,), None)), (12, (3, (), None)),
                          (79, (20, (), 3))):
        r = R.route("stats", 256 * nchunks, 8, True, cus)
        assert (r["per"], r["empty"], r["short"]) == want, nchunks


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_exact_data_results_are_fp32_numbers(c):
    """On the generator's data, at every shape of the table: every term is a multiple of 1/8 whose column magnitudes stay below
    2^24 / 8 (so every partial sum, in any order, is exact), and every sum, every y and every inference-mode dz the GPU tests
    compare bit for bit is an fp32 number."""
    for cus in CUS:
        n, f = rows(c, cus), c.f
        for seed in (1000, 2000):                                  # the forward and the backward test's draws
            d = R.exact_data(n, f, seed + CASES.index(c))
            for k in ("inv", "gamma"):
                m, e = np.frexp(d[k])
                assert np.all(np.abs(m) == 0.5), k                 # powers of two
            assert set(np.unique(d["alpha"])) <= {0.25, 0.5} and np.abs(d["z"]).max() <= 3 and np.abs(d["dy"]).max() <= 3
            acts = R.ACTS if n <= 2305 else (c.act,)
            for act in acts:
                al = R.alpha_of(d, act)
                R.assert_exact(d, act)
                host = (d["mean"], d["inv"], d["gamma"], d["beta"])
                assert R.is_f32(R.stats(d["z"])) and R.is_f32(R.stats(d["z"], d["shift"]))
                assert R.is_f32(R.bn_act(d["z"], *host, act, al))
                w = R.bn_act_bwd(d["dy"], d["z"], *host, act, al, training=False)
                assert R.is_f32(w["sums"]) and R.is_f32(w["dz"])
                assert w["dalpha"] is None or R.is_f32(w["dalpha"])

"""tests/head_ref.py checked on the host: its float64 head against the oracle's softmax / cce and against torch.autograd, its
route model against the route every case of tests/test_gpu_head_routes.py names, and the conditions on the data that let the
GPU tests compare hits exactly and trust the clip mask."""
import numpy as np
import pytest

import head_ref as R
from test_gpu_head_routes import (CASES, DENSE_CASES, GAUSS, KNOBS, POOL_CASES, POOLED_CASES, case_id, claim, data, graphs,
                                  layouts, variants, x_layout)

CUS = (256, 64, 304)               # the MI355X, a smaller and a larger chip: the shapes that depend on the CU count move with it


def O():
    from oracle import gcn_oracle
    return gcn_oracle


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and float(np.max(np.abs(a - b), initial=0.0)) <= tol * max(1.0, float(np.max(np.abs(b), initial=0.0)))


def _labels(kind, b, c, rng):
    if kind == "one-hot":
        return np.eye(c)[rng.integers(0, c, b)]
    y = rng.random((b, c)) + 0.1                                     # soft: rows that do not sum to one
    if kind == "zero-row":
        y[b // 2] = 0.0
    return y


def _problem(b, h, c, kind, seed):
    rng = np.random.default_rng(seed)
    pooled = 3 * rng.standard_normal((b, h))
    w = rng.standard_normal((h, c)) / np.sqrt(h)
    bias = rng.standard_normal(c)
    y = _labels(kind, b, c, rng)
    if c == 2:                                                       # saturated graphs: where the two cce modes differ
        pooled[0] = 0; pooled[0, 0] = 400.0; w[0] = [1.0, -1.0]
        pooled[1] = 0; pooled[1, 0] = -30.0
        y[0] = [0, 1]; y[1] = [1, 0]
    return pooled, w, bias, y


@pytest.mark.parametrize("cce", ["logits", "probs"])
@pytest.mark.parametrize("kind", ["one-hot", "soft", "zero-row"])
@pytest.mark.parametrize("b,h,c", [(1, 4, 1), (40, 16, 2), (50, 7, 3), (33, 20, 32)])
def test_head_agrees_with_the_oracle(b, h, c, kind, cce):
    """The same calls tests/test_gpu_kernels.py makes through O(): softmax, cce (loss and dlogits), categorical_accuracy."""
    o = O()
    pooled, w, bias, y = _problem(b, h, c, kind, b + c)
    denom = float(b + 3)
    r = R.head(pooled, w, bias, y, denom, cce)
    z = pooled @ w + bias
    p = o.softmax(z)
    loss, dl = o.cce(y, z, p, denom, cce)
    assert _close(r["probs"], p) and _close(r["loss"], loss) and _close(r["dlogits"], dl)
    assert r["hits"] == round(o.categorical_accuracy(y, p) * b)
    assert _close(r["dw"], pooled.T @ dl) and _close(r["db"], dl.sum(0)) and _close(r["dpooled"], dl @ w.T)
    ymsum = (r["probs"] * 0 + y).sum(1)
    assert (kind == "one-hot") == bool(np.allclose(ymsum, 1.0)), "one-hot rows sum to one, soft rows do not"
    if kind == "zero-row" and cce == "logits":
        assert not r["dlogits"][b // 2].any()                        # p * 0 - 0
    if c == 2:                                                       # the clipped rows get no gradient in the eager form only
        assert (not r["dlogits"][0].any()) == (cce == "probs") and (not r["dlogits"][1].any()) == (cce == "probs")
    assert list(R.head(pooled, w, bias, None, denom, cce)) == ["probs"]


@pytest.mark.parametrize("cce", ["logits", "probs"])
@pytest.mark.parametrize("kind", ["one-hot", "soft", "zero-row"])
def test_head_gradients_agree_with_autograd(kind, cce):
    import torch
    b, h, c = 24, 9, 5
    rng = np.random.default_rng(5)
    pooled, w, bias = rng.standard_normal((b, h)), rng.standard_normal((h, c)) / 3, rng.standard_normal(c)
    pooled[0] *= 40                                                  # one row beyond the clip
    y = _labels(kind, b, c, rng)
    denom = float(b + 3)
    P, W, B = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (pooled, w, bias))
    Y = torch.tensor(y, dtype=torch.float64)
    z = P @ W + B
    if cce == "logits":
        loss = (Y * (torch.logsumexp(z, 1, keepdim=True) - z)).sum() / denom
    else:
        loss = -(Y * torch.log(torch.clamp(torch.softmax(z, 1), 1e-7, 1 - 1e-7))).sum() / denom
    loss.backward()
    r = R.head(pooled, w, bias, y, denom, cce)
    assert r["probs"].min() < 1e-7                                   # the clip is reached
    assert _close(r["loss"], loss.item(), 1e-11)
    assert _close(r["dw"], W.grad.numpy(), 1e-10) and _close(r["db"], B.grad.numpy(), 1e-10) and _close(r["dpooled"], P.grad.numpy(), 1e-10)


@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_db_relu_from_counts_is_the_pool_backward_column_sum(mode):
    """pooled_head's db_relu (from counts) and pool_head's (reduce_ref.pool_bwd_colsum over x) are the same sum."""
    d = R.gauss_data(9, 12, 3, mode, 77)
    a = R.pool_head(d["x"], d["gp"], mode, d["w"], d["bias"], d["y"], 12.0, "logits", db_relu=True)
    b = R.pooled_head(d["pooled"], d["cnt"], d["gp"], mode, d["w"], d["bias"], d["y"], 12.0, "logits", db_relu=True)
    assert np.array_equal(a["pooled"], d["pooled"]) and _close(a["dw"], b["dw"])
    assert _close(a["db_relu"], b["db_relu"], 1e-6)                  # pool_bwd_colsum rounds its terms to fp32
    assert np.diff(d["gp"]).min() == 0 and R.is_f32(d["cnt"]) and np.array_equal(d["cnt"], np.round(d["cnt"]))


# ------------------------------------------------------------------------------------------- the data of the GPU file
@pytest.mark.parametrize("k", CASES + GAUSS, ids=case_id)
def test_data_conditions(k):
    """No probability of a non-saturated row near the clip, min p < 1e-10 in the saturated rows (one labelled correctly, one
    not), no two classes within 1e-4 -- on every row of every case, for every chip size its shape depends on."""
    for cus in CUS if k.b == "2cus" else CUS[:1]:
        d = data(k, cus)
        b = graphs(k, cus)
        assert d["pooled"].shape == (b, k.h) and d["y"].shape == (b, k.c) and d["gp"][-1] == d["x"].shape[0]
        R.check_conditions(d, float(b + 3), k.dbr is not None)
        print(case_id(k), cus, "seed", d["seed"], {key: round(v, 1) for key, v in R.conditioning(d, float(b + 3), "logits", k.dbr is not None).items()} if b else "")
        assert d["sat"].any() == (k not in GAUSS and k.h >= 4 and k.c == 2 and b >= 2)
        if k in GAUSS:
            continue
        assert np.abs(d["x"]).max(initial=0) <= R.SAT and np.array_equal(d["x"], np.round(d["x"])) and (d["x"] == 0).any() == (d["x"].size > 0)
        if d["x"].size:
            assert (d["x"] > 0).any() and (d["x"] < 0).any()
        if k.mode == "sum":                                          # integers below 2^24: exact in any order
            assert np.abs(d["x"]).sum(0).max(initial=0) < 2 ** 24 and R.is_f32(d["pooled"])
        if k.soft:
            assert not np.allclose(d["y"].sum(1), 1.0)
        if k.sizes == "mixed" and b >= 5:
            n = np.diff(d["gp"])
            assert n[b // 2] == 0 and n[-1] == 0 and (n == 1).any() and n.max() >= 17


def test_conditioning_sees_cancellation():
    """h == 0: every graph has the probabilities softmax(bias), and label counts that match them cancel db."""
    b, c = 40, 2
    d = R.exact_data(b, 0, c, "sum", 1)
    d["bias"] = np.zeros(c, R.F32)
    d["y"] = np.eye(c, dtype=R.F32)[np.arange(b) % 2]                # 20 + 20 labels against p = (0.5, 0.5): db == 0
    assert R.conditioning(d, 43.0, "logits")["db"] == 0.0            # an exact zero is not a rounded sum
    d["y"][0] = [0, 1]                                               # 19 + 21: db = -+1 / 43 from terms that sum to 20 / 43
    assert abs(R.conditioning(d, 43.0, "logits")["db"] - 20.0) < 1e-9
    d["bias"] = np.array([0.001, 0.0], R.F32)
    d["y"] = np.eye(c, dtype=R.F32)[np.arange(b) % 2]
    assert R.conditioning(d, 43.0, "logits")["db"] > R.COND_MAX
    with pytest.raises(AssertionError, match="ill-conditioned"):
        R.check_conditions(d, 43.0)


# ------------------------------------------------------------------------------------------- the routes
def _records(cus):
    for k in CASES + GAUSS:
        for grads, _ in variants(k):
            for li in range(3):
                yield k, grads, li, claim(k, li, grads, cus)


@pytest.mark.parametrize("cus", CUS)
def test_every_case_reaches_the_route_it_names_and_the_table_covers_every_route(cus):
    seen = {key: set() for key in ("route", "kernel", "ct", "nblk", "nsplit", "slabs", "st4")}
    combos = set()
    for k, grads, li, r in _records(cus):
        for key in seen:
            seen[key].add(r[key])
        combos.add((k.entry, r["route"], r["kernel"], r["ct"], grads))
    assert seen["route"] == {"fused", "counts", "calls", "dense"}
    assert seen["kernel"] == {"parts", "staged", "global", None}
    assert seen["ct"] == {"ct2", "generic", None}
    assert {1, 2, 7, 8, 9, 18} <= seen["nblk"] and 0 in seen["nblk"]
    assert set(KNOBS[1:]) | {1} <= seen["nsplit"]
    assert seen["slabs"] == {True, False} and seen["st4"] == {True, False, None}
    for grads in R.GRADS:                                            # every kind of call on one and on several workgroups
        assert ("dense", "dense", "staged", "ct2", grads) in combos and ("dense", "dense", "global", "generic", grads) in combos
        assert ("pool", "fused", "parts", "ct2", grads) in combos and ("pool", "fused", "parts", "generic", grads) in combos
    assert ("pool", "calls", "global", "generic", "train") in combos and ("pool", "counts", "staged", "ct2", "train") in combos
    # the default slice count of the fused route differs from every forced one on the MI355X
    if cus == 256:
        assert {R.pool_split(cus, b, h, "sum", 1) for b, h in ((5, 200), (33, 128), (70, 64))} == {7, 2}


def test_layouts_and_section_lists():
    for h in sorted({k.h for k in CASES}):
        (_, ld_a, lead_a), (_, ld_b, lead_b), (_, ld_c, lead_c) = layouts(h)
        assert ld_a == h and lead_a == 0
        assert ld_b % 4 == 0 and lead_b % 4 == 0 and ld_b > h
        assert ld_c % 2 == 1 and lead_c in (1, 3) and ld_c >= h and (h == 0 or ld_c > h)
    k = POOL_CASES[0]
    assert x_layout(k._replace(x="aligned"), 2)[2] % 4 == 0 and x_layout(k._replace(x="off1"), 0)[2] % 4 == 1
    assert x_layout(k._replace(x="off1"), 0)[1] % 4 == 0
    dense = [k for k in DENSE_CASES if k.name.startswith("wgs-")]
    assert [k.b for k in dense] == [1, 31, 32, 33, 224, 256, 257, 545] and [R.cdiv(k.b, 32) for k in dense] == [1, 1, 1, 2, 7, 8, 9, 18]
    assert all(k.h == 64 and k.c == 2 for k in dense)
    assert {k.c for k in DENSE_CASES} >= {1, 2, 3, 9, 32}
    assert {k.h for k in DENSE_CASES} >= {0, 1, 3, 4, 63, 64, 65, 130}
    assert {(k.h * k.c > 256) for k in DENSE_CASES if k.h} == {True, False}
    assert {k.b for k in POOLED_CASES} == {0, 1, 33, 257} and {k.mode for k in POOLED_CASES} == {"sum", "avg"}
    fused = [k for k in POOL_CASES if k.want == ("fused",) * 3]
    assert {(k.b, k.knob, k.mode, k.dbr) for k in fused} >= {(b, kn, m, d) for b in (5, 33, 70) for kn in KNOBS for m in ("sum", "avg")
                                                            for d in (None, "aligned")}
    calls = {k.name for k in POOL_CASES if "calls" in k.want}
    assert len(calls) >= 10 and {k.mode for k in POOL_CASES} == {"sum", "avg", "max"}


def test_staging_edges():
    """The last staged and the first unstaged shapes, from head_lds_floats restated."""
    lim = R.HEAD_LDS_FLOATS
    assert lim == 14 * 1024 and R.head_lds_floats(64, 2, False) == 32 * 65 + 128
    for h, c in ((420, 2), (408, 3), (223, 32)):
        assert R.head_lds_floats(h, c, False) <= lim < R.head_lds_floats(h + 1, c, False), (h, c)
        assert R.route("dense", 33, h, c, 256)["kernel"] == "staged" and R.route("dense", 33, h + 1, c, 256)["kernel"] == "global"
    # the fused call with db_relu and two classes: widths are multiples of 4
    assert R.head_lds_floats(200, 2, True) <= lim < R.head_lds_floats(204, 2, True) and R.head_lds_floats(204, 2, False) <= lim
    for cus in CUS:
        assert R.route("pool", 5, 200, 2, cus, dbr="aligned")["route"] == "fused"
        assert R.route("pool", 5, 204, 2, cus, dbr="aligned")["route"] == "calls"
        assert R.route("pool", 5, 204, 2, cus)["route"] == "fused" and R.route("pool", 5, 204, 2, cus, grads="nodb")["route"] == "fused"


def test_route_thresholds():
    """The rules themselves, at their edges."""
    for cus in CUS:
        b = 2 * cus
        assert R.pool_split(cus, b - 1, 64, "sum", 1) == 2 and R.pool_split(cus, b, 64, "sum", 1) == 1
        assert R.pool_split(cus, b - 1, 64, "sum", 1, knob=16) == 16 and R.pool_split(cus, b, 64, "sum", 1, knob=16) == 1
        assert R.pool_split(cus, 1, 64, "avg", 4) == 16 and R.pool_split(cus, 1, 64, "max", 4) == 1
        assert R.pool_split(cus, 1, 64, "sum", 1, knob=1) == 16 and R.pool_split(cus, 1, 64, "sum", 1, knob=17) == 16
        common = dict(dbr="aligned")
        assert R.route("pool", b, 64, 2, cus, **common)["route"] == "counts"
        assert R.route("pool", b - 1, 64, 2, cus, **common)["route"] == "fused"
        assert R.route("pool", b, 64, 2, cus, ldp=72, **common)["route"] == "calls"
        assert R.route("pool", b, 64, 2, cus, dbr="unaligned")["route"] == "calls"
        assert R.route("pool", b, 64, 2, cus)["route"] == "calls"                       # nothing to count for
        assert R.route("pool", b, 64, 2, cus, mode="max")["route"] == "calls"
        assert R.route("pool", 4096, 8, 2, cus, **common)["route"] == "counts" and R.route("pool", 4097, 8, 2, cus, **common)["route"] == "calls"
        assert R.route("pool", 33, 64, 2, cus, x_aligned=False, **common)["route"] == "calls"
        assert R.route("pool", 33, 66, 2, cus, **common)["route"] == "calls"
        r = R.route("pool", 33, 64, 2, cus, ldp=67, pooled_aligned=False)
        assert r["route"] == "fused" and r["st4"] is False and R.route("pool", 33, 64, 2, cus, ldp=72)["st4"] is True
        assert R.route("pool", 33, 64, 2, cus, ldp=72, pooled_aligned=False)["st4"] is False
    assert R.route("dense", 32, 64, 2, 256)["slabs"] is False and R.route("dense", 33, 64, 2, 256)["slabs"] is True
    assert R.route("dense", 33, 64, 2, 256, grads="infer")["slabs"] is False and R.route("dense", 33, 64, 2, 256, grads="loss")["slabs"] is True
    assert R.route("dense", 33, 64, 3, 256)["ct"] == "generic" and R.route("dense", 33, 421, 2, 256)["ct"] == "generic"
    assert R.route("pooled", 0, 64, 2, 256, dbr="aligned")["kernel"] is None

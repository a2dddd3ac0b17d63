"""Every launch route of the classifier head of csrc/head.hip -- gcnx_dense_softmax_cce, gcnx_pooled_dense_softmax_cce,
gcnx_pool_dense_softmax_cce -- on strided views inside sentinel frames, against the float64 reference of tests/head_ref.py.

A call picks its code path from b, h, c, the pool mode and the CU count, from the alignment of x, pooled and db_relu, from
ldp == h, from which of db_relu / dw / db / y are given and from the pool_split knob.  CASES names, per shape, the entry route
(fused / counts / calls / dense) and the kernel variant (parts / staged / global) it is there for; every call asserts through
head_ref.route(...) that it reaches them (shapes that depend on the chip are derived from cus = ctx.info()["cus"]), so a later
change of a threshold fails loudly.

Each case runs in three layouts of x, pooled and dpooled: (a) dense, (b) an aligned base with ld = h + pad, ld % 4 == 0,
(c) a view 1 or 3 elements into its buffer with an odd ld.  w, bias, y, probs, dw, db, loss_acc, cnt and db_relu are contiguous
by contract and live in frames with a lead.  Inputs must come back untouched, outputs must leave their sentinels intact.

Inputs are head_ref.exact_data: small integers in x, so pooled (SUM, AVG, MAX; an empty graph's zero row included) must equal
the reference BIT FOR BIT on every route; hits is an exact integer (tests/test_head_ref_host.py checks that no two
probabilities of a row are within 1e-4 and that no fp32 rounding can flip the PROBS-mode clip mask); loss_acc is pre-filled
with 7 and must be overwritten.  probs, dw, db, dpooled and db_relu meet float64 at TIGHT, loss within 2e-5 max(1, |loss|);
the seed of a case is the first of its sequence on which no sum is conditioned worse than head_ref.COND_MAX (chosen from
the reference alone), so that bar measures the kernel and not the cancellation in the draw.
Every call runs twice: all outputs agree bit for bit.  gcnx_dense_softmax_cce must give the same bits in the three layouts
(its route does not depend on them); for the pool-fused entry point the layout changes the route, so db_relu is held to TIGHT
across layouts.  Every case runs "train" (dw, db, dpooled) in both cce modes; cases without db_relu also run "nodb" (db NULL),
"loss" (dw NULL: the slabs hold the two sums alone) and "infer" (y NULL).  denom is b + 3: a shard of a larger batch."""
from collections import namedtuple

import numpy as np
import pytest

import head_ref as R
from conftest import assert_close, rel_err
from gpu_frames import Frame, same

pytestmark = pytest.mark.gpu

TIGHT = 2e-5                       # as tests/test_gpu_kernels.py holds these calls to
F32 = np.float32

# b: a graph count, or "2cus": 2 cus / cdiv(h, 64), the first count the stand-alone pool does not split at.
# x: the layout of x for gcnx_pool_dense_softmax_cce -- "follow" (as pooled), "aligned" (layout (b) whatever pooled's is) or
# "off1" (ld % 4 == 0, the base one element past an aligned address).  dbr: None, "aligned" or "unaligned" (db_relu's base).
# dlay: the layout of dpooled where it is not pooled's.  want: the entry route in layouts (a), (b), (c); kernel: the head
# kernel of the training call.
Case = namedtuple("Case", "name entry b h c mode sizes knob x dbr dlay want kernel soft")


def _case(name, entry, b, h, c, want, kernel, mode="sum", sizes="small", knob=0, x="follow", dbr=None, dlay=None, soft=False):
    want = (want,) * 3 if isinstance(want, str) else tuple(want)
    return Case(name, entry, b, h, c, mode, sizes, knob, x, dbr, dlay, want, kernel, soft)


def _dense_cases():
    out = []
    for b in (1, 31, 32, 33, 224, 256, 257, 545):                                   # nblk 1, 1, 1, 2, 7, 8, 9, 18
        out.append(_case("wgs-b%d" % b, "dense", b, 64, 2, "dense", "staged"))
    for c in (1, 3, 9, 32):                                                         # (2: above); 32 rows x 9 classes > 256 labels
        out.append(_case("classes-c%d" % c, "dense", 33, 64, c, "dense", "staged"))
    for h, c in ((0, 2), (1, 2), (3, 2), (4, 2), (63, 2), (65, 2), (130, 2), (65, 3), (130, 9)):
        out.append(_case("width-h%dc%d" % (h, c), "dense", 33, h, c, "dense", "staged"))
    for h, c, kernel in ((420, 2, "staged"), (421, 2, "global"), (408, 3, "staged"), (409, 3, "global"), (223, 32, "staged"),
                         (224, 32, "global")):
        out.append(_case("edge-h%dc%d" % (h, c), "dense", 33, h, c, "dense", kernel))
    out.append(_case("soft-labels", "dense", 33, 64, 3, "dense", "staged", soft=True))
    return out


def _pooled_cases():
    out = []
    for b in (0, 1, 33, 257):
        for mode in ("sum", "avg"):
            for dbr in (None, "aligned"):
                out.append(_case("b%d-%s-%s" % (b, mode, "dbr" if dbr else "plain"), "pooled", b, 64, 2, "dense",
                                 "staged" if b else None, mode=mode, dbr=dbr))
    return out


FUSED_SHAPES = {5: (200, 204), 33: (128, 128), 70: (64, 64)}       # b: h with db_relu (200: the last fused width), h without
KNOBS = (0, 2, 3, 4, 5, 16)


def _pool_cases():
    out = []
    for b in (5, 33, 70):
        for knob in KNOBS:
            for mode in ("sum", "avg"):
                for dbr in ("aligned", None):
                    h = FUSED_SHAPES[b][0 if dbr else 1]
                    out.append(_case("fused-b%d-k%d-%s-%s" % (b, knob, mode, "dbr" if dbr else "plain"), "pool", b, h, 2, "fused",
                                     "parts", mode=mode, sizes="mixed", knob=knob, x="aligned", dbr=dbr))
    for dbr in ("aligned", None):                                                   # a run-time class count on the fused route
        out.append(_case("fused-c3-%s" % ("dbr" if dbr else "plain"), "pool", 33, 128, 3, "fused", "parts", mode="avg",
                         sizes="mixed", x="aligned", dbr=dbr))
    # the pool's own count of positive entries: many graphs, ldp == h, an aligned db_relu.  Layouts (b) and (c) have ldp > h:
    # the separate calls, which must write pooled at stride ldp
    for mode in ("sum", "avg"):
        out.append(_case("counts-%s" % mode, "pool", "2cus", 64, 2, ("counts", "calls", "calls"), "staged", mode=mode, dbr="aligned"))
    out.append(_case("counts-lddp", "pool", "2cus", 64, 2, ("counts", "calls", "calls"), "staged", dbr="aligned", dlay=1))
    # the separate calls, one case per reason
    out.append(_case("calls-unaligned-db_relu", "pool", "2cus", 64, 2, "calls", "staged", dbr="unaligned"))
    out.append(_case("calls-max", "pool", 6, 32, 2, "calls", "staged", mode="max", sizes="mixed"))
    out.append(_case("calls-x-off1", "pool", 33, 64, 2, "calls", "staged", sizes="mixed", x="off1", dbr="aligned"))
    out.append(_case("calls-h66", "pool", 33, 66, 2, "calls", "staged", mode="avg", sizes="mixed", x="aligned", dbr="aligned"))
    out.append(_case("calls-wide", "pool", 3, 600, 2, "calls", "global", sizes="mixed", x="aligned", dbr="aligned"))
    out.append(_case("calls-b4097", "pool", 4097, 8, 2, "calls", "staged", sizes="ones", x="aligned", dbr="aligned"))
    out.append(_case("calls-h204-dbr", "pool", 5, 204, 2, "calls", "staged", mode="avg", sizes="mixed", x="aligned", dbr="aligned"))
    return out


DENSE_CASES, POOLED_CASES, POOL_CASES = _dense_cases(), _pooled_cases(), _pool_cases()
CASES = DENSE_CASES + POOLED_CASES + POOL_CASES
# one Gaussian run per entry point: (case, seed)
GAUSS = [_case("gauss-dense", "dense", 257, 65, 3, "dense", "staged"),
         _case("gauss-pooled", "pooled", 33, 64, 2, "dense", "staged", mode="avg", sizes="mixed", dbr="aligned"),
         _case("gauss-pool-fused", "pool", 33, 128, 2, "fused", "parts", sizes="mixed", x="aligned", dbr="aligned"),
         _case("gauss-pool-calls", "pool", 33, 66, 3, "calls", "staged", mode="avg", sizes="mixed", dbr="aligned")]


def case_id(k):
    return "%s-%s" % (k.entry, k.name)


def graphs(k, cus):
    return 2 * cus // R.cdiv(k.h, 64) if k.b == "2cus" else k.b


def seed_of(k):
    return 1000 + (CASES + GAUSS).index(k)


def data(k, cus):
    """The case's data: the first seed of its sequence on which head_ref.check_conditions holds on every row."""
    make = R.gauss_data if k in GAUSS else R.exact_data
    b = graphs(k, cus)
    return R.pick(lambda seed: make(b, k.h, k.c, k.mode, seed, sizes=k.sizes, soft=k.soft), seed_of(k), float(b + 3),
                  db_relu=k.dbr is not None)


def variants(k):
    """(grads, cce) of the calls a case makes.  db_relu needs dw, so a case with db_relu makes the training calls alone (its twin
    without db_relu makes the others)."""
    v = [("train", "logits"), ("train", "probs"), ("nodb", "probs")]
    return v if k.dbr else v + [("loss", "logits"), ("loss", "probs"), ("infer", "logits")]


def layouts(f):
    """(name, ld, lead): (a) dense; (b) an aligned base and ld % 4 == 0 with padding; (c) 1 or 3 elements in, an odd ld."""
    return [("dense", f, 0), ("aligned view", (f + 3) // 4 * 4 + 8, 4), ("unaligned view", (f | 1) + 2, 1 if f % 2 else 3)]


def x_layout(k, li):
    ld4 = (k.h + 3) // 4 * 4 + 8
    return {"follow": layouts(k.h)[li], "aligned": ("aligned view", ld4, 4), "off1": ("one element off", ld4, 5)}[k.x]


def claim(k, li, grads, cus):
    """The route of this call is the one the table names; returns the record."""
    name, ld, lead = layouts(k.h)[li]
    r = R.route(k.entry, graphs(k, cus), k.h, k.c, cus, mode=k.mode, grads=grads, dbr=k.dbr if grads in ("train", "nodb") else None,
                x_aligned=x_layout(k, li)[2] % 4 == 0, ldp=ld, pooled_aligned=lead % 4 == 0, knob=k.knob)
    what = (case_id(k), name, grads, cus, r)
    assert r["route"] == k.want[li], what
    assert r["kernel"] == k.kernel and (r["ct"] is None or (r["ct"] == "ct2") == (k.c == 2 and k.kernel != "global")), what
    assert r["nblk"] == R.cdiv(graphs(k, cus), 32), what
    if r["route"] == "fused":
        assert r["nsplit"] > 1 and (k.knob == 0 or r["nsplit"] == k.knob), what
        assert r["st4"] == (li < 2 and ld % 4 == 0), what
    else:
        assert r["nsplit"] == 1 and r["st4"] is None, what
    return r


def _vector(ctx, size, data=None, lead=3):
    """A contiguous [size] device vector inside a frame (lead = 3: an unaligned base unless the contract asks for one)."""
    return Frame(ctx, 1, size, size, lead, None if data is None else np.asarray(data, F32))


# ------------------------------------------------------------------------------------------- one call
def _run(ctx, k, d, li, grads, cce, cus, seg):
    """One call of case k in layout li; returns its outputs after checking every frame."""
    from gcnx import device as D
    name, ld, lead = layouts(k.h)[li]
    b, h, c = graphs(k, cus), k.h, k.c
    r = claim(k, li, grads, cus)
    train = grads in ("train", "nodb")
    what = (case_id(k), name, grads, cce)
    w, bias = Frame(ctx, h, c, c, 3, d["w"]), _vector(ctx, c, d["bias"])
    y = Frame(ctx, b, c, c, 3, d["y"]) if grads != "infer" else None
    ins = [w, bias] + ([y] if y else [])
    probs, la = Frame(ctx, b, c, c, 3), _vector(ctx, 2, [7.0, 7.0])
    dw = Frame(ctx, h, c, c, 3) if train else None
    db = _vector(ctx, c) if grads == "train" else None
    _, dld, dlead = layouts(h)[li if k.dlay is None else k.dlay]
    dp = Frame(ctx, b, h, dld, dlead) if train else None
    dbr = _vector(ctx, h, lead=4 if k.dbr == "aligned" else 3) if train and k.dbr else None
    assert dbr is None or (dbr.view.ptr % 16 == 0) == (k.dbr == "aligned")
    kw = dict(loss_acc=la.row(0), denom=float(b + 3), cce=cce, dw=dw.view if dw else None, db=db.row(0) if db else None,
              dpooled=dp.view if dp else None)
    args = (w.view, bias.row(0), y.view if y else None, probs.view)
    pout = arg = None
    if k.entry == "dense":
        pin = Frame(ctx, b, h, ld, lead, d["pooled"])
        ins.append(pin)
        D.dense_softmax_cce(ctx, pin.view, *args, **kw)
    elif k.entry == "pooled":
        pin = Frame(ctx, b, h, ld, lead, d["pooled"])
        cnt = Frame(ctx, b, h, h, 3, d["cnt"]) if dbr else None
        ins += [pin] + ([cnt] if cnt else [])
        D.pooled_dense_softmax_cce(ctx, seg, pin.view, cnt.view if cnt else None, *args, mode=k.mode,
                                   db_relu=dbr.row(0) if dbr else None, **kw)
    else:
        xname, xld, xlead = x_layout(k, li)
        x = Frame(ctx, d["x"].shape[0], h, xld, xlead, d["x"])
        assert (x.view.ptr % 16 == 0) == (xlead % 4 == 0)
        ins.append(x)
        pout = Frame(ctx, b, h, ld, lead)
        assert (pout.view.ptr % 16 == 0) == (lead % 4 == 0)
        arg = ctx.to_device(np.full((b, h), -7, np.int32)) if k.mode == "max" else None
        D.pool_dense_softmax_cce(ctx, seg, x.view, pout.view, *args, mode=k.mode, argmax=arg, db_relu=dbr.row(0) if dbr else None, **kw)
    out = {"route": r["route"], "probs": probs.numpy(), "la": la.numpy()[0]}
    for key, fr in (("dw", dw), ("dpooled", dp), ("pooled", pout)):
        if fr is not None:
            out[key] = fr.numpy()
    for key, fr in (("db", db), ("db_relu", dbr)):
        if fr is not None:
            out[key] = fr.numpy()[0]
    if arg is not None:
        out["argmax"] = arg.numpy()
    for fr in ins:
        fr.untouched(what)
    return out


def _same_outputs(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        if key != "route":
            assert same(np.asarray(a[key], F32), np.asarray(b[key], F32)), (what, key)


def _check(out, ref, d, k, grads, what, exact=True):
    b = d["pooled"].shape[0]
    assert_close(out["probs"], ref["probs"], TIGHT, (what, "probs"))
    if "pooled" in out:
        if exact:
            assert same(out["pooled"], ref["pooled"]), (what, "pooled")
        else:
            assert_close(out["pooled"], ref["pooled"], TIGHT, (what, "pooled"))
    if "argmax" in out:
        nonempty = np.diff(d["gp"]) > 0
        assert np.array_equal(out["argmax"][nonempty], ref["argmax"][nonempty]), (what, "argmax")
    loss, hits = out["la"]
    if grads == "infer":
        assert loss == 7.0 and hits == 7.0, (what, "loss_acc written without labels")
        return
    print(what, "loss", float(loss), "reference", ref["loss"], "hits", float(hits), ref["hits"])
    assert abs(float(loss) - ref["loss"]) < 2e-5 * max(1.0, abs(float(loss))), (what, "loss", loss, ref["loss"])
    assert float(hits) == ref["hits"], (what, "hits", hits, ref["hits"])
    for key in ("dw", "db", "dpooled", "db_relu"):
        if key in out:
            if b == 0:
                assert same(out[key], np.zeros_like(out[key])), (what, key, "not zeroed for an empty batch")
            else:
                assert_close(out[key], ref[key], TIGHT, (what, key))


def _reference(k, d, cce, b):
    denom = float(b + 3)
    if k.entry == "pool":
        return R.pool_head(d["x"], d["gp"], k.mode, d["w"], d["bias"], d["y"], denom, cce, db_relu=k.dbr is not None)
    r = R.pooled_head(d["pooled"], d["cnt"], d["gp"], k.mode, d["w"], d["bias"], d["y"], denom, cce,
                      db_relu=k.entry == "pooled" and k.dbr is not None)
    r["pooled"] = d["pooled"]
    return r


def _run_case(ctx, k, exact=True):
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    b = graphs(k, cus)
    d = data(k, cus)
    seg = Segments(ctx, d["gp"]) if k.entry != "dense" else None
    refs = {cce: _reference(k, d, cce, b) for cce in ("logits", "probs")}
    ctx.set_tuning("pool_split", k.knob)
    try:
        for grads, cce in variants(k):
            outs = []
            for li in range(3):
                what = (case_id(k), layouts(k.h)[li][0], grads, cce)
                out = _run(ctx, k, d, li, grads, cce, cus, seg)
                _same_outputs(out, _run(ctx, k, d, li, grads, cce, cus, seg), (what, "two runs differ"))
                _check(out, refs[cce], d, k, grads, what, exact)
                outs.append(out)
            for o in outs[1:]:
                if k.entry == "dense":
                    _same_outputs(o, outs[0], (case_id(k), grads, cce, "the layouts differ"))
                elif "db_relu" in o and b:
                    assert rel_err(o["db_relu"], outs[0]["db_relu"]) < TIGHT, (case_id(k), grads, cce, "db_relu across layouts")
    finally:
        ctx.set_tuning("pool_split", 0)


@pytest.mark.parametrize("k", DENSE_CASES, ids=case_id)
def test_dense_routes(ctx, k):
    """gcnx_dense_softmax_cce: workgroup counts and the slab reduction, class counts, widths, the staging edges."""
    _run_case(ctx, k)


@pytest.mark.parametrize("k", POOLED_CASES, ids=case_id)
def test_pooled_routes(ctx, k):
    """gcnx_pooled_dense_softmax_cce: pooled rows and positive counts that are already there; b == 0 zeroes dw, db, db_relu."""
    _run_case(ctx, k)


@pytest.mark.parametrize("k", POOL_CASES, ids=case_id)
def test_pool_routes(ctx, k):
    """gcnx_pool_dense_softmax_cce: the fused route under every slice count, the pool's own counts, the separate calls for each
    reason -- pooled at stride ldp on all of them."""
    _run_case(ctx, k)


@pytest.mark.parametrize("k", GAUSS, ids=case_id)
def test_gaussian_rows_against_float64(ctx, k):
    """Gaussian x: every pooled entry, every product and every sum rounds."""
    _run_case(ctx, k, exact=False)


# ------------------------------------------------------------------------------------------- state between calls
def _named(name):
    return next(k for k in CASES if k.name == name)


def _one(ctx, k, grads, cce="logits", li=0):
    from gcnx.device import Segments
    cus = ctx.info()["cus"]
    d = data(k, cus)
    seg = Segments(ctx, d["gp"]) if k.entry != "dense" else None
    ctx.set_tuning("pool_split", k.knob)
    try:
        return _run(ctx, k, d, li, grads, cce, cus, seg)
    finally:
        ctx.set_tuning("pool_split", 0)


def test_ticket_is_reset_between_launches(ctx):
    """The last workgroup to arrive resets the ticket: a multi-workgroup training call, a single-workgroup call, a
    multi-workgroup loss-only call and training again each repeat the bits of their own first run."""
    calls = [(_named("wgs-b257"), "train"), (_named("wgs-b31"), "train"), (_named("wgs-b545"), "loss"), (_named("wgs-b257"), "train"),
             (_named("wgs-b545"), "infer"), (_named("wgs-b545"), "loss")]
    first = {}
    for k, grads in calls:
        if (k.name, grads) not in first:
            first[(k.name, grads)] = _one(ctx, k, grads)
    for k, grads in calls:
        _same_outputs(_one(ctx, k, grads), first[(k.name, grads)], (k.name, grads, "differs from its first run"))


def test_workspace_growth_between_calls(ctx):
    """A small fused call, the 4097-graph call (the workspace grows), the small call again: the same bits."""
    small, big = _named("fused-b33-k0-sum-dbr"), _named("calls-b4097")
    a = _one(ctx, small, "train")
    _one(ctx, big, "train")
    _same_outputs(_one(ctx, small, "train"), a, "the small call after the large one")


# ------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx):
    """33 classes; db_relu with h % 4 != 0 or an unaligned db_relu on gcnx_pooled_dense_softmax_cce: GCNX_ERR_INVALID with its
    message, and the context serves the next call."""
    from gcnx import _lib
    from gcnx import device as D
    from gcnx.device import Segments
    b = 4
    la = _vector(ctx, 2, [7.0, 7.0])
    pooled, w33, y33, p33 = ctx.zeros((b, 8)), ctx.zeros((8, 33)), ctx.zeros((b, 33)), _vector(ctx, b * 33)
    with pytest.raises(_lib.GcnxError, match="at most 32 classes") as e:
        D.dense_softmax_cce(ctx, pooled, w33, None, y33, p33.row(0).flat(0, b * 33, (b, 33)), la.row(0), float(b))
    assert e.value.code == 1
    p33.untouched()
    la.untouched()
    for h, lead, message in ((6, 4, "db_relu needs h % 4 == 0"), (8, 3, "16-byte aligned")):
        d = R.exact_data(b, h, 2, "sum", 9000 + h)
        seg = Segments(ctx, d["gp"])
        dbr = _vector(ctx, h, lead=lead)
        dev = {key: ctx.to_device(d[key]) for key in ("pooled", "cnt", "w", "bias", "y")}
        with pytest.raises(_lib.GcnxError, match=message) as e:
            D.pooled_dense_softmax_cce(ctx, seg, dev["pooled"], dev["cnt"], dev["w"], dev["bias"], dev["y"], ctx.empty((b, 2)),
                                       ctx.zeros(2), float(b), dw=ctx.empty((h, 2)), db=ctx.empty(2), dpooled=ctx.empty((b, h)),
                                       db_relu=dbr.row(0))
        assert e.value.code == 1, message
        dbr.untouched(message)
        probs = ctx.empty((b, 2))
        D.pooled_dense_softmax_cce(ctx, seg, dev["pooled"], None, dev["w"], dev["bias"], None, probs)
        assert_close(probs.numpy(), R.head(d["pooled"], d["w"], d["bias"], None, 1.0, "logits")["probs"], TIGHT, ("after", message))

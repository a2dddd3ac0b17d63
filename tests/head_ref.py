"""Host reference for the classifier head of csrc/head.hip (gcnx_dense_softmax_cce, gcnx_pooled_dense_softmax_cce,
gcnx_pool_dense_softmax_cce), in NumPy alone (no GPU, no torch).

head(): Dense + softmax + CategoricalCrossentropy + categorical_accuracy and the head gradients in float64, both cce modes as
include/gcnx.h states them for gcnx_softmax_cce.  pool_head() / pooled_head(): the pool of tests/reduce_ref.py in front of it
and db_relu, the bias gradient of the ReLU layer under the pool, behind it.

route(): the host decisions of head.hip and of gcnx_pool_split restated -- which entry route a call takes (fused / counts /
calls / dense), which kernel variant (parts / staged / global), the class-count variant, the workgroup count, the slice count,
whether slabs are reduced and whether the fused route stores pooled as float4.

exact_data(): x holds small integers on both sides of zero with exact zeros, so every pooled SUM is exact in fp32 whatever
the order, AVG is one correctly rounded division and the positive counts are integers.  gauss_data(): the same shapes with
Gaussian rows, where everything rounds."""
import numpy as np

import reduce_ref as RR

F32 = np.float32
HEAD_ROWS = 32                     # kHeadRows: graphs per workgroup
HEAD_MAX_C = 32                    # kHeadMaxC
HEAD_LDS_FLOATS = 14 * 1024        # kHeadLdsFloats: dynamic LDS of the staged operands
CLIP = 1e-7
SAT = 40.0                         # the entry that saturates a graph: logits +-40, min p = e^-80


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- the reference
def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def first_max(a):
    """The first maximal class of every row (numpy's argmax; the kernel's strict > scan)."""
    return np.argmax(a, 1)


def head(pooled, w, bias, y, denom, cce):
    """probs, loss, hits, dlogits, dw, db, dpooled in float64; y None: probs alone.
    "logits": loss_g = sum_c y_c (logsumexp(z) - z_c), dlogits = (p sum_c y_c - y) / denom, no clip.
    "probs":  loss_g = -sum_c y_c log clip(p_c, 1e-7, 1 - 1e-7), dlogits = (p sum(y m) - y m) / denom, m = [1e-7 < p < 1 - 1e-7]."""
    P, W = np.asarray(pooled, np.float64), np.asarray(w, np.float64)
    b, c = P.shape[0], W.shape[1]
    z = P @ W + (0.0 if bias is None else np.asarray(bias, np.float64))
    z = np.broadcast_to(z, (b, c)).copy()
    p = softmax(z) if b else np.zeros((0, c))
    out = {"probs": p}
    if y is None:
        return out
    Y = np.asarray(y, np.float64)
    if cce == "logits":
        m = z.max(1, keepdims=True) if b else np.zeros((0, 1))
        lse = m + np.log(np.exp(z - m).sum(1, keepdims=True))
        per = (Y * (lse - z)).sum(1)
        ym = Y
    elif cce == "probs":
        per = -(Y * np.log(np.clip(p, CLIP, 1 - CLIP))).sum(1)
        ym = Y * ((p > CLIP) & (p < 1 - CLIP))
    else:
        raise ValueError(cce)
    dl = (p * ym.sum(1, keepdims=True) - ym) / float(denom)
    out.update(loss=per.sum() / float(denom), hits=int((first_max(p) == first_max(Y)).sum()) if b else 0, dlogits=dl,
               dw=P.T @ dl, db=dl.sum(0), dpooled=dl @ W.T)
    return out


def positive_counts(x, graph_ptr):
    """float32 [b, f]: the number of positive entries per (graph, column)."""
    gp = np.asarray(graph_ptr, np.int64)
    x = np.asarray(x)
    out = np.zeros((len(gp) - 1, x.shape[1]), F32)
    for g in range(len(gp) - 1):
        out[g] = (x[gp[g]:gp[g + 1]] > 0).sum(0)
    return out


def db_relu_from_counts(dpooled, cnt, graph_ptr, mode):
    """sum_g dPooled[g] * s_g * cnt[g], s_g = 1 / rows of graph g for AVG (float64)."""
    n = np.maximum(np.diff(np.asarray(graph_ptr, np.int64)), 1).astype(np.float64)
    sc = 1.0 / n if mode == "avg" else np.ones_like(n)
    return (np.asarray(dpooled, np.float64) * sc[:, None] * np.asarray(cnt, np.float64)).sum(0)


def pooled_head(pooled, cnt, graph_ptr, mode, w, bias, y, denom, cce, db_relu=False):
    r = head(pooled, w, bias, y, denom, cce)
    if db_relu:
        assert mode in ("sum", "avg")
        r["db_relu"] = db_relu_from_counts(r["dpooled"], cnt, graph_ptr, mode)
    return r


def pool_head(x, graph_ptr, mode, w, bias, y, denom, cce, db_relu=False):
    """reduce_ref.pool_fwd, then head(); db_relu = reduce_ref.pool_bwd_colsum of the reference dPooled (SUM / AVG)."""
    pooled, arg = RR.pool_fwd(x, graph_ptr, mode)
    r = head(pooled, w, bias, y, denom, cce)
    r["pooled"], r["argmax"] = pooled, arg
    if db_relu:
        assert mode in ("sum", "avg")
        r["db_relu"] = RR.pool_bwd_colsum(r["dpooled"], graph_ptr, x, mode)
    return r


# ------------------------------------------------------------------------------------------- the routes
def head_lds_floats(h, c, with_db_relu):
    """head_lds_floats of head_body.h: pooled rows [32][h + 1] | w [h c] | with db_relu: counts [32][h + 1] | 4 x [h]."""
    return HEAD_ROWS * (h + 1) + h * c + (HEAD_ROWS * (h + 1) + 4 * h if with_db_relu else 0)


def pool_split(cus, b, f, mode, half_wgs_per_cu, knob=0):
    """gcnx_pool_split: slices per graph of a SUM / AVG pool (1: none).  4 halves per CU for the stand-alone pool, 1 where the
    head reads the partial sums."""
    base = cdiv(f, 64) * b
    if mode == "max" or base >= 2 * cus:
        return 1
    ns = min(16, max(2, cdiv(half_wgs_per_cu * cus // 2, base)))
    return knob if 2 <= knob <= 16 else ns


GRADS = ("train", "nodb", "loss", "infer")       # dw + db + dpooled | dw + dpooled, db NULL | labels alone | y NULL


def route(entry, b, h, c, cus, mode="sum", grads="train", dbr=None, x_aligned=True, ldp=None, pooled_aligned=True, knob=0):
    """entry: "dense" (gcnx_dense_softmax_cce), "pooled" (gcnx_pooled_dense_softmax_cce) or "pool"
    (gcnx_pool_dense_softmax_cce).  dbr: None, "aligned" or "unaligned" (db_relu and its base).  ldp: the row stride of pooled
    (None: h).  Returns route / kernel / ct / nblk / nsplit / slabs / st4; kernel is None where no head kernel runs (b == 0)
    and st4 is None off the fused route."""
    assert entry in ("dense", "pooled", "pool") and grads in GRADS and dbr in (None, "aligned", "unaligned")
    assert c <= HEAD_MAX_C
    ldp = h if ldp is None else ldp
    with_dbr = dbr is not None
    rt = "dense"
    if entry == "pool":
        fused = (b > 0 and h > 0 and h % 4 == 0 and head_lds_floats(h, c, with_dbr) <= HEAD_LDS_FLOATS and x_aligned
                 and pool_split(cus, b, h, mode, 1, knob) > 1)
        counts = (not fused and with_dbr and 0 < b <= 4096 and h > 0 and h % 4 == 0 and ldp == h and dbr == "aligned"
                  and pool_split(cus, b, h, mode, 4, knob) == 1)
        rt = "fused" if fused else "counts" if counts else "calls"
    r = {"route": rt, "kernel": None, "ct": None, "nblk": cdiv(b, HEAD_ROWS), "nsplit": 1, "slabs": False, "st4": None}
    if b == 0:
        return r
    want_db = rt == "fused" and with_dbr and grads in ("train", "nodb")
    staged = head_lds_floats(h, c, want_db) <= HEAD_LDS_FLOATS
    r["kernel"] = "parts" if rt == "fused" else "staged" if staged else "global"
    r["ct"] = "ct2" if c == 2 and r["kernel"] != "global" else "generic"
    r["slabs"] = r["nblk"] > 1 and grads != "infer"
    if rt == "fused":
        r["nsplit"] = pool_split(cus, b, h, mode, 1, knob)
        r["st4"] = ldp % 4 == 0 and pooled_aligned
    return r


# ------------------------------------------------------------------------------------------- data
def graph_sizes(b, kind, rng):
    """kind "small": 1-3 rows; "mixed": 1 row (fewer rows than slices), tens of rows, an empty graph in the middle and one at
    the end (b >= 5); "ones": one row each."""
    if kind == "ones":
        return np.ones(b, np.int64)
    if kind == "small":
        return rng.integers(1, 4, b)
    assert kind == "mixed"
    s = rng.integers(1, 41, b)
    if b >= 5:
        s[b // 2] = 0
        s[-1] = 0
        free = [i for i in range(2, b - 1) if i != b // 2]           # (graphs 0 and 1 may become the saturated single rows)
        s[free[-1]] = 17
        if len(free) > 1:
            s[free[0]] = 1
    return s


def _finish(d, rng, b, h, c, mode, soft, sat):
    """w scaled so that the logits spread by about one (0.6 for many classes), labels, the saturated graphs 0 and 1."""
    gp = d["gp"]
    x = d["x"]
    d["pooled"], d["argmax"] = RR.pool_fwd(x, gp, mode)
    w = rng.standard_normal((h, c)) / np.sqrt(max(h, 1))
    if sat:
        w[0] = 0.0
    spread = float((d["pooled"].astype(np.float64) @ w).std()) if b and h else 0.0
    w *= (1.0 if c <= 3 else 0.6) / max(spread, 1e-3) if spread > 0 else 1.0
    if sat:
        w[0] = [1.0, -1.0]
    d["w"] = w.astype(F32)
    d["bias"] = (0.3 * rng.standard_normal(c)).astype(F32)
    if soft:
        y = rng.random((b, c)).astype(F32)                           # rows that do not sum to one
    else:
        y = np.eye(c, dtype=F32)[rng.integers(0, c, b)]
    if sat:
        y[0] = [0, 1]                                                # p = [1, 0]: mislabelled
        y[1] = [0, 1]                                                # p = [0, 1]: correctly labelled
    d["y"] = y
    d["cnt"] = positive_counts(x, gp)
    d["sat"] = np.zeros(b, bool)
    d["sat"][:2 if sat else 0] = True
    d["mode"] = mode
    return d


def _rows(b, h, c, mode, seed, sizes, sat):
    rng = np.random.default_rng(seed)
    sat = bool(sat) and h >= 4 and c == 2 and b >= 2
    s = graph_sizes(b, sizes, rng)
    if sat:
        s[:2] = 1
    gp = np.concatenate([[0], np.cumsum(s)]).astype(np.int64)
    return rng, sat, gp, int(gp[-1])


def exact_data(b, h, c, mode, seed, sizes="small", soft=False, sat=True):
    """x: integers in [-3, 3], a third of them zero.  sat (only where h >= 4, c == 2, b >= 2): graphs 0 and 1 are single rows
    (+-SAT, 0, ...), column 0 is zero everywhere else and w[0] = (1, -1): their logits are +-40 and -+40."""
    rng, sat, gp, n = _rows(b, h, c, mode, seed, sizes, sat)
    x = rng.integers(-3, 4, (n, h)).astype(F32)
    x[rng.random((n, h)) < 0.2] = 0.0
    if sat:
        x[:, 0] = 0.0
        x[:2] = 0.0
        x[0, 0], x[1, 0] = SAT, -SAT
    return _finish({"x": x, "gp": gp}, rng, b, h, c, mode, soft, sat)


def gauss_data(b, h, c, mode, seed, sizes="mixed", soft=False):
    rng, _, gp, n = _rows(b, h, c, mode, seed, sizes, False)
    x = rng.standard_normal((n, h)).astype(F32)
    return _finish({"x": x, "gp": gp}, rng, b, h, c, mode, soft, False)


COND_MAX = 80.0


def conditioning(d, denom, cce, db_relu=False):
    """max over entries of sum |terms| / max |result| for every sum the head forms: logits (against 1: their absolute error is
    the relative error of the probabilities), dw, db, dpooled and db_relu.  An fp32 sum carries an error of about one ulp
    (2^-23) of its largest partial sum, that is cond 2^-23 of the result, whatever the kernel does: the GPU tests hold results
    to 2e-5 of float64, so the data keeps cond <= COND_MAX = 80 < 1e-5 2^23 (half of that bar).  Without it a test would
    measure the cancellation in its own data (h == 0: every graph has the same probabilities and db = (b p - label counts) /
    denom cancels to any degree)."""
    P, W = np.abs(d["pooled"].astype(np.float64)), np.abs(d["w"].astype(np.float64))
    r = pooled_head(d["pooled"], d["cnt"], d["gp"], d["mode"] if d["mode"] != "max" else "sum", d["w"], d["bias"], d["y"], denom, cce,
                    db_relu=db_relu)
    A = np.abs(r["dlogits"])
    L = P @ W + np.abs(d["bias"].astype(np.float64))                 # per logit: the largest partial sum it can pass through
    out = {"logits": float(L.max(initial=0.0))}
    # a logit's rounding (an ulp of L) is the relative error of its probability and reaches dlogits = (p ysum - y) / denom as
    # p ysum L 2^-23 / denom: against the largest dlogit of the batch, the norm dw, db, dpooled and db_relu are read in
    # (a batch whose every unmasked graph is classified with p close to 1 has dlogits that are all cancellation)
    keep = ((r["probs"] > CLIP) & (r["probs"] < 1 - CLIP)) if cce == "probs" else 1.0      # a clipped entry is an exact zero
    ysum = (np.abs(d["y"].astype(np.float64)) * keep).sum(1, keepdims=True)
    top = float(A.max(initial=0.0))
    out["dlogits"] = float((r["probs"] * ysum * L).max(initial=0.0)) / float(denom) / top if top > 0 else 0.0
    terms = {"dw": P.T @ A, "db": A.sum(0), "dpooled": A @ W.T}
    if db_relu:
        terms["db_relu"] = db_relu_from_counts(np.abs(r["dpooled"]), d["cnt"], d["gp"], d["mode"])
    for key, t in terms.items():
        top = float(np.abs(r[key]).max(initial=0.0))
        out[key] = float(t.max(initial=0.0)) / top if top > 0 else 0.0
    return out


def check_conditions(d, denom=None, db_relu=False):
    """What lets the GPU tests compare hits exactly, trust the PROBS-mode clip mask and hold the sums to their tolerance:
    non-saturated rows keep every probability inside [1e-5, 1 - 1e-5] (c == 1 aside: its one probability is exactly 1 in
    every precision), saturated rows have min p < 1e-10, the two largest probabilities of every row differ by more than
    1e-4, and no sum is conditioned worse than COND_MAX (conditioning())."""
    p = head(d["pooled"], d["w"], d["bias"], None, 1.0, "logits")["probs"]
    b, c = p.shape
    if b == 0:
        return
    for cce in ("logits", "probs"):
        for key, cond in conditioning(d, float(b if denom is None else denom), cce, db_relu).items():
            assert cond <= COND_MAX, ("ill-conditioned", key, cce, cond)
    sat = d["sat"]
    if c > 1:
        q = p[~sat]
        assert q.size == 0 or (q.min() >= 1e-5 and q.max() <= 1 - 1e-5), ("probabilities near the clip", q.min(), q.max())
        top = np.sort(p, 1)
        assert (top[:, -1] - top[:, -2]).min() > 1e-4, "two classes within 1e-4"
    assert sat.sum() in (0, 2) and (not sat.any() or p[sat].min(1).max() < 1e-10), "saturated rows"
    if sat.any():
        hit = first_max(p[sat]) == first_max(d["y"][sat])
        assert hit.sum() == 1, "one saturated graph labelled correctly, one not"


def pick(make, seed, denom, db_relu=False, tries=50):
    """The first of make(seed), make(seed + 100000), ... on which check_conditions holds for EVERY row: a seed is chosen, never
    a graph left out.  Decided by the float64 reference alone."""
    for t in range(tries):
        d = make(seed + 100000 * t)
        try:
            check_conditions(d, denom, db_relu)
        except AssertionError:
            continue
        d["seed"] = seed + 100000 * t
        return d
    raise AssertionError(("no seed meets the conditions", seed))


def is_f32(a):
    a = np.asarray(a, np.float64)
    return bool(np.array_equal(a.astype(F32).astype(np.float64), a))

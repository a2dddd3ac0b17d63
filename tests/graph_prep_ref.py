"""NumPy reference of graph preparation (gcnx_coo_to_csr, gcnx_gcn_norm, gcnx_csr_inspect, gcnx_csr_transpose[_perm]) and of the
node side of the device collate (gcnx_collate / gcnx_collate2), with the inputs their tests share.

tests/test_graph_prep_host.py pins every function here against what the project already trusts (oracle.gcn_oracle,
gcnx.loader.collate_disjoint) and asserts the properties of the case matrices the GPU tests rely on;
tests/test_gpu_graph_prep.py compares the entry points with it through the C ABI.  Values are float64 computed from the float32
inputs; integers are exact."""
import numpy as np

import ecc_loader_ref as L

SYMMETRIC, BLOCK_DIAGONAL, GRAPH_PTR_OK = 1, 2, 4
U24 = 2.0 ** -24                                 # the unit roundoff of float32


def _rowptr(rows, n):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(rows, np.int64), minlength=n))]).astype(np.int32)


def _rows(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


# ---- gcnx_coo_to_csr -----------------------------------------------------------------------------------------------------------
def coo_to_csr(rows, cols, n):
    """Row-major sorted COO -> (rowptr int32[n + 1], colidx int32[nnz]); the entries keep their stored order, duplicates too."""
    rows = np.asarray(rows, np.int64)
    assert rows.size == 0 or (np.all(np.diff(rows) >= 0) and rows[0] >= 0 and rows[-1] < n)
    return _rowptr(rows, n), np.asarray(cols, np.int64).astype(np.int32)


def _unique_coo(rng, n, nnz, rows_from=None):
    """nnz distinct (row, col) pairs of an n x n matrix in row-major order (rows drawn from ``rows_from``, default all)."""
    rows_from = np.arange(n) if rows_from is None else np.asarray(rows_from)
    key = rng.choice(len(rows_from) * n, nnz, replace=False)
    r, c = rows_from[key // n], key % n
    order = np.lexsort((c, r))
    return r[order].astype(np.int64), c[order].astype(np.int64)


def coo_cases():
    """name -> (rows int64, cols int64, n).  One thread per entry in blocks of 256 plus a tail thread (e == nnz): the sizes put
    the tail thread last in a block (255), first in a new one (256), and past it; the named cases put a row change, a long run
    of empty rows and a single row across the block boundary."""
    rng = np.random.default_rng(11)
    out = {}
    for nnz in (0, 1, 255, 256, 257, 513):
        r, c = _unique_coo(rng, 40, nnz)
        out[f"nnz{nnz}"] = (r, c, 40)
    z = np.zeros(0, np.int64)
    out["n0"] = (z, z, 0)
    out["n1_empty"] = (z, z, 1)
    out["n1"] = (np.zeros(1, np.int64), np.zeros(1, np.int64), 1)
    out["first_row_7"] = _unique_coo(rng, 30, 100, np.arange(7, 30)) + (30,)
    out["trailing_empty"] = _unique_coo(rng, 50, 120, np.arange(0, 31)) + (50,)
    out["gap_300"] = _unique_coo(rng, 700, 400, np.concatenate([np.arange(0, 101), np.arange(401, 650)])) + (700,)
    out["one_row"] = (np.full(300, 5, np.int64), rng.permutation(400)[:300].astype(np.int64), 400)
    r = np.concatenate([np.full(256, 3), np.full(257, 4)]).astype(np.int64)      # the row changes between entries 255 and 256
    out["change_255_256"] = (r, np.concatenate([np.arange(256), np.arange(257)]).astype(np.int64), 600)
    r, c = _unique_coo(rng, 20, 60)
    r, c = np.insert(r, 31, r[30]), np.insert(c, 31, c[30])                      # entry 30 stored twice
    out["duplicate"] = (r, c, 20)
    return out


def coo_refusals():
    """name -> (rows, cols, n) that gcnx_coo_to_csr must refuse; 513 entries each, the defect at or across entry 256."""
    rng = np.random.default_rng(12)
    n = 60
    r, c = _unique_coo(rng, n, 513)
    out = {}
    ru = r.copy()
    ru[:256], ru[256:] = np.sort(rng.integers(30, n, 256)), np.sort(rng.integers(0, 30, 257))
    out["unsorted_255_256"] = (ru, c.copy(), n)
    for name, arr, val in (("row_eq_n", 0, n), ("col_eq_n", 1, n), ("row_negative", 0, -5), ("col_negative", 1, -1)):
        rc = [r.copy(), c.copy()]
        rc[arr][256] = val
        out[name] = (rc[0], rc[1], n)
    return out


# ---- gcnx_gcn_norm -------------------------------------------------------------------------------------------------------------
def gcn_norm(rowptr, colidx, vals, mode):
    """gcn_filter of a CSR that stores every diagonal entry: float64 from the float32 inputs (vals None = ones).
    spektral: diagonal + 1; pyg: as stored.  deg = row sums, out = a~ d_r^-1/2 d_c^-1/2 with d^-1/2 := 0 where deg <= 0."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    rows, colidx = _rows(rowptr), colidx[:nnz]
    v = np.ones(nnz, np.float64) if vals is None else np.asarray(vals, np.float32)[:nnz].astype(np.float64)
    if mode == "spektral":
        v = v + (rows == colidx)
    elif mode != "pyg":
        raise ValueError(mode)
    deg = np.bincount(rows, weights=v, minlength=n)
    dinv = np.zeros(n, np.float64)
    dinv[deg > 0] = 1.0 / np.sqrt(deg[deg > 0])
    return v * dinv[rows] * dinv[colidx]


def gcn_norm_bound(rowptr, colidx):
    """The relative error allowed to float32 gcn_norm per entry (r, c): ((m_r + m_c) / 2 + 8) * 2^-24, m = a row's entry count.
    A sequential float32 sum of m non-negative terms and the +1 carry at most m units of relative error into deg, the square
    root halves it, then a correctly rounded sqrtf and division (2), the diagonal's + 1 (1), two multiplications (2) and the
    second-order terms (the rest of the 8)."""
    rowptr = np.asarray(rowptr, np.int64)
    m = np.diff(rowptr).astype(np.float64)
    rows = _rows(rowptr)
    return ((m[rows] + m[np.asarray(colidx, np.int64)[:len(rows)]]) / 2 + 8) * U24


NORM_SIZES = (1, 255, 256, 257, 600, 1100)       # 1100: the case that has room for a hub row of 1000 distinct columns


def norm_case(n, weighted, mode):
    """A directed pattern with every diagonal stored.  n >= 255: about six entries per row, row 3 holds only its diagonal, and
    (weighted) rows 7 and n - 1 have degree exactly 0 -- spektral: only a stored diagonal of -1; pyg: three stored zeros -- with
    entries of other rows pointing at them.  n == 1100: row 300 is a hub of 1000 entries.  Values in [0.1, 2] (float32).
    Returns rowptr, colidx, vals (None if not weighted), the zero-degree rows."""
    rng = np.random.default_rng(1000 + n)
    if n == 1:
        return (np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([-1.0 if mode == "spektral" else 0.0], np.float32) if weighted else None,
                [0] if weighted else [])
    zero = [7, n - 1]
    cols = []
    for r in range(n):
        k = set(rng.choice(n, 5, replace=False).tolist()) | {r, zero[r % 2]}
        if r == 3:
            k = {r}
        if r in zero:
            k = {r} if mode == "spektral" else {r, (r + 1) % n, (r + 100) % n}
        if n == 1100 and r == 300:
            k = set(rng.choice(np.setdiff1d(np.arange(n), [r]), 999, replace=False).tolist()) | {r}
        cols.append(np.sort(np.fromiter(k, np.int64)))
    rowptr = np.concatenate([[0], np.cumsum([len(k) for k in cols])]).astype(np.int32)
    colidx = np.concatenate(cols).astype(np.int32)
    if not weighted:
        return rowptr, colidx, None, []
    vals = rng.uniform(0.1, 2.0, colidx.size).astype(np.float32)
    for r in zero:
        vals[rowptr[r]:rowptr[r + 1]] = -1.0 if mode == "spektral" else 0.0
    return rowptr, colidx, vals, zero


def drop_diagonal(rowptr, colidx, vals, r):
    """The same CSR without the stored diagonal of row r."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx)
    e = int(rowptr[r] + np.nonzero(colidx[rowptr[r]:rowptr[r + 1]] == r)[0][0])
    rp = rowptr.copy()
    rp[r + 1:] -= 1
    return rp.astype(np.int32), np.delete(colidx, e), (None if vals is None else np.delete(vals, e))


# ---- gcnx_csr_inspect ----------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """How many float32 values lie between a and b (0: the same bits), on the line of ordered bit patterns."""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def inspect(rowptr, colidx, vals, n, graph_ptr, ulp=4):
    """The property bits of gcnx_csr_inspect.  SYMMETRIC: every off-diagonal entry (r, c) has an entry (c, r) whose value
    differs by at most ``ulp`` float32 ulp (the kernel's 4.8e-7 * max(|v|, |w|) lies between 4 and 8.05 ulp: a case must give the
    same answer for ulp = 4 and ulp = 8).  GRAPH_PTR_OK: graph_ptr[0] == 0, graph_ptr[b] == n, non-decreasing; without it
    BLOCK_DIAGONAL is cleared too and graph_ptr is not read further.  BLOCK_DIAGONAL: every column inside its row's block, the
    block of row r being the LAST g with graph_ptr[g] <= r (empty graphs own no row).  A column outside [0, n) clears
    SYMMETRIC and BLOCK_DIAGONAL.  graph_ptr None: only SYMMETRIC can be reported."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    props = SYMMETRIC | (0 if graph_ptr is None else BLOCK_DIAGONAL | GRAPH_PTR_OK)
    gp = None if graph_ptr is None else np.asarray(graph_ptr, np.int64)
    if gp is not None and not (gp[0] == 0 and gp[-1] == n and np.all(np.diff(gp) >= 0)):
        props &= ~(BLOCK_DIAGONAL | GRAPH_PTR_OK)
        gp = None
    if n == 0:
        return props
    nnz = int(rowptr[n])
    rows, colidx = _rows(rowptr[:n + 1]), colidx[:nnz]
    v = np.ones(nnz, np.float32) if vals is None else np.asarray(vals, np.float32)[:nnz]
    inside = (colidx >= 0) & (colidx < n)
    if not inside.all():
        props &= ~(SYMMETRIC | BLOCK_DIAGONAL)
    if gp is not None:
        g = np.searchsorted(gp, rows, side="right") - 1
        if np.any(inside & ((colidx < gp[g]) | (colidx >= gp[g + 1]))):
            props &= ~BLOCK_DIAGONAL
    stored = {}
    for r, c, w in zip(rows[inside].tolist(), colidx[inside].tolist(), v[inside]):
        stored.setdefault((r, c), []).append(w)
    for (r, c), ws in stored.items():
        if r != c and not all(any(w == m or ulp_distance(w, m) <= ulp for m in stored.get((c, r), [])) for w in ws):
            props &= ~SYMMETRIC
            break
    return props


INSPECT_SIZES = [0, 5, 0, 1, 70, 0]              # empty graphs at the start, in the middle and at the end of graph_ptr


def inspect_base():
    """A symmetric, block-diagonal, weighted batch: a 5-node ring, a single node and a complete 70-node graph (rows of 70 entries:
    the 64-lane row loop runs twice), all with self loops; values in [0.1, 2), equal on both sides of the diagonal."""
    rng = np.random.default_rng(21)
    gp = np.concatenate([[0], np.cumsum(INSPECT_SIZES)]).astype(np.int32)
    n = int(gp[-1])
    a = np.zeros((n, n), bool)
    for i in range(5):
        a[i, i] = a[i, (i + 1) % 5] = a[(i + 1) % 5, i] = True
    a[5, 5] = True
    a[6:76, 6:76] = True
    w = rng.uniform(0.1, 1.99, (n, n)).astype(np.float32)
    w = np.triu(w) + np.triu(w, 1).T
    r, c = np.nonzero(a)
    return {"n": n, "rowptr": _rowptr(r, n), "colidx": c.astype(np.int32), "vals": w[r, c].astype(np.float32), "graph_ptr": gp}


def entry(m, r, c):
    """The position of entry (r, c) in the CSR of case m."""
    lo, hi = int(m["rowptr"][r]), int(m["rowptr"][r + 1])
    return lo + int(np.nonzero(m["colidx"][lo:hi] == c)[0][0])


def _without(m, r, c):
    e = entry(m, r, c)
    rp = m["rowptr"].copy()
    rp[r + 1:] -= 1
    return dict(m, rowptr=rp, colidx=np.delete(m["colidx"], e), vals=np.delete(m["vals"], e))


def _with(m, pairs, value=1.0):
    rows = np.concatenate([_rows(m["rowptr"]), [p[0] for p in pairs]])
    cols = np.concatenate([m["colidx"], [p[1] for p in pairs]])
    vals = np.concatenate([m["vals"], np.full(len(pairs), value, np.float32)])
    order = np.lexsort((cols, rows))
    return dict(m, rowptr=_rowptr(rows, m["n"]), colidx=cols[order].astype(np.int32), vals=vals[order].astype(np.float32))


def _moved(m, r, c, magnitude, ulps):
    """Entry (r, c) = magnitude, entry (c, r) = the float32 ``ulps`` steps above it."""
    v = m["vals"].copy()
    v[entry(m, r, c)] = np.float32(magnitude)
    v[entry(m, c, r)] = (np.array([magnitude], np.float32).view(np.int32) + ulps).view(np.float32)[0]
    return dict(m, vals=v)


def inspect_cases():
    """name -> (case, bits cleared): the base and one change at a time."""
    m = inspect_base()
    n, gp = m["n"], m["graph_ptr"]
    b = len(gp) - 1
    out = {"base": (m, 0)}
    # row 16 keeps (16, 74) at position 68 of its 70 entries -- checked in the second pass of the lane loop -- and finds no (74, 16)
    out["one_way_survivor_at_68"] = (_without(m, 74, 16), SYMMETRIC)
    out["one_way_removed_at_68"] = (_without(m, 16, 74), SYMMETRIC)
    out["one_way_short_row"] = (_without(m, 2, 1), SYMMETRIC)
    for mag in (1.0, 1.99):
        for ulps, cleared in ((2, 0), (4, 0), (9, SYMMETRIC), (16, SYMMETRIC)):
            out[f"value_{mag}_{ulps}ulp"] = (_moved(m, 20, 75, mag, ulps), cleared)       # (20, 75): position 69 of row 20
        out[f"value_{mag}_16ulp_short_row"] = (_moved(m, 0, 1, mag, 16), SYMMETRIC)
    out["edge_between_graphs"] = (_with(m, [(1, 5), (5, 1)]), BLOCK_DIAGONAL)
    out["edge_between_graphs_long_row"] = (_with(m, [(4, 75), (75, 4)]), BLOCK_DIAGONAL)     # (75, 4): first entry of a 71-entry row
    bad = BLOCK_DIAGONAL | GRAPH_PTR_OK
    for name, k, val in (("gp_first_1", 0, 1), ("gp_last_n_minus_1", b, n - 1), ("gp_decreasing", 3, 4)):
        g = gp.copy()
        g[k] = val
        out[name] = (dict(m, graph_ptr=g), bad)
        out[name + "_asymmetric"] = (dict(_without(m, 74, 16), graph_ptr=g), bad | SYMMETRIC)
    for name, val in (("col_n", n), ("col_minus_1", -1)):
        c = m["colidx"].copy()
        c[entry(m, 70, 70)] = val                  # a diagonal entry: it has no mirror entry that would miss it
        out[name] = (dict(m, colidx=c), SYMMETRIC | BLOCK_DIAGONAL)
    return out


# ---- gcnx_csr_transpose / gcnx_csr_transpose_perm ---------------------------------------------------------------------------------
def transpose(rowptr, colidx, vals):
    """(rowptr_t, colidx_t, perm_t, vals_t): ecc_loader_ref.transpose_perm, and the values following perm_t."""
    rp_t, ci_t, pm_t = L.transpose_perm(rowptr, colidx)
    return rp_t, ci_t, pm_t, (None if vals is None else np.asarray(vals, np.float32)[pm_t])


def transpose_cases():
    """name -> (rowptr, colidx, vals)."""
    rng = np.random.default_rng(31)
    out = {"n0": (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)),
           "n5_empty": (np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))}
    live_rows = np.setdiff1d(np.arange(200), np.arange(0, 200, 7))              # rows 0, 7, 14, ... are empty
    live_cols = np.setdiff1d(np.arange(200), np.arange(3, 200, 5))              # columns 3, 8, 13, ... are empty
    key = rng.choice(len(live_rows) * len(live_cols), 1500, replace=False)
    r, c = live_rows[key // len(live_cols)], live_cols[key % len(live_cols)]
    order = np.lexsort((c, r))
    out["directed_200"] = (_rowptr(r, 200), c[order].astype(np.int32), rng.random(1500).astype(np.float32))
    r, c = _unique_coo(rng, 12, 40)
    r, c = np.repeat(r, 3), np.repeat(c, 3)                                      # every entry three times, with three values
    out["duplicates"] = (_rowptr(r, 12), c.astype(np.int32), rng.random(r.size).astype(np.float32))
    u = collate_union(1)
    out["union_large"] = (u["rowptr"], u["colidx"], u["vals"])
    return out


# ---- gcnx_collate / gcnx_collate2: the node side of a batch -------------------------------------------------------------------------
LARGE_N = 4100                                    # a ring with self loops: 4100 rows, 12300 entries
LARGE = len(L.SIZES)                              # its index in the dataset
SELECTIONS = tuple(L.SELECTIONS) + ([LARGE, 0, 7], [2, LARGE, 3], [6, 5, LARGE], [LARGE, 5, LARGE], [1, 8, 2, 4], [4, LARGE, 1])
FS, CS, LAYOUTS = (0, 1, 3, 4, 16), (0, 1, 2, 300), ("dense", "wide_in", "wide_out", "mixed")
_cache = {}


def collate_union(f, s=2, seed=0):
    """ecc_loader_ref.union (its SIZES: one-node graphs and graphs without entries among them) followed by the large graph;
    with values ``vals``, labels ``y300`` [G, 300] (a test takes its first c columns) and a second node matrix ``ax`` [N, f].
    The collate launch is 16 x 256 = 4096 threads per graph: the large graph's rows, entries and rows * f (f >= 1) each take
    more than one pass of their grid-stride loop, the last pass a ragged one."""
    if (f, s, seed) in _cache:
        return _cache[(f, s, seed)]
    u = L.union(f=f, s=s, seed=seed)
    rng = np.random.default_rng(40 + seed)
    n0, e0 = int(u["node_ptr"][-1]), int(u["rowptr"][-1])
    i = np.arange(LARGE_N)
    cols = np.sort(np.stack([(i - 1) % LARGE_N, i, (i + 1) % LARGE_N], 1), 1)
    idx = np.stack([np.repeat(i, 3), cols.ravel()], 1) + n0
    u = dict(u)
    u["node_ptr"] = np.concatenate([u["node_ptr"], [n0 + LARGE_N]]).astype(np.int32)
    u["rowptr"] = np.concatenate([u["rowptr"], e0 + 3 * (i + 1)]).astype(np.int32)
    u["colidx"] = np.concatenate([u["colidx"], idx[:, 1]]).astype(np.int32)
    u["idx"] = np.concatenate([u["idx"], idx]).astype(np.int64)
    u["x"] = np.concatenate([u["x"], rng.standard_normal((LARGE_N, f)).astype(np.float32)])
    u["e"] = np.concatenate([u["e"], rng.random((3 * LARGE_N, s)).astype(np.float32)])
    u["vals"] = rng.uniform(0.1, 2.0, u["colidx"].size).astype(np.float32)
    u["y300"] = rng.standard_normal((len(u["node_ptr"]) - 1, 300)).astype(np.float32)
    u["ax"] = rng.standard_normal(u["x"].shape).astype(np.float32)
    _cache[(f, s, seed)] = u
    return u


def gather_nodes(u, sel, c=2):
    """The node side of the batch of the graphs ``sel`` as gcnx_collate2 gathers it: rowptr [n + 1], colidx / vals [nnz],
    x / ax [n, f], y [b, c], graph_ptr [b + 1] and ids [n] (the batch position of every row's graph)."""
    gp, rp, ci = u["node_ptr"].astype(np.int64), u["rowptr"].astype(np.int64), u["colidx"].astype(np.int64)
    desc, n, nnz = L.descriptor(u, sel)
    b, f = len(sel), u["x"].shape[1]
    o = {"rowptr": np.zeros(n + 1, np.int32), "colidx": np.zeros(nnz, np.int32), "vals": np.zeros(nnz, np.float32),
         "x": np.zeros((n, f), np.float32), "ax": np.zeros((n, f), np.float32), "y": np.zeros((b, c), np.float32),
         "graph_ptr": np.zeros(b + 1, np.int32), "ids": np.zeros(n, np.int32)}
    for j, src in enumerate(sel):
        bn, be = int(desc[(b + 1) + j]), int(desc[2 * (b + 1) + j])
        n0, ng = gp[src], gp[src + 1] - gp[src]
        e0, ne = rp[n0], rp[n0 + ng] - rp[n0]
        o["rowptr"][bn:bn + ng] = rp[n0:n0 + ng] - e0 + be
        o["colidx"][be:be + ne] = ci[e0:e0 + ne] - n0 + bn
        o["vals"][be:be + ne] = u["vals"][e0:e0 + ne]
        o["x"][bn:bn + ng] = u["x"][n0:n0 + ng]
        o["ax"][bn:bn + ng] = u["ax"][n0:n0 + ng]
        o["y"][j] = u["y300"][src, :c]
        o["graph_ptr"][j] = bn
        o["ids"][bn:bn + ng] = j
    o["rowptr"][n] = nnz
    o["graph_ptr"][b] = n
    return o


def collate_configs():
    """(layout, f, c, vals, ids, s) for the collate tests: every value of every parameter, and every pair that involves the
    layout (tests/test_graph_prep_host.py asserts that), without the full product.
    dense: ldx == f == ldo; wide_in: ldx > f, x a view offset into its buffer; wide_out: ldo > f; mixed: all four leading
    dimensions differ (lds != ldx, ldos != ldo)."""
    out = []
    for li, layout in enumerate(LAYOUTS):
        for fi, f in enumerate(FS):
            k = fi + li
            out.append((layout, f, CS[k % 4], k % 2 == 0, (k // 2) % 2 == 0, (fi + li // 2) % 2 == 1))
    return out


def leading_dims(layout, f):
    """(ldx, x offset, ldo, o_x offset, lds, ldos) of a layout."""
    return {"dense": (f, 0, f, 0, f, f), "wide_in": (f + 3, 2, f, 0, f + 3, f), "wide_out": (f, 0, f + 5, 2, f, f + 5),
            "mixed": (f + 3, 1, f + 5, 3, f + 2, f + 7)}[layout]

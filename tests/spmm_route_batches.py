"""The two disjoint batches of tests/test_gpu_spmm_routes.py, built with scipy on the host, and the float64 reference they are
held to.  Each batch is only as large as the limits of csrc/spmm.hip force; tests/test_spmm_route_batches_host.py pins what
each of them has to deliver, so that a later change here cannot quietly drop a scheduling class.

The limits (csrc/spmm.hip):
  kDuoCap32 = 632      rows of a tier-1 tile (two 512-thread workgroups per CU)
  kSoloCap32 = 1276    rows of a tier-2 tile (one 1024-thread workgroup); taller graphs go as plan-listed row chunks
  kDblCap = 624        rows up to which a tier-2 tile is double buffered
  kPipeCap32 = 624     pipelined kernel: graph rows with 32-column slabs
  kPipeCap16 = 1024    ... with 16-column slabs; taller graphs as 32-row chunks
  kHubDeg = 256        rows of more entries are hub rows: 256-entry segments plus a combine launch (with a bound plan); on
  kLongRowSmall = 256  the plain row gather such a row is split over the workgroup's four waves
  kStageCap = 2048     CSR entries a chunk stages in LDS; a chunk of more overflows to global memory
  kCbMinRows = 4096    graphs of at least this many rows are column-block graphs (and make DeviceCSR.plan build a plan)
  kCbMinF = 128        ... from this width on
  kCbShort = 32        column blocks: "short" rows up to here
"""
import functools
from collections import namedtuple

import numpy as np

DUO_CAP, SOLO_CAP, DBL_CAP, PIPE_CAP32, PIPE_CAP16 = 632, 1276, 624, 624, 1024
HUB_DEG, STAGE_CAP, CB_MIN_ROWS, CB_MIN_F, CB_SHORT = 256, 2048, 4096, 128, 32
FMAX = 512                                    # widest feature matrix of the tests: narrower ones are its leading columns

Batch = namedtuple("Batch", "sizes gp rowptr colidx n")

# one graph on each side of every limit; the empty graph in the middle; the hub graph; the column-block graph
SIZES1 = [1, 7, 40, 100, 624, 625, 0, 632, 633, 1024, 1025, 1276, 1277, 1400, 4096]
EMPTY1, HUB1, CB1 = 6, 13, 14                 # positions in SIZES1
DENSE8 = 96                                   # the hub graph's local rows [96, 104) hold 300 entries each: one 8-row chunk


def _sym(m, seed, extra=()):
    """m x m symmetric 0 / 1 pattern with self-loops, ~ 19 entries per row (40 / 100 rows: ~ 20 / ~ 50); `extra`: (row, count)
    pairs -- that row is joined to `count` random columns (and they to it)."""
    import scipy.sparse as sp
    dens = 0.3 if m in (40, 100) else min(1.0, 9.0 / m)          # (0.3 in either direction: about half of the pairs)
    a = sp.random(m, m, density=dens, random_state=seed, format="csr")
    a = ((a + a.T) > 0).astype(np.float32) + sp.identity(m, dtype=np.float32, format="csr")
    if extra:
        rng = np.random.default_rng(1000 + seed)
        rows = np.concatenate([np.full(k, r) for r, k in extra])
        cols = np.concatenate([rng.choice(m, k, replace=False) for r, k in extra])
        e = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(m, m)).tocsr()
        a = a + e + e.T
    return (a > 0).astype(np.float32)


def _assemble(blocks, sizes):
    import scipy.sparse as sp
    a = sp.block_diag([b for b in blocks if b.shape[0] > 0]).tocsr()
    a.sort_indices()
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return Batch(list(sizes), gp, a.indptr.astype(np.int32), a.indices.astype(np.int32), int(gp[-1]))


def _blocks1():
    import scipy.sparse as sp
    blocks = []
    for i, m in enumerate(SIZES1):
        if m == 0:
            blocks.append(sp.csr_matrix((0, 0), dtype=np.float32))
        elif i == HUB1:        # rows of 300 entries in one aligned 8-row chunk: hub rows, and 2 400 staged entries in that chunk
            blocks.append(_sym(m, i, [(r, 300) for r in range(DENSE8, DENSE8 + 8)]))
        elif i == CB1:         # 40 rows of 60 .. 200 entries, a hub row of 400, a row of 2 500 (past the LDS staging of a chunk)
            mid = [(50 + 97 * k, 60 + (140 * k) // 39) for k in range(40)]
            blocks.append(_sym(m, i, mid + [(7, 400), (4001, 2500)]))
        else:
            blocks.append(_sym(m, i))
    return blocks


@functools.lru_cache(None)
def batch1(with_cb=True):
    """Every scheduling class at minimum size (about 12 800 rows); with_cb=False: without the 4 096-row graph, so that
    DeviceCSR.plan builds no plan."""
    k = len(SIZES1) if with_cb else CB1
    return _assemble(_blocks1()[:k], SIZES1[:k])


def batch2_sizes(cus, f):
    """max(80, ceil(4 cus / (2 f / 32))) graphs of 5 .. 60 rows -- tier 2 alone fills the chip: 2 n2 (f / 32) >= 4 cus -- an
    empty graph between the two tall graphs (about 1 300 rows: the 8-row-chunk side of the bf16-result forms), which sit in
    the middle of the small ones."""
    nsmall = max(80, -(-4 * cus // (2 * f // 32)))
    small = (5 + np.random.default_rng(77).integers(0, 56, nsmall)).tolist()
    half = nsmall // 2
    return small[:half] + [1300, 0, 1310] + small[half:], half + 1


@functools.lru_cache(None)
def batch2(cus, f, hub=False):
    """hub=True: a row of 300 entries in the first tall graph (a hub row in a graph taller than a tile)."""
    import scipy.sparse as sp
    sizes, empty = batch2_sizes(cus, f)
    blocks = []
    for i, m in enumerate(sizes):
        if m == 0:
            blocks.append(sp.csr_matrix((0, 0), dtype=np.float32))
        else:
            blocks.append(_sym(m, 500 + i, [(11, 300)] if hub and i == empty - 1 else ()))
    return _assemble(blocks, sizes)


def gcn_vals(b):
    """Symmetric GCN normalisation of the 0 / 1 pattern (every row has its self-loop): 1 / sqrt(deg_i deg_j)."""
    deg = np.diff(b.rowptr).astype(np.float64)
    rows = np.repeat(np.arange(b.n), np.diff(b.rowptr))
    return (1.0 / np.sqrt(deg[rows] * deg[b.colidx])).astype(np.float32)


def skew_vals(b, seed=7):
    """Non-symmetric values in [0.25, 1.25): the transpose matters."""
    return (np.random.default_rng(seed).random(len(b.colidx)) + 0.25).astype(np.float32)


def features(n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, FMAX), dtype=np.float32)


def ref_spmm(b, vals, h):
    """The oracle's float64 aggregation (oracle.gcn_oracle.spmm_csr), 64 columns at a time to bound its scratch."""
    from oracle import gcn_oracle as o
    rp, ci = b.rowptr.astype(np.int64), b.colidx.astype(np.int64)
    v = None if vals is None else np.asarray(vals, np.float64)
    h = np.asarray(h, np.float64)
    return np.concatenate([o.spmm_csr(rp, ci, v, np.ascontiguousarray(h[:, c:c + 64])) for c in range(0, h.shape[1], 64)], 1)


def ref_spmm_t(b, vals, g):
    """A^T g in float64 (oracle.gcn_oracle.spmm_csr_T), 64 columns at a time."""
    from oracle import gcn_oracle as o
    rp, ci = b.rowptr.astype(np.int64), b.colidx.astype(np.int64)
    v = None if vals is None else np.asarray(vals, np.float64)
    g = np.asarray(g, np.float64)
    return np.concatenate([o.spmm_csr_T(rp, ci, v, np.ascontiguousarray(g[:, c:c + 64])) for c in range(0, g.shape[1], 64)], 1)


def degrees(b, g):
    """Entries per row of graph g."""
    return np.diff(b.rowptr)[b.gp[g]:b.gp[g + 1]]


def rows_of(b, keep):
    """Global row indices of the graphs g with keep(rows of g)."""
    parts = [np.arange(b.gp[g], b.gp[g + 1]) for g in range(len(b.sizes)) if keep(b.sizes[g])]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)

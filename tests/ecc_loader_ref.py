"""NumPy reference of the device loader's edge side (gcnx_collate_edges) and the inputs its tests share.

The resident dataset is one block-diagonal union.  Graph g has node offset n0 = node_ptr[g] and entry offset e0 = rowptr[n0];
its block of the union's transposed CSR occupies the same entry range [e0, e0 + ne), so the transposed pattern of a batch is a
gather of the union's, re-based by the batch offsets -- ``gather`` below states that, and ``transpose_perm`` (a stable argsort
by column: what gcnx_csr_transpose_perm's counting sort computes) is what it must equal on the batch's own CSR."""
import numpy as np

import ecc_ref as R

SIZES = [7, 1, 12, 3, 1, 5, 9, 2, 6]           # 9 directed graphs; at density 0.25 without self loops some have no entry at all
SELECTIONS = ([4, 0, 7], [1], [8, 2, 2, 3], [5, 3, 8, 0, 2, 7, 1, 6, 4])


def transpose_perm(rowptr, colidx):
    """(rowptr_t, colidx_t, perm_t) of a CSR pattern: entries sorted by column, a column's entries in their stored order."""
    rowptr, colidx = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    colidx = colidx[:nnz]
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    perm = np.argsort(colidx, kind="stable")
    rowptr_t = np.concatenate([[0], np.cumsum(np.bincount(colidx, minlength=n))])
    return rowptr_t.astype(np.int32), rows[perm].astype(np.int32), perm.astype(np.int32)


def union(sizes=SIZES, f=4, s=2, seed=0, directed=True, density=0.25, self_loops=False):
    """The disjoint union of random graphs as host arrays: x, node_ptr, rowptr, colidx, e (float32 [nnz, s])."""
    x, idx, e, gp = R.random_batch(list(sizes), f, s, density=density, directed=directed, seed=seed, self_loops=self_loops)
    n = x.shape[0]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(idx[:, 0], minlength=n))]).astype(np.int32)
    return {"x": x.astype(np.float32), "node_ptr": gp.astype(np.int32), "rowptr": rowptr, "colidx": idx[:, 1].astype(np.int32),
            "e": e.astype(np.float32), "idx": idx}


def descriptor(u, sel):
    """desc of gcnx_collate for the graphs ``sel``: ids (one pad), node offsets, entry offsets; and the batch totals."""
    sel = np.asarray(sel, np.int64)
    gp, rp = u["node_ptr"].astype(np.int64), u["rowptr"].astype(np.int64)
    bn = np.concatenate([[0], np.cumsum(gp[sel + 1] - gp[sel])])
    be = np.concatenate([[0], np.cumsum(rp[gp[sel + 1]] - rp[gp[sel]])])
    return np.concatenate([sel, [0], bn, be]).astype(np.int32), int(bn[-1]), int(be[-1])


def gather(u, sel, union_t=None):
    """The batch of the graphs ``sel`` by the gather gcnx_collate_edges performs: its CSR (rowptr, colidx), its transposed
    pattern (rowptr_t, colidx_t, perm_t) out of the UNION's, and its rows of e."""
    gp, rp, ci = u["node_ptr"].astype(np.int64), u["rowptr"].astype(np.int64), u["colidx"].astype(np.int64)
    rp_t, ci_t, pm_t = (np.asarray(v, np.int64) for v in (union_t or transpose_perm(rp, ci)))
    desc, n, nnz = descriptor(u, sel)
    b = len(sel)
    o = {"rowptr": np.zeros(n + 1, np.int32), "colidx": np.zeros(nnz, np.int32), "rowptr_t": np.zeros(n + 1, np.int32),
         "colidx_t": np.zeros(nnz, np.int32), "perm_t": np.zeros(nnz, np.int32), "e": np.zeros((nnz, u["e"].shape[1]), np.float32)}
    for j, src in enumerate(sel):
        bn, be = int(desc[(b + 1) + j]), int(desc[2 * (b + 1) + j])
        n0, ng = gp[src], gp[src + 1] - gp[src]
        e0, ne = rp[n0], rp[n0 + ng] - rp[n0]
        o["rowptr"][bn:bn + ng] = rp[n0:n0 + ng] - e0 + be
        o["colidx"][be:be + ne] = ci[e0:e0 + ne] - n0 + bn
        o["rowptr_t"][bn:bn + ng] = rp_t[n0:n0 + ng] - e0 + be
        o["colidx_t"][be:be + ne] = ci_t[e0:e0 + ne] - n0 + bn
        o["perm_t"][be:be + ne] = pm_t[e0:e0 + ne] - e0 + be
        o["e"][be:be + ne] = u["e"][e0:e0 + ne]
    o["rowptr"][n] = o["rowptr_t"][n] = nnz
    return o


def graphs(u, labels=None):
    """The union split back into gcnx.Graph objects (x, scipy CSR a, e, one-hot y)."""
    import scipy.sparse as sp
    import gcnx
    gp, idx = u["node_ptr"].astype(np.int64), u["idx"]
    out = []
    for g in range(len(gp) - 1):
        lo, hi = gp[g], gp[g + 1]
        sel = (idx[:, 0] >= lo) & (idx[:, 0] < hi)
        a = sp.csr_matrix((np.ones(int(sel.sum())), (idx[sel, 0] - lo, idx[sel, 1] - lo)), shape=(hi - lo, hi - lo))
        y = np.eye(2)[(g * 7 // 3) % 2 if labels is None else labels[g]]
        out.append(gcnx.Graph(x=u["x"][lo:hi], a=a, e=u["e"][sel], y=y))
    return out

"""Host side of the device loader's edge features: gcnx.device_loader.union_edge_features (pure NumPy), and the reference the
GPU tests of gcnx_collate_edges compare with -- the gather of the union's transposed pattern (tests/ecc_loader_ref.py) against
a stable argsort by column of every batch's own CSR."""
import numpy as np
import pytest

import ecc_loader_ref as L
import ecc_ref as R


class _G:
    def __init__(self, e=None):
        self.e = e


def _per_graph(u):
    gp, rp = u["node_ptr"].astype(np.int64), u["rowptr"].astype(np.int64)
    ent = rp[gp]
    return [u["e"][ent[g]:ent[g + 1]] for g in range(len(gp) - 1)], np.diff(ent)


def test_union_edge_features_concatenates_in_dataset_order():
    from gcnx.device_loader import union_edge_features
    u = L.union(s=3, seed=2)
    parts, nnz_sizes = _per_graph(u)
    assert (nnz_sizes == 0).sum() >= 2 and nnz_sizes.sum() == u["e"].shape[0]
    out = union_edge_features([_G(p.astype(np.float64)) for p in parts], nnz_sizes)      # float64 in, as the loaders hold it
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == u["e"].shape
    assert np.array_equal(out, u["e"])
    rev = union_edge_features([_G(p) for p in parts[::-1]], nnz_sizes[::-1])
    assert np.array_equal(rev, np.concatenate(parts[::-1], 0))
    # graphs without entries contribute [0, S] blocks, and a dataset of such graphs alone is an empty [0, S]
    empty = union_edge_features([_G(np.zeros((0, 3))), _G(np.zeros((0, 3)))], [0, 0])
    assert empty.shape == (0, 3) and empty.dtype == np.float32


def test_union_edge_features_names_the_offending_graph():
    from gcnx.device_loader import union_edge_features
    # undirected graphs: one row per stored entry means both directions of an edge
    x, idx, e, gp = R.random_batch([6, 9, 4], 5, 2, density=0.4, directed=False, seed=3)
    rp = np.concatenate([[0], np.cumsum(np.bincount(idx[:, 0], minlength=x.shape[0]))])
    ent = rp[gp]
    parts, nnz_sizes = [e[ent[g]:ent[g + 1]] for g in range(3)], np.diff(ent)
    assert np.array_equal(union_edge_features([_G(p) for p in parts], nnz_sizes), e.astype(np.float32))

    def bad(k, value):
        gs = [_G(p) for p in parts]
        gs[k] = _G(value)
        return gs
    lo = idx[ent[1]:ent[2]]
    per_edge = parts[1][lo[:, 0] <= lo[:, 1]]                    # use_edge_data=True: one row per UNDIRECTED edge
    assert 0 < per_edge.shape[0] < parts[1].shape[0]
    with pytest.raises(ValueError, match=r"graph 1\b.*one row per stored entry"):
        union_edge_features(bad(1, per_edge), nnz_sizes)
    with pytest.raises(ValueError, match=r"graph 2\b.*one row per stored entry"):
        union_edge_features(bad(2, parts[2][:, 0]), nnz_sizes)   # 1-D
    with pytest.raises(ValueError, match=r"graph 0\b.*one row per stored entry"):
        union_edge_features(bad(0, np.zeros((6, 6, 2))), nnz_sizes)   # dense [n, n, S]
    with pytest.raises(ValueError, match=r"graph 1\b.*no edge features"):
        union_edge_features(bad(1, None), nnz_sizes)
    with pytest.raises(ValueError, match=r"graph 2\b.*3 columns.*2"):
        union_edge_features(bad(2, np.zeros((int(nnz_sizes[2]), 3))), nnz_sizes)
    with pytest.raises(ValueError, match=r"graph 0\b"):
        union_edge_features([_G(np.zeros((0, 0)))], [0])         # S = 0


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_gather_of_the_unions_transpose_is_the_batchs_own_transpose(seed):
    """The statement gcnx_collate_edges implements: for every selection (repeats, a single graph without entries, a full
    permutation) the re-based blocks of the union's transposed pattern equal the stable sort of the batch's own CSR."""
    u = L.union(seed=seed)
    gp, rp = u["node_ptr"].astype(np.int64), u["rowptr"].astype(np.int64)
    assert (np.diff(rp[gp]) == 0).sum() >= (3 if seed == 0 else 2)      # graphs without any entry (the one-node graphs at least)
    union_t = L.transpose_perm(u["rowptr"], u["colidx"])
    assert np.array_equal(union_t[0].astype(np.int64)[gp], rp[gp])      # the block-diagonality the re-basing rests on
    for sel in L.SELECTIONS:
        o = L.gather(u, sel, union_t)
        n, nnz = len(o["rowptr"]) - 1, len(o["colidx"])
        rows = np.repeat(np.arange(n), np.diff(o["rowptr"]))
        assert o["rowptr"][0] == 0 and o["rowptr"][-1] == nnz and np.all(np.diff(o["rowptr"]) >= 0)
        want = L.transpose_perm(o["rowptr"], o["colidx"])
        for name, w in zip(("rowptr_t", "colidx_t", "perm_t"), want):
            assert o[name].dtype == np.int32 and np.array_equal(o[name], w), (seed, sel, name)
        # and it is a transpose: entry p of it is entry perm_t[p] of the batch, read the other way round
        dst = np.repeat(np.arange(n), np.diff(o["rowptr_t"]))
        assert np.array_equal(rows[o["perm_t"]], o["colidx_t"]) and np.array_equal(o["colidx"][o["perm_t"]], dst)

"""GPU tests of graph preparation and of the node side of the device collate, through the C ABI: gcnx_coo_to_csr, gcnx_gcn_norm,
gcnx_csr_inspect, gcnx_csr_transpose, gcnx_csr_transpose_perm, gcnx_collate / gcnx_collate2 (and gcnx_collate_edges over a graph
that takes more than one pass of its loops) against the NumPy reference of tests/graph_prep_ref.py, which
tests/test_graph_prep_host.py pins on the CPU.  Outputs are sentinel frames (tests/gpu_frames.py; a 1-D array is a one-row
frame): integers and float bit patterns are compared exactly -- gcn_norm's values against a derived bound -- every element
outside the written range must still hold the sentinel, every input is downloaded afterwards and must be unchanged, and a
second call must give the same bits."""
import ctypes as C

import numpy as np
import pytest

import ecc_loader_ref as L
import graph_prep_ref as P
from gpu_frames import Frame, bits

pytestmark = pytest.mark.gpu
OK, ERR_INVALID, ERR_DATA = 0, 1, 6
MODES = {"spektral": 0, "pyg": 1}
EVERY = P.SYMMETRIC | P.BLOCK_DIAGONAL | P.GRAPH_PTR_OK


def _vec(ctx, n, dtype, data=None, lead=5, tail=9):
    return Frame(ctx, 1, n, n, lead, data=data, tail=tail, dtype=dtype)


class _In:
    """An input operand: uploaded once, and unchanged() after the calls."""

    def __init__(self, ctx, host, dtype):
        self.host = np.ascontiguousarray(host, dtype)
        self.dev = ctx.to_device(self.host)
        self.ptr = self.dev.ptr

    def unchanged(self):
        assert self.dev.numpy().tobytes() == self.host.tobytes(), "an input was written"


def _message(ctx, rc, code, match):
    from gcnx import _lib
    with pytest.raises(_lib.GcnxError, match=match) as e:
        ctx._ck(rc)
    assert e.value.code == code


# ---- gcnx_coo_to_csr -----------------------------------------------------------------------------------------------------------
def _coo(ctx, rows, cols, n):
    nnz = len(rows)
    r, c = _In(ctx, rows, np.int64), _In(ctx, cols, np.int64)
    rp, ci = _vec(ctx, n + 1, np.int32), _vec(ctx, nnz, np.int32, tail=7)
    return r, c, rp, ci, lambda: ctx.lib.gcnx_coo_to_csr(ctx.h, r.ptr, c.ptr, nnz, n, rp.view.ptr, ci.view.ptr)


@pytest.mark.parametrize("name", sorted(P.coo_cases()))
def test_coo_to_csr_equals_the_reference(ctx, name):
    rows, cols, n = P.coo_cases()[name]
    r, c, rp, ci, call = _coo(ctx, rows, cols, n)
    want_rp, want_ci = P.coo_to_csr(rows, cols, n)
    for again in (False, True):
        assert call() == OK
        rp.check(want_rp, (name, "rowptr", again))
        ci.check(want_ci, (name, "colidx", again))
    r.unchanged()
    c.unchanged()


@pytest.mark.parametrize("name", sorted(P.coo_refusals()))
def test_coo_to_csr_refuses_and_stays_inside_its_outputs(ctx, name):
    rows, cols, n = P.coo_refusals()[name]
    r, c, rp, ci, call = _coo(ctx, rows, cols, n)
    rc = call()
    assert rc == ERR_DATA
    _message(ctx, rc, ERR_DATA, "gcnx_coo_to_csr")
    rp.numpy()                                                              # asserts: nothing outside rowptr[0..n] ...
    ci.numpy()                                                              # ... and colidx[0..nnz) was written
    r.unchanged()
    c.unchanged()
    # the flag is cleared per call: a correct conversion straight afterwards, into the same outputs
    good_r, good_c = np.sort(np.clip(rows, 0, n - 1)), np.clip(cols, 0, n - 1)
    r2, c2 = _In(ctx, good_r, np.int64), _In(ctx, good_c, np.int64)
    assert ctx.lib.gcnx_coo_to_csr(ctx.h, r2.ptr, c2.ptr, len(rows), n, rp.view.ptr, ci.view.ptr) == OK
    want_rp, want_ci = P.coo_to_csr(good_r, good_c, n)
    rp.check(want_rp)
    ci.check(want_ci)


def test_coo_to_csr_refuses_sizes_beyond_int32_before_any_launch(ctx):
    r, c, rp, ci, _ = _coo(ctx, np.zeros(4, np.int64), np.arange(4), 4)
    for nnz, n in ((4, 2 ** 31 - 1), (2 ** 31 - 1, 4), (4, 2 ** 31), (-1, 4), (4, -1)):
        assert ctx.lib.gcnx_coo_to_csr(ctx.h, r.ptr, c.ptr, nnz, n, rp.view.ptr, ci.view.ptr) == ERR_INVALID, (nnz, n)
    assert ctx.lib.gcnx_coo_to_csr(ctx.h, r.ptr, c.ptr, 4, 4, None, ci.view.ptr) == ERR_INVALID
    assert ctx.lib.gcnx_coo_to_csr(ctx.h, None, c.ptr, 4, 4, rp.view.ptr, ci.view.ptr) == ERR_INVALID
    rp.untouched()
    ci.untouched()


# ---- gcnx_gcn_norm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.NORM_SIZES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", ["spektral", "pyg"])
def test_gcn_norm_within_the_derived_bound(ctx, mode, weighted, n):
    """Per entry (r, c) the float32 result lies within ((m_r + m_c) / 2 + 8) * 2^-24 relative of the float64 reference
    (graph_prep_ref.gcn_norm_bound: derived from the operations, not measured); entries of and towards a zero-degree row are
    exactly 0.  Largest error / bound observed on an MI355X over all cases: 0.377 (spektral, stored values, n = 257;
    every case prints its own figure)."""
    rp, ci, vals, zero = P.norm_case(n, weighted, mode)
    nnz = ci.size
    d_rp, d_ci = _In(ctx, rp, np.int32), _In(ctx, ci, np.int32)
    d_v = _In(ctx, vals, np.float32) if weighted else None
    out = _vec(ctx, nnz, np.float32)

    def call(v_in, v_out):
        return ctx.lib.gcnx_gcn_norm(ctx.h, d_rp.ptr, d_ci.ptr, v_in, n, MODES[mode], v_out)
    assert call(d_v.ptr if weighted else None, out.view.ptr) == OK
    got = out.numpy()[0]
    ref, bound = P.gcn_norm(rp, ci, vals, mode), P.gcn_norm_bound(rp, ci)
    nz = ref != 0
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err[nz] / (bound[nz] * np.abs(ref[nz])))) if nz.any() else 0.0
    print(f"gcn_norm {mode} weighted={weighted} n={n}: largest error / bound = {ratio:.3f}")
    assert np.all(np.isfinite(got))
    assert np.all(bits(got[~nz]) == 0), "an entry of or towards a zero-degree row is not exactly 0"
    rows = P._rows(rp)
    assert np.array_equal(~nz, np.isin(rows, zero) | np.isin(ci, zero))
    worst = int(np.argmax(err - bound * np.abs(ref)))
    assert np.all(err <= bound * np.abs(ref)), (rows[worst], ci[worst], got[worst], ref[worst], err[worst] / abs(ref[worst]), bound[worst])
    assert call(d_v.ptr if weighted else None, out.view.ptr) == OK          # again: the same bits
    out.check(got)
    if weighted:                                                            # in place: the same bits as out of place
        io = _vec(ctx, nnz, np.float32, data=vals)
        assert call(io.view.ptr, io.view.ptr) == OK
        io.check(got, "in place")
        d_v.unchanged()
    d_rp.unchanged()
    d_ci.unchanged()


@pytest.mark.parametrize("mode", ["spektral", "pyg"])
def test_gcn_norm_reports_a_single_missing_diagonal_and_clears_its_flag(ctx, mode):
    n = 600
    rp, ci, vals, _ = P.norm_case(n, True, mode)
    good = [_In(ctx, rp, np.int32), _In(ctx, ci, np.int32), _In(ctx, vals, np.float32)]
    want = None
    for r in (0, 255, 256, n - 1):
        rp2, ci2, v2 = P.drop_diagonal(rp, ci, vals, r)
        bad = [_In(ctx, rp2, np.int32), _In(ctx, ci2, np.int32), _In(ctx, v2, np.float32)]
        out = _vec(ctx, ci2.size, np.float32)
        rc = ctx.lib.gcnx_gcn_norm(ctx.h, bad[0].ptr, bad[1].ptr, bad[2].ptr, n, MODES[mode], out.view.ptr)
        assert rc == ERR_DATA, r
        _message(ctx, rc, ERR_DATA, "diagonal")
        out.numpy()                                                         # asserts: nothing outside vals_out[0..nnz)
        # pattern only: the same row is missed
        assert ctx.lib.gcnx_gcn_norm(ctx.h, bad[0].ptr, bad[1].ptr, None, n, MODES[mode], out.view.ptr) == ERR_DATA, r
        full = _vec(ctx, ci.size, np.float32)
        assert ctx.lib.gcnx_gcn_norm(ctx.h, good[0].ptr, good[1].ptr, good[2].ptr, n, MODES[mode], full.view.ptr) == OK, r
        want = full.numpy() if want is None else want
        full.check(want, r)
        for a in bad:
            a.unchanged()
    for a in good:
        a.unchanged()


def test_gcn_norm_empty_and_unknown_mode(ctx):
    assert ctx.lib.gcnx_gcn_norm(ctx.h, None, None, None, 0, 0, None) == OK
    assert ctx.lib.gcnx_gcn_norm(ctx.h, None, None, None, 0, 1, None) == OK
    rp, ci, vals, _ = P.norm_case(255, True, "pyg")
    d = [_In(ctx, rp, np.int32), _In(ctx, ci, np.int32), _In(ctx, vals, np.float32)]
    out = _vec(ctx, ci.size, np.float32)
    for mode in (2, -1, 7):
        rc = ctx.lib.gcnx_gcn_norm(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, 255, mode, out.view.ptr)
        assert rc == ERR_INVALID
        _message(ctx, rc, ERR_INVALID, "gcnx_gcn_norm: unknown mode")
    assert ctx.lib.gcnx_gcn_norm(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, -1, 0, out.view.ptr) == ERR_INVALID
    assert ctx.lib.gcnx_gcn_norm(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr, 255, 0, None) == ERR_INVALID
    assert ctx.lib.gcnx_gcn_norm(ctx.h, None, d[1].ptr, d[2].ptr, 255, 0, out.view.ptr) == ERR_INVALID
    out.untouched()
    for a in d:
        a.unchanged()


# ---- gcnx_csr_inspect ----------------------------------------------------------------------------------------------------------
def _inspect(ctx, m, vals=True, graph_ptr=True):
    d = {k: _In(ctx, m[k], np.float32 if k == "vals" else np.int32) for k in ("rowptr", "colidx", "vals", "graph_ptr")}
    b = len(m["graph_ptr"]) - 1 if graph_ptr else 0
    got = []
    for _ in range(2):
        props = C.c_int(-1)
        assert ctx.lib.gcnx_csr_inspect(ctx.h, d["rowptr"].ptr, d["colidx"].ptr, d["vals"].ptr if vals else None, m["n"],
                                        d["graph_ptr"].ptr if graph_ptr else None, b, C.byref(props)) == OK
        got.append(props.value)
    for a in d.values():
        a.unchanged()
    assert got[0] == got[1]
    return got[0]


@pytest.mark.parametrize("name", sorted(P.inspect_cases()))
def test_csr_inspect_truth_table(ctx, name):
    """One change to a symmetric, block-diagonal, weighted batch at a time clears exactly the bits the table names
    (graph_prep_ref.inspect_cases; the reference gives the same answer for a tolerance of 4 and of 8 ulp)."""
    m, cleared = P.inspect_cases()[name]
    assert _inspect(ctx, m) == EVERY & ~cleared == P.inspect(m["rowptr"], m["colidx"], m["vals"], m["n"], m["graph_ptr"])
    # without graph_ptr only SYMMETRIC can be reported
    assert _inspect(ctx, m, graph_ptr=False) == P.SYMMETRIC & ~cleared
    # without values only the pattern counts
    want = P.inspect(m["rowptr"], m["colidx"], None, m["n"], m["graph_ptr"])
    assert _inspect(ctx, m, vals=False) == want and (want == EVERY & ~cleared or name.startswith("value_"))


def test_csr_inspect_empty_and_arguments(ctx):
    gp = _In(ctx, np.zeros(3, np.int32), np.int32)
    props = C.c_int(-1)
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, 0, gp.ptr, 2, C.byref(props)) == OK and props.value == EVERY
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, 0, None, 0, C.byref(props)) == OK and props.value == P.SYMMETRIC
    bad = _In(ctx, np.array([0, 1, 0], np.int32), np.int32)                 # graph_ptr[b] != n
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, 0, bad.ptr, 2, C.byref(props)) == OK and props.value == P.SYMMETRIC
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, 0, gp.ptr, 2, None) == ERR_INVALID
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, 5, gp.ptr, 2, C.byref(props)) == ERR_INVALID and props.value == 0
    assert ctx.lib.gcnx_csr_inspect(ctx.h, None, None, None, -1, gp.ptr, 2, C.byref(props)) == ERR_INVALID
    gp.unchanged()
    bad.unchanged()


def test_device_csr_acts_on_the_inspected_bits(ctx):
    from gcnx.device import DeviceCSR
    cases = P.inspect_cases()

    def csr(name, **kw):
        m, _ = cases[name]
        return DeviceCSR.from_host_csr(ctx, m["rowptr"], m["colidx"], m["vals"], graph_ptr=m["graph_ptr"], **kw)
    assert csr("base").symmetric is True
    assert csr("one_way_survivor_at_68").symmetric is False and csr("value_1.99_16ulp").symmetric is False
    assert csr("value_1.99_4ulp").symmetric is True
    for name in ("edge_between_graphs", "edge_between_graphs_long_row", "gp_decreasing", "col_n"):
        with pytest.raises(ValueError, match="block-diagonal"):
            csr(name)
    assert csr("edge_between_graphs", symmetric=True).symmetric is True      # told by the caller: not inspected


# ---- gcnx_csr_transpose / gcnx_csr_transpose_perm ---------------------------------------------------------------------------------
def _transposes(ctx, rp, ci, vals, n, nnz):
    """Inputs, output frames and the two calls (vals None: the pattern alone)."""
    d = [_In(ctx, rp, np.int32), _In(ctx, ci, np.int32), _In(ctx, vals, np.float32) if vals is not None else None]
    o = {"rp": _vec(ctx, n + 1, np.int32), "ci": _vec(ctx, nnz, np.int32, tail=7), "v": _vec(ctx, nnz, np.float32, tail=7),
         "rp2": _vec(ctx, n + 1, np.int32), "ci2": _vec(ctx, nnz, np.int32, tail=7), "pm": _vec(ctx, nnz, np.int32, tail=7)}

    def plain(vals_t=True):
        return ctx.lib.gcnx_csr_transpose(ctx.h, d[0].ptr, d[1].ptr, d[2].ptr if d[2] is not None else None, n, nnz,
                                          o["rp"].view.ptr, o["ci"].view.ptr, o["v"].view.ptr if vals_t else None)

    def perm():
        return ctx.lib.gcnx_csr_transpose_perm(ctx.h, d[0].ptr, d[1].ptr, n, nnz, o["rp2"].view.ptr, o["ci2"].view.ptr, o["pm"].view.ptr)
    return d, o, plain, perm


@pytest.mark.parametrize("name", sorted(P.transpose_cases()))
def test_both_transposes_equal_the_reference(ctx, name):
    rp, ci, vals = P.transpose_cases()[name]
    n, nnz = len(rp) - 1, ci.size
    rp_t, ci_t, pm_t, v_t = P.transpose(rp, ci, vals)
    d, o, plain, perm = _transposes(ctx, rp, ci, vals, n, nnz)
    for again in (False, True):
        assert plain() == OK and perm() == OK
        for k, want in (("rp", rp_t), ("rp2", rp_t), ("ci", ci_t), ("ci2", ci_t), ("pm", pm_t), ("v", v_t)):
            o[k].check(want, (name, k, again))
        assert np.array_equal(bits(o["v"].numpy()[0]), bits(vals[o["pm"].numpy()[0]]))       # vals_t == vals[perm_t]
    # the pattern alone: the same integers, no values written
    d0, o0, plain0, _ = _transposes(ctx, rp, ci, None, n, nnz)
    assert plain0(vals_t=False) == OK
    o0["rp"].check(rp_t)
    o0["ci"].check(ci_t)
    o0["v"].untouched()
    for a in d + d0:
        if a is not None:
            a.unchanged()


_SMALL = ([0, 2, 3, 3, 5], [1, 3, 0, 0, 2])                                 # a well-formed 4-row CSR of 5 entries
MALFORMED = {"rowptr0_not_0": ([1, 2, 3, 3, 5], _SMALL[1], "rowptr"), "rowptr_decreasing": ([0, 4, 3, 3, 5], _SMALL[1], "rowptr"),
             "rowptr_decreasing_far": ([0, 10, 3], [0, 1, 0], "rowptr"), "rowptr_n_not_nnz": ([0, 2, 3, 3, 4], _SMALL[1], "rowptr"),
             "col_eq_n": (_SMALL[0], [1, 3, 0, 4, 2], "colidx"), "col_negative": (_SMALL[0], [1, 3, -1, 0, 2], "colidx")}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_both_transposes_refuse_a_malformed_csr(ctx, name):
    """GCNX_ERR_DATA with a message that names the function and the array, before the counting sort reads past its host copies;
    nothing is written."""
    rp, ci, what = MALFORMED[name]
    n, nnz = len(rp) - 1, len(ci)
    d, o, plain, perm = _transposes(ctx, rp, ci, np.arange(nnz, dtype=np.float32), n, nnz)
    for call, fn in ((plain, "gcnx_csr_transpose: "), (perm, "gcnx_csr_transpose_perm: ")):
        rc = call()
        assert rc == ERR_DATA, fn
        _message(ctx, rc, ERR_DATA, fn + ".*" + what)
    for f in o.values():
        f.untouched(name)
    for a in d:
        a.unchanged()


def test_transposes_validate_their_arguments(ctx):
    rp, ci = _SMALL
    d, o, plain, perm = _transposes(ctx, rp, ci, np.arange(5, dtype=np.float32), 4, 5)
    rc = plain(vals_t=False)                                                # vals given without vals_t
    assert rc == ERR_INVALID
    _message(ctx, rc, ERR_INVALID, "gcnx_csr_transpose: vals and vals_t")
    h, lib = ctx.h, ctx.lib
    assert lib.gcnx_csr_transpose(h, d[0].ptr, d[1].ptr, None, 4, 5, o["rp"].view.ptr, o["ci"].view.ptr, o["v"].view.ptr) == ERR_INVALID
    assert lib.gcnx_csr_transpose(h, None, d[1].ptr, None, 4, 5, o["rp"].view.ptr, o["ci"].view.ptr, None) == ERR_INVALID
    assert lib.gcnx_csr_transpose(h, d[0].ptr, d[1].ptr, None, 4, 5, o["rp"].view.ptr, None, None) == ERR_INVALID
    assert lib.gcnx_csr_transpose(h, d[0].ptr, d[1].ptr, None, -1, 5, o["rp"].view.ptr, o["ci"].view.ptr, None) == ERR_INVALID
    assert lib.gcnx_csr_transpose_perm(h, d[0].ptr, d[1].ptr, 4, 5, o["rp2"].view.ptr, o["ci2"].view.ptr, None) == ERR_INVALID
    assert lib.gcnx_csr_transpose_perm(h, d[0].ptr, d[1].ptr, 4, 5, None, o["ci2"].view.ptr, o["pm"].view.ptr) == ERR_INVALID
    assert lib.gcnx_csr_transpose_perm(h, d[0].ptr, d[1].ptr, 4, -5, o["rp2"].view.ptr, o["ci2"].view.ptr, o["pm"].view.ptr) == ERR_INVALID
    for f in o.values():
        f.untouched()
    assert plain() == OK and perm() == OK
    rp_t, ci_t, pm_t, v_t = P.transpose(np.array(rp), np.array(ci), np.arange(5, dtype=np.float32))
    for k, want in (("rp", rp_t), ("rp2", rp_t), ("ci", ci_t), ("ci2", ci_t), ("pm", pm_t), ("v", v_t)):
        o[k].check(want, k)


# ---- gcnx_collate / gcnx_collate2: the node side -----------------------------------------------------------------------------------
class _Union:
    """The resident dataset of graph_prep_ref.collate_union(f) on the device, x and the second node matrix in a layout."""

    def __init__(self, ctx, f, c, layout):
        self.ctx, self.f, self.c, self.u = ctx, f, c, P.collate_union(f)
        u = self.u
        self.ldx, xo, self.ldo, self.oo, self.lds, self.ldos = P.leading_dims(layout, f)
        n_all = u["x"].shape[0]
        x_host = np.full((n_all, self.ldx), 9.0, np.float32)
        x_host[:, xo:xo + f] = u["x"]
        s_host = np.full((n_all, self.lds), 7.0, np.float32)
        s_host[:, :f] = u["ax"]
        self.ins = {"x": _In(ctx, x_host, np.float32), "s": _In(ctx, s_host, np.float32), "node_ptr": _In(ctx, u["node_ptr"], np.int32),
                    "rowptr": _In(ctx, u["rowptr"], np.int32), "colidx": _In(ctx, u["colidx"], np.int32),
                    "vals": _In(ctx, u["vals"], np.float32), "y": _In(ctx, u["y300"][:, :c], np.float32)}
        self.x_ptr = self.ins["x"].ptr + 4 * xo

    def outputs(self, sel):
        """Capacity-sized sentinel frames for the batch ``sel``: n + 5 rows, nnz + 7 entries, b + 2 label rows."""
        ctx, f, c = self.ctx, self.f, self.c
        desc, n, nnz = L.descriptor(self.u, sel)
        b = len(sel)
        o = {"rowptr": _vec(ctx, n + 1, np.int32, tail=5), "colidx": _vec(ctx, nnz, np.int32, tail=7),
             "vals": _vec(ctx, nnz, np.float32, tail=7), "x": Frame(ctx, n, f, self.ldo, 4 + self.oo, tail=5 * self.ldo + 3),
             "ax": Frame(ctx, n, f, self.ldos, 3, tail=5 * self.ldos + 1), "y": Frame(ctx, b, c, c, 2, tail=2 * c + 1),
             "graph_ptr": _vec(ctx, b + 1, np.int32, tail=2), "ids": _vec(ctx, n, np.int32, tail=5)}
        return _In(ctx, desc, np.int32), o

    def call(self, desc_in, n_graphs, o, /, use_vals=True, use_ids=True, use_s=True, **over):
        """gcnx_collate2, or gcnx_collate when there is no second matrix.  ``over``: arguments replaced by name."""
        i = self.ins
        a = dict(desc=desc_in.ptr, b=n_graphs, node_ptr=i["node_ptr"].ptr, rowptr=i["rowptr"].ptr, colidx=i["colidx"].ptr,
                 vals=i["vals"].ptr if use_vals else None, x=self.x_ptr, ldx=self.ldx, f=self.f, y=i["y"].ptr if self.c else None,
                 c=self.c, o_rowptr=o["rowptr"].view.ptr, o_colidx=o["colidx"].view.ptr, o_vals=o["vals"].view.ptr if use_vals else None,
                 o_x=o["x"].view.ptr, ldo=self.ldo, o_y=o["y"].view.ptr, o_graph_ptr=o["graph_ptr"].view.ptr,
                 o_ids=o["ids"].view.ptr if use_ids else None, s=i["s"].ptr, lds=self.lds, o_s=o["ax"].view.ptr, ldos=self.ldos)
        a.update(over)
        head = (self.ctx.h, a["desc"], a["b"], a["node_ptr"], a["rowptr"], a["colidx"], a["vals"], a["x"], a["ldx"], a["f"], a["y"], a["c"],
                a["o_rowptr"], a["o_colidx"], a["o_vals"], a["o_x"], a["ldo"], a["o_y"], a["o_graph_ptr"], a["o_ids"])
        if not use_s:
            return self.ctx.lib.gcnx_collate(*head)
        return self.ctx.lib.gcnx_collate2(*head, a["s"], a["lds"], a["o_s"], a["ldos"])

    def unchanged(self):
        for a in self.ins.values():
            a.unchanged()


@pytest.mark.parametrize("layout,f,c,vals,ids,s", P.collate_configs())
def test_collate_equals_gather_nodes(ctx, layout, f, c, vals, ids, s):
    """Every selection (the large graph first, in the middle, last and twice; graphs without entries first and last): the batch
    equals graph_prep_ref.gather_nodes exactly, and what the call was not given or lies outside the batch keeps its sentinel."""
    d = _Union(ctx, f, c, layout)
    for sel in P.SELECTIONS:
        want = P.gather_nodes(d.u, sel, c)
        desc, o = d.outputs(sel)
        b, n, nnz = len(sel), len(want["ids"]), len(want["colidx"])
        written = {"rowptr", "colidx", "graph_ptr", "x"} | ({"vals"} if vals else set()) | ({"ids"} if ids else set()) | \
                  ({"ax"} if s else set()) | ({"y"} if c else set())
        for again in (False, True):
            assert d.call(desc, b, o, use_vals=vals, use_ids=ids, use_s=s) == OK
            for k, frame in o.items():
                if k in written:
                    frame.check(want[k], (sel, k, again))
                else:
                    frame.untouched((sel, k))
        got_rp, got_gp = o["rowptr"].numpy()[0], o["graph_ptr"].numpy()[0]
        assert got_rp[n] == nnz and got_gp[b] == n and got_rp[0] == 0 and got_gp[0] == 0
        if ids:
            assert np.array_equal(o["ids"].numpy()[0], np.repeat(np.arange(b), np.diff(got_gp)))
        desc.unchanged()
    d.unchanged()


def test_collate_validates_its_arguments_and_writes_nothing(ctx):
    d = _Union(ctx, 3, 2, "dense")
    sel = [4, 0, 7]
    desc, o = d.outputs(sel)
    required = ("desc", "node_ptr", "rowptr", "colidx", "o_rowptr", "o_colidx", "o_graph_ptr", "x", "o_x")
    for k in required:
        for s in (False, True):
            assert d.call(desc, 3, o, use_s=s, **{k: None}) == ERR_INVALID, k
    assert d.call(desc, 3, o, ldx=2) == ERR_INVALID and d.call(desc, 3, o, ldo=2) == ERR_INVALID
    assert d.call(desc, 3, o, o_vals=None) == ERR_INVALID                   # vals without o_vals
    assert d.call(desc, 3, o, vals=None) == ERR_INVALID                     # o_vals without vals
    assert d.call(desc, 3, o, o_y=None) == ERR_INVALID                      # y without o_y
    assert d.call(desc, 3, o, o_s=o["x"].view.ptr) == ERR_INVALID           # o_s == o_x
    assert d.call(desc, 3, o, o_s=None) == ERR_INVALID and d.call(desc, 3, o, lds=2) == ERR_INVALID and d.call(desc, 3, o, ldos=2) == ERR_INVALID
    assert d.call(desc, -1, o) == ERR_INVALID and d.call(desc, 3, o, f=-1) == ERR_INVALID and d.call(desc, 3, o, c=-1) == ERR_INVALID
    rc = d.call(desc, 3, o, ldo=2)
    _message(ctx, rc, ERR_INVALID, "gcnx_collate")
    assert d.call(desc, 0, o) == OK and d.call(desc, 0, o, use_s=False) == OK   # b == 0: nothing to do
    assert ctx.lib.gcnx_collate(ctx.h, *([None, 0] + [None] * 5 + [0, 0, None, 0] + [None] * 4 + [0] + [None] * 3)) == OK
    for k, frame in o.items():
        frame.untouched(k)
    assert d.call(desc, 3, o) == OK                                         # and the same arguments, unreplaced, are served
    want = P.gather_nodes(d.u, sel, 2)
    for k, frame in o.items():
        frame.check(want[k], k)
    d.unchanged()


@pytest.mark.parametrize("layout", ["dense", "strided"])
def test_collate_edges_over_a_graph_of_more_than_one_pass(ctx, layout):
    """gcnx_collate_edges with the 12300-entry graph first and again in the middle, s = 3: its three loops (rows, entries,
    entries * s) run more than one pass of the 4096 threads a graph gets, in the flat and in the row / column copy."""
    s = 3
    u = P.collate_union(1, s=s)
    union_t = L.transpose_perm(u["rowptr"], u["colidx"])
    sel = [P.LARGE, 0, P.LARGE, 4]
    desc, n, nnz = L.descriptor(u, sel)
    want = L.gather(u, sel, union_t)
    lde, eo, ldoe, oo = (s, 0, s, 0) if layout == "dense" else (s + 3, 1, s + 5, 2)
    e_host = np.full((u["e"].shape[0], lde), 9.0, np.float32)
    e_host[:, eo:eo + s] = u["e"]
    ins = [_In(ctx, desc, np.int32), _In(ctx, u["node_ptr"], np.int32), _In(ctx, u["rowptr"], np.int32), _In(ctx, union_t[0], np.int32),
           _In(ctx, union_t[1], np.int32), _In(ctx, union_t[2], np.int32), _In(ctx, e_host, np.float32)]
    o = {"rowptr_t": _vec(ctx, n + 1, np.int32, tail=5), "colidx_t": _vec(ctx, nnz, np.int32, tail=7), "perm_t": _vec(ctx, nnz, np.int32, tail=7),
         "e": Frame(ctx, nnz, s, ldoe, 4 + oo, tail=7 * ldoe + 1)}
    for again in (False, True):
        assert ctx.lib.gcnx_collate_edges(ctx.h, ins[0].ptr, len(sel), *[a.ptr for a in ins[1:6]], ins[6].ptr + 4 * eo, lde, s, o["rowptr_t"].view.ptr,
                                          o["colidx_t"].view.ptr, o["perm_t"].view.ptr, o["e"].view.ptr, ldoe) == OK
        for k, frame in o.items():
            frame.check(want[k], (k, again))
    # and it is the transpose of the batch's own CSR
    batch_t = L.transpose_perm(want["rowptr"], want["colidx"])
    for k, w in zip(("rowptr_t", "colidx_t", "perm_t"), batch_t):
        assert np.array_equal(want[k], w)
    for a in ins:
        a.unchanged()


# ---- loader level ------------------------------------------------------------------------------------------------------------------
def test_a_last_batch_of_graphs_without_entries_equals_the_host_loaders(ctx):
    """DeviceDisjointLoader: the last batch holds only graphs without entries and reuses the buffers of a full batch -- nnz == 0, an
    all-zero rowptr of n + 1, and x, y, graph_ptr and ids as DeviceBatch.from_host of the host loader's batch."""
    import scipy.sparse as sp
    import gcnx
    from gcnx.models import DeviceBatch
    rng = np.random.default_rng(5)
    full = L.graphs(L.union(f=5, s=2, seed=1))
    graphs = [gcnx.Graph(x=full[j].x, a=full[j].a, y=full[j].y) for j in (0, 2, 6)]
    assert all(g.a.nnz > 0 for g in graphs)
    graphs += [gcnx.Graph(x=rng.standard_normal((k, 5)).astype(np.float32), a=sp.csr_matrix((k, k)), y=np.eye(2)[k % 2]) for k in (1, 3)]
    ds = gcnx.ListDataset(graphs)
    dev = gcnx.DeviceDisjointLoader(gcnx.DeviceDataset(ctx, ds, normalize=None), batch_size=3, epochs=1, shuffle=False)
    host = gcnx.DisjointLoader(ds, batch_size=3, epochs=1, shuffle=False)
    seen = []
    for (inputs, target), (db, none) in zip(host, dev):
        hb = DeviceBatch.from_host(ctx, inputs, target)
        n, nnz = hb.n, hb.a.nnz
        assert none is None and (db.n, db.a.nnz, db.n_graphs) == (n, nnz, hb.n_graphs)
        assert np.array_equal(bits(db.x.numpy()), bits(hb.x.numpy())) and np.array_equal(bits(db.y.numpy()), bits(hb.y.numpy()))
        assert db.a.rowptr.shape == (n + 1,) and np.array_equal(db.a.rowptr.numpy(), hb.a.rowptr.numpy())
        assert np.array_equal(db.a.colidx.numpy()[:nnz], hb.a.colidx.numpy()[:nnz])
        assert np.array_equal(db.seg.dev.numpy(), hb.seg.dev.numpy()) and np.array_equal(db.seg.host, hb.seg.host)
        assert np.array_equal(db.seg.ids.numpy()[:n], hb.seg.ids.numpy()[:n])
        seen.append((db.n_graphs, n, nnz, db.a.rowptr.numpy().tolist()))
    assert [s[0] for s in seen] == [3, 2] and seen[0][2] > 0
    assert seen[1][1:] == (4, 0, [0] * 5)

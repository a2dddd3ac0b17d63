"""CPU tests of the mask-product route of dW2 (gcnx_gemm_dw2_graph): the exact three-way bf16 split the kernel relies on
(NumPy emulation of round-to-nearest-even), the slice plan against a Python restatement, the identity behind the route in
float64, and the ABI."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gcnx_dw2_slice_plan", "gcnx_dw2_slices_ok", "gcnx_gemm_dw2_graph_kchunk", "gcnx_gemm_dw2_graph_ok", "gcnx_gemm_dw2_graph"]


# ---- 1. hi + mid + lo == x ------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite inputs; gradual underflow."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r1 = x - hi                                   # exact in fp32: at most 16 significant bits
    mid = bf16_rne(r1)
    r2 = r1 - mid                                 # exact: at most 8
    lo = bf16_rne(r2)
    return hi, mid, lo


def f32_from(sign, exp, frac):
    return ((np.asarray(sign, np.uint32) << 31) | (np.asarray(exp, np.uint32) << 23) | np.asarray(frac, np.uint32)).view(np.float32)


def assert_exact(x):
    hi, mid, lo = split3(x)
    for piece in (hi, mid, lo):                   # each piece IS a bfloat16
        assert not (piece.view(np.uint32) & 0xFFFF).any()
    total = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64))


def test_three_way_split_is_exact_on_random_floats():
    """10^5 floats over the normal exponents the split serves: 2^-110 <= |x|, and below the top binade's last bf16 step
    (from 0x7F7F8000 on, bf16(x) itself rounds to infinity -- as every bf16 conversion does)."""
    rng = np.random.default_rng(0)
    n = 100_000
    x = f32_from(rng.integers(0, 2, n), rng.integers(127 - 110, 255, n), rng.integers(0, 1 << 23, n))
    x = x[np.abs(x) < f32_from(0, 254, 0x7F8000)]
    assert x.size > 99_000
    assert_exact(x)


def test_three_way_split_is_exact_on_adversarial_significands():
    fracs = [0x7FFFFF,                            # all ones: hi rounds up into the next binade, mid and lo are negative
             0x7FFF80,                            # all ones above the last 7 bits
             0x008000, 0x018000,                  # ties at the first rounding step: to even down / up
             0x000080, 0x000180, 0x7F0080,        # ties at the second step
             0x008080, 0x018180,                  # ties at both
             0x000001, 0x000000, 0x400000, 0x3FFFFF, 0x7F7F7F, 0x010101]
    exps = [127 - 110, 1 + 16, 100, 127, 128, 200, 253]
    x = np.array([f32_from(s, e, f) for s in (0, 1) for e in exps for f in fracs], np.float32)
    assert_exact(x)
    assert_exact(np.array([0.0, -0.0], np.float32))
    hi, mid, lo = split3(np.array([-0.0], np.float32))
    assert np.signbit(hi[0]) and mid[0] == 0 and lo[0] == 0


def test_the_one_exclusion_is_bounded():
    """|x| < 2^-110: lo's last bits fall below the smallest bf16 subnormal, 2^-133; the split is then off by less than that
    (an entry of S2 = A Y1 of that size is ~1e-33)."""
    rng = np.random.default_rng(1)
    n = 50_000
    x = f32_from(rng.integers(0, 2, n), rng.integers(0, 127 - 110, n), rng.integers(0, 1 << 23, n))      # subnormals included
    hi, mid, lo = split3(x)
    err = np.abs(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) - x.astype(np.float64))
    assert err.max() < 2.0 ** -133 and err.max() > 0


# ---- 2. the slice plan ----------------------------------------------------------------------------------------------------------
def plan_ref(sizes, kchunk):
    out, r0 = [], 0
    for g, k in enumerate(sizes):
        for r in range(r0, r0 + k, kchunk):
            out.append((r, min(r + kchunk, r0 + k), g, int((np.float32(1.0) / np.float32(k)).view(np.int32))))
        r0 += k
    return np.array(out, np.int32).reshape(-1, 4)


@pytest.mark.parametrize("sizes", [[1], [31, 32, 33], [352, 353, 705], [1] * 90], ids=lambda s: "x".join(map(str, s[:3])) + f"-{len(s)}g")
def test_slice_plan(sizes):
    from gcnx import _lib
    from gcnx import device as D
    lib = _lib.load()
    kchunk = 352
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(gp[-1])
    plan = D.dw2_slice_plan(gp, kchunk)
    assert np.array_equal(plan, plan_ref(sizes, kchunk))
    covered = np.zeros(n, int)
    for r0, r1, g, inv in plan:
        assert gp[g] <= r0 < r1 <= gp[g + 1]                                 # no slice spans graphs, none is empty
        assert np.int32(inv).view(np.float32) == np.float32(1.0) / np.float32(sizes[g])   # AVG's factor, as the backward forms it
        assert r1 - r0 <= kchunk and (r0 - gp[g]) % 32 == 0                  # cuts on multiples of the K step from the graph's start
        assert r1 == gp[g + 1] or (r1 - gp[g]) % kchunk == 0                 # only a graph's last slice is ragged
        covered[r0:r1] += 1
    assert (covered == 1).all()                                              # every row in exactly one slice
    uniform = -(-n // kchunk)
    ok = lib.gcnx_dw2_slices_ok(n, kchunk, len(plan))
    assert ok == (1 if len(plan) <= max(2 * uniform, 64) else 0)
    assert ok == (0 if len(sizes) == 90 else 1)                              # 90 graphs of one row: refused
    if len(sizes) == 3 and sizes[0] == 352:
        assert len(plan) == 6 and uniform == 5
    # counting without a table, a short table, bad arguments
    assert lib.gcnx_dw2_slice_plan(gp.ctypes.data, len(sizes), kchunk, None, 0) == len(plan)
    short = np.full((1, 4), -7, np.int32)
    assert lib.gcnx_dw2_slice_plan(gp.ctypes.data, len(sizes), kchunk, short.ctypes.data, 1) == len(plan) and np.array_equal(short[0], plan[0])
    assert lib.gcnx_dw2_slice_plan(gp.ctypes.data, len(sizes), 350, None, 0) == -1 and lib.gcnx_dw2_slice_plan(None, 1, kchunk, None, 0) == -1


def test_config2_slice_count():
    """E. coli-shaped graph sizes of the benchmark batch at the launch's 352-row slices: 79 slices against 65 uniform ones."""
    from gcnx import device as D
    from gcnx import synth
    sizes = synth.ecoli_sizes(32, seed=1)
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert int(gp[-1]) == 22576
    assert len(D.dw2_slice_plan(gp, 352)) == 79 and -(-22576 // 352) == 65


# ---- 3. the identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_identity_in_float64(mode):
    rng = np.random.default_rng(2)
    sizes = [5, 40, 1, 17]
    n, fi, fo = sum(sizes), 12, 9
    ids = np.repeat(np.arange(len(sizes)), sizes)
    s2, mask, dp = rng.standard_normal((n, fi)), (rng.random((n, fo)) < 0.5).astype(np.float64), rng.standard_normal((len(sizes), fo))
    scale = dp if mode == "sum" else dp / np.asarray(sizes, np.float64)[:, None]
    direct = s2.T @ (mask * scale[ids])
    by_graph = sum(scale[g] * (s2[ids == g].T @ mask[ids == g]) for g in range(len(sizes)))
    assert np.allclose(direct, by_graph, rtol=1e-13, atol=1e-13)


# ---- 4. the ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_entry_points():
    from gcnx import _lib
    hdr = open(os.path.join(ROOT, "include", "gcnx.h")).read()
    for nm in NAMES:
        assert re.search(r"GCNX_API\s+(int|int64_t)\s+" + nm + r"\s*\(", hdr), nm
        assert nm in _lib.SIGNATURES, nm
    assert [len(_lib.SIGNATURES[nm]) for nm in NAMES] == [5, 3, 6, 10, 28]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gcnx_\w+)", out))
    lib = _lib.load()
    assert lib.gcnx_version() >= 429
    assert lib.gcnx_gemm_dw2_graph_ok(None, 1000, 128, 128, 128, 128, 352, 3, 0, 0) == 0          # no context: not served
    assert lib.gcnx_gemm_dw2_graph_kchunk(None, 1000, 128, 128, 128, 128) == 0

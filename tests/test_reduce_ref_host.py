"""tests/reduce_ref.py against the float64 oracle and against what a dropout stream has to be (no GPU).

The float32 pool references round once per output, so they sit within a few float32 roundings of the float64 oracle.  The
restated hash has to behave as a Bernoulli(1 - rate) stream: over N = 2^20 elements the kept fraction k / N has standard
deviation sqrt(rate (1 - rate) / N), and every statistic below is held to five of those."""
import numpy as np
import pytest

import reduce_ref as R
from conftest import rel_err

N = 1 << 20
EPS = 2.0 ** -23            # float32 spacing relative to the value: a single rounding is within EPS / 2


def O():
    from oracle import gcn_oracle
    return gcn_oracle


def _graphs(rng):
    sizes = [0, 1, 15, 16, 0, 17, 63, 64, 65, 300, 0]
    gp = np.concatenate([[0], np.cumsum(sizes)])
    x = rng.standard_normal((int(gp[-1]), 37)).astype(np.float32)
    return gp, x


@pytest.mark.parametrize("mode", ["sum", "avg", "max"])
def test_pool_references_agree_with_the_oracle(mode):
    rng = np.random.default_rng(11)
    gp, x = _graphs(rng)
    n, b = len(x), len(gp) - 1
    x[40:44, 5] = 9.0                                    # a tie: the first maximal row
    got, arg = R.pool_fwd(x, gp, mode)
    want, warg = O().global_pool_fwd(x.astype(np.float64), gp, mode)
    assert got.dtype == np.float32
    # one rounding of the sum, one of the quotient
    assert np.all(np.abs(got - want) <= 2 * EPS * np.abs(want))
    nonempty = np.diff(gp) > 0
    assert not got[~nonempty].any()
    if mode == "max":
        assert np.array_equal(arg[nonempty], warg[nonempty]) and (arg[~nonempty] == -1).all()
        assert arg[5, 5] == 40                             # rows 32 .. 48 are graph 5
    dp = rng.standard_normal((b, 37)).astype(np.float32)
    y = rng.standard_normal((n, 37)).astype(np.float32)
    dx = R.pool_bwd(dp, gp, n, mode, arg)
    wdx = O().global_pool_bwd(dp.astype(np.float64), gp, n, mode, warg)
    assert dx.dtype == np.float32 and dx.shape == (n, 37)
    assert np.all(np.abs(dx - wdx) <= 2 * EPS * np.abs(wdx))            # the reciprocal and the product
    dxm = R.pool_bwd(dp, gp, n, mode, arg, y=y)
    assert np.array_equal(dxm, np.where(y > 0, dx, 0))
    if mode != "max":
        db = R.pool_bwd_colsum(dp, gp, y, mode)
        assert rel_err(db, (wdx * (y > 0)).sum(0)) < 1e-6


def test_pool_references_are_exact_on_integers():
    rng = np.random.default_rng(12)
    gp = np.array([0, 0, 1, 17, 17, 81, 593, 593])
    n = int(gp[-1])
    x = rng.integers(-3, 4, (n, 9)).astype(np.float32)
    s, _ = R.pool_fwd(x, gp, "sum")
    a, _ = R.pool_fwd(x, gp, "avg")
    for g in range(len(gp) - 1):
        rows = x[gp[g]:gp[g + 1]].astype(np.int64)
        assert np.array_equal(s[g], rows.sum(0))
        if len(rows):
            assert np.array_equal(a[g], (rows.sum(0) / np.float32(len(rows))).astype(np.float32))
    dp = rng.integers(-3, 4, (len(gp) - 1, 9)).astype(np.float32)
    y = rng.integers(-3, 4, (n, 9)).astype(np.float32)
    dx = R.pool_bwd(dp, gp, n, "avg", y=y)                            # power-of-two graphs: exact quotients
    assert np.array_equal(dx.astype(np.float64).sum(0).astype(np.float32), R.pool_bwd_colsum(dp, gp, y, "avg"))
    dx = R.pool_bwd(dp, gp, n, "sum", y=y)
    assert np.array_equal(dx.astype(np.float64).sum(0).astype(np.float32), R.pool_bwd_colsum(dp, gp, y, "sum"))


def _bound(rate):
    return 5.0 * np.sqrt(rate * (1.0 - rate) / N)


@pytest.mark.parametrize("rate", [0.1, 0.4, 0.9])
def test_the_hash_keeps_one_minus_rate(rate):
    keep = R.dropout_keep(N // 256, 256, rate, seed=1234, stream_id=3)
    frac = keep.mean()
    print(f"rate {rate}: kept {frac:.6f}, bound {_bound(rate):.6f}")
    assert abs(frac - (1.0 - rate)) <= _bound(rate)


@pytest.mark.parametrize("rate", [0.1, 0.4, 0.9])
def test_streams_and_steps_are_independent(rate):
    base = R.dropout_keep(N // 256, 256, rate, seed=77, stream_id=1, step=0)
    want = (1.0 - rate) ** 2 + rate ** 2
    for name, other in (("stream", R.dropout_keep(N // 256, 256, rate, seed=77, stream_id=2, step=0)),
                        ("step", R.dropout_keep(N // 256, 256, rate, seed=77, stream_id=1, step=1)),
                        ("stream 1 step 1 / stream 2 step 0", None)):
        if other is None:                                        # stream_id and step do not collide
            a, other = R.dropout_keep(N // 256, 256, rate, 77, 1, 1), R.dropout_keep(N // 256, 256, rate, 77, 2, 0)
            agree = (a == other).mean()
        else:
            agree = (base == other).mean()
        print(f"rate {rate}, {name}: agree {agree:.6f}, independent {want:.6f}, bound {_bound(rate):.6f}")
        assert abs(agree - want) <= _bound(rate), name


def test_the_mask_is_that_of_the_flat_index():
    rng = np.random.default_rng(5)
    n, f = 300, 37
    wide = rng.standard_normal((n, f + 11)).astype(np.float32)
    view = wide[:, 4:4 + f]                                      # ld = f + 11
    assert not view.flags["C_CONTIGUOUS"]
    a = R.dropout(view, 0.4, 9, 2, 5)
    b = R.dropout(np.ascontiguousarray(view), 0.4, 9, 2, 5)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    keep = R.dropout_keep(n, f, 0.4, 9, 2, 5)
    k0, k1 = R.stream_keys(9, 2, 5)
    r, c = 123, 17
    assert keep[r, c] == (R.keep_bits(k0, k1, np.uint64(r * f + c))[0] >= R.dropout_thresh(0.4))
    assert np.array_equal(keep.ravel(), R.dropout_keep(1, n * f, 0.4, 9, 2, 5).ravel())
    # the high word of the index enters the hash
    lo = np.arange(4096, dtype=np.uint64)
    assert np.mean(R.keep_bits(k0, k1, lo) == R.keep_bits(k0, k1, lo + np.uint64(1 << 32))) < 0.01


def test_rate_zero_keeps_everything():
    x = np.random.default_rng(6).standard_normal((500, 37)).astype(np.float32)
    assert R.dropout_thresh(0.0) == 0 and R.dropout_scale(0.0) == np.float32(1)
    assert R.dropout_keep(500, 37, 0.0, 3, 4, 5).all()
    assert np.array_equal(R.dropout(x, 0.0, 3, 4, 5).view(np.uint32), x.view(np.uint32))
    assert R.dropout_thresh(0.999) == int(float(np.float32(0.999)) * 2.0 ** 32) < 0xFFFFFFFF
    assert R.dropout_thresh(np.nextafter(np.float32(1), np.float32(0))) <= 0xFFFFFFFF


def test_mix32_known_values():
    """murmur3's fmix32 (public test vectors of the finaliser): 0 -> 0, and a bijection on a sample."""
    assert R.mix32(0)[0] == 0
    assert R.mix32(1)[0] == 0x514E28B7
    v = R.mix32(np.arange(1 << 16, dtype=np.uint32))
    assert len(np.unique(v)) == 1 << 16

"""gcnx_dropout, gcnx_add and gcnx_sgd past the size at which their grids are capped and every thread loops.

grid_for (csrc/elementwise.hip) caps the grid at 16 cus workgroups of 256 threads, gcnx_sgd at 2048: beyond cap * 256
elements a thread takes a second trip through its grid-stride loop.  The totals below sit one element under the cap (one
trip), one over it (a second trip by a single thread) and at 2.5 times it (a third trip by half the grid); f = 1 reaches
them exactly, for f = 37 and f = 256 the row count is the nearest that stays on the same side, which each case asserts.

Dropout is held bit for bit to the stream restated in tests/reduce_ref.py -- a mask taken from gcnx_dropout itself cannot see
an index that depends on a leading dimension, or seed, stream and step running into each other.  (The index's high word is
zero below 2^32 elements: only the host test of the restatement reaches it.)  add and sgd are a single rounding: exact."""
import numpy as np
import pytest

import reduce_ref as R
from gpu_frames import SENTINEL, Frame, same as _same

pytestmark = pytest.mark.gpu

SEEDS = (20240607, 0xFFFFFFF1)
STREAMS = (0, 5)


def _cap(ctx):
    return 16 * ctx.info()["cus"] * 256                            # elements one trip of grid_for's grid covers


def _rows(ctx, which, f):
    """Rows of an [n, f] operand whose total sits where `which` says, and the trips the busiest thread takes."""
    cap = _cap(ctx)
    if which == "under":
        n, trips = (cap - 1) // f, 1
    elif which == "over":
        n, trips = -(-(cap + 1) // f), 2
    else:
        n, trips = (5 * cap // 2) // f, 3
    total = n * f
    assert (trips - 1) * cap < total <= trips * cap                # the grid-stride rule
    if f == 1:
        assert total == {"under": cap - 1, "over": cap + 1, "third": 5 * cap // 2}[which]
    return n, total


def _gauss(seed, n, f):
    return np.random.default_rng(seed).standard_normal((n, f), dtype=np.float32)


# ------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("f", [1, 37, 256])
@pytest.mark.parametrize("which", ["under", "over", "third"])
def test_dropout_is_the_restated_stream_at_every_trip_count(ctx, which, f):
    from gcnx import device as D
    n, total = _rows(ctx, which, f)
    x = _gauss(total, n, f)
    out = ctx.empty((n, f))
    D.dropout(ctx, ctx.to_device(x), 0.4, SEEDS[0], 3, None, out)
    assert _same(out.numpy(), R.dropout(x, 0.4, SEEDS[0], 3))


@pytest.mark.parametrize("rate", [0.0, 0.1, 0.4, 0.999])
def test_dropout_rates(ctx, rate):
    from gcnx import device as D
    n, _ = _rows(ctx, "over", 37)
    x = _gauss(11, n, 37)
    out = ctx.empty((n, 37))
    D.dropout(ctx, ctx.to_device(x), rate, SEEDS[1], 2, None, out)
    got = out.numpy()
    assert _same(got, R.dropout(x, rate, SEEDS[1], 2))
    if rate == 0.0:
        assert _same(got, x)                                      # everything kept, scale exactly 1


def test_dropout_seeds_and_streams(ctx):
    from gcnx import device as D
    n, _ = _rows(ctx, "over", 37)
    x = _gauss(12, n, 37)
    xd, out = ctx.to_device(x), ctx.empty((n, 37))
    masks = []
    for seed in SEEDS:
        for stream in STREAMS:
            D.dropout(ctx, xd, 0.4, seed, stream, None, out)
            got = out.numpy()
            assert _same(got, R.dropout(x, 0.4, seed, stream)), (seed, stream)
            masks.append(got != 0)
    for i in range(4):
        for j in range(i):                                        # independent streams agree on 0.6^2 + 0.4^2 of the elements
            assert abs((masks[i] == masks[j]).mean() - 0.52) <= 5 * np.sqrt(0.24 / x.size), (i, j)


def test_dropout_step_counter_on_the_device(ctx):
    """step = NULL is step 0; a device counter moved by gcnx_counter_add from 0 to 1 to 7 gives the streams of those steps."""
    from gcnx import device as D
    n, _ = _rows(ctx, "over", 37)
    x = _gauss(13, n, 37)
    xd, out = ctx.to_device(x), ctx.empty((n, 37))
    D.dropout(ctx, xd, 0.4, SEEDS[0], STREAMS[1], None, out)
    null = out.numpy()
    assert _same(null, R.dropout(x, 0.4, SEEDS[0], STREAMS[1], 0))
    step = ctx.zeros(1, np.int32)
    seen = {}
    for inc, now in ((0, 0), (1, 1), (6, 7)):
        if inc:
            D.counter_add(ctx, step, inc)
        assert int(step.numpy()[0]) == now
        D.dropout(ctx, xd, 0.4, SEEDS[0], STREAMS[1], step, out)
        seen[now] = out.numpy()
        assert _same(seen[now], R.dropout(x, 0.4, SEEDS[0], STREAMS[1], now)), now
    assert _same(seen[0], null)
    # a step is not a stream: (stream 5, step 1) against (stream 6, step 0) and (stream 4, step 2)
    for stream, st in ((STREAMS[1] + 1, 0), (STREAMS[1] - 1, 2)):
        other = R.dropout(x, 0.4, SEEDS[0], stream, st) != 0
        assert abs(((seen[1] != 0) == other).mean() - 0.52) <= 5 * np.sqrt(0.24 / x.size)


@pytest.mark.parametrize("f", [37, 256])
def test_dropout_strided_and_in_place(ctx, f):
    """x and out with different leading dimensions inside sentinel frames: the mask is that of the flat index r f + c."""
    from gcnx import device as D
    n, _ = _rows(ctx, "third", f)
    x = _gauss(14, n, f)
    want = R.dropout(x, 0.1, SEEDS[1], STREAMS[0], 7)
    step = ctx.to_device(np.array([7], np.int32))
    src = Frame(ctx, n, f, f + 3, 2, x)
    dst = Frame(ctx, n, f, f + 8, 4)
    D.dropout(ctx, src.view, 0.1, SEEDS[1], STREAMS[0], step, dst.view)
    dst.check(want, "out")
    src.check(x, "x is left alone")
    D.dropout(ctx, src.view, 0.1, SEEDS[1], STREAMS[0], step)     # in place: out == x
    src.check(want, "in place")


# ------------------------------------------------------------------------------------------- add
@pytest.mark.parametrize("f", [1, 37, 256])
@pytest.mark.parametrize("which", ["under", "over", "third"])
def test_add_at_every_trip_count(ctx, which, f):
    from gcnx import device as D
    n, total = _rows(ctx, which, f)
    a, b = _gauss(total + 1, n, f), _gauss(total + 2, n, f)
    out = ctx.empty((n, f))
    D.add(ctx, ctx.to_device(a), ctx.to_device(b), out)
    assert _same(out.numpy(), a + b)


def test_add_strided_and_in_place_into_either_operand(ctx):
    from gcnx import device as D
    f = 37
    n, _ = _rows(ctx, "third", f)
    a, b = _gauss(21, n, f), _gauss(22, n, f)
    fa, fb, fo = Frame(ctx, n, f, f + 1, 1, a), Frame(ctx, n, f, f + 5, 3, b), Frame(ctx, n, f, f + 2, 0)
    D.add(ctx, fa.view, fb.view, fo.view)
    fo.check(a + b, "out")
    fa.check(a, "a is left alone")
    fb.check(b, "b is left alone")
    D.add(ctx, fa.view, fb.view, fa.view)                         # out == a
    fa.check(a + b, "into a")
    D.add(ctx, fo.view, fb.view, fb.view)                         # out == b
    fb.check((a + b) + b, "into b")


# ------------------------------------------------------------------------------------------- sgd
def test_sgd_grid_stride_and_lr_source(ctx):
    """n = 2048 * 256 * 2 + 17: every thread of the capped grid takes two trips, seventeen take a third.  lr is a power of
    two: lr * g is exact, so p - lr * g is one rounding with or without a fused multiply-add."""
    from gcnx import device as D
    n = 2048 * 256 * 2 + 17
    assert -(-n // 256) > 2048 and 2 * 2048 * 256 < n <= 3 * 2048 * 256
    rng = np.random.default_rng(31)
    p0, g = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    lr = np.float32(2.0 ** -6)
    buf = np.full(n + 16, SENTINEL, np.float32)
    buf[8:8 + n] = p0
    pd, gd = ctx.to_device(buf), ctx.to_device(g)
    D.sgd(ctx, pd.flat(8, n), gd, float(lr))
    got = pd.numpy()
    want = p0 - lr * g
    assert _same(got[8:8 + n], want)
    assert (got[:8] == SENTINEL).all() and (got[8 + n:] == SENTINEL).all()
    lr2 = np.float32(2.0 ** -5)
    lrd = ctx.to_device(np.array([lr2], np.float32))              # has to outlive the launch
    ctx.set_lr_source(lrd)
    try:
        D.sgd(ctx, pd.flat(8, n), gd, 0.75)                       # the argument is ignored
        ctx.sync()
    finally:
        ctx.set_lr_source(None)
    got = pd.numpy()
    assert _same(got[8:8 + n], want - lr2 * g)
    assert (got[:8] == SENTINEL).all() and (got[8 + n:] == SENTINEL).all()

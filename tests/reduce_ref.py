"""Host references for csrc/reduce.hip and csrc/elementwise.hip, in NumPy alone (no GPU, no torch).

Segment pool and its backward in float32, written so that every output is rounded ONCE from exact operands: the sums are
taken in float64 (exact for the integer-valued test data, whatever the order) and rounded to float32, AVG divides that by
float32(cnt), the backward multiplies by float32(1) / float32(cnt).  On integer-valued inputs every launch route of the
kernels must give these bits.

The dropout stream of elementwise.hip restated in uint32 / uint64 arithmetic: element (r, c) of an [n, f] operand has the
FLAT index i = r f + c whatever the leading dimensions of x and out are, and is kept iff keep_bits(k0, k1, i) >= thresh."""
import numpy as np

F32 = np.float32
U32 = np.uint32


# ------------------------------------------------------------------------------------------- pool
def pool_fwd(x, graph_ptr, mode):
    """(pooled float32 [b, f], argmax int32 [b, f] or None).  An empty graph pools to 0; MAX reports the FIRST maximal row
    and -1 for an empty graph (it has no row: callers compare the rows of the non-empty graphs)."""
    x = np.asarray(x, F32)
    gp = np.asarray(graph_ptr, np.int64)
    b, f = len(gp) - 1, x.shape[1]
    out = np.zeros((b, f), F32)
    arg = np.full((b, f), -1, np.int32) if mode == "max" else None
    for g in range(b):
        lo, hi = int(gp[g]), int(gp[g + 1])
        if hi == lo:
            continue
        seg = x[lo:hi]
        if mode == "sum":
            out[g] = seg.sum(0, dtype=np.float64).astype(F32)
        elif mode == "avg":
            out[g] = seg.sum(0, dtype=np.float64).astype(F32) / F32(hi - lo)
        elif mode == "max":
            out[g] = seg.max(0)
            arg[g] = lo + seg.argmax(0)            # numpy's argmax: the first maximal row
        else:
            raise ValueError(mode)
    return out, arg


def graph_of_row(graph_ptr):
    cnt = np.diff(np.asarray(graph_ptr, np.int64))
    return np.repeat(np.arange(len(cnt)), cnt)


def pool_bwd(dp, graph_ptr, n, mode, arg=None, y=None):
    """dx float32 [n, f]: SUM dp[g], AVG dp[g] * (float32(1) / float32(cnt_g)), MAX dp[g] at the argmax row; zero where
    y <= 0 when y is given."""
    dp = np.asarray(dp, F32)
    gp = np.asarray(graph_ptr, np.int64)
    gid = graph_of_row(gp)
    assert len(gid) == n and gp[0] == 0
    if mode == "sum":
        dx = dp[gid]
    elif mode == "avg":
        sc = F32(1) / np.maximum(np.diff(gp), 1).astype(F32)          # float32 division: one rounding
        dx = dp[gid] * sc[gid][:, None]
    elif mode == "max":
        dx = np.where(np.asarray(arg)[gid] == np.arange(n)[:, None], dp[gid], F32(0))
    else:
        raise ValueError(mode)
    if y is not None:
        dx = np.where(np.asarray(y) > 0, dx, F32(0))
    return np.ascontiguousarray(dx, F32)


def pool_bwd_colsum(dp, graph_ptr, y, mode):
    """float32(sum_g float32(count_g * dp_g * sc_g)), count_g = positives of y per column inside graph g."""
    dp = np.asarray(dp, F32)
    gp = np.asarray(graph_ptr, np.int64)
    acc = np.zeros(dp.shape[1], np.float64)
    for g in range(len(gp) - 1):
        lo, hi = int(gp[g]), int(gp[g + 1])
        if hi == lo:
            continue
        sc = F32(1) / F32(hi - lo) if mode == "avg" else F32(1)
        cnt = (np.asarray(y)[lo:hi] > 0).sum(0).astype(np.float64)
        acc += (cnt * dp[g].astype(np.float64) * np.float64(sc)).astype(F32).astype(np.float64)
    return acc.astype(F32)


# ---------------------------------------------------------------------------------------- dropout
def mix32(h):
    """murmur3's finaliser on uint32 (wrapping)."""
    h = np.array(h, dtype=U32, ndmin=1)
    h ^= h >> U32(16)
    h *= U32(0x85EBCA6B)
    h ^= h >> U32(13)
    h *= U32(0xC2B2AE35)
    h ^= h >> U32(16)
    return h


def stream_keys(seed, stream_id, step=0):
    """(k0, k1) of the stream (seed, stream_id, step), each a uint32."""
    seed, stream_id, step = (np.array([int(v) & 0xFFFFFFFF], U32) for v in (seed, stream_id, step))
    k0 = mix32(seed * U32(0x9E3779B9) + stream_id)
    k1 = mix32(step * U32(0x85EBCA6B) + (seed ^ U32(0x27D4EB2F)))
    return k0[0], k1[0]


def keep_bits(k0, k1, idx):
    """uniform 32 bits of element idx (uint64) of the stream with keys (k0, k1)."""
    idx = np.asarray(idx, np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(U32)
    hi = (idx >> np.uint64(32)).astype(U32)
    return mix32(mix32(lo ^ U32(k0)) + ((hi * U32(0x9E3779B9)) ^ U32(k1)))


def dropout_thresh(rate):
    return min(int(float(F32(rate)) * 4294967296.0), 0xFFFFFFFF)


def dropout_scale(rate):
    return F32(1) / (F32(1) - F32(rate))


def dropout_keep(n, f, rate, seed, stream_id, step=0):
    """bool [n, f]: element (r, c) has the flat index r f + c."""
    k0, k1 = stream_keys(seed, stream_id, step)
    idx = np.arange(int(n) * int(f), dtype=np.uint64)
    return (keep_bits(k0, k1, idx) >= U32(dropout_thresh(rate))).reshape(int(n), int(f))


def dropout(x, rate, seed, stream_id, step=0):
    """out = keep ? x * scale : 0 in float32.  x: any 2-D array (a strided view included): only its SHAPE enters the mask."""
    x = np.asarray(x, F32)
    n, f = x.shape
    return np.where(dropout_keep(n, f, rate, seed, stream_id, step), x * dropout_scale(rate), F32(0)).astype(F32)

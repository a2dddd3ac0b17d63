"""Host references and the route model for csrc/bn.hip, in NumPy alone (no GPU, no torch).

References (float64): the column sums of gcnx_bn_stats, gcnx_bn_finalize in both modes with the moving-statistics update,
the two-pass gcnx_bn_moments, gcnx_bn_act and gcnx_bn_act_bwd (whole, or from given sums and a global count as the sync-BN
halves take them) for the four activations and both training modes.  Every column sum is returned as `s + 0.0`: a device
accumulator starts at +0, so a column whose terms are all -0 sums to +0 there.

route(kind, n, f, aligned, cus) restates the dispatch rules of bn.hip as they stand and names the code path a call takes.

exact_data(n, f, seed) makes inputs on which every product the kernels form and every partial column sum is exact in
fp32, whatever the order and with or without fused multiply-adds (assert_exact proves it for a given draw): z and dy are
integers in [-3, 3], mean and shift integers in [-1, 1], inv and |gamma| in {1/2, 1, 2}, beta an integer in [-2, 2], alpha
1/4 or 1/2.  Then z - mean is an integer, xhat a multiple of 1/2, zb = (z - mean) (gamma inv) + beta a multiple of 1/4,
dzb a multiple of 1/4 and dzb xhat a multiple of 1/8."""
import numpy as np

F32 = np.float32
EPS, MOMENTUM = 1e-3, 0.99           # Keras BatchNormalization defaults (gcnx.device.BN_EPS / BN_MOMENTUM)
ACTS = (None, "relu", "prelu", "prelu_shared")
KINDS = ("stats", "finalize", "moments", "bn_act", "bn_act_bwd", "bwd_stats", "bwd_apply")
K_ROWS = 256                         # kRows: rows per first-stage workgroup
COL_TILE, APPLY_TILE = 64, 256       # columns per workgroup: column sums / apply kernels


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- references
def stats(z, shift=None):
    """[2, f]: column sums of (z - shift) and of (z - shift)^2."""
    d = _f64(z) - (0.0 if shift is None else _f64(shift))
    return np.stack([d.sum(0) + 0.0, (d * d).sum(0) + 0.0])


def finalize(sums, count, shift=None, moving_mean=None, moving_var=None, momentum=MOMENTUM, eps=EPS):
    """(mean, inv, new moving_mean, new moving_var).  sums None: inference, mean / var are the moving statistics, which
    stay as they are."""
    mm, mv = _f64(moving_mean), _f64(moving_var)
    if sums is None:
        mean, var = mm, mv
    else:
        sums = _f64(sums)
        d = sums[0] / count
        mean = d + (0.0 if shift is None else _f64(shift))
        var = np.maximum(sums[1] / count - d * d, 0.0)                 # biased variance
        if mm is not None:
            mm = momentum * mm + (1 - momentum) * mean
            mv = momentum * mv + (1 - momentum) * var
    return mean, 1.0 / np.sqrt(var + eps), mm, mv


def moments(z, moving_mean=None, moving_var=None, momentum=MOMENTUM, eps=EPS):
    """gcnx_bn_moments: a pass for the mean, a second one centred on it; the moving statistics move once."""
    n = np.shape(z)[0]
    m1 = finalize(stats(z), n, eps=eps)[0]
    return finalize(stats(z, m1), n, m1, moving_mean, moving_var, momentum, eps)


def _alpha(act, alpha, f):
    if act == "prelu":
        return _f64(alpha).reshape(f)
    if act == "prelu_shared":
        return np.full(f, float(np.asarray(alpha).reshape(-1)[0]))
    return np.zeros(f)


def pre_activation(z, mean, inv, gamma, beta):
    """zb = (z - mean) (gamma inv) + beta: the activation's input, in the device's association."""
    return (_f64(z) - _f64(mean)) * (_f64(gamma) * _f64(inv)) + _f64(beta)


def device_sides(z, mean, inv, gamma, beta):
    """zb > 0 as the device decides it: the sign of the exact fma(fl32(z - mean), fl32(gamma inv), beta).  On Gaussian data
    a pre-activation within an fp32 rounding of zero may lie on the other side in float64; passing these sides to
    bn_act_bwd keeps the comparison one of arithmetic."""
    z, mean, inv, gamma, beta = (np.asarray(v, F32) for v in (z, mean, inv, gamma, beta))
    return (z - mean).astype(np.float64) * (gamma * inv).astype(np.float64) + beta.astype(np.float64) > 0


def bn_act(z, mean, inv, gamma, beta, act=None, alpha=None):
    zb = pre_activation(z, mean, inv, gamma, beta)
    if act is None:
        return zb
    if act == "relu":
        return np.maximum(zb, 0.0)
    return np.where(zb > 0, zb, _alpha(act, alpha, zb.shape[1]) * zb)


def bwd_terms(dy, z, mean, inv, gamma, beta, act=None, alpha=None, pos=None):
    """(dzb, xhat, dy min(zb, 0)) per element; the third is zero without a PReLU."""
    dy = _f64(dy)
    xhat = (_f64(z) - _f64(mean)) * _f64(inv)
    zb = pre_activation(z, mean, inv, gamma, beta)
    pos = zb > 0 if pos is None else np.asarray(pos, bool)
    if act is None:
        return dy, xhat, np.zeros_like(dy)
    if act == "relu":
        return np.where(pos, dy, 0.0), xhat, np.zeros_like(dy)
    return np.where(pos, dy, _alpha(act, alpha, dy.shape[1]) * dy), xhat, dy * np.where(pos, 0.0, zb)


def bn_act_bwd(dy, z, mean, inv, gamma, beta, act=None, alpha=None, training=True, sums=None, count=None, pos=None):
    """dict: dz, sums [3, f] (the local column sums: sum dzb, sum dzb xhat, sum dy min(zb, 0)), dbeta, dgamma, dalpha
    ([f], [1] for the shared slope, None without a PReLU).  `sums` / `count`: the reduced sums and the global row count dz
    is formed from (default: the local ones)."""
    dzb, xhat, da = bwd_terms(dy, z, mean, inv, gamma, beta, act, alpha, pos)
    local = np.stack([dzb.sum(0) + 0.0, (dzb * xhat).sum(0) + 0.0, da.sum(0) + 0.0])
    red = local if sums is None else _f64(sums)
    count = dzb.shape[0] if count is None else count
    scale = _f64(gamma) * _f64(inv)
    if training:
        dz = scale * (dzb - red[0] / count - xhat * (red[1] / count))
    else:
        dz = scale * dzb
    dalpha = {"prelu": local[2], "prelu_shared": np.array([local[2].sum() + 0.0])}.get(act)
    return {"dz": dz, "sums": local, "dbeta": local[0], "dgamma": local[1], "dalpha": dalpha}


# ------------------------------------------------------------------------------------------- routes
def _colsum_lanes(f, vec):
    """What the lanes of the 64-column tiles of a column-sum kernel do: "fast" (a full tile of aligned operands: plain float4
    loads, two rows in flight), in the generic instance "float4" (aligned, four or more columns left), "tail" (aligned, the
    last 1-3 columns: scalar loads next to float4 lanes) or "scalar" (operands not aligned)."""
    lanes = set()
    for t in range(_cdiv(f, COL_TILE)):
        if vec and t * COL_TILE + COL_TILE <= f:
            lanes.add("fast")
            continue
        for c in range(t * COL_TILE, min(f, t * COL_TILE + COL_TILE), 4):
            lanes.add("scalar" if not vec else ("float4" if f - c >= 4 else "tail"))
    return frozenset(lanes)


def _chunk_groups(nchunks):
    """The four-group chunk reduction: per = cdiv(nchunks, 4) chunks per group; (per, the groups that get no chunk, the
    group that min(nchunks, .) cuts short or None)."""
    per = _cdiv(nchunks, 4)
    empty = tuple(g for g in range(4) if g * per >= nchunks)
    short = [g for g in range(4) if g * per < nchunks < g * per + per]
    return per, empty, (short[0] if short else None)


def _apply(n, f, vec, cus):
    gy = min(_cdiv(n, 4), 8 * cus)
    step = 4 * gy
    full = f // APPLY_TILE if vec else 0                  # tiles that may take the two-row loop
    two_row = full > 0 and n > step
    loops, tail_from = "tail", 0
    if two_row:
        r = np.arange(min(step, n), dtype=np.int64)          # a thread's first row; it runs while r + step < n
        its = np.maximum(_cdiv(n - step - r, 2 * step), 0)
        left = r + its * 2 * step < n                        # a row left to the tail loop
        behind = bool((left & (its > 0)).any())              # ... behind at least one two-row iteration
        loops = "two_row+tail" if behind else "two_row"
        if not bool(left.any()):
            tail_from = full * APPLY_TILE                    # an exact fit: the full tiles never enter the tail loop
        if f % APPLY_TILE:
            loops += ",tail"                                 # the partial tile next to the full ones
    lanes = set()
    for c in range(tail_from, f, 4):
        lanes.add("scalar" if not vec else ("float4" if f - c >= 4 else "tail"))
    return {"step": step, "gy": gy, "loops": loops, "exact_fit": two_row and tail_from > 0, "lanes": frozenset(lanes)}


def route(kind, n, f, aligned, cus):
    """The code path of one call: kind in KINDS, [n, f] operands, aligned = every operand base is 16-byte aligned and every
    leading dimension a multiple of 4 (the kernels' `vec`), cus = the chip's CU count.  A dict:
      launch   "small" (one launch, nchunks == 1: gcnx_bn_moments, gcnx_bn_act_bwd), "chunked" (first stage + chunk
               reduction), "apply" (gcnx_bn_act, gcnx_bn_act_bwd_apply) or "elementwise" (gcnx_bn_finalize)
      lanes    of the column-sum stage (see _colsum_lanes), None without one
      nchunks, per, empty, short   of the chunk reduction (None in a small launch: it is folded into the kernel)
      apply    of the apply kernel: gy = min(cdiv(n, 4), 8 cus) workgroup rows and step = 4 gy rows per pass; loops: "tail" (no
               aligned full 256-column tile, or n <= step), "two_row" (the two-rows-in-flight loop on the full tiles; threads
               whose second row would lie past n take the tail loop instead), "two_row+tail" (some thread has a row left for
               the tail loop behind its two-row iterations), each + ",tail" for a partial tile next to the full ones; exact_fit:
               the two-row loop covers every row of the full tiles; lanes of the tail loop where it runs.  None where there is no
               apply kernel (a small launch writes dz itself)."""
    assert kind in KINDS and n >= 1 and f >= 1
    vec = bool(aligned)
    rec = {"kind": kind, "vec": vec, "launch": None, "lanes": None, "nchunks": None, "per": None, "empty": None, "short": None,
           "apply": None}
    if kind == "finalize":
        rec["launch"] = "elementwise"
        return rec
    nchunks = _cdiv(n, K_ROWS)
    if kind in ("stats", "moments", "bn_act_bwd", "bwd_stats"):
        rec["lanes"] = _colsum_lanes(f, vec)
        if nchunks == 1 and kind in ("moments", "bn_act_bwd"):
            rec["launch"] = "small"
            return rec
        rec["launch"] = "chunked"
        rec["nchunks"] = nchunks
        rec["per"], rec["empty"], rec["short"] = _chunk_groups(nchunks)
    if kind in ("bn_act", "bn_act_bwd", "bwd_apply"):
        rec["launch"] = rec["launch"] or "apply"
        rec["apply"] = _apply(n, f, vec, cus)
    return rec


# ------------------------------------------------------------------------------------------- exact data
def exact_data(n, f, seed):
    rng = np.random.default_rng(seed)
    ints = lambda lo, hi, *shape: rng.integers(lo, hi + 1, shape).astype(F32)
    pow2 = lambda *shape: np.exp2(rng.integers(-1, 2, shape)).astype(F32)
    d = {"z": ints(-3, 3, n, f), "dy": ints(-3, 3, n, f), "mean": ints(-1, 1, f), "shift": ints(-1, 1, f), "inv": pow2(f),
         "gamma": pow2(f) * rng.choice(np.array([-1, 1], F32), f), "beta": ints(-2, 2, f),
         "alpha": rng.choice(np.array([0.25, 0.5], F32), f)}
    d["alpha_shared"] = d["alpha"][:1].copy()
    return d


def alpha_of(d, act):
    return {"prelu": d["alpha"], "prelu_shared": d["alpha_shared"]}.get(act)


def is_f32(x):
    """Every element of the float64 array is a float32 number."""
    x = np.asarray(x, np.float64)
    return bool(np.array_equal(x, x.astype(F32).astype(np.float64)))


def assert_exact(d, act):
    """Every term a column-sum kernel adds on this data is a multiple of 1/8 and the magnitudes of a column's terms sum to
    less than 2^24 / 8: every partial sum, in any order, is an exact fp32 number.  The same for the column sums the shared
    slope's gradient adds."""
    z, sh = _f64(d["z"]), _f64(d["shift"])
    dzb, xhat, da = bwd_terms(d["dy"], z, d["mean"], d["inv"], d["gamma"], d["beta"], act, alpha_of(d, act))
    for name, t in (("z", z), ("z^2", z * z), ("z - shift", z - sh), ("(z - shift)^2", (z - sh) ** 2), ("dzb", dzb),
                    ("dzb xhat", dzb * xhat), ("dy min(zb, 0)", da)):
        assert np.array_equal(t * 8, np.rint(t * 8)), name
        assert np.abs(t).sum(0).max(initial=0.0) * 8 < 2 ** 24, name
    assert np.abs(da.sum(0)).sum() * 8 < 2 ** 24, "the shared slope's sum over the columns"

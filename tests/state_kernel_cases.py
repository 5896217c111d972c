"""Cases and plain restatements for the per-state kernels and the stream compaction (tests/test_gpu_state_kernels.py).

Host only, and nothing here is shared with the library: the restatements are written from the reference's text
(KinematicChain.h:118-130, ConstraintFunction.h:43-55) in plain Python, and tests/test_state_kernel_cases.py checks them
against the CPU oracle without a GPU."""
import math

import numpy as np

PI = math.pi
TWO_PI = 2.0 * math.pi
DBL_MAX = float(np.finfo(np.float64).max)


# ---- KinematicChainSpace::enforceBounds -----------------------------------------------------------------------------------
def wrap_pi_restated(x):
    """One value through KinematicChain.h:118-130: fmod(x, 2 pi), then the two branches.  A non-finite x gives NaN (C's fmod;
    Python's raises for an infinite x instead)."""
    x = float(x)
    if not math.isfinite(x):
        return float("nan")
    v = math.fmod(x, TWO_PI)
    if v < -PI:
        v += TWO_PI
    elif v >= PI:
        v -= TWO_PI
    return v


def wrap_restated(a):
    """wrap_pi_restated over an array of any shape"""
    a = np.asarray(a, dtype=np.float64)
    return np.array([wrap_pi_restated(v) for v in a.reshape(-1)], dtype=np.float64).reshape(a.shape)


def wrap_values():
    """(19, 14): 25 edge values, then 40 uniform draws in [-m, m] at each of six magnitudes m, padded to whole rows.  The
    first row holds edge values only, so a batch of one still meets them."""
    up, down = math.inf, -math.inf
    edge = [0.0, -0.0, PI, -PI,
            np.nextafter(PI, up), np.nextafter(PI, down), np.nextafter(-PI, up), np.nextafter(-PI, down),
            TWO_PI, np.nextafter(TWO_PI, up), np.nextafter(TWO_PI, down),
            -TWO_PI, np.nextafter(-TWO_PI, up), np.nextafter(-TWO_PI, down),
            3.0 * PI, -3.0 * PI, 5e-324, -5e-324, 1e-310, 1e300, -1e300, DBL_MAX, math.inf, -math.inf, math.nan]
    rng = np.random.RandomState(0x57A7E)
    draws = [m * rng.uniform(-1.0, 1.0, 40) for m in (1.0, 10.0, 1e3, 1e8, 1e16, 1e100)]
    v = np.concatenate([np.array(edge, dtype=np.float64)] + draws)
    pad = (-len(v)) % 14
    v = np.concatenate([v, np.full(pad, 0.5)])
    return v.reshape(-1, 14).copy()


# ---- KinematicChainConstraint::jointValid ---------------------------------------------------------------------------------
LIMIT_KINDS = ("lb+eps", "ub-eps", "lb+eps up", "lb+eps down", "ub-eps up", "ub-eps down", "nan", "+inf", "-inf", "lb")


def limit_rows(P):
    """(140, 14): the mid-range state with ONE coordinate replaced, row 10 * e + k = coordinate e, LIMIT_KINDS[k].  The two
    limits with the margin are each the single double operation the library stores (lb + eps, ub - eps)."""
    lb, ub, eps = np.array(P.lb[:]), np.array(P.ub[:]), float(P.joint_eps)
    base = np.concatenate([(lb + ub) / 2.0] * 2)
    rows = []
    for e in range(14):
        lo, hi = lb[e % 7] + eps, ub[e % 7] - eps
        for v in (lo, hi, np.nextafter(lo, math.inf), np.nextafter(lo, -math.inf), np.nextafter(hi, math.inf), np.nextafter(hi, -math.inf),
                  math.nan, math.inf, -math.inf, lb[e % 7]):
            r = base.copy()
            r[e] = v
            rows.append(r)
    return np.array(rows)


def joint_valid_restated(P, x):
    """ConstraintFunction.h:43-55 for the rows of x, (B, 14) or (14,): uint8 (B,).  Both comparisons are strict and false for a
    NaN, which therefore passes."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 14)
    lb, ub, eps = [float(v) for v in P.lb[:]], [float(v) for v in P.ub[:]], float(P.joint_eps)
    out = np.ones(x.shape[0], dtype=np.uint8)
    for b in range(x.shape[0]):
        q = [float(v) for v in x[b]]
        for arm in range(2):
            for i in range(7):
                if q[arm * 7 + i] < lb[i] + eps or q[arm * 7 + i] > ub[i] - eps:
                    out[b] = 0
    return out


def fit_rows(rows, B):
    """the batch cut or tiled to B rows"""
    rows = np.asarray(rows)
    reps = -(-B // rows.shape[0])
    return np.ascontiguousarray(np.concatenate([rows] * reps)[:B])


# ---- stream compaction ------------------------------------------------------------------------------------------------------
def compact_restated(q, ok, cap):
    """(the rows of q whose flag is not zero, in order, cut to cap; how many there were before the cut)"""
    q, ok = np.asarray(q), np.asarray(ok)
    keep = ok != 0
    return q[keep][:cap], int(keep.sum())


def index_rows(B):
    """(B, 14): row i holds i in all 14 entries, exact in a double — a misplaced row names itself"""
    return np.ascontiguousarray(np.repeat(np.arange(B, dtype=np.float64)[:, None], 14, axis=1))


FLAG_PATTERNS = ("none", "all", "first", "last", "mod64_63", "mod256_0", "p0.01", "p0.5", "p0.99", "bytes")


def flags(B, pattern):
    """(B,) uint8 flag bytes of one named pattern; the random ones are seeded by (B, pattern)"""
    ok = np.zeros(B, dtype=np.uint8)
    idx = np.arange(B)
    rng = np.random.RandomState((0xF1A6 + 31 * B + FLAG_PATTERNS.index(pattern)) & 0x7FFFFFFF)
    if pattern == "none":
        pass
    elif pattern == "all":
        ok[:] = 1
    elif pattern == "first":  # the sparse patterns say "valid" with bytes other than 1: the contract is ok != 0
        ok[0] = 2
    elif pattern == "last":
        ok[B - 1] = 255
    elif pattern == "mod64_63":
        ok[idx % 64 == 63] = 128
    elif pattern == "mod256_0":
        ok[idx % 256 == 0] = 1
    elif pattern.startswith("p"):
        ok[rng.uniform(size=B) < float(pattern[1:])] = 1
    elif pattern == "bytes":  # the contract is ok != 0: the extend step's ok == 2 and any other byte count as valid
        ok = np.where(rng.uniform(size=B) < 0.5, rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=B), 0).astype(np.uint8)
    else:
        raise ValueError(pattern)
    return ok


# ---- bit comparisons --------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """elementwise: the same 64 bits, or both NaN (IEEE 754 leaves the sign and payload of a produced NaN open)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))

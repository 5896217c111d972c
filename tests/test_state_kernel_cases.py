"""The expected values of tests/test_gpu_state_kernels.py, proven without a GPU: the plain restatements of
tests/state_kernel_cases.py against the CPU oracle, and the case builders against what they promise."""
import math

import numpy as np
import pytest

import state_kernel_cases as sk
from conftest import OBJECTS, load_cfg


def test_wrap_restated_is_the_oracle_bit_for_bit(oracle_det):
    v = sk.wrap_values()
    assert v.shape == (19, 14) and np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
    want = np.array([oracle_det.enforce_bounds(r) for r in v])
    got = sk.wrap_restated(v)
    assert sk.same_bits(got, want).all(), v[~sk.same_bits(got, want)]
    # a non-finite input gives NaN and nothing else does
    assert np.array_equal(np.isnan(want), ~np.isfinite(v))
    fin = np.isfinite(want)
    assert (want[fin] >= -math.pi).all() and (want[fin] < math.pi).all()
    # the three that a reader gets wrong: +pi wraps to -pi, -pi stays, the sign of a zero survives
    bits = lambda x: np.float64(x).view(np.uint64)
    for x, y in ((math.pi, -math.pi), (-math.pi, -math.pi), (-0.0, -0.0), (0.0, 0.0), (np.nextafter(math.pi, 0), np.nextafter(math.pi, 0)),
                 (5e-324, 5e-324), (-5e-324, -5e-324)):
        row = np.full(14, x)
        assert bits(oracle_det.enforce_bounds(row)[3]) == bits(y) == bits(sk.wrap_pi_restated(x)), x
    # the first row alone (a batch of one) holds edge values only
    assert set(np.abs(v[0])) <= {0.0, math.pi, 2 * math.pi} | {float(np.nextafter(s * math.pi, d)) for s in (1, 2) for d in (0, 9)}


@pytest.mark.parametrize("obj", OBJECTS)
def test_joint_valid_restated_is_the_oracle_on_the_limit_rows(oracle_det, obj):
    P = oracle_det.problem(load_cfg(obj))
    rows = sk.limit_rows(P)
    assert rows.shape == (140, 14)
    want = np.array([oracle_det.joint_valid(P, r) for r in rows], dtype=np.uint8)
    assert np.array_equal(sk.joint_valid_restated(P, rows), want)
    # per coordinate: on either limit and one step inside it is accepted, a NaN passes; one step outside, +-inf and the bare bound are refused
    kinds = dict(zip(sk.LIMIT_KINDS, range(10)))
    accepted = {kinds[k] for k in ("lb+eps", "ub-eps", "lb+eps up", "ub-eps down", "nan")}
    for e in range(14):
        for k in range(10):
            assert want[10 * e + k] == (k in accepted), (e, sk.LIMIT_KINDS[k])
        assert 0 < want[10 * e: 10 * e + 10].sum() < 10
    # the mid-range state itself is valid, and every row differs from it in exactly one coordinate
    base = np.concatenate([(np.array(P.lb[:]) + np.array(P.ub[:])) / 2.0] * 2)
    assert oracle_det.joint_valid(P, base)
    assert ((rows != base).sum(axis=1) == 1).all() and all((rows[10 * e: 10 * e + 10, e] != base[e]).all() for e in range(14))
    # the margin is the library's single operation
    assert rows[0, 0] == P.lb[0] + P.joint_eps and rows[1, 0] == P.ub[0] - P.joint_eps


def test_compact_restated_and_flag_patterns():
    q = sk.index_rows(6)
    ok = np.array([0, 2, 0, 255, 1, 0], dtype=np.uint8)
    rows, n = sk.compact_restated(q, ok, 6)
    assert n == 3 and rows[:, 0].tolist() == [1.0, 3.0, 4.0] and (rows == rows[:, :1]).all()
    rows, n = sk.compact_restated(q, ok, 2)
    assert n == 3 and rows[:, 0].tolist() == [1.0, 3.0]
    rows, n = sk.compact_restated(q, np.zeros(6, dtype=np.uint8), 6)
    assert n == 0 and rows.shape == (0, 14)
    for B in (1, 63, 65, 257, 1023):
        pats = {p: sk.flags(B, p) for p in sk.FLAG_PATTERNS}
        assert all(f.shape == (B,) and f.dtype == np.uint8 for f in pats.values())
        assert pats["none"].sum() == 0 and (pats["all"] == 1).all()
        assert np.flatnonzero(pats["first"]).tolist() == [0] and np.flatnonzero(pats["last"]).tolist() == [B - 1]
        assert np.flatnonzero(pats["mod64_63"]).tolist() == list(range(63, B, 64))
        assert np.flatnonzero(pats["mod256_0"]).tolist() == list(range(0, B, 256))
        assert set(pats["bytes"]) <= {0, 1, 2, 128, 255}
        assert np.array_equal(sk.flags(B, "p0.5"), pats["p0.5"])  # seeded
    by = sk.flags(1023, "bytes")
    assert set(by) == {0, 1, 2, 128, 255} and 400 < (by != 0).sum() < 620
    assert 0 < sk.flags(1023, "p0.01").sum() < 40 and 980 < sk.flags(1023, "p0.99").sum() < 1023
    assert np.array_equal(sk.fit_rows(q, 4), q[:4]) and np.array_equal(sk.fit_rows(q, 13)[6:], np.concatenate([q, q[:1]]))

"""The throughput layout's minimum-norm solve, spread over a group's six lanes (ccmp_fd_newton_phase2.inc), checked on the host.  tests/cpp/group_solve_check.cpp composes the pieces of ccmp_solve.h as the kernels do —
six virtual lanes on one group record: lane r owns columns r, r + 6, r + 12, one serial sum per lane read from the record, the
sums published in the record, the scalar part in every lane, rotated columns written back in place — and runs the one-lane
solve_minnorm beside it, compiled with the det oracle's flags.  All 14 entries of both must be the bits of the oracle's
orc_solve_minnorm, and the iterate updated by the six lanes the bits of the one-lane update, on

  * Jacobians and residuals recorded from real Newton rounds (the oracle's own iteration on ambient samples, three objects);
  * random Jacobians over many magnitudes;
  * b == 0 exactly in the first sweep (orthogonal rows) and in the second (equal rows of powers of two: the first rotation
    leaves a row of exact zeros);
  * nearly parallel rows, a row of zeros (singular value under the threshold: coefficient 0), zero Jacobians, huge and tiny ones;
  * NaN and infinity in the Jacobian or the residual (a NaN must be a NaN in the same entries; which NaN is the compiler's choice
    of operand order, not the algorithm's).
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import OBJECTS, config_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group_solve") / "group_solve_check")
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read().split() else []
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCCMP_USE_FMA"] + fma + ["-Wall", "-I", CSRC,
           os.path.join(ROOT, "tests", "cpp", "group_solve_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cases(checker, oracle, tmp_path, cases):
    """cases (n, 30): J row 0, J row 1, f.  Returns (dx one lane, dx six lanes, oracle's dx, b == 0 flags per sweep)."""
    cases = np.ascontiguousarray(cases, dtype=np.float64)
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases.tofile(fin)
    r = subprocess.run([checker, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    n = json.loads(r.stdout.strip().splitlines()[-1])
    assert n["cases"] == len(cases) and n["update_differ"] == 0, n
    out = np.fromfile(fout).reshape(-1, 30)
    ref = np.stack([oracle.solve_minnorm(c[:28], c[28:]) for c in cases])
    return out[:, :14], out[:, 14:28], ref, out[:, 28:]


def assert_same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    both_nan = np.isnan(a) & np.isnan(b)
    differ = (a.view(np.uint64) != b.view(np.uint64)) & ~both_nan
    assert not differ.any(), "%s: %d of %d entries differ, first in case %d" % (what, differ.sum(), differ.size, np.argwhere(differ)[0][0])


def check(checker, oracle, tmp_path, cases):
    one, six, ref, bzero = run_cases(checker, oracle, tmp_path, cases)
    assert_same_bits(one, ref, "solve_minnorm against the oracle")
    assert_same_bits(six, ref, "six lanes against the oracle")
    assert_same_bits(six, one, "six lanes against solve_minnorm")
    return ref, bzero


@pytest.mark.parametrize("obj", OBJECTS)
def test_jacobians_of_real_rounds(checker, oracle_det, tmp_path, obj):
    O = oracle_det
    P = O.checker_problem(config_path(obj))
    cases = []
    for i in range(24):  # the reference's iteration, recorded round by round
        x = O.ambient_uniform(P, 0x6501, i)
        for _ in range(40):
            f = O.function(P, x)
            if not (f[0] > P.tol_pos or f[1] > P.tol_rot):
                break
            J = O.jacobian(P, x)
            cases.append(np.concatenate([J.reshape(28), f]))
            x = x - P.step * O.solve_minnorm(J, f)
    assert len(cases) > 400
    ref, bzero = check(checker, O, tmp_path, np.array(cases))
    assert np.isfinite(ref).all() and (np.abs(ref).max(axis=1) > 0).all() and not bzero.any()


def test_random_jacobians(checker, oracle_det, tmp_path):
    rng = np.random.default_rng(0x6502)
    n = 20000
    J = rng.standard_normal((n, 28)) * 10.0 ** rng.integers(-12, 13, size=(n, 1))
    J[n // 2:, 14:] *= 10.0 ** rng.integers(-8, 9, size=(n - n // 2, 1))  # rows of very different length
    J[::7] = np.where(rng.random((len(J[::7]), 28)) < 0.5, 0.0, J[::7])   # sparse ones
    f = rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-6, 3, size=(n, 1))
    ref, _ = check(checker, oracle_det, tmp_path, np.hstack([J, f]))
    assert np.isfinite(ref).all()


def test_exact_zero_products_parallel_rows_and_zero_rows(checker, oracle_det, tmp_path):
    rng = np.random.default_rng(0x6503)
    cases = []

    def add(r0, r1, f=(0.3, -0.2)):
        cases.append(np.concatenate([r0, r1, f]))

    first, second = [], []
    for k in range(200):
        # orthogonal rows on disjoint columns: b == 0 exactly in the first sweep (and in the second)
        r0, r1 = rng.standard_normal(14), rng.standard_normal(14)
        mask = rng.random(14) < 0.5
        first.append(len(cases))
        add(np.where(mask, r0, 0.0), np.where(mask, 0.0, r1))
        # equal rows of signed powers of two: zeta == 0, t == 1, c == s and every product with an entry exact, so the first
        # rotation leaves row 0 exactly zero — b == 0 in the second sweep, a singular value of zero under the threshold
        second.append(len(cases))
        p2 = np.ldexp(np.where(rng.random(14) < 0.5, 1.0, -1.0), rng.integers(-20, 21, size=14)) * (rng.random(14) < 0.8)
        p2[k % 14] = 1.0
        add(p2, p2.copy(), rng.standard_normal(2))
        # nearly parallel rows
        add(r0, r0 * (1.0 + 2.0 ** -rng.integers(20, 53)) + rng.standard_normal(14) * 10.0 ** -rng.integers(6, 17))
        add(r0, -3.0 * r0 + rng.standard_normal(14) * 1e-15)
        # a row of zeros; the zero Jacobian
        add(r0, np.zeros(14))
        add(np.zeros(14), r1)
        add(np.zeros(14), np.zeros(14))
        # the ends of the range: sums that overflow or vanish
        add(r0 * 1e160, r1 * 1e-170)
        add(r0 * 1e-170, r1 * 1e-165)
        add(r0 * 5e-324 * 1e10, r1)
    cases = np.array(cases)
    ref, bzero = check(checker, oracle_det, tmp_path, cases)
    assert bzero[first, 0].all(), "orthogonal rows did not give b == 0 in the first sweep"
    assert (bzero[second, 0] == 0).all() and bzero[second, 1].all(), "equal rows did not give b == 0 in the second sweep"
    # a row of zeros counts with coefficient 0: the step is the other row's alone, and finite
    zero_row = [i for i in range(len(cases)) if i % 10 == 4]
    assert np.isfinite(ref[zero_row]).all() and (np.abs(ref[zero_row]).max(axis=1) > 0).all()
    assert (ref[[i for i in range(len(cases)) if i % 10 == 6]] == 0).all()  # the zero Jacobian: no step


def test_nan_and_infinity(checker, oracle_det, tmp_path):
    rng = np.random.default_rng(0x6504)
    cases = []
    for k in range(300):
        c = np.concatenate([rng.standard_normal(28), rng.standard_normal(2)])
        where = rng.integers(0, 30, size=1 + k % 3)
        c[where] = [np.nan, np.inf, -np.inf][k % 3] if k % 4 else np.nan
        cases.append(c)
    ref, _ = check(checker, oracle_det, tmp_path, np.array(cases))
    assert (~np.isfinite(ref)).any(axis=1).all()  # none of these has a finite step

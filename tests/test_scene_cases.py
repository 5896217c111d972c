"""The scenes of tests/scene_cases.py and the checker they are compared with, on the CPU: the restated pair rule against
orc_clearance's own count and reported pairs at every shape; orc_clearance against an exact (60-digit) evaluation of the same
operation; and the domain of the tile kernel's squared-distance prune (ccmp_kernels_scene.hip: consider_pair)."""
import numpy as np
import pytest

import scene_cases as SC
from conftest import NCPU, load_cfg

ALL = sorted(SC.CASES) + ["twin:" + t for t in SC.TWINS]


@pytest.fixture(scope="module")
def problem(oracle_det):
    return oracle_det.problem(load_cfg("stefan"))


def _states(oracle, P, n, seed):
    """half ambient samples, half their projections (tests/test_gpu_scene.py)"""
    q = oracle.ambient_uniform_batch(P, seed, 0, n)
    proj, _, _ = oracle.project_batch(P, q[: n // 2], NCPU)
    return np.concatenate([q[n // 2:], proj])


def test_table_holds_every_shape_the_kernels_distinguish():
    got = {(SC.CASES[n]["n_ss"], SC.CASES[n]["n_sb"]) for n in SC.CASES}
    assert set(SC.SHAPES) <= got
    totals = {a + b for a, b in got}
    assert {1, 2, 3, 4, 5, 15, 16, 17, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2432} <= totals
    assert {a % 4 for a, _ in SC.TAILS} == {0, 1, 2, 3}
    assert {len(SC.scene(n)[0]) for n in ("ns15", "ns16", "ns17", "ns64")} == {15, 16, 17, 64}
    sph = SC.scene("statics9")[0]
    assert sum(1 for s in sph if s[0] == SC.FRAME_WORLD) == 5 and sum(1 for s in sph if s[0] in (8, 17)) == 4
    sph, boxes, _ = SC.scene("1920+512")
    assert len(sph) == 64 and len(boxes) == 8 and all(sum(1 for s in sph if s[0] == f) == 4 for f in SC.MOVING)
    for n in SC.CASES:
        assert any(s[3] == 0.0 for s in SC.scene(n)[0]) or len(SC.scene(n)[0]) < 4


@pytest.mark.parametrize("name", ALL)
def test_restated_pair_rule_against_the_oracle(oracle_det, problem, name):
    sph, boxes, allowed = SC.scene(name)
    codes = SC.pair_codes(sph, boxes, allowed)
    q = _states(oracle_det, problem, 32, 0x5CE5)
    assert oracle_det.clearance(problem, sph, boxes, allowed, q[0])[2] == len(codes)
    _, pair = oracle_det.clearance_batch(problem, sph, boxes, allowed, q)
    assert set(pair.tolist()) <= set(codes)
    if len(sph) <= 17:  # pair by pair: the oracle tests a two-proxy scene exactly when the restatement lists the pair
        listed = set(codes)
        for i in range(len(sph)):
            for j in range(i + 1, len(sph)):
                n = oracle_det.clearance(problem, [sph[i], sph[j]], [], allowed, q[0])[2]
                assert n == int((i | (j << 8)) in listed), (i, j)
            for b in range(len(boxes)):
                n = oracle_det.clearance(problem, [sph[i]], [boxes[b]], allowed, q[0])[2]
                assert n == int((i | ((64 + b) << 8)) in listed), (i, b)


def test_twins_list_the_copies_of_every_pair():
    for t in SC.TWINS:
        base = SC.scene(t)
        sph, boxes, allowed = SC.scene("twin:" + t)
        n, nb = len(base[0]), len(base[1])
        assert sph == (base[0] * 2)[:64] and len(sph) > n and len(boxes) == min(2 * nb, 8)
        ss, sb = (set(v) for v in SC.tested_pairs(sph, boxes, allowed))
        bss, bsb = SC.tested_pairs(*base)
        for i, j in bss:
            assert (i, j) in ss and (j + n >= len(sph) or (i, j + n) in ss) and (i + n >= len(sph) or (j, i + n) in ss)
        for i, b in bsb:
            assert (i, b) in sb and (b + nb >= len(boxes) or (i, b + nb) in sb) and (i + n >= len(sph) or (i + n, b) in sb)


@pytest.mark.parametrize("name", SC.LAST_WINS)
def test_last_wins_keeps_the_table_and_makes_its_last_pair_the_minimum(oracle_det, problem, name):
    base, sc = SC.scene(name), SC.scene("last:" + name)
    codes = SC.pair_codes(*sc)
    assert codes == SC.pair_codes(*base)
    q = _states(oracle_det, problem, 130, 0x5CE3)  # the states of tests/test_gpu_scene_shapes.py
    _, pair = oracle_det.clearance_batch(problem, *sc, q)
    assert (pair == codes[-1]).mean() >= 0.9, (pair == codes[-1]).mean()


# ---- the oracle against an exact evaluation of the same operation -------------------------------------------------------------
MEASURED_ULPS = 1.20  # the largest |orc_clearance - exact| over the cases below, in ulp(M) (see the test's docstring)
ORACLE_ULPS = 2.0 * MEASURED_ULPS  # what is asserted


def _exact_clearances(mp, P, sph, boxes, allowed, x):
    """the clearance of every tested pair of the list, in mpmath: PandaModel's chain (orc_fk's order of frames), the centres
    t_wb (o + R c) and both distance formulas — the oracle's operations on its own inputs (doubles), without its roundings"""
    mpf = mp.mpf
    A = lambda name, shape: np.ctypeslib.as_array(getattr(P, name)).reshape(shape)
    axis, off, ee, Rt, bR, bp = A("axis", (2, 7, 3)), A("offset", (2, 7, 3)), A("ee", (2, 3)), A("R_tool", (2, 3, 3)), A("base_R", (2, 3, 3)), A("base_p", (2, 3))
    M = lambda a: mp.matrix([[mpf(float(v)) for v in row] for row in np.atleast_2d(a)])
    V = lambda a: mp.matrix([mpf(float(v)) for v in a])
    frames = []
    for arm in range(2):
        R, o, fr = mp.eye(3), mp.zeros(3, 1), []
        for i in range(7):
            a = [mpf(float(v)) for v in axis[arm, i]]
            s, c = mp.sin(mpf(float(x[arm * 7 + i]))), mp.cos(mpf(float(x[arm * 7 + i])))
            t = 1 - c
            Rj = mp.matrix([[a[0] * a[0] * t + c, a[0] * a[1] * t - a[2] * s, a[0] * a[2] * t + a[1] * s],
                            [a[1] * a[0] * t + a[2] * s, a[1] * a[1] * t + c, a[1] * a[2] * t - a[0] * s],
                            [a[2] * a[0] * t - a[1] * s, a[2] * a[1] * t + a[0] * s, a[2] * a[2] * t + c]])
            o = o + R * V(off[arm, i])
            R = R * Rj
            fr.append((R, o))
        fr.append((R * M(Rt[arm]), o + R * V(ee[arm])))
        frames.append(fr)
    cen = []
    for f, _, c, _ in sph:
        if f < 0:
            cen.append(V(c))
            continue
        arm, k = divmod(f, 9)
        v = V(c) if k == 8 else frames[arm][k][1] + frames[arm][k][0] * V(c)
        cen.append(V(bp[arm]) + M(bR[arm]) * v)
    ss, sb = SC.tested_pairs(sph, boxes, allowed)
    out = []
    for i, j in ss:
        d = cen[i] - cen[j]
        out.append(mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) - (mpf(sph[i][3]) + mpf(sph[j][3])))
    for i, b in sb:
        loc = M(boxes[b][2]).T * (cen[i] - V(boxes[b][1]))
        e = [max(abs(loc[k]) - mpf(float(boxes[b][3][k])), mpf(0)) for k in range(3)]
        out.append(mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2) - mpf(sph[i][3]))
    return out, max(abs(float(v)) for c in cen for v in c)


def test_oracle_against_exact_arithmetic(oracle_det, problem):
    """orc_clearance (FP64, the canonical rounding model) against the same operation at 60 digits, 64 states per case.  Measured on
    the cases below: the largest |oracle - exact| is 1.20 ulp(M), M the largest centre coordinate of the case (1.2 .. 2.3 m, so
    ulp(M) = 2.2e-16 or 4.4e-16; the 1.20 is the 4+0 shape's, 2.7e-16 m); asserted: twice that, 2.40 ulp(M).  The oracle's pair is the lowest-numbered one whose exact clearance lies within that tolerance of the
    exact minimum."""
    import mpmath as mp

    mp.mp.dps = 60
    worst = 0.0
    for name in ["%d+%d" % s for s in SC.TINY] + ["19+3", "256+44", "statics9"]:
        sph, boxes, allowed = SC.scene(name)
        codes = SC.pair_codes(sph, boxes, allowed)
        q = _states(oracle_det, problem, 64, 0x5CE6 + len(codes))
        clr, pair = oracle_det.clearance_batch(problem, sph, boxes, allowed, q)
        exact = [_exact_clearances(mp, problem, sph, boxes, allowed, x) for x in q]
        ulp = float(np.spacing(max(m for _, m in exact)))
        tol = ORACLE_ULPS * ulp
        dev = 0.0
        for n, (vals, _) in enumerate(exact):
            lo = min(vals)
            dev = max(dev, abs(float(mp.mpf(float(clr[n])) - lo)) / ulp)
            first = next(k for k, v in enumerate(vals) if v <= lo + tol)
            assert pair[n] == codes[first], (name, n)
        print("%s: %d pairs, |oracle - exact| <= %.2f ulp(M), M = %.3f" % (name, len(codes), dev, max(m for _, m in exact)))
        worst = max(worst, dev)
    print("largest deviation: %.2f ulp(M)" % worst)
    assert worst <= ORACLE_ULPS


# ---- the prune's domain -------------------------------------------------------------------------------------------------
def test_prune_never_drops_a_minimum_below_2_22():
    """t = (best + rsum) + 1e-9, skipped iff t <= 0 or d2 > t t, against the plain rule sqrt(d2) - rsum < best on adversarial triples
    (S in {t, pred(t)}, d2 every double whose square root rounds to S): nothing is dropped while best + rsum < 2^22"""
    tried = 0
    for k, scale in enumerate([1e-3, 1.0, 3.7, 2.0 ** 10, 2.0 ** 20, 2.0 ** 21, 0.999 * 2.0 ** 22]):
        n, bad = SC.dropped_minima(scale, 4000, 0x5CE7 + k)
        assert not bad, (scale, bad[0])
        tried += n
    assert tried > 50000


def test_prune_drops_minima_at_2_25():
    """the threshold the host's guard is built on: at 2^25 the rounding of best + rsum alone (3.7e-9) swallows the nanometre"""
    n, bad = SC.dropped_minima(2.0 ** 25, 4000, 0x5CE8)
    assert len(bad) >= 1
    best, rsum, d2 = bad[0]
    assert SC.prune_skips(best, rsum, d2) and SC.becomes_minimum(best, rsum, d2)
    print("2^25: %d of %d candidates dropped; the first by %.3g" % (len(bad), n, best - (np.sqrt(d2) - rsum)))


def test_trigger_scene_and_its_bound(oracle_det, problem):
    """the huge-sphere scene: the oracle makes pair 4 the minimum, the restated predicate skips it behind pair 0's `best`; the host's
    bound puts it beyond 2^22 and the scene at 1.3e6 m within"""
    x0 = SC.fixed_state(oracle_det, problem)
    for dist in (2.0 ** 25, 2.0 ** 27):
        sph, facts = SC.huge_pair_scene(oracle_det, problem, x0, dist, True)
        assert SC.prune_skips(facts["best"], facts["rsum"], facts["d2"]) and facts["clearance"] < facts["best"]
        assert SC.prune_bound(problem, sph, [], None) >= SC.PRUNE_LIMIT
        print({k: (float(v) if isinstance(v, float) else v) for k, v in facts.items()})
    sph, facts = SC.huge_pair_scene(oracle_det, problem, x0, 1.3e6, False)
    assert 0.9 * SC.PRUNE_LIMIT < SC.prune_bound(problem, sph, [], None) < SC.PRUNE_LIMIT
    for name, (s, b, a) in SC.prune_cases(oracle_det, problem, x0).items():
        assert SC.prune_bound(problem, s, b, a) < 100.0, name
    for name in SC.CASES:
        s, b, a = SC.scene(name)
        assert SC.prune_bound(problem, s, b, a) < 100.0, name

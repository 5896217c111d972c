"""Scenes, restatements and inputs shared by the vetted-IK tests (tests/test_ik_vet_ref.py, tests/test_gpu_ik_vet.py,
tests/test_gpu_grow_vetted.py).  Host only.

  * `moving_arm`, `sub_scene`, `arm_pairs`, `cross_scenes`: the partition of a scene's tested pairs (csrc/ccmp_ik_vet.h) restated on the
    caller's arrays.  Arm a's sub-scene is the caller's spheres minus those moving on the other arm.  The cross pairs come as one
    sub-scene per sphere i that moves on arm 0: sphere i (group 0) and the arm-1 spheres it is tested against (group 1, allowed against
    itself) — everything allowed but sphere i's cross pairs.  (One sub-scene for all of them would need a group per (arm, group) pair:
    up to 48, and a scene has 32.)  The clearance of a scene without tested pairs is +inf, so the minimum over them is the cross term.
  * `counted_scene(n, arm)`: spheres on every frame kind — a body and the hand of `arm`, its own base, the other base, the world — a
    box, and a body and the hand of the other arm, with EXACTLY n tested pairs in `arm`'s set; `ARM_SCENES`: the table by those counts
    (0, 1, 15, 16, 17: the sixteen-lane row's stride) plus the largest scenes tests/scene_cases.py offers.
  * `select_vetted`: the vetted selection in plain Python over the candidates' records, as pose_ik_cases.select is for the plain rule.
  * `plain_run` / `branch_scenes`: the 40-target inputs of tests/test_pose_ik_host.py through the plain rule, and scenes built FROM ITS
    RECORDS so that each branch of the vetted rule is taken by some target:
      (a) a world sphere on the elbow origin (frame k of the arm, k in 2..5) of a converged seeded candidate and a sphere on that frame:
          radii a quarter each of the elbow's displacement to the arm's farthest converged restart, so the seeded candidate overlaps by
          half that displacement and the farthest restart clears by as much;
      (b) one sphere on each arm's k = 3 frame and nothing else (both arm sets empty, the one pair is a cross pair): radii summing to the
          mean of the elbow-to-elbow distances of the first two slots that assemble, the first one's being the smaller;
      (c) the scene of (b) with radii of 10 m: no assembled state clears;
    the margin is 0 on all of them.  Wine_Bottle's set with rng_seed 0x1CE (tests/test_pose_ik_host.py's) contains (a) and (b); so does
    dumbbell's."""
import functools
from fractions import Fraction

import numpy as np

import scene_cases
from arm_model_cases import HostScene, default_scene_host, host_constraint
from pose_ik_cases import sampled_case

RNG_SEED = 0x1CE  # tests/test_pose_ik_host.py
OBJECTS = ("Wine_Bottle", "dumbbell")
DEFAULT_MARGIN = -0.03  # scene.DEFAULT_SKELETON_MARGIN
FRAME_WORLD = -1


# ---- the partition of the tested pairs ----------------------------------------------------------------------------------------------
def moving_arm(frame):
    """the arm a sphere on `frame` moves with, -1 for a static one (a base, the world)"""
    return -1 if frame < 0 or frame % 9 == 8 else frame // 9


def sub_scene(spheres, arm):
    """the caller's spheres minus those moving on the other arm, in their order"""
    return [s for s in spheres if moving_arm(s[0]) in (-1, arm)]


def arm_pairs(spheres, boxes, allowed, arm):
    """the number of tested pairs in arm `arm`'s set"""
    ss, sb = scene_cases.tested_pairs(sub_scene(spheres, arm), boxes, allowed)
    return len(ss) + len(sb)


def cross_pairs(spheres, allowed):
    ss, _ = scene_cases.tested_pairs(spheres, [], allowed)
    return [(i, j) for i, j in ss if {moving_arm(spheres[i][0]), moving_arm(spheres[j][0])} == {0, 1}]


def cross_scenes(spheres, allowed):
    """[(spheres, allowed)]: per sphere i moving on arm 0 with cross pairs, i and its partners on arm 1"""
    out = []
    pairs = cross_pairs(spheres, allowed)
    for i in sorted({(i if moving_arm(spheres[i][0]) == 0 else j) for i, j in pairs}):
        partners = sorted({(j if a == i else a) for a, j in pairs if i in (a, j)})
        al = [0] * 32
        al[1] = 1 << 1
        out.append(([(spheres[i][0], 0) + tuple(spheres[i][2:])] + [(spheres[j][0], 1) + tuple(spheres[j][2:]) for j in partners], al))
    return out


def cross_clearance(oracle, P, spheres, allowed, q):
    """(B,) the smallest signed distance over the cross pairs at the states q (B,14), by the oracle; +inf without cross pairs"""
    best = np.full(len(q), np.inf)
    for sp, al in cross_scenes(spheres, allowed):
        best = np.minimum(best, oracle.clearance_batch(P, sp, [], al, q)[0])
    return best


def _other(frame):
    return frame if frame < 0 else (frame + 9) % 18


def counted_scene(n, arm, seed=0x1CE7):
    """(spheres, boxes, allowed) with exactly n tested pairs in arm `arm`'s set (n <= 1 or n >= 9).  Groups: 0 body k = 3 of `arm`, 1 its
    hand, 2 its own base, 3 the other base, 4 a world sphere, 5 the box, 6 / 7 the other arm's body and hand, 8 world fillers tested
    against the body alone.  The body and the hand have nine pairs: each other, the two bases, the world sphere and the box for each."""
    rng = np.random.default_rng(seed + 31 * n + arm)
    c = lambda lo=-0.1, hi=0.1: tuple(float(v) for v in rng.uniform(lo, hi, 3))  # noqa: E731
    w = lambda: tuple(float(v) for v in rng.uniform([0.0, -0.6, 0.7], [0.8, 0.6, 1.7]))  # noqa: E731
    f = (lambda k: k) if arm == 0 else (lambda k: _other(k))
    spheres = [(f(3), 0, c(), 0.06), (f(7), 1, c(), 0.04), (f(8), 2, c(), 0.05), (f(17), 3, c(), 0.05), (FRAME_WORLD, 4, w(), 0.07),
               (f(12), 6, c(), 0.06), (f(16), 7, c(), 0.04)]
    boxes = [(5, w(), np.linalg.qr(rng.standard_normal((3, 3)))[0], tuple(float(v) for v in rng.uniform(0.05, 0.3, 3)))]
    allowed = [0] * 32
    allow = lambda g, h: scene_cases_allow(allowed, g, h)  # noqa: E731
    if n <= 1:
        for g in (0, 1):
            for h in range(8):
                if not (n == 1 and (g, h) == (0, 4)):
                    allow(g, h)
    else:
        assert n >= 9
        for _ in range(n - 9):
            spheres.append((FRAME_WORLD, 8, w(), float(rng.uniform(0.0, 0.05))))
        for h in (1, 6, 7):
            allow(8, h)
    assert arm_pairs(spheres, boxes, allowed, arm) == n, (arm_pairs(spheres, boxes, allowed, arm), n)
    return spheres, boxes, allowed


def scene_cases_allow(allowed, g, h):
    allowed[g] |= 1 << h
    allowed[h] |= 1 << g


COUNTS = (0, 1, 15, 16, 17)
LARGE = ("1920+512", "statics9", "ns17")  # tests/scene_cases.py: its largest scene; world and base spheres; seventeen spheres
ARM_SCENES = tuple("n%d/arm%d" % (n, a) for n in COUNTS for a in (0, 1)) + LARGE


@functools.lru_cache(maxsize=None)
def arm_scene(name):
    if name in LARGE:
        return scene_cases.scene(name)
    n, a = name[1:].split("/arm")
    return counted_scene(int(n), int(a))


def candidates(oracle, P, n, seed=0xCA7D):
    """(n,7) joint rows inside the limits: the first arm's half of the oracle's ambient uniform samples"""
    return np.ascontiguousarray(oracle.ambient_uniform_batch(P, seed, 0, n)[:, :7])


def state_of(P, arm, q7):
    """(B,14): the candidates in arm `arm`'s half, the problem's start joints in the other"""
    x = np.tile(np.array(P.start_joint[:], dtype=np.float64), (len(q7), 1))
    x[:, 7 * arm:7 * arm + 7] = q7
    return x


# ---- the selection, restated -----------------------------------------------------------------------------------------------------------
def _d2(q, s):
    acc = 0.0
    for i in range(7):
        d = float(q[i]) - float(s[i])
        acc = float(Fraction(d) * Fraction(d) + Fraction(acc))  # one FMA: the exact value, rounded once
    return acc


def arm_pick(rounds, clear, cand_q, seed7, margin):
    """the candidate an arm takes under the vetted rule, or None.  margin None: the plain rule"""
    ok = [r for r in range(len(rounds)) if rounds[r] >= 0 and (margin is None or clear[r] > margin)]
    if not ok:
        return None
    if ok[0] == 0:
        return 0
    return min(ok, key=lambda r: (_d2(cand_q[r], seed7), r))


def assemble(cand_q, cand_rounds, cand_clear, seeds, margin):
    """per (t, s): the assembled row or None"""
    T, S = cand_rounds.shape[:2]
    rows = [[None] * S for _ in range(T)]
    for t in range(T):
        for s in range(S):
            pick = [arm_pick(cand_rounds[t, s, a], None if cand_clear is None else cand_clear[t, s, a], cand_q[t, s, a], seeds[t, s, 7 * a:7 * a + 7], margin)
                    for a in (0, 1)]
            if None not in pick:
                rows[t][s] = np.concatenate([cand_q[t, s, 0, pick[0]], cand_q[t, s, 1, pick[1]]])
    return rows


def select_vetted(cand_q, cand_rounds, cand_clear, slot_clear, seeds, margin):
    """(q (T,14), ok (T,), which (T,)) and the assembled rows: admissible = converged and arm clearance > margin; candidate 0 if
    admissible, else the admissible restart closest to the seed, ties to the lowest r; the first assembled slot whose slot clearance
    > margin"""
    T, S = cand_rounds.shape[:2]
    rows = assemble(cand_q, cand_rounds, cand_clear, seeds, margin)
    q = np.full((T, 14), np.nan)
    ok = np.zeros(T, dtype=np.uint8)
    which = np.full(T, -1, dtype=np.int32)
    for t in range(T):
        for s in range(S):
            if rows[t][s] is not None and slot_clear[t, s] > margin:
                q[t], ok[t], which[t] = rows[t][s], 1, s
                break
    return q, ok, which, rows


# ---- the 40-target inputs and the scenes built from their records ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem_of(obj):
    return host_constraint(obj=obj).problem


@functools.lru_cache(maxsize=None)
def plain_run(obj):
    """(P, targets, seeds, the plain rule's outputs with the candidates' records) on tests/test_pose_ik_host.py's inputs"""
    from closed_chain_motion_planner_amd import pose_ik_ref

    targets, seeds = sampled_case(obj)[4:]
    P = problem_of(obj)
    return P, targets, seeds, pose_ik_ref(P, targets, seeds, rng_seed=RNG_SEED, want_candidates=True)


def vetted_ref(obj, scene, margin, rows=None, **kw):
    """ccmp_pose_ik_vetted_ref on those inputs with the records; rows: a slice of the targets (the caller passes the matching first_index)"""
    from closed_chain_motion_planner_amd import pose_ik_vetted_ref

    P, targets, seeds, _ = plain_run(obj)
    sel = slice(None) if rows is None else rows
    return pose_ik_vetted_ref(P, targets[sel], seeds[sel], scene.spheres, scene.boxes, scene.allowed, margin, rng_seed=RNG_SEED, want_candidates=True, **kw)


def default_scene(obj):
    return default_scene_host(problem_of(obj))


def _origin(oracle, OP, frame, q7):
    """world position of the origin of `frame` with its arm at q7 (the other arm's joints do not enter)"""
    return oracle.proxy_centres(OP, [(frame, 0, (0.0, 0.0, 0.0), 0.0)], state_of(OP, frame // 9, q7[None])[0])[0]


@functools.lru_cache(maxsize=None)
def branch_scenes(obj):
    """{"a": (HostScene, facts), "b": ..., "c": ...} from the plain run's records, by the det oracle's forward kinematics"""
    from oracle_binding import Oracle

    O = Oracle("det")
    P, targets, seeds, out = plain_run(obj)
    OP = O.problem_from_bytes(bytes(P))
    cq, cr = out["cand_q"], out["cand_rounds"]
    scenes = {}
    # (a): the winning slot of a solved target, an arm whose seeded candidate converged, the farthest converged restart of that arm
    for t in np.flatnonzero(out["ok"]):
        s = int(out["which"][t])
        for a in (0, 1):
            rest = [r for r in range(1, cr.shape[3]) if cr[t, s, a, r] >= 0]
            if cr[t, s, a, 0] < 0 or not rest or "a" in scenes:
                continue
            for k in (3, 2, 4, 5):
                f = 9 * a + k
                e0 = _origin(O, OP, f, cq[t, s, a, 0])
                disp = max(float(np.linalg.norm(_origin(O, OP, f, cq[t, s, a, r]) - e0)) for r in rest)
                if disp > 1e-3:
                    sc = HostScene([(FRAME_WORLD, 0, tuple(float(v) for v in e0), disp / 4), (f, 1, (0.0, 0.0, 0.0), disp / 4)])
                    scenes["a"] = (sc, dict(target=int(t), slot=s, arm=a, frame=f, displacement=disp))
                    break
    # (b): the first two slots of a target that assemble under the plain rule, the first with the smaller elbow-to-elbow distance
    rows = assemble(cq, cr, None, seeds, None)
    for t in range(len(targets)):
        have = [s for s in range(len(rows[t])) if rows[t][s] is not None]
        if len(have) < 2:
            continue
        d = [float(np.linalg.norm(_origin(O, OP, 3, rows[t][s][:7]) - _origin(O, OP, 12, rows[t][s][7:]))) for s in have[:2]]
        if d[1] - d[0] > 1e-3:
            rsum = 0.5 * (d[0] + d[1])
            sc = HostScene([(3, 0, (0.0, 0.0, 0.0), rsum / 2), (12, 1, (0.0, 0.0, 0.0), rsum / 2)])
            scenes["b"] = (sc, dict(target=t, slots=tuple(have[:2]), distances=tuple(d)))
            break
    scenes["c"] = (HostScene([(3, 0, (0.0, 0.0, 0.0), 10.0), (12, 1, (0.0, 0.0, 0.0), 10.0)]), {})
    return scenes


def kinds(plain, vet, margin):
    """per target the branches its vetted answer took: a set of "a" (an arm of the winning slot whose seeded candidate converged, was
    refused, and an admissible restart was taken), "b" (an earlier slot was assembled and refused by the slot test alone), "c" (solved
    by the plain rule, failed here), "d" (the plain rule's row, ok and which)"""
    out = []
    for t in range(len(vet["ok"])):
        k = set()
        if vet["ok"][t]:
            s = int(vet["which"][t])
            for a in (0, 1):
                picked = vet["q"][t, 7 * a:7 * a + 7]
                if (vet["cand_rounds"][t, s, a, 0] >= 0 and not vet["cand_clear"][t, s, a, 0] > margin
                        and not np.array_equal(picked, vet["cand_q"][t, s, a, 0])):
                    k.add("a")
            if any(np.isfinite(vet["slot_clear"][t, e]) and not vet["slot_clear"][t, e] > margin for e in range(s)):
                k.add("b")
        elif plain["ok"][t]:
            k.add("c")
        if (vet["ok"][t] == plain["ok"][t] and vet["which"][t] == plain["which"][t]
                and np.array_equal(vet["q"][t].view(np.uint64), plain["q"][t].view(np.uint64))):
            k.add("d")
        out.append(k)
    return out

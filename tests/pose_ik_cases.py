"""Inputs and numpy restatements shared by the pose-IK tests (tests/test_pose_ik_host.py, tests/test_gpu_pose_ik.py).

Targets are object poses of states that exist: the valid states among orc_sample_project_batch(seed 0x4B4E, first 0, 1 500) of the libm
oracle (both `ok` and orc_joint_valid), their poses ccmp_pose_from_t_wo of orc_compute_t_wo.  The first 40 are targets; the rest
supply each target's 5 pose-nearest states as seed slots, nearest first (ccmp_pose_distance, ties to the lower index) — what the
store's object-metric k-NN hands growTree.  Everything is computed once per object and shared."""
import functools

import numpy as np

from conftest import load_cfg

SEED, SAMPLES, TARGETS, SLOTS = 0x4B4E, 1500, 40, 5


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle_binding import Oracle

    return Oracle("libm")


def pose_of(orc, OP, q):
    from closed_chain_motion_planner_amd import pose_from_t_wo

    R, p = orc.compute_t_wo(OP, np.asarray(q)[:7])
    return pose_from_t_wo(np.concatenate([R.reshape(9), p]))


@functools.lru_cache(maxsize=None)
def sampled_case(obj):
    """(oracle, oracle problem, valid states (n,14), their poses (n,8), targets (40,8), seeds (40,5,14))"""
    from closed_chain_motion_planner_amd import pose_distance

    orc = _oracle()
    OP = orc.problem(load_cfg(obj))
    q, ok, _ = orc.sample_project_batch(OP, SEED, 0, SAMPLES)
    valid = np.array([x for x, o in zip(q, ok) if o and orc.joint_valid(OP, x)])
    poses = np.array([pose_of(orc, OP, x) for x in valid])
    seeds = np.empty((TARGETS, SLOTS, 14))
    for t in range(TARGETS):
        d = np.array([pose_distance(poses[t], poses[j]) for j in range(TARGETS, len(valid))])
        seeds[t] = valid[TARGETS + np.argsort(d, kind="stable")[:SLOTS]]
    for a in (valid, poses, seeds):
        a.setflags(write=False)
    return orc, OP, valid, poses, poses[:TARGETS], seeds


def rot_of_quat(q):
    """Eigen's toRotationMatrix on (x, y, z, w), not normalised"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hand_target(P, pose, arm):
    """T_obj * t_o7[arm] -> (R (3,3), p (3,)); P: any problem struct with t_o7_R / t_o7_p"""
    Ro = rot_of_quat(pose[3:7])
    toR = np.array(P.t_o7_R[:]).reshape(2, 3, 3)[arm]
    top = np.array(P.t_o7_p[:]).reshape(2, 3)[arm]
    return Ro @ toR, pose[:3] + Ro @ top


def twist(Rt, pt, R, p):
    """the six error components in the world frame: p_t - p and the rotation vector of R_t R^T"""
    Re = Rt @ R.T
    v = 0.5 * np.array([Re[2, 1] - Re[1, 2], Re[0, 2] - Re[2, 0], Re[1, 0] - Re[0, 1]])
    n = np.linalg.norm(v)
    rot = v * (np.arctan2(n, 0.5 * (np.trace(Re) - 1.0)) / n) if n > 0 else v
    return np.concatenate([pt - p, rot])


def select(cand_q, cand_rounds, seeds):
    """the rule over the candidates' records in numpy: (q (T,14), ok (T,), which (T,)).  cand_q (T,S,2,1+R,7), cand_rounds (T,S,2,1+R),
    seeds (T,S,14).  The squared distance is the solver's FMA chain in joint order; each FMA is formed in exact rational arithmetic
    and rounded once."""
    from fractions import Fraction

    def fma(a, b, c):
        return float(Fraction(a) * Fraction(b) + Fraction(c))  # correctly rounded: the exact value, rounded once by float()

    def d2(q, s):
        acc = 0.0
        for i in range(7):
            d = float(q[i]) - float(s[i])
            acc = fma(d, d, acc)
        return acc

    T, S = cand_rounds.shape[:2]
    q = np.full((T, 14), np.nan)
    ok = np.zeros(T, dtype=np.uint8)
    which = np.full(T, -1, dtype=np.int32)
    for t in range(T):
        for s in range(S):
            pick = []
            for a in range(2):
                rounds = cand_rounds[t, s, a]
                if rounds[0] >= 0:
                    pick.append(0)
                    continue
                best = None
                for r in range(1, len(rounds)):
                    if rounds[r] < 0:
                        continue
                    d = d2(cand_q[t, s, a, r], seeds[t, s, 7 * a:7 * a + 7])
                    if best is None or d < best[0]:
                        best = (d, r)
                if best is None:
                    break
                pick.append(best[1])
            if len(pick) == 2:
                q[t] = np.concatenate([cand_q[t, s, 0, pick[0]], cand_q[t, s, 1, pick[1]]])
                ok[t], which[t] = 1, s
                break
    return q, ok, which

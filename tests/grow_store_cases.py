"""Inputs and the host reference chain shared by the tests of Roadmap.grow on a store that also holds pose-only vertices
(tests/test_grow_store_host.py, tests/test_gpu_grow_store.py).  Host only: nothing here touches a device.

The chain restates what ccmp_roadmap_grow promises, out of the host forms of its parts:
  1. neighbours: pose_knn_reference.reference (one ccmp_pose_distance call per pair, lexsort by (distance, index));
  2. seeds[q, r]: the store's joint row at nbr_idx[q, r], a NaN row for an empty slot (a pose-only vertex's row is NaN already);
  3. pose_ik_ref (csrc/ccmp_ik.h compiled for the host) on them: q_new, ik_ok, ik_which;
  4. masked[q, r] = nbr_idx[q, r] where target q has a state, the slot is occupied and all 14 joints of that row are finite, else -1;
  5. the edges are the slots with masked >= 0, from the store's row to q_new[q].

The mixed store: the object's valid sampled states behind the 40 targets of pose_ik_cases (194 for Wine_Bottle) as joint vertices,
then, for target q of the first 12, q % 6 pose-only vertices at the target's pose with x += 1e-4 * (1 + i): closer to their target
than any joint vertex (those are tenths of a unit away), so they take its first q % 6 slots."""
import functools

import numpy as np

from knn_reference import KNN_ALL
from pose_ik_cases import TARGETS, sampled_case
from pose_knn_reference import reference as pose_knn

OBJ = "Wine_Bottle"
K, RNG_SEED, FIRST_INDEX, N_QUERIES = 5, 0x51CA, 5, 12


def bits(a):
    """the bytes of an array, every NaN as one canonical NaN (a NaN's sign and payload are no result), everything else bit for bit"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def mixed_store(obj=OBJ):
    """(joints (n,14) of the joint vertices, their libm-oracle poses (n,8), query poses (12,8), pose-only poses (m,8), owner (m,): the
    target each pose-only vertex was made for)"""
    _, _, valid, poses, targets, _ = sampled_case(obj)
    queries = np.array(targets[:N_QUERIES])
    extra, owner = [], []
    for q in range(N_QUERIES):
        for i in range(q % 6):
            p = queries[q].copy()
            p[0] += 1e-4 * (1 + i)
            extra.append(p)
            owner.append(q)
    out = (np.array(valid[TARGETS:]), np.array(poses[TARGETS:]), queries, np.array(extra), np.array(owner))
    for a in out:
        a.setflags(write=False)
    return out


def with_pose_only(joints, poses, extra):
    """the store's two arrays once `extra` has been appended as pose-only vertices: NaN joint rows, the given poses with a zero pad"""
    e = np.array(extra, dtype=np.float64).reshape(-1, 8)
    e[:, 7] = 0.0
    return np.concatenate([joints, np.full((len(e), 14), np.nan)]), np.concatenate([poses, e])


def chain(problem, store_joints, store_poses, query_poses, k=K, mode=KNN_ALL, self_base=0, rng_seed=RNG_SEED, first_index=FIRST_INDEX, opts=None):
    """steps 1-4 above on the store's arrays as they stand (store_joints (N,14) with NaN rows, store_poses (N,8)); a dict with grow's
    names plus seeds (Q,k,14) and masked (Q,k)"""
    from closed_chain_motion_planner_amd import pose_ik_ref

    store_joints = np.asarray(store_joints, dtype=np.float64).reshape(-1, 14)
    query_poses = np.ascontiguousarray(query_poses, dtype=np.float64).reshape(-1, 8)
    Q = len(query_poses)
    idx, dist = pose_knn(store_poses, query_poses, k, mode, self_base)
    occupied = idx >= 0
    seeds = np.full((Q, k, 14), np.nan)
    seeds[occupied] = store_joints[idx[occupied]]
    ik = pose_ik_ref(problem, query_poses, seeds, rng_seed=rng_seed, first_index=first_index, opts=opts)
    finite = np.ones((Q, k), dtype=bool)
    finite[occupied] = np.isfinite(store_joints[idx[occupied]]).all(axis=1)
    masked = np.where(occupied & finite & (ik["ok"] != 0)[:, None], idx, -1).astype(np.int32)
    return {"nbr_idx": idx, "nbr_dist": dist, "seeds": seeds, "q_new": ik["q"], "ik_ok": ik["ok"], "ik_which": ik["which"], "masked": masked}


def leading_empty(ref):
    """per target, the number of leading slots whose seed is not finite (pose-only vertices and -1 slots)"""
    bad = ~np.isfinite(ref["seeds"]).all(axis=2)
    return np.array([len(row) if row.all() else int(np.argmin(row)) for row in bad])

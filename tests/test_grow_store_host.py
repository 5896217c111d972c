"""The inputs of tests/test_gpu_grow_store.py are not degenerate: the host reference chain of tests/grow_store_cases.py on the mixed
store (joint vertices and pose-only ones), no device.  What is asserted are properties, not recorded numbers: the libm oracle draws
the samples, so another C library may give other states."""
import numpy as np
import pytest

from conftest import config_path
from grow_store_cases import FIRST_INDEX, K, N_QUERIES, OBJ, RNG_SEED, bits, chain, leading_empty, mixed_store, with_pose_only
from knn_reference import KNN_ALL, KNN_EARLIER, KNN_NOT_SELF


@pytest.fixture(scope="module")
def case(ccmp_built):
    from closed_chain_motion_planner_amd import load_config

    P = load_config(config_path(OBJ))
    joints, poses, queries, extra, owner = mixed_store()
    sj, sp = with_pose_only(joints, poses, extra)
    return P, sj, sp, queries, owner, len(joints), chain(P, sj, sp, queries)


def test_the_mixed_store_reaches_every_kind_of_slot(case):
    P, sj, sp, queries, owner, n_joint, ref = case
    assert len(queries) == N_QUERIES and len(owner) == sum(q % 6 for q in range(N_QUERIES)) and len(sj) == n_joint + len(owner)
    idx, lead = ref["nbr_idx"], leading_empty(ref)
    assert (idx >= 0).all()  # more than k vertices: every slot has a neighbour
    pose_only = idx >= n_joint
    # a target's own pose-only vertices rank first, in the order they were made (1e-4 apart against tenths of a unit to a joint vertex)
    for q in range(N_QUERIES):
        own = n_joint + np.flatnonzero(owner == q)
        assert list(idx[q, :min(K, len(own))]) == list(own[:K]) and lead[q] >= min(K, len(own)), q
    # the solver skipped exactly the leading pose-only slots and solved from the first slot that has joints
    assert np.array_equal(ref["ik_which"], np.where(lead < K, lead, -1)), (ref["ik_which"], lead)
    assert np.array_equal(ref["ik_ok"], (lead < K).astype(np.uint8))
    assert np.isnan(ref["q_new"][lead == K]).all() and np.isfinite(ref["q_new"][lead < K]).all()
    # the masking rule: a slot is an edge iff the target has a state and the neighbour has joints
    want = np.where((~pose_only) & (lead < K)[:, None], idx, -1)
    assert np.array_equal(ref["masked"], want)
    empty = (ref["masked"] < 0).sum(axis=1)
    assert (empty == K).any() and (empty == 0).any() and ((empty > 0) & (empty < K)).any()
    # a pose-only vertex made for another target is somebody's neighbour: such a vertex is an ordinary node of the object metric
    other = [(q, int(j)) for q in range(N_QUERIES) for j in idx[q][pose_only[q]] if owner[j - n_joint] != q]
    assert other, "no target sees another target's pose-only vertex"
    print("ik_which", list(ref["ik_which"]), "nearest joint vertex %.3g..%.3g" % tuple(np.percentile([ref["nbr_dist"][q][~pose_only[q]].min()
                                                                                                    for q in range(N_QUERIES) if (~pose_only[q]).any()], [0, 100])),
          "foreign pose-only neighbours", other[:4])


def test_masking_follows_the_joint_row_not_the_index(case):
    """an +inf in a joint row masks the slot as a NaN row does and the solver skips it; restoring the row restores the edge"""
    P, sj, sp, queries, owner, n_joint, ref = case
    q = int(np.flatnonzero(ref["ik_which"] == 0)[0])
    j = int(ref["nbr_idx"][q, 0])
    assert j < n_joint
    broken = sj.copy()
    broken[j, 9] = np.inf
    out = chain(P, broken, sp, queries)
    assert np.array_equal(out["nbr_idx"], ref["nbr_idx"])  # the object metric does not read the joints
    assert not (out["masked"] == j).any() and (ref["masked"] == j).any()
    assert out["ik_which"][q] >= 1 or out["ik_which"][q] == -1


def test_modes_on_a_short_store(case):
    """fewer vertices than k, and KNN_EARLIER with a small self_base: -1 slots next to pose-only ones"""
    P, sj, sp, queries, owner, n_joint, _ = case
    short_j, short_p = with_pose_only(sj[:2], sp[:2], queries[1:2])
    short_j, short_p = np.concatenate([short_j, sj[2:3]]), np.concatenate([short_p, sp[2:3]])  # joints, joints, pose-only, joints
    out = chain(P, short_j, short_p, queries[:3])
    assert ((out["nbr_idx"] >= 0).sum(axis=1) == 4).all() and (out["nbr_idx"][:, 4] == -1).all()
    assert out["nbr_idx"][1, 0] == 2 and (out["masked"] != 2).all()
    early = chain(P, sj, sp, queries[:4], mode=KNN_EARLIER, self_base=n_joint - 1)
    assert ((early["nbr_idx"] >= 0).sum(axis=1) == K).all() and (early["nbr_idx"][0] < n_joint - 1).all()
    tiny = chain(P, short_j, short_p, queries[:4], mode=KNN_EARLIER, self_base=1)
    assert list((tiny["nbr_idx"] >= 0).sum(axis=1)) == [1, 2, 3, 4]
    assert (tiny["masked"][tiny["nbr_idx"] == 2] == -1).all()


def test_append_first_equals_query_first(case):
    """the targets appended as pose-only vertices t .. t + Q - 1 and queried with KNN_NOT_SELF, self_base = t; for one
    target that is the query-first result on the store without the vertex"""
    P, sj, sp, queries, owner, n_joint, ref = case
    t = len(sj)
    aj, ap = with_pose_only(sj, sp, queries)
    first = chain(P, aj, ap, queries, mode=KNN_NOT_SELF, self_base=t)
    assert not (first["nbr_idx"] == (t + np.arange(N_QUERIES))[:, None]).any()
    for q in (0, 3, 5):  # no pose-only slot, three, all five
        oj, op = with_pose_only(sj, sp, queries[q:q + 1])
        a = chain(P, oj, op, queries[q:q + 1], mode=KNN_NOT_SELF, self_base=t, first_index=FIRST_INDEX + q)
        b = chain(P, sj, sp, queries[q:q + 1], mode=KNN_ALL, first_index=FIRST_INDEX + q)
        for name in a:
            assert np.array_equal(bits(a[name]), bits(b[name])), (q, name)
            assert np.array_equal(bits(b[name][0]), bits(ref[name][q])), (q, name)  # and a call over one target is a row of the call over 12
    assert RNG_SEED == 0x51CA

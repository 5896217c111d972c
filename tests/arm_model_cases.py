"""The arm models the library chooses its kernels by, and the inputs the planner-side tests share on them.

make_consts (csrc/ccmp_problem.cpp) sets K.stock, K.twin_arms, K.rot_x0 and K.base_diag from the problem; every launcher that depends
on the kinematics switches on them:

    stock              stock = 1, twin_arms = 1, base_diag = 3: the shipped configs
    general_kernels    the same problem with option stock_kernels = 0: all three flags cleared, the same numbers
    tilted             stock = 1, twin_arms = 0, base_diag = 1: stock arms, arm 1 on a rotated base
    calibrated         stock = 0: ccmp_set_calibration with offsets that differ per arm
    calibrated_tilted  both

Nothing here needs a device: `host_constraint` is a constraint without a context (its problem struct and the host set-up calls are all
that is used), `HostScene` the proxies of a scene as ProxyScene keeps them, `oracle_edges` / `oracle_pick_margin` the det oracle's
restatement of `edges` / test_gpu_geodesic_scene._pick_margin.  tests/test_arm_model_cases.py checks with them, on the oracle alone,
that the seeds below give every GPU test the cases it is about."""
import contextlib
import ctypes as C

import numpy as np

from conftest import NCPU, config_path

MODELS = ("stock", "general_kernels", "tilted", "calibrated", "calibrated_tilted")
OBJ = "Wine_Bottle"

# sizes of the GPU tests (tests/test_gpu_arm_models_scene.py, tests/test_gpu_arm_models_planner.py)
B_CLEAR = 130            # two 64-state tiles plus two lanes
E_SCENE, MS_SCENE = 32, 16
E_PLAIN, MS_PLAIN = 64, 8
F_PATHS, L_PATHS = 4, 6
# seeds, chosen in tests/test_arm_model_cases.py so that the oracle alone meets each test's conditions on every model and mode
CLEAR_SEED = 0xA2C0
PLAIN_SEED = 0xA2D0
EXTEND_SEED = {(m, j): 0xA2E0 for m in MODELS for j in (0, 1)}
PATH_SEED = {("tilted", 0): 0xB600, ("tilted", 1): 0xB600, ("calibrated", 0): 0xB0B8, ("calibrated", 1): 0xB0B8}
# smoothing (test_gpu_arm_models_planner.test_smooth): the paths of waypoint_paths(.., F_PATHS, L_PATHS, SMOOTH_SEED), SMOOTH_STEPS passes,
# a result of ccmp_smooth_len_after(L_PATHS, SMOOTH_STEPS) = 21 vertices per path
# (PATH_SEED's paths do not serve: on them no candidate is refused or below min_change without a scene)
SMOOTH_SEED = {("tilted", 0): 0xBA88, ("tilted", 1): 0xBA88, ("calibrated", 0): 0xB708, ("calibrated", 1): 0xB708}
SMOOTH_STEPS, SMOOTH_CAP = 2, 21


def tilt(c):
    """stock arms on a tilted base: the general base-frame instantiation (DIAG = false)"""
    a, b = 0.3, -0.7
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    for k, v in enumerate((Rz @ Rx).reshape(-1)):
        c.problem.base_R[9 + k] = float(v)
    c.setInitialPosition(np.array(c.problem.start_joint[:]))


def calibrate(c):
    """PandaModel::initModel(dh) with offsets of the order of 1e-3 that differ between the arms (test_gpu_pose_ik._constraint)"""
    from closed_chain_motion_planner_amd import _lib

    for arm in (0, 1):
        dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    c.setInitialPosition(np.array(c.problem.start_joint[:]))


@contextlib.contextmanager
def apply(c, gpu_ctx, model):
    """constraint `c` as `model` inside the block.  tilted / calibrated change c.problem for good (c is the test's own); general_kernels
    changes an option of the shared context and puts it back.  gpu_ctx None: a host constraint, which has no kernels to choose"""
    assert model in MODELS, model
    if model in ("calibrated", "calibrated_tilted"):
        calibrate(c)
    if model in ("tilted", "calibrated_tilted"):
        tilt(c)
    if model == "general_kernels" and gpu_ctx is not None:
        gpu_ctx.set_option("stock_kernels", 0)
    try:
        yield c
    finally:
        if model == "general_kernels" and gpu_ctx is not None:
            gpu_ctx.set_option("stock_kernels", 1)


def edges(c, E, seed):
    """growTree-shaped edges (src/planner/stefanBiPRM.cpp:307-351): a valid projected state -> a projected sampleUniformNear state"""
    q, okq, _, _ = c.sample_project_batch(seed, 0, 8 * E + 64, want_iters=False)
    frm = q[okq == 1][:E].contiguous()
    assert frm.shape[0] == E
    to, _, _, _ = c.sample_near_project_batch(seed + 1, 0, frm, 0.6, E, want_iters=False)
    return frm, to


# ---- the same without a device -------------------------------------------------------------------------------------------------------
class _NoDevice:
    handle, device = None, None


def host_constraint(mode=0, obj=OBJ):
    """a KinematicChainConstraint without a context: the problem struct and the host set-up calls (calibration, start state) only"""
    from closed_chain_motion_planner_amd import KinematicChainConstraint
    from closed_chain_motion_planner_amd.constraint import load_config

    c = KinematicChainConstraint(14, ctx=_NoDevice(), problem=load_config(config_path(obj)))
    c.setJacobianMode(mode)
    c._fixture = obj
    return c


class HostScene:
    """the proxies of a scene as ProxyScene keeps them (spheres, boxes, allowed), without the device object"""

    def __init__(self, spheres, boxes=(), allowed=None):
        self.spheres = [(int(f), int(g), tuple(float(v) for v in c), float(r)) for f, g, c, r in spheres]
        self.boxes = [(int(g), tuple(float(v) for v in c), np.asarray(R, dtype=np.float64).reshape(3, 3).copy(), tuple(float(v) for v in h))
                      for g, c, R, h in boxes]
        self.allowed = None if allowed is None else [int(v) & 0xFFFFFFFF for v in allowed]


def default_scene_host(problem):
    """what ProxyValidityChecker(c).scene holds: the skeleton of the problem's own chain constants, sub_table, the default matrix"""
    from closed_chain_motion_planner_amd import scene as S

    return HostScene(S.skeleton_spheres(problem), [S.ProxyValidityChecker.SUB_TABLE], S.default_allowed())


def clear_margin(scene, clr_oracle):
    """the margin of the clearance test's flags: 0 on the default scene (both signs occur there); the oracle's median on the random
    scene, whose overlapping spheres keep the clearance negative at every state"""
    return 0.0 if scene == "default" else float(np.median(clr_oracle))


def project_wrapped(O, P, amb):
    """project, then enforceBounds: what the samplers return"""
    q, ok, _ = O.project_batch(P, amb, NCPU)
    return np.array([O.enforce_bounds(x) for x in q]).reshape(-1, 14), ok


def oracle_edges(O, P, E, seed):
    """`edges` by the oracle's samplers: the same rows bit for bit (the GPU tests assert that)"""
    q, ok, _ = O.sample_project_batch(P, seed, 0, 8 * E + 64, NCPU)
    frm = np.ascontiguousarray(q[ok == 1][:E])
    assert frm.shape[0] == E
    to, _ = project_wrapped(O, P, O.ambient_ref_batch(P, "near", seed + 1, 0, frm, 0.6, E))
    return frm, to


def oracle_pick_margin(O, P, sc, frm, to, ms):
    """test_gpu_geodesic_scene._pick_margin by the oracle: the median of each edge's smallest clearance over the unfiltered traversal"""
    st, n, _, _ = O.discrete_geodesic_batch(P, frm, to, ms, NCPU)
    mins = []
    for e in range(len(n)):
        m = min(int(n[e]), ms)
        if m >= 2:
            mins.append(O.clearance_batch(P, sc.spheres, sc.boxes, sc.allowed, st[e, 1:m])[0].min())
    return float(np.median(mins))


def waypoint_paths(c, oracle, P, F, max_len, seed):
    """Synthetic solution paths on the model's own manifold (the recorded files are stock problems): F chains of valid projected states,
    each the sample_near_project of its predecessor at distance 0.6, by the oracle's samplers; ragged lengths 2, 3, max_len and one path
    of length 1.  -> path_joints (F,max_len,14), path_len (F,) int32.  Rows behind a path's length are chain states too (never read)."""
    assert bytes(P) == bytes(c.problem)  # the oracle samples on the constraint's own model
    n = 8 * F
    q, ok, _ = oracle.sample_project_batch(P, seed, 0, 8 * n, NCPU)
    cols = [np.ascontiguousarray(q[ok == 1][:n])]
    assert cols[0].shape[0] == n
    alive = np.ones(n, dtype=bool)
    for j in range(1, max_len):
        nxt, okj = project_wrapped(oracle, P, oracle.ambient_ref_batch(P, "near", seed + j, 0, cols[-1], 0.6, n))
        alive &= okj == 1
        cols.append(nxt)
    keep = np.flatnonzero(alive)[:F]  # the first F chains whose every state is a valid projected one
    assert len(keep) == F
    path_joints = np.ascontiguousarray(np.stack(cols, axis=1)[keep])
    path_len = np.array([(2, 3, max_len, 1)[f % 4] for f in range(F)], dtype=np.int32)
    return path_joints, path_len


def scene_edge(orc_scene, blocked=None):
    """shortcut_cases.oracle_pairs' `edge` for a scene: one uninterrupted traversal behind the validity callback"""
    def edge(a, b):
        r, _, n, its, _, bl, _ = orc_scene.edge(a, b, 4096)
        assert n <= 4096
        if blocked is not None:
            blocked.append(bl)
        return r, n, its

    return edge

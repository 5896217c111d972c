"""Dense solution paths on the device (ccmp_path_densify: the continuation loop over the extend step, dense_gather / dense_pack /
dense_arc / dense_clear kernels) through the device form and the host form.  Expected values are the det oracle's uninterrupted
`discrete_geodesic(..., interpolate=True, max_states=1024)` per segment, joined by the plain-Python rule of tests/dense_path_cases.py;
comparisons are bit for bit: rows, path_first, seg_first, seg_ok, seg_newton.  Arc against dense_arc_ref on the downloaded rows, the
clearance summary against ccmp_clearance_batch and numpy."""
import ctypes as C

import numpy as np
import pytest

from dense_path_cases import RECORDED, bits, distinct_of_reference, join, oracle_segments, recorded_case, recorded_roadmap, same_paths
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL, EOVERFLOW = -1, -8
CHAIN_SEED = 0xD5E  # case 3: with it at least one extend call contributes no row to its segment (asserted there)
PAIR_SEED = 0x12D   # case 4: both seg_ok values occur among the eight segments (asserted there)


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _np(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """one constraint per (object, Jacobian mode), delta as the object's file was recorded with"""
    made = {}

    def get(obj, mode):
        if (obj, mode) not in made:
            c = _constraint(obj, gpu_ctx, mode)
            c.problem.delta = RECORDED[obj]["delta"] if obj in RECORDED else c.problem.delta
            made[(obj, mode)] = c
        return made[(obj, mode)]

    return get


@pytest.fixture(scope="module")
def recorded(oracle_det):
    made = {}

    def get(obj, mode):
        if (obj, mode) not in made:
            made[(obj, mode)] = recorded_case(oracle_det, obj, mode)
        return made[(obj, mode)]

    return get


# ---- 1. the recorded files -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [False, True])
@pytest.mark.parametrize("chunk", [2, 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("obj", sorted(RECORDED))
def test_recorded_files(cons, recorded, oracle_det, obj, mode, chunk, distinct):
    from closed_chain_motion_planner_amd import format_path_matrix, parse_path_matrix

    c, rec = cons(obj, mode), RECORDED[obj]
    P, pj, pl, segs, file_rows = recorded(obj, mode)
    assert bytes(_oracle_problem(oracle_det, c)) == bytes(P)  # the oracle's own set-up and the product's agree, delta and mode included
    want = join(pj, pl, pj.shape[1], segs, distinct=distinct)
    got = _np(c.densify_paths(_dev(pj), _dev(pl), distinct=distinct, chunk_states=chunk))
    same_paths(got, want, (obj, mode, chunk, distinct))
    longest = max(len(s[1]) for s in segs.values())
    assert got["rows"] == len(want["rows"]) == (rec["distinct_rows"] if distinct else rec["rows"])
    if chunk == 2:  # every continuation contributes exactly one row: at least n - 1 extend calls for the longest list
        assert got["calls"] >= longest - 1
    else:
        assert got["calls"] >= 1
    if obj == OBJ:
        assert got["seg_ok"][0].tolist() == [1, 0, 1, 1]  # the unreached segment is part of the contract
    keep = distinct_of_reference(join(pj, pl, pj.shape[1], segs)) if distinct else np.arange(rec["rows"])
    if mode == 0:
        worst = float(np.abs(got["joints"] - file_rows[keep]).max())
        print("%s chunk %d distinct %d: max |dq| against the file = %.3e rad" % (obj, chunk, distinct, worst))
        assert worst <= rec["bound"]
    back = parse_path_matrix(format_path_matrix(got["joints"]))
    assert len(back) == len(file_rows[keep]) and (distinct or len(back) == len(file_rows))


# ---- 2. the recorded roadmap through the store -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def roadmap_case(cons, oracle_det):
    from closed_chain_motion_planner_amd import Roadmap

    c = cons(OBJ, 0)
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    rm.append(_dev(nodes))
    assert rm.add_edges(_dev(uv)) == 0
    src = np.array([i for i in range(8) for _ in range(8)], dtype=np.int32)
    dst = np.array([j for _ in range(8) for j in range(8)], dtype=np.int32)
    sp = rm.shortest_paths(_dev(src), _dev(dst), max_len=8)
    assert sp["joints"].shape == (64, 8, 14)  # every path fitted
    plen = sp["path_len"].clone()
    plen[5], plen[11] = 0, 1  # set by the test: an empty path and a single waypoint among real ones
    yield c, rm, sp["joints"], plen
    rm.close()


def test_roadmap_paths_device_equals_host_equals_oracle(roadmap_case, oracle_det):
    c, rm, pj_d, pl_d = roadmap_case
    P = _oracle_problem(oracle_det, c)
    pj, pl = np.nan_to_num(pj_d.cpu().numpy(), nan=0.0), pl_d.cpu().numpy()
    segs = oracle_segments(oracle_det, P, pj, pl)
    assert sum(len(s[1]) == 1 for s in segs.values()) >= 1  # edges with dist <= delta: a list that is its starting state alone
    for distinct in (False, True):
        want = join(pj, pl, 8, segs, distinct=distinct)
        dev = _np(c.densify_paths(pj_d, pl_d, distinct=distinct))  # the store's device outputs, handed straight on
        same_paths(dev, want, ("device", distinct))
        a, b = dev["path_first"][5:7], dev["path_first"][11:13]
        assert a[1] - a[0] == 0 and b[1] - b[0] == 1 and (dev["seg_first"][5] == -1).all() and (dev["seg_first"][11] == -1).all()
        host = c.densify_paths(pj_d.cpu().numpy(), pl, distinct=distinct)
        assert host["rows"] == dev["rows"] and host["calls"] == dev["calls"]
        for k in ("joints", "arc", "length"):
            assert np.array_equal(bits(host[k]), bits(dev[k])), k
        for k in ("path_first", "seg_first", "seg_ok", "seg_newton"):
            assert np.array_equal(host[k], dev[k]), k


def test_dense_solution_is_solution_then_densify(roadmap_case, oracle_det):
    c, rm, _, _ = roadmap_case
    P = _oracle_problem(oracle_det, c)
    cost, idx, joints = rm.solution([0, 1], [9, 6])
    cost2, idx2, dense = rm.dense_solution(c, [0, 1], [9, 6])
    assert cost2 == cost and np.array_equal(idx, idx2)
    pj, pl = joints.cpu().numpy()[None], np.array([len(idx)], dtype=np.int32)
    same_paths(_np(dense), join(pj, pl, len(idx), oracle_segments(oracle_det, P, pj, pl)), "dense_solution")
    goal = rm.read(host=True)[1][9]
    d, cost3, idx3, dense3 = rm.dense_approximate_solution(c, [0], goal, distinct=True)
    pj, pl = rm.read(host=True)[0][idx3][None], np.array([len(idx3)], dtype=np.int32)
    same_paths(_np(dense3), join(pj, pl, len(idx3), oracle_segments(oracle_det, P, pj, pl), distinct=True), "dense_approximate_solution")


# ---- 3. more segments than a block has lanes, and ragged ----------------------------------------------------------------------------
F3, L3 = 64, 24


@pytest.fixture(scope="module")
def chain(cons):
    """near-sampling chains: the first waypoint of each path by sample_project_batch, each next one around the previous"""
    import torch

    c = cons(OBJ, 0)
    cols = [c.sample_project_batch(CHAIN_SEED, 0, F3)[0]]
    for j in range(1, L3):
        cols.append(c.sample_near_project_batch(CHAIN_SEED + j, 0, cols[-1], 0.6, F3)[0])
    pj = torch.stack(cols, dim=1).contiguous()
    rng = np.random.default_rng(3)
    pl = rng.integers(3, L3, size=F3).astype(np.int32)
    pl[:6] = [0, 1, 2, L3, L3, 2]
    return pj, _dev(pl)


@pytest.fixture(scope="module")
def chain_results(cons, chain, oracle_det):
    """per mode: the oracle's segments and the device results of both layouts (shared by cases 3 and 5)"""
    made = {}

    def get(mode):
        if mode not in made:
            c = cons(OBJ, mode)
            pj_d, pl_d = chain
            pj, pl = pj_d.cpu().numpy(), pl_d.cpu().numpy()
            segs = oracle_segments(oracle_det, _oracle_problem(oracle_det, c), pj, pl)
            res = {d: _np(c.densify_paths(pj_d, pl_d, distinct=d, chunk_states=3, round_budget=8)) for d in (False, True)}
            made[mode] = (pj, pl, segs, res)
        return made[mode]

    return get


@pytest.mark.parametrize("mode", [0, 1])
def test_ragged_chains(cons, chain, chain_results, mode):
    import torch

    c = cons(OBJ, mode)
    pj_d, pl_d = chain
    pj, pl, segs, res = chain_results(mode)
    assert F3 * (L3 - 1) == 1472 and {0, 1, 2, L3} <= set(pl.tolist()) and len(set(pl.tolist())) > 6
    # The precondition, from existing code alone (plain discrete_geodesic_batch calls with the same list length and budget): the zero-row
    # chunk — an extend call that contributes no row to its segment.  The extend step tests its round budget only behind a state it has
    # just stored (ccmp_geo_edge_body.inc, ccmp_row16_geo_body.inc: `n++` precedes the test), so no call of it is ever suspended (ok == 2)
    # with its starting state alone, whatever the seed; the calls that store nothing are continuations whose first projection is refused:
    # n_states == 1 behind a suspension.  Their Newton rounds still count.  At least one must occur.
    sel = [(f, i) for f in range(F3) for i in range(int(pl[f]) - 1)]
    frm = torch.stack([pj_d[f, i] for f, i in sel]).contiguous()
    to = torch.stack([pj_d[f, i + 1] for f, i in sel]).contiguous()
    s, n, ok, _, carry = c.discrete_geodesic_batch(frm, to, 3, want_carry=True, round_budget=8)
    suspended_alone = int(((ok == 2) & (n == 1)).sum())
    zero_row, calls = 0, 1
    for _ in range(64):
        open_ = torch.nonzero((n > 3) | (ok == 2)).flatten()
        if open_.numel() == 0:
            break
        last = (n.clamp(max=3)[open_] - 1).long()
        frm, to = s[open_, last].contiguous(), to[open_].contiguous()
        s, n, ok, _, carry = c.discrete_geodesic_batch(frm, to, 3, carry_in=carry[open_].contiguous(), want_carry=True, round_budget=8)
        zero_row += int((n == 1).sum())
        calls += 1
    print("mode %d: %d segments, %d extend calls; calls that stored no new state: %d (suspended with the starting state alone: %d)"
          % (mode, len(sel), calls, zero_row, suspended_alone))
    assert suspended_alone == 0 and zero_row >= 1 and calls == res[False]["calls"]
    for distinct in (False, True):
        same_paths(res[distinct], join(pj, pl, L3, segs, distinct=distinct), (mode, distinct))
    assert res[False]["calls"] == res[True]["calls"] > 2


# ---- 4. long, unreached segments; the two refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_long_and_unreached_segments(cons, oracle_det, mode):
    q = cons(OBJ, 0).sample_project_batch(PAIR_SEED, 0, 16)[0]  # independent uniform projected samples (the FD constraint's, for both modes)
    c = cons(OBJ, mode)
    pj_d, pl = q.reshape(8, 2, 14).contiguous(), np.full(8, 2, dtype=np.int32)
    pj = pj_d.cpu().numpy()
    segs = oracle_segments(oracle_det, _oracle_problem(oracle_det, c), pj, pl)
    oks = [s[0] for s in segs.values()]
    assert 0 in oks and 1 in oks
    got = _np(c.densify_paths(pj_d, _dev(pl), chunk_states=4))
    same_paths(got, join(pj, pl, 2, segs), mode)
    longest = max(len(s[1]) for s in segs.values())
    assert longest >= 16 and got["calls"] >= (longest - 4 + 2) // 3 + 1  # many rounds: a continuation adds three rows at most


def test_max_calls_spent_creates_nothing_and_bad_path_len_is_refused(cons, recorded):
    from closed_chain_motion_planner_amd import CcmpError, _lib

    c = cons(OBJ, 0)
    _, pj, pl, _, _ = recorded(OBJ, 0)
    pj_d, pl_d = _dev(pj), _dev(pl)
    L = _lib.lib()
    opts = _lib.CcmpDenseOpts(0, 2, 128, 1)
    h = C.c_void_p(0x1234)
    rc = L.ccmp_path_densify(c.ctx.handle, C.byref(c.problem), None, 0.0, pj_d.data_ptr(), pl_d.data_ptr(), 1, pj.shape[1], C.byref(opts), C.byref(h), None)
    assert rc == EOVERFLOW and not h.value  # a cut list never looks complete: no handle
    with pytest.raises(CcmpError) as e:
        c.densify_paths(pj_d, pl_d, chunk_states=2, max_calls=1)
    assert e.value.code == EOVERFLOW
    for bad in (pj.shape[1] + 1, -1):
        h = C.c_void_p(0x1234)
        pl_bad = _dev(np.array([bad], dtype=np.int32))
        rc = L.ccmp_path_densify(c.ctx.handle, C.byref(c.problem), None, 0.0, pj_d.data_ptr(), pl_bad.data_ptr(), 1, pj.shape[1], None, C.byref(h), None)
        assert rc == EINVAL and not h.value
        hp = np.array([bad], dtype=np.int32)
        rc = L.ccmp_path_densify_host(c.ctx.handle, C.byref(c.problem), None, 0.0, pj.ctypes.data_as(C.POINTER(C.c_double)),
                                      hp.ctypes.data_as(C.POINTER(C.c_int32)), 1, pj.shape[1], None, C.byref(h))
        assert rc == EINVAL and not h.value
    with pytest.raises(CcmpError) as e:
        c.densify_paths(pj_d, pl_d, chunk_states=1)
    assert e.value.code == EINVAL
    empty = c.densify_paths(pj_d[:0], pl_d[:0])  # F == 0: an empty result
    assert empty["rows"] == 0 and empty["calls"] == 0 and empty["path_first"].cpu().tolist() == [0]


# ---- 5. arc and length -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_arc_and_length(chain_results, mode):
    from closed_chain_motion_planner_amd import dense_arc_ref

    _, pl, _, res = chain_results(mode)
    for distinct in (False, True):
        r = res[distinct]
        arc, length = dense_arc_ref(r["joints"], r["path_first"])
        assert np.array_equal(bits(r["arc"]), bits(arc)) and np.array_equal(bits(r["length"]), bits(length)), distinct
        for f in range(F3):
            a, b = r["path_first"][f], r["path_first"][f + 1]
            assert bits(r["length"][f : f + 1])[0] == (bits(r["arc"][b - 1 : b])[0] if b > a else 0)
    ref, dis = res[False], res[True]
    assert (np.diff(ref["path_first"]) > 64).any()  # a path longer than the 64 distances a wavefront fetches at a time
    keep = distinct_of_reference(dict(rows=ref["joints"], seg_first=ref["seg_first"]))
    assert np.array_equal(bits(ref["arc"][keep]), bits(dis["arc"])) and np.array_equal(bits(ref["length"]), bits(dis["length"]))


# ---- 6. the clearance summary -----------------------------------------------------------------------------------------------------------
def test_clearance_summary(cons, chain, chain_results):
    from closed_chain_motion_planner_amd import scene as S

    c = cons(OBJ, 0)
    sc = S.ProxyValidityChecker(c).scene
    pj_d, pl_d = chain
    plain = chain_results(0)[3][False]
    clr = sc.clearance_batch(_dev(plain["joints"]))[0].cpu().numpy()  # ccmp_clearance_batch on the same rows
    pf = plain["path_first"]
    mins = np.array([clr[pf[f] : pf[f + 1]].min() for f in range(F3) if pf[f + 1] > pf[f]])
    margin = float(np.median(mins))  # chosen from the observed values: some paths are blocked and some are not
    got = _np(c.densify_paths(pj_d, pl_d, scene=sc, margin=margin, chunk_states=3, round_budget=8))
    assert np.array_equal(bits(got["joints"]), bits(plain["joints"])) and np.array_equal(bits(got["clearance"]), bits(clr))
    blocked = 0
    for f in range(F3):
        a, b = int(pf[f]), int(pf[f + 1])
        if b == a:
            assert np.isposinf(got["min_clear"][f]) and got["min_row"][f] == -1 and got["first_blocked"][f] == -1
            continue
        v = clr[a:b]
        below = np.nonzero(v < margin)[0]
        assert bits(got["min_clear"][f : f + 1])[0] == bits(np.array([v.min()]))[0] and got["min_row"][f] == a + int(np.argmin(v))
        assert got["first_blocked"][f] == (a + int(below[0]) if len(below) else -1)
        blocked += len(below) > 0
    assert 0 < blocked < F3 - 2
    # a result made without a scene has no summary to copy
    from closed_chain_motion_planner_amd import _lib

    L, h = _lib.lib(), C.c_void_p()
    pj, pl = chain_results(0)[0], chain_results(0)[1]
    assert L.ccmp_path_densify_host(c.ctx.handle, C.byref(c.problem), None, 0.0, pj.ctypes.data_as(C.POINTER(C.c_double)),
                                    pl.ctypes.data_as(C.POINTER(C.c_int32)), 2, L3, None, C.byref(h)) == 0
    one = np.zeros(2)
    rc = L.ccmp_dense_paths_copy_host(h, None, None, None, None, None, None, None, None, one.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    L.ccmp_dense_paths_destroy(h)
    assert rc == EINVAL

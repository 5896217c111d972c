"""The resident service kernel in analytic mode (option "resident" with jacobian_mode = CCMP_JAC_ANALYTIC; csrc/ccmp_resident.h,
resident_row16_kernel in csrc/ccmp_kernels_fast.hip): single-state calls and up to eight edges of discreteGeodesic / checkMotion
per request, carry_in included, without a launch on the call path — bit for bit what the launched kernels give, which the other
tests pin to the oracle's analytic mode.  "resident_served" tells a served call from one that fell back to the launch path (both
give the same bits)."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import config_path, load_roadmap

pytestmark = pytest.mark.gpu

CASES = [(64, 0, 0), (64, 0, 1), (3, 0, 0), (16, 8, 0)]  # (max_states, round_budget, check_target)
DP = C.POINTER(C.c_double)


def _constraint(obj="Wine_Bottle", mode=1, ctx=None):
    from closed_chain_motion_planner_amd import Context, KinematicChainConstraint

    ctx = ctx or Context(0)
    c = KinematicChainConstraint.from_yaml(config_path(obj), ctx=ctx)
    c.setJacobianMode(mode)
    ctx.set_option("resident_idle_ms", 200)  # no idle exit between two back-to-back calls
    return c, ctx


def _tilt(c):
    """a tilted base frame (arm 2) and a 1-ulp-off identity (arm 1): the general product, resident_row16_kernel<false>
    (tests/test_gpu_parity.py: test_general_base_frames_take_the_full_product)"""
    a, b = 0.3, -0.7
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    tilt = (Rz @ Rx).reshape(-1)
    for k in range(9):
        c.problem.base_R[9 + k] = float(tilt[k])
    c.problem.base_R[0] = float(np.nextafter(1.0, 0.0))
    c.setInitialPosition(np.array(c.problem.start_joint[:]))


CALLS_PER_STATE = 6


def _single_calls(c, xs):
    out = []
    for x in xs:
        y = x.copy()
        ok = c.project(y)
        out.append((y, ok, c.function(x).copy(), c.isSatisfied(x), c.jointValid(x), c.isSatisfied(y), c.jointValid(y)))
    return out


def _bits(a, b):
    """bit for bit — except that a NaN need only be a NaN on both sides"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def _same(a, b):
    bad = [(k, u, v) for k, (u, v) in enumerate(zip(a, b)) if not (_bits(u[0], v[0]) and u[1] == v[1] and _bits(u[2], v[2]) and u[3:] == v[3:])]
    if bad:
        print("first difference (state %d):\n  launched %r\n  resident %r" % bad[0])
    return not bad and len(a) == len(b)


def _counters(ctx):
    return ctx.get_option("resident_served"), ctx.get_option("resident_gave_up")


def _check_served(ctx, before, calls, what):
    """resident_served has risen by exactly `calls` — unless a start of the service gave up meanwhile (those calls took the launch
    path): then it has only to have risen"""
    served, gave_up = _counters(ctx)
    print("%s: resident_served +%d for %d calls, resident_gave_up +%d" % (what, served - before[0], calls, gave_up - before[1]))
    if gave_up == before[1]:
        assert served - before[0] == calls, (what, served - before[0], calls)
    else:
        assert served - before[0] > 0, (what, served, before)


def _iters(L, ctx, c, xs):
    out = []
    for x in xs:
        y, okb, it = np.zeros(14), (C.c_uint8 * 1)(), (C.c_uint16 * 1)()
        assert L.ccmp_project_host(ctx.handle, C.byref(c.problem), x.ctypes.data_as(DP), y.ctypes.data_as(DP), okb, it, 1) == 0
        out.append((int(it[0]), int(okb[0]), y.tobytes()))
    return out


@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan"])
def test_single_state_calls_through_the_analytic_service_are_bitwise_the_launched_ones(obj):
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint(obj)
    far = c.ambient_uniform_batch(0x4E5, 0, 48).cpu().numpy()
    q, ok, _ = c.project_batch(c.ambient_uniform_batch(0x4E6, 0, 512))
    near = q[ok == 1][:24].cpu().numpy() + np.random.default_rng(5).uniform(-0.05, 0.05, (24, 14))
    xs = np.concatenate([far, near, np.full((1, 14), np.nan)])
    torch.cuda.synchronize()
    assert c.problem.jacobian_mode == 1 and ctx.get_option("resident") == 0

    def both(xs, what):
        ctx.set_option("resident", 0)
        before = _counters(ctx)
        want, want_it = _single_calls(c, xs), _iters(L, ctx, c, xs[:8])
        assert _counters(ctx)[0] == before[0]  # the launch path counts nothing
        ctx.set_option("resident", 1)
        before = _counters(ctx)
        got, got_it = _single_calls(c, xs), _iters(L, ctx, c, xs[:8])
        _check_served(ctx, before, CALLS_PER_STATE * len(xs) + 8, what)
        assert _same(want, got), what
        assert want_it == got_it, what
        return want

    w1 = both(xs, obj + " analytic")
    assert any(w[1] for w in w1) and not all(w[1] for w in w1)  # projections that succeed and ones that do not
    c.setTolerance(5e-4, 2.5e-3)  # another problem through the same service: the constants travel through the mailbox
    both(xs[:16], obj + " analytic, other tolerances")
    _tilt(c)  # general base frames: the other instantiation of the kernel (one stop and one start)
    both(np.concatenate([xs[:16], xs[-9:]]), obj + " analytic, tilted base frame")
    ctx.set_option("resident", 0)
    torch.cuda.synchronize()


def _geo(L, ctx, c, frm, to, ms, budget, chk, carry_in=None):
    """ccmp_geodesic_host_ex on E edges: [(n, ok, listed rows' bytes, carry_out bytes)] per edge, and the raw arrays"""
    E = len(frm)
    frm, to = np.ascontiguousarray(frm, dtype=np.float64), np.ascontiguousarray(to, dtype=np.float64)
    st, n, okb, carry = np.full((E, ms, 14), 7.0), (C.c_int32 * E)(), (C.c_uint8 * E)(), np.zeros((E, 2))
    ci = None if carry_in is None else np.ascontiguousarray(carry_in, dtype=np.float64)
    rc = L.ccmp_geodesic_host_ex(ctx.handle, C.byref(c.problem), frm.ctypes.data_as(DP), to.ctypes.data_as(DP), E, ms, st.ctypes.data_as(DP), n, okb,
                                 None if ci is None else ci.ctypes.data_as(DP), carry.ctypes.data_as(DP), budget, chk)
    assert rc == 0, rc
    out = [(int(n[e]), int(okb[e]), st[e, :min(int(n[e]), ms)].tobytes(), carry[e].tobytes()) for e in range(E)]
    return out, st, carry


def _grouped(L, ctx, c, frm, to, group, ms, budget, chk):
    out, calls = [], 0
    for k in range(0, len(frm), group):
        out += _geo(L, ctx, c, frm[k:k + group], to[k:k + group], ms, budget, chk)[0]
        calls += 1
    return out, calls


def _roadmap_edges():
    nodes, edges = load_roadmap("Wine_Bottle")
    assert len(edges) == 28
    return np.array([nodes[a] for a, b in edges]), np.array([nodes[b] for a, b in edges])


def test_several_edges_per_request_are_bitwise_the_launched_ones():
    """the 28 directed edges of the recorded Wine_Bottle roadmap in groups of 1, 2, 3, 4, 5 and 8 edges per call: states, counts,
    flags and carries of the service are those of the launch path, one request per call; the sample holds every kind of ending
    (arrivals, a give-up, edges within delta at once, lists too short, targets that fail isSatisfied, a round budget spent)"""
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint()
    frm, to = _roadmap_edges()
    launched = {}
    for ms, budget, chk in CASES:
        ctx.set_option("resident", 0)
        want, _ = _grouped(L, ctx, c, frm, to, 28, ms, budget, chk)
        launched[(ms, budget, chk)] = want
        for group in (1, 2, 3, 4, 5, 8):
            ctx.set_option("resident", 0)
            before = _counters(ctx)
            off, calls = _grouped(L, ctx, c, frm, to, group, ms, budget, chk)
            assert _counters(ctx)[0] == before[0]
            ctx.set_option("resident", 1)
            before = _counters(ctx)
            on, calls = _grouped(L, ctx, c, frm, to, group, ms, budget, chk)
            _check_served(ctx, before, calls, "roadmap edges, %d per call, case %r" % (group, (ms, budget, chk)))  # one per call, not per edge
            assert [w[:2] for w in off] == [g[:2] for g in on], (group, ms, budget, chk)
            assert off == on, (group, ms, budget, chk)
            assert off == want, (group, ms, budget, chk)  # (and the grouping does not matter)
    ctx.set_option("resident", 0)
    plain, chk, short, budget = launched[CASES[0]], launched[CASES[1]], launched[CASES[2]], launched[CASES[3]]
    print("max_states 64: arrived %d, gave up %d, list lengths %d..%d, within delta at once %d; max_states 3: overflow %d; check_target: refused %d; "
          "budget 8: suspended %d" % (sum(w[1] == 1 for w in plain), sum(w[1] == 0 for w in plain), min(w[0] for w in plain), max(w[0] for w in plain),
                                      sum(w[0] == 1 and w[1] == 1 for w in plain), sum(w[0] == 4 for w in short),
                                      sum(w[1] == 0 and w[0] == 1 for w in chk), sum(w[1] == 2 for w in budget)))
    assert any(w[1] == 1 and w[0] > 1 for w in plain)      # arrives
    assert any(w[1] == 0 and w[0] > 1 for w in plain)      # gives up on the way
    assert any(w[0] == 1 and w[1] == 1 for w in plain)     # within delta at once
    assert max(w[0] for w in plain) >= 8 and all(w[0] <= 64 for w in plain)
    assert any(w[0] == 4 for w in short)                   # the list is full: n = max_states + 1
    assert any(w[1] == 0 and w[0] == 1 for w in chk) and any(w[1] == 1 for w in chk)  # a target that fails isSatisfied, and one that passes
    assert any(w[1] == 2 for w in budget)                  # the round budget spent between two states
    torch.cuda.synchronize()


def test_continuations_with_carry_in_go_through_the_service():
    """the roadmap edges whose list of three states overflows, continued with carry_in — through the service, five edges per
    request — until done: the rows of one uninterrupted launched traversal with 64 states, bit for bit"""
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint()
    frm, to = _roadmap_edges()
    ctx.set_option("resident", 0)
    whole, st_whole, _ = _geo(L, ctx, c, frm, to, 64, 0, 0)
    first, st3, carry3 = _geo(L, ctx, c, frm, to, 3, 0, 0)
    over = [e for e in range(28) if first[e][0] == 4]
    assert len(over) >= 5
    ctx.set_option("resident", 1)
    before = _counters(ctx)
    rows = {e: [st3[e, k].copy() for k in range(3)] for e in over}
    carry = {e: carry3[e].copy() for e in over}
    ok_end, live, calls = {}, list(over), 0
    for _ in range(64):  # (a list of at most 64 states grows by two per call)
        if not live:
            break
        nxt = []
        for k in range(0, len(live), 5):
            grp = live[k:k + 5]
            out, st, co = _geo(L, ctx, c, np.array([rows[e][-1] for e in grp]), to[grp], 3, 0, 0, carry_in=np.array([carry[e] for e in grp]))
            calls += 1
            for j, e in enumerate(grp):
                n, okb = out[j][0], out[j][1]
                rows[e] += [st[j, r].copy() for r in range(1, min(n, 3))]  # row 0 repeats the state the continuation started from
                carry[e] = co[j].copy()
                if n <= 3 and okb != 2:
                    ok_end[e] = okb
                else:
                    nxt.append(e)
        live = nxt
    assert not live
    _check_served(ctx, before, calls, "continuations")
    ctx.set_option("resident", 0)
    for e in over:
        n, okb = whole[e][0], whole[e][1]
        assert n <= 64
        assert len(rows[e]) == n and ok_end[e] == okb, (e, len(rows[e]), n, ok_end[e], okb)
        assert np.array(rows[e]).tobytes() == st_whole[e, :n].tobytes(), e
    torch.cuda.synchronize()


def _growth_edges(c, seed=0x4EA):
    """as tests/test_gpu_resident.py builds them: projected samples -> a sample near each at 0.6, one far pair, one target off the
    manifold"""
    import torch

    q, ok, _ = c.project_batch(c.ambient_uniform_batch(seed, 0, 2048))
    good = q[ok == 1].cpu().numpy()
    frm = good[:25]
    to = np.array([c.sample_near_project_batch(seed + 1, 0, torch.as_tensor(frm).cuda(), 0.6, len(frm), want_iters=False)[0].cpu().numpy()][0])
    to[3] = good[100]
    to[4] = to[4] + 0.3
    torch.cuda.synchronize()
    return frm, to


def test_growth_shaped_edges_five_per_request():
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint()
    frm, to = _growth_edges(c)
    kinds = set()
    for ms, budget, chk in CASES:
        ctx.set_option("resident", 0)
        off, calls = _grouped(L, ctx, c, frm, to, 5, ms, budget, chk)
        ctx.set_option("resident", 1)
        before = _counters(ctx)
        on, calls = _grouped(L, ctx, c, frm, to, 5, ms, budget, chk)
        _check_served(ctx, before, calls, "growth-shaped edges, case %r" % ((ms, budget, chk),))
        assert [w[:2] for w in off] == [g[:2] for g in on], (ms, budget, chk)
        assert off == on, (ms, budget, chk)
        kinds |= {w[1] for w in off}
    ctx.set_option("resident", 0)
    assert {0, 1, 2} <= kinds
    torch.cuda.synchronize()


def test_routing_of_everything_else_is_left_alone():
    """nine edges, or lists longer than the mailbox holds, in analytic mode, and five edges in the reference arithmetic keep the
    launch path (the same bits, nothing served); one edge in the reference arithmetic is served by the FD service as before"""
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint()
    frm, to = _roadmap_edges()
    fd, _ = _constraint(mode=0, ctx=ctx)
    for what, con, f, t, ms, served in (("analytic, E = 9", c, frm[:9], to[:9], 64, 0), ("analytic, max_states = 65", c, frm[:3], to[:3], 65, 0),
                                        ("FD, E = 5", fd, frm[:5], to[:5], 64, 0), ("FD, E = 1", fd, frm[:1], to[:1], 64, 1),
                                        ("analytic, E = 8", c, frm[:8], to[:8], 64, 1)):
        ctx.set_option("resident", 0)
        off = _geo(L, ctx, con, f, t, ms, 0, 0)[0]
        ctx.set_option("resident", 1)
        before = _counters(ctx)
        on = _geo(L, ctx, con, f, t, ms, 0, 0)[0]
        assert off == on, what
        if served:
            _check_served(ctx, before, served, what)
        else:
            assert _counters(ctx)[0] == before[0], what
    ctx.set_option("resident", 0)
    torch.cuda.synchronize()


def test_mode_changes_and_coexistence_with_batches_and_synchronisation():
    """one context, service on: problems of the two modes in turn (each change stops one kernel and starts the other), a
    workspace-growing batch in between (the library stops the service before its hipFree), a device-wide synchronise behind a
    resident call (bounded by the idle time) — the same bits throughout"""
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    ca, ctx = _constraint()
    cf, _ = _constraint(mode=0, ctx=ctx)
    ctx.set_option("resident_idle_ms", 20)
    xs = ca.ambient_uniform_batch(0x4E7, 0, 8).cpu().numpy()
    frm, to = _roadmap_edges()
    torch.cuda.synchronize()

    def round_of_calls():
        out = []
        for k in range(24):
            con = cf if k % 2 else ca
            out.append(_single_calls(con, xs[k % 8: k % 8 + 1])[0])
            if k % 4 == 0:
                out.append(_geo(L, ctx, ca, frm[k:k + 5], to[k:k + 5], 16, 0, 1)[0])
            if k % 4 == 1:
                out.append(_geo(L, ctx, cf, frm[k:k + 1], to[k:k + 1], 16, 0, 1)[0])
        return out

    def same(a, b):
        return len(a) == len(b) and all((u == v) if isinstance(u, list) else _same([u], [v]) for u, v in zip(a, b))

    ctx.set_option("resident", 0)
    want = round_of_calls()
    ctx.set_option("resident", 1)
    before = _counters(ctx)
    assert same(want, round_of_calls())
    for B in (20000, 70000):  # each larger than the last: the buffers grow under a live service
        q = ca.ambient_uniform_batch(0x4E8, 0, B)
        qo, ok, it = ca.project_batch(q)
        h = ca.project_host(q[:3000].cpu().numpy())
        torch.cuda.synchronize()
        assert np.array_equal(h[0].view(np.uint64), qo[:3000].cpu().numpy().view(np.uint64))
        assert same(want, round_of_calls())
    y = xs[0].copy()
    ca.project(y)
    t0 = time.perf_counter()
    torch.cuda.synchronize()
    waited = time.perf_counter() - t0
    assert waited < 2.0, waited
    assert same(want, round_of_calls())
    time.sleep(0.1)  # idle exit on its own
    assert same(want, round_of_calls())
    served, gave_up = _counters(ctx)
    print("mode changes: resident_served +%d, resident_gave_up %d, synchronise behind a resident call %.1f ms" % (served - before[0], gave_up, waited * 1e3))
    assert served > before[0]
    ctx.set_option("resident", 0)
    torch.cuda.synchronize()


def test_analytic_resident_latency_is_reported():
    """median host-to-host latency, launched against resident, interleaved (off, on, off, on), median per pass, minimum of the
    passes.  The launched figure is what these calls cost without this service: they fell back to it.  Measured on one MI355X
    (profiles/r09_resident_analytic_ab.log): see DESIGN.md 5.6."""
    import torch

    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, ctx = _constraint()
    q, ok, _ = c.project_batch(c.ambient_uniform_batch(0x4E6, 0, 1024))
    near = q[ok == 1][:64].cpu().numpy() + np.random.default_rng(7).uniform(-0.05, 0.05, (64, 14))
    far = c.ambient_uniform_batch(0xC1, 0, 64).cpu().numpy()
    frm, to = _growth_edges(c)
    torch.cuda.synchronize()
    groups = (1, 2, 3, 4, 5, 8)
    res = {}
    for on in (0, 1, 0, 1):
        ctx.set_option("resident", on)
        for name, xs, fn in (("project(uniform)", far, c.project), ("project(near)", near, c.project), ("isSatisfied", near, c.isSatisfied),
                             ("function", near, c.function)):
            ts = []
            for x in xs:
                y = x.copy()
                t0 = time.perf_counter()
                fn(y)
                ts.append(time.perf_counter() - t0)
            res.setdefault((name, on), []).append(float(np.median(ts[8:]) * 1e6))
        for E in groups:
            st, n, okb, carry = np.zeros((E, 64, 14)), (C.c_int32 * E)(), (C.c_uint8 * E)(), np.zeros((E, 2))
            ts = []
            for rep in range(3):
                for k in range(0, 25 - E + 1, max(1, E // 2)):
                    a, b = np.ascontiguousarray(frm[k:k + E]), np.ascontiguousarray(to[k:k + E])
                    t0 = time.perf_counter()
                    L.ccmp_geodesic_host_ex(ctx.handle, C.byref(c.problem), a.ctypes.data_as(DP), b.ctypes.data_as(DP), E, 64, st.ctypes.data_as(DP), n, okb, None,
                                            carry.ctypes.data_as(DP), 0, 1)
                    ts.append(time.perf_counter() - t0)
            res.setdefault(("checkMotion x %d" % E, on), []).append(float(np.median(ts[4:]) * 1e6))
    ctx.set_option("resident", 0)
    names = ["project(uniform)", "project(near)", "isSatisfied", "function"] + ["checkMotion x %d" % E for E in groups]
    for name in names:
        print("analytic %-18s launched %6.1f us   resident %6.1f us" % (name, min(res[(name, 0)]), min(res[(name, 1)])))
    print("resident_gave_up %d" % ctx.get_option("resident_gave_up"))
    assert min(res[("isSatisfied", 1)]) < min(res[("isSatisfied", 0)])
    for E in (2, 3, 4, 5, 8):  # every several-edge size that is routed to the service has to be faster there: that is its only purpose
        assert min(res[("checkMotion x %d" % E, 1)]) < min(res[("checkMotion x %d" % E, 0)]), E
    torch.cuda.synchronize()

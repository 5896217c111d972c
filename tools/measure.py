#!/usr/bin/env python3
"""One parametrised timing harness for the GPU box (development aid; bench.py is the contract).

    python tools/measure.py sizes   [obj] [--schedules]    run time against batch size (1 .. 1048576), default policy;
                                                           --schedules adds latency-kernel-only and throughput-only columns
    python tools/measure.py single                          latency of the reference-signature single-state calls
    python tools/measure.py geodesic [E ...] [--analytic]   batched discreteGeodesic (near-neighbour edges); --analytic: in analytic mode,
                                                           lists of 16 with and without the round budget, lists of 64
    python tools/measure.py geodesic --scene [--analytic] [E ...]   the same with the default skeleton scene's pre-filter (margin -3 cm):
                                                           the mirror's host loop (one clearance call per listed state) against its
                                                           device path, and the plain call against the scene call (lists of 16, budget 128)
    python tools/measure.py analytic                        analytic mode against batch size and waves per CU
    python tools/measure.py host                            PCIe-inclusive rate of ccmp_project_host (pageable / pinned)
    python tools/measure.py sharded [n_gpus [B]]            one process, n GPUs, RCCL all-gather inside the C ABI: per-GPU stream times
    python tools/measure.py sampler                         project_batch vs the fused sampler
    python tools/measure.py soak                            25 repeats of the default policy, outputs compared bit for bit
    python tools/measure.py soak_resident [N] [--analytic]  N states as single calls through the resident service kernel against the batched kernels
                                                            (--analytic: analytic mode, and five checkMotion edges per request instead of one)
    python tools/measure.py scout                           FP32 scout's predictions against the true iteration counts
    python tools/measure.py roadmap [reps]                  the device-resident roadmap store: host-form single-query k-NN against ccmp_knn_host, the object
                                                           metric's many-query kernel against the joint metric's (k = 5 and 16), appends, pose derivation
    python tools/measure.py mirror [calls] [warm]           host wall time of the Python mirror's own wrappers in the planner's per-vertex loop (numpy append,
                                                           nearest_k and read, device connect) on a store of 1 024 vertices: median of `calls` calls, one JSON line
    python tools/measure.py connect [reps]                  the connection step: ccmp_knn_batch against FP64 torch distances + torch.topk (throughput shape and
                                                           single queries), ccmp_connect_batch against torch k-NN + gather + ccmp_geodesic_batch_ex, both
                                                           contenders alternating in one process, device events, medians with their spread
    python tools/measure.py ik [reps_a] [reps_b] [T_b]      pose-targeted IK (growTree's sampleCalibGoal): (a) one pose x 5 seeds x 14 restarts through the host
                                                           form, (b) T_b = 4096 poses x 5 x 14 through the device form, each against ccmp_pose_ik_ref on one
                                                           thread on the same inputs, alternating in one process; histogram of rounds, idle lane-rounds
    python tools/measure.py ik --scene [reps_a] [reps_b] [T_b]  the vetted IK (ccmp_pose_ik_vetted_*) against today's route, ccmp_pose_ik_* plus one ccmp_clearance_*
                                                           call on the answers, on the default skeleton scene at -0.03, same two shapes: time, targets solved
                                                           and clear by each route, the vet kernel's share of the call and its registers / LDS / occupancy
    python tools/measure.py object [reps_a] [reps_b] [G_b]  the head of growTree (object-pose proposal + mesh test): (a) propose with G = 1, 2 attempts, a dumbbell of
                                                           ~1 000 triangles against the six fixture boxes through the host form, (b) G_b = 4096 through the device form,
                                                           (c) valid on 4096 poses of a ~8 600-triangle sphere, each against the *_ref form on one thread on the same inputs
    python tools/measure.py graph [reps]                    the roadmap graph (growTree's tail, closestFromGoal's scan, labels): (a) commit with Q = 1, k = 5, lists of 64
                                                           through the host form, (b) Q = 4096 through the device form, (c) closest and (d) a one-edge label update at
                                                           N = 65 536, each against the *_ref form on one thread on the same inputs; writes profiles/roadmap_graph.md
    python tools/measure.py path [reps]                     shortest paths on the device roadmap (the solution step): N = 65 536 with ~65 000 edges and N = 2 000 with 5 000,
                                                           F = 1 and F = 64, the device form (events) and the host form (wall clock) against ccmp_graph_shortest_paths_ref on
                                                           one thread, the rounds each phase took, and the full round trip (read_edges_host + _ref + re-upload of the rows
                                                           against shortest_paths with the rows left on the device); writes profiles/roadmap_path.md
    python tools/measure.py dense [reps]                    dense solution paths (PathGeometric::interpolate): ccmp_path_densify against discrete_geodesic_batch +
                                                           continue_geodesics + the host join + the upload of the joined rows, one path and 64 paths of 32 waypoints,
                                                           both Jacobian modes, the extend calls made and the bytes that crossed to the host; writes profiles/dense_path.md
    python tools/measure.py shortcut [reps]                 shortcut solution paths (vertex removal): ccmp_path_shortcut against check_target extend calls over all pairs, their
                                                           continuation and the selection in numpy, 1 and 64 paths of 32 waypoints; writes profiles/shortcut.md
    python tools/measure.py smooth [reps] [file.npz]        smooth solution paths (B-spline passes on the manifold): ccmp_path_smooth, three passes on 1 and 64 paths of 32
                                                           waypoints, both Jacobian modes, the extend calls made and the bytes read on the host; writes profiles/smooth.md
    python tools/measure.py retime [reps]                   resample and time stamps: ccmp_path_resample and ccmp_path_timestamps on the smooth measurement's inputs,
                                                           continued (1 and 64 paths), the kind counts; the recorded paths' durations on the CPU; writes profiles/retime.md
    python tools/measure.py setpoints [reps]                setpoints and the execution audit: ccmp_path_setpoints at 1 ms on the retime measurement's inputs, continued
                                                           (1 and 64 paths); the recorded paths' five peaks and stretch from the library; writes profiles/setpoints.md
    python tools/measure.py fit [reps]                      time stamps fitted to the limits at the controller's rate: ccmp_path_fit_timestamps at 1 ms on the retime
                                                           measurement's inputs, continued (1 and 64 paths), beside the loop a caller would write without it
                                                           (ccmp_path_setpoints, copy qd out, dilate on the host, repeat), the same stamps bit for bit; the recorded
                                                           paths' passes and durations beside the uniform stretch; writes profiles/fit.md
    python tools/measure.py jerk [reps]                     jerk-bounded setpoints: first, on one host core, the plain-Python restatement on the recorded paths (the unfiltered
                                                           jerk ratio, the chosen windows at 1 and 4 ms); then ccmp_path_jerk_setpoints at 1 ms on the setpoints measurement's
                                                           inputs (1 and 64 paths) beside the loop a caller would write without it (ccmp_path_setpoints, copy qd out, numpy
                                                           windows); the recorded paths' windows and six peaks, without and behind the fit; writes profiles/jerk.md
    python tools/measure.py plan [cycles]                   the planner's loop on the store (ccmp_plan_*): the three shipped configs at width 1, 8, 32 and 128 for `cycles`
                                                           (64) cycles each — status, cycles, vertices, edges, the counters and wall time —, the same towards a goal that one
                                                           motion does not reach, beside the same cycles BY HAND over the mirror's calls (tests/plan_cases.py: HandPlan, what a
                                                           caller can write without the unit) with its host reads, and which branches six cycles reach at width 1, 5, 64 and 65;
                                                           writes profiles/plan.md
    python tools/measure.py rrtc [cpu] [out.md]             RRT-Connect on the store (ccmp_rrtc_*): the CPU figure of its difference (a) from OMPL (the oracle's first steps beyond 0.2),
                                                           nearest-in-tree beside the k-NN with k = 1 at 10^3 .. 10^6 rows, time per cycle at width 1, 32, 256 beside the loop by hand,
                                                           cycles and vertices to SOLVED per range beside Plan, the densify share; `cpu`: the CPU figure alone; writes profiles/rrtc.md
    python tools/measure.py smooth_restate <file.npz> [n]  the plain-Python restatement on one host core on the inputs `smooth` wrote, compared with its results
    python tools/measure.py run <workload> [reps]           a fixed workload for rocprofv3 (tools/profile.sh):
                                                           c3 | flat4096 | mid<B> | flat1 | geodesic[<E>] | geodesic_analytic[<E>] | analytic[<B>] | stefan |
                                                           stefan_tight | calibrated | clearance
"""
import ctypes as C
import sys
import time

import numpy as np
import torch

import os
if len(sys.argv) > 1 and sys.argv[1] == "scout":
    os.environ.setdefault("CCMP_LIBRARY", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "closed_chain_motion_planner_amd", "lib", "libccmp_debug.so"))  # reads the scout's predictions: a hook of include/ccmp_debug.h
sys.path.insert(0, ".")
from closed_chain_motion_planner_amd import Context, KinematicChainConstraint, _lib  # noqa: E402

CFG = "tests/golden/config/%s.yaml"


def timed(fn, reps=3):
    """best of `reps`, HIP events on the launch stream"""
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def near_edges(c, E, seed=0x6E0, dist=0.6):
    """growTree-shaped edges: a valid projected state -> a projected sampleUniformNear state within `dist` per joint"""
    q, ok, _, _ = c.sample_project_batch(seed, 0, 8 * E, want_iters=False)
    frm = q[ok == 1][:E].contiguous()
    to, _, _, _ = c.sample_near_project_batch(seed + 1, 0, frm, dist, E, want_iters=False)
    return frm, to


def sizes(argv):
    obj = next((a for a in argv if not a.startswith("-")), "Wine_Bottle")
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
    variants = [("default", None)]
    if "--schedules" in argv:
        variants += [("latency-only", (2, 0)), ("throughput-only", (0, 0))]
    for B in (1, 64, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576):
        q = c.ambient_uniform_batch(0xC2 if B <= 16384 else 0xC3, 0, B)
        out = torch.empty_like(q)
        res = []
        for name, sched in variants:
            if sched is None:
                ctx.set_schedule(1)
            else:
                if name == "latency-only" and B > 65536:
                    continue
                ctx.set_schedule(*sched)
            ms = timed(lambda: c.project_batch(q, out=out), reps=3 if B > 65536 else 5)
            res.append("%s %8.3f ms (%.3e/s)" % (name, ms, B / ms * 1e3))
        ctx.set_schedule(1)
        print("%s B=%-8d " % (obj, B) + "   ".join(res), flush=True)


def single(argv):
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    q = c.ambient_uniform_batch(1, 0, 64).cpu().numpy()
    for name, fn in (("project", c.project), ("function", c.function), ("isSatisfied", c.isSatisfied), ("jointValid", c.jointValid)):
        ts = []
        for i in range(64):
            x = q[i].copy()
            t0 = time.perf_counter()
            fn(x)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[4:]) * 1e6
        print("%-12s median %.1f us  p90 %.1f us  min %.1f us" % (name, np.median(ts), np.percentile(ts, 90), ts.min()))
    x0 = np.array(c.problem.start_joint[:])
    ts = []
    for i in range(40):  # near-manifold projections (the geodesic regime): few Newton iterations
        x = x0 + 0.02 * np.sin(np.arange(14) + i)
        t0 = time.perf_counter()
        c.project(x)
        ts.append(time.perf_counter() - t0)
    print("project near the manifold: median %.1f us" % (np.median(np.array(ts[4:])) * 1e6))
    # analytic mode, launched against the resident service (option "resident"): interleaved passes, median per pass, minimum of the passes
    c.setJacobianMode(1)
    ctx.set_option("resident_idle_ms", 200)
    near = np.array([x0 + 0.02 * np.sin(np.arange(14) + i) for i in range(64)])
    res = {}
    for on in (0, 1, 0, 1):
        ctx.set_option("resident", on)
        for name, xs, fn in (("project(uniform)", q, c.project), ("project(near)", near, c.project), ("function", near, c.function),
                             ("isSatisfied", near, c.isSatisfied), ("jointValid", near, c.jointValid)):
            ts = []
            for x in xs:
                y = x.copy()
                t0 = time.perf_counter()
                fn(y)
                ts.append(time.perf_counter() - t0)
            res.setdefault((name, on), []).append(float(np.median(ts[8:]) * 1e6))
    print("analytic mode, served by the resident service: %d requests" % ctx.get_option("resident_served"))
    ctx.set_option("resident", 0)
    c.setJacobianMode(0)
    for name in ("project(uniform)", "project(near)", "function", "isSatisfied", "jointValid"):
        print("analytic %-17s launched %6.1f us   resident %6.1f us" % (name, min(res[(name, 0)]), min(res[(name, 1)])))


def geodesic(argv):
    """batched extend step: the call with lists of 16 and of 64 states, the edges that did not fit, and the complete
    operation (continuation of those edges until every list is whole)"""
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    analytic = "--analytic" in argv
    if "--scene" in argv:
        return geodesic_scene(c, analytic, [int(a) for a in argv if not a.startswith("--")] or [5, 16384])
    shapes = ((16, 128), (64, 0))  # bench.py's first pass: lists of 16 states, 128 Newton rounds per edge; lists of 64
    if analytic:  # the edges are drawn in the default mode (the same edges as without the switch), then traversed in analytic mode
        shapes = ((16, 128), (16, 0), (64, 0))
    for E in [int(a) for a in argv if not a.startswith("--")] or [5, 64, 1024, 16384]:
        frm, to = near_edges(c, E)
        if analytic:
            c.setJacobianMode(1)
        row = []
        for cap, budget in shapes:
            ms = timed(lambda: c.discrete_geodesic_batch(frm, to, cap, want_carry=True, round_budget=budget), reps=3)
            st, n, okg, its, carry = c.discrete_geodesic_batch(frm, to, cap, want_carry=True, round_budget=budget)
            over = int(((n > cap) | (okg == 2)).sum())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = c.discrete_geodesic_batch(frm, to, cap, want_carry=True, round_budget=budget)
            whole = c.continue_geodesics(to, r[0], r[1], r[2], r[3], r[4], cap, round_budget=budget)
            torch.cuda.synchronize()
            ms_all = (time.perf_counter() - t0) * 1e3
            # Newton rounds of the longest edge's serial chain in this call: its updates plus one per projection (its stored states
            # after `from`, and the state that ended it)
            rounds = int((its + n.clamp(max=cap)).max().item())
            row.append("lists of %d, budget %d: %.3f ms, %d edges did not fit, %.3e complete edges/s, longest edge %d rounds; "
                       "everything continued to the end: %.2f ms" % (cap, budget, ms, over, (E - over) / ms * 1e3, rounds, ms_all))
        print("E=%-6d %s%s | mean states %.2f (first %d), reached %.3f, Newton iterations per edge %.1f"
              % (E, "analytic mode: " if analytic else "", "; ".join(row), n.clamp(max=cap).float().mean().item(), cap, (okg == 1).float().mean().item(),
                 its.float().mean().item()), flush=True)
        if analytic and E <= 8:  # the host ABI on these edges (growTree's shape), launched against the resident service
            L, dp = _lib.lib(), C.POINTER(C.c_double)
            fh, th = np.ascontiguousarray(frm.cpu().numpy()), np.ascontiguousarray(to.cpu().numpy())
            st, nn, okb, cr = np.zeros((E, 64, 14)), (C.c_int32 * E)(), (C.c_uint8 * E)(), np.zeros((E, 2))
            ctx.set_option("resident_idle_ms", 200)
            res = {}
            for on in (0, 1, 0, 1):
                ctx.set_option("resident", on)
                ts = []
                for _ in range(72):
                    t0 = time.perf_counter()
                    L.ccmp_geodesic_host_ex(ctx.handle, C.byref(c.problem), fh.ctypes.data_as(dp), th.ctypes.data_as(dp), E, 64, st.ctypes.data_as(dp), nn, okb,
                                            None, cr.ctypes.data_as(dp), 0, 1)
                    ts.append(time.perf_counter() - t0)
                res.setdefault(on, []).append(float(np.median(ts[8:]) * 1e6))
            ctx.set_option("resident", 0)
            print("E=%-6d analytic mode, ccmp_geodesic_host_ex (lists of 64, checkMotion): launched %.1f us   resident %.1f us" % (E, min(res[0]), min(res[1])), flush=True)
        c.setJacobianMode(0)


def geodesic_scene(c, analytic, sizes_):
    """the extend step with the proxy pre-filter (default skeleton scene, margin -3 cm): up to 64 edges through the mirror
    (space.jy_ProjectedStateSpace, lists of 64) — host loop (isValid hidden in a lambda: the unfiltered traversal, then one
    ccmp_clearance_host per listed state) against the device path (isValid = the checker's bound isValid: the scene call) — and
    for every size the device calls alone, lists of 16 and a budget of 128 rounds: plain against scene"""
    from closed_chain_motion_planner_amd.scene import ProxyValidityChecker
    from closed_chain_motion_planner_amd.space import jy_ProjectedStateSpace

    for E in sizes_:
        frm, to = near_edges(c, E)
        if analytic:
            c.setJacobianMode(1)
        chk = ProxyValidityChecker(c)
        row = []
        if E <= 64:
            f, t = frm.cpu().numpy(), to.cpu().numpy()
            for name, valid in (("host loop", lambda x: chk.isValid(x)), ("device path", chk.isValid)):
                sp = jy_ProjectedStateSpace(c, isValid=valid)
                sp.discreteGeodesicBatch(f, t, False)
                ts = []
                for _ in range(30):
                    t0 = time.perf_counter()
                    sp.discreteGeodesicBatch(f, t, False)
                    ts.append(time.perf_counter() - t0)
                row.append("mirror %s %.3f ms" % (name, np.median(ts) * 1e3))
        plain = timed(lambda: c.discrete_geodesic_batch(frm, to, 16, want_carry=True, round_budget=128), reps=7)
        scene = timed(lambda: c.discrete_geodesic_scene_batch(frm, to, chk.scene, chk.margin, 16, want_carry=True, round_budget=128), reps=7)
        st, n, ok, its, bl, carry = c.discrete_geodesic_scene_batch(frm, to, chk.scene, chk.margin, 16, want_carry=True, round_budget=128)
        tested = int((n.clamp(max=16) - 1).sum().item() + bl.sum().item())
        row.append("device call, lists of 16, budget 128: plain %.3f ms, scene %.3f ms (%d states tested, %d edges blocked)"
                   % (plain, scene, tested, int(bl.sum().item())))
        print("E=%-6d %s%s" % (E, "analytic mode: " if analytic else "", "; ".join(row)), flush=True)
        c.setJacobianMode(0)


_ANALYTIC = ("analytic_small_batch", "analytic_waves_per_cu", "analytic_handover")


def analytic(argv):
    """analytic mode: run time against batch size — the latency kernel alone ('lat'), the lane-pair kernel alone (h0) and with
    its hand-over to the latency kernel at <= h samples per wavefront, for w wavefronts per CU; argv: sizes"""
    ctx = Context(0)
    sizes_ = [int(a) for a in argv] or [1024, 4096, 8192, 16384, 32768, 65536, 262144, 2097152]
    shapes = [(12, 0), (12, 4), (12, 8), (12, 12), (12, 16), (12, 24), (8, 8), (10, 8)]
    for obj in ("Wine_Bottle", "stefan"):
        c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        c.setJacobianMode(1)
        for B in sizes_:
            q = c.ambient_uniform_batch(0xC3, 0, B)
            out = torch.empty_like(q)
            res = []
            if B <= 65536:
                ctx.set_option("analytic_small_batch", 1 << 40)
                res.append("lat %.3f" % timed(lambda: c.project_batch(q, out=out), reps=7))
            ctx.set_option("analytic_small_batch", 0)
            for w, h in shapes:
                ctx.set_option("analytic_waves_per_cu", w)
                ctx.set_option("analytic_handover", h)
                res.append("w%d h%d %.3f" % (w, h, timed(lambda: c.project_batch(q, out=out), reps=7)))
            for name in _ANALYTIC:
                ctx.set_option(name, _lib.get_option(None, name))
            ms = timed(lambda: c.project_batch(q, out=out), reps=7)
            print("analytic %s B=%-8d DEFAULT %7.3f ms (%.3e/s) | " % (obj, B, ms, B / ms * 1e3) + "  ".join(res), flush=True)


def host(argv):
    ctx = Context(0)
    L = _lib.lib()
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    B = 262144
    q = c.ambient_uniform_batch(0xC3, 0, B).cpu()
    for name, pin in (("pageable", False), ("pinned", True)):
        mk = (lambda t: t.pin_memory()) if pin else (lambda t: t)
        qi, qo = mk(q.clone()), mk(torch.empty_like(q))
        ok, it = mk(torch.empty(B, dtype=torch.uint8)), mk(torch.empty(B, dtype=torch.int16))
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            rc = L.ccmp_project_host(ctx.handle, C.byref(c.problem), C.cast(qi.data_ptr(), C.POINTER(C.c_double)),
                                     C.cast(qo.data_ptr(), C.POINTER(C.c_double)), C.cast(ok.data_ptr(), C.POINTER(C.c_uint8)),
                                     C.cast(it.data_ptr(), C.POINTER(C.c_uint16)), B)
            ts.append(time.perf_counter() - t0)
            assert rc == 0
        ms = np.median(ts[1:]) * 1e3
        print("%-9s host buffers: %.2f ms per 262144 -> %.2e projections/s (device-resident: bench.py)" % (name, ms, B / ms * 1e3))


def sharded(argv):
    """one process, every visible GPU (ccmp_comm_* + ccmp_sample_project_sharded: the reference's shape, RCCL inside the C
    ABI): wall time per call, per-GPU stream time of the shard's kernels and of the all-gather behind them, and the
    identity of the gathered valid states with those of the same samples on GPU 0 alone"""
    from closed_chain_motion_planner_amd import Communicator

    n = int(argv[0]) if argv else torch.cuda.device_count()
    B = int(argv[1]) if len(argv) > 1 else 262144 * n
    ctxs = [Context(g) for g in range(n)]
    comm = Communicator(ctxs)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctxs[0])
    c.sample_project_sharded(0xC5, 0, B, comm, want_full=False)  # communicator and workspaces
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        valid, counts, _ = c.sample_project_sharded(0xC5, 0, B, comm, want_full=False)
        ts.append(time.perf_counter() - t0)
    k, g = comm.last_timing()
    print("%d GPUs, %d samples: %.2f ms per call (host wall, upload-free sampler form) -> %.3e projections/s" % (n, B, min(ts) * 1e3, B / min(ts)))
    print("  per-GPU kernel ms:", " ".join("%.2f" % v for v in k), "| all-gather ms behind them:", " ".join("%.3f" % v for v in g))
    print("  valid states per GPU:", counts)
    probe = 4096
    vp, cp, _ = c.sample_project_sharded(0xC5, 0, probe, comm, want_full=False)
    q, ok, _, _ = c.sample_project_batch(0xC5, 0, probe, want_iters=False)
    alone = q[ok == 1].cpu().numpy()
    print("  4096-sample probe: gathered == one GPU alone, bit for bit: %s (%d valid)"
          % (bool(alone.shape == np.asarray(vp).shape and np.array_equal(alone.view(np.uint64), np.asarray(vp).view(np.uint64))), len(alone)))
    comm.close()


def afterload(argv):
    """Does a latency-bound batch (4 096 / 32 768 samples: the serial chain of its longest sample) run slower right behind a
    saturated launch?  bench.py times its secondaries behind 20 C3 steps (0.33 s of FP64 at the power limit: the chip holds
    2.27 GHz there, 2.4 idle).  Mean of 10 launches back to back: cold, immediately behind 20 x C3, and after pauses."""
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    big = c.ambient_uniform_batch(0xC3, 0, 262144)
    bout = torch.empty_like(big)
    qs = {B: c.ambient_uniform_batch(0xC2 if B == 4096 else 0xC3, 0, B) for B in (4096, 32768)}
    outs = {B: torch.empty_like(q) for B, q in qs.items()}

    def mean10(B):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            c.project_batch(qs[B], out=outs[B])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 10

    def load():
        for _ in range(20):
            c.project_batch(big, out=bout)
        torch.cuda.synchronize()

    for B in qs:
        c.project_batch(qs[B], out=outs[B])
    torch.cuda.synchronize()
    for B in qs:
        row = ["cold %.3f %.3f" % (mean10(B), mean10(B))]
        for pause in (0.0, 0.05, 0.25, 1.0, 3.0):
            load()
            time.sleep(pause)
            row.append("load+%.2fs %.3f %.3f" % (pause, mean10(B), mean10(B)))
        print("B=%6d  mean-of-10 ms  %s" % (B, " | ".join(row)), flush=True)


def sampler(argv):
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    B = 262144
    q = c.ambient_uniform_batch(0xC3, 0, B)
    out = torch.empty_like(q)
    a = timed(lambda: c.project_batch(q, out=out), reps=4)
    b = timed(lambda: c.sample_project_batch(0xC3, 0, B), reps=4)
    print("project_batch %.3f ms   sample_project_batch (fused sampler + wrap) %.3f ms" % (a, b))


def soak(argv):
    ctx = Context(0)
    for obj, B in (("Wine_Bottle", 262144), ("stefan", 98304), ("dumbbell", 40000), ("Wine_Bottle", 20000)):
        c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        q = c.ambient_uniform_batch(0x50A, 0, B)
        ref = c.project_batch(q)
        bad = sum(not all(torch.equal(a, b) for a, b in zip(c.project_batch(q), ref)) for _ in range(25))
        print(obj, B, "repeats differing from the first run:", bad, flush=True)
    # the analytic mode (lane-pair kernel + hand-over to the latency kernel) and the proxy clearance, the same way
    from closed_chain_motion_planner_amd.scene import ProxyValidityChecker

    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    c.setJacobianMode(1)
    q = c.ambient_uniform_batch(0x50B, 0, 200000)
    ref = c.project_batch(q)
    bad = sum(not all(torch.equal(a, b) for a, b in zip(c.project_batch(q), ref)) for _ in range(25))
    print("Wine_Bottle analytic 200000 (lane-pair kernel + latency kernel) repeats differing:", bad, flush=True)
    for obj, B in (("stefan", 262144), ("Wine_Bottle", 2097152), ("dumbbell", 5000)):  # the hand-over's order is decided by atomics; the latency kernel alone
        ca = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        ca.setJacobianMode(1)
        qa = ca.ambient_uniform_batch(0x50E, 0, B)
        ra = ca.project_batch(qa)
        bad = sum(not all(torch.equal(a, b) for a, b in zip(ca.project_batch(qa), ra)) for _ in range(25))
        print(obj, "analytic", B, "repeats differing:", bad, flush=True)
    # the extend step beyond the resident blocks: ticket queue + FP32 scout order (atomics decide who takes which edge,
    # the sort's ties fall as they fall) — counts, flags, Newton counts and every listed state, the same 25 times over
    cg = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    frm, to = near_edges(cg, 16384)
    rg = cg.discrete_geodesic_batch(frm, to, 16)
    live = torch.arange(16, device=frm.device)[None, :] < rg[1].clamp(max=16)[:, None]
    bad = 0
    for _ in range(25):
        g = cg.discrete_geodesic_batch(frm, to, 16)
        bad += not (all(torch.equal(a, b) for a, b in zip(g[1:], rg[1:])) and torch.equal(g[0][live], rg[0][live]))
    print("Wine_Bottle extend step, 16384 edges, scout order: repeats differing:", bad, flush=True)
    sc = ProxyValidityChecker(c).scene
    refc = sc.clearance_batch(ref[0])
    bad = sum(not all(torch.equal(a, b) for a, b in zip(sc.clearance_batch(ref[0]), refc)) for _ in range(25))
    print("proxy clearance 200000 repeats differing:", bad, flush=True)


def soak_resident(argv):
    """the resident service kernel under a long run: N distinct states, each through project / function / isSatisfied / jointValid as
    single calls on the service, against the BATCHED kernels' results on the same states (both are bit-identical to the oracle, so
    they must be to each other) — with idle exits (the service leaves after 2 ms here and restarts), batch launches and workspace
    growth on the same context in between, and every 64th state a single checkMotion edge towards the next one.  --analytic: the
    same in analytic mode (the row16 service kernel), with FIVE edges per request at every 64th state"""
    import time

    analytic = "--analytic" in argv
    argv = [a for a in argv if a != "--analytic"]
    per_req = 5 if analytic else 1
    N = int(argv[0]) if argv else 20000
    ctx = Context(0)
    for obj in ("Wine_Bottle", "stefan"):
        c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        c.setJacobianMode(1 if analytic else 0)
        far = c.ambient_uniform_batch(0x50C, 0, N)
        qp, okp, _ = c.project_batch(c.ambient_uniform_batch(0x50D, 0, 4 * N))
        near = qp[okp == 1][: N // 2] + 0.04 * (torch.rand((min(N // 2, int((okp == 1).sum())), 14), dtype=torch.float64, device=qp.device) - 0.5)
        xs = torch.cat([far, near])[torch.randperm(N + near.shape[0], device=far.device)]
        qb, okb, itb = c.project_batch(xs)
        fb, sb, jb = c.function_batch(xs), c.is_satisfied_batch(xs), c.joint_valid_batch(xs)
        torch.cuda.synchronize()
        xs_h, qb_h, okb_h = xs.cpu().numpy(), qb.cpu().numpy(), okb.cpu().numpy()
        fb_h, sb_h, jb_h = fb.cpu().numpy(), sb.cpu().numpy(), jb.cpu().numpy()
        # single checkMotion edges, launched (the service off) for the expected values
        edges = list(range(0, xs_h.shape[0] - 1, 64))
        frm_e, to_e = qb[edges], qb[[e + 1 for e in edges]]
        exp_e = c.discrete_geodesic_batch(frm_e, to_e, 16, check_target=True)
        torch.cuda.synchronize()
        frm_h, to_h = frm_e.cpu().numpy(), to_e.cpu().numpy()
        exp_st, exp_n, exp_ok = exp_e[0].cpu().numpy(), exp_e[1].cpu().numpy(), exp_e[2].cpu().numpy()
        L, dp = _lib.lib(), C.POINTER(C.c_double)
        ctx.set_option("resident_idle_ms", 2)
        ctx.set_option("resident", 1)
        served0 = ctx.get_option("resident_served")
        bad = restarts = 0
        grow = 30000
        t0 = time.perf_counter()
        for k in range(xs_h.shape[0]):
            x = xs_h[k]
            y = x.copy()
            ok = c.project(y)
            f = c.function(x)
            same = (np.array_equal(np.isnan(y), np.isnan(qb_h[k])) and np.array_equal(y[~np.isnan(y)].view(np.uint64), qb_h[k][~np.isnan(y)].view(np.uint64))
                    and bool(ok) == bool(okb_h[k]) and np.array_equal(np.isnan(f), np.isnan(fb_h[k])) and np.array_equal(f[~np.isnan(f)].view(np.uint64), fb_h[k][~np.isnan(f)].view(np.uint64))
                    and bool(c.isSatisfied(x)) == bool(sb_h[k]) and bool(c.jointValid(x)) == bool(jb_h[k]))
            if k % 64 == 0 and k // 64 < len(edges):
                # one edge (analytic mode: five) from host buffers, as the unchanged planner asks for them: through the service
                es = [(k // 64 + j) % len(edges) for j in range(per_req)]
                fa, ta = np.ascontiguousarray(frm_h[es]), np.ascontiguousarray(to_h[es])
                st, n1, ok1 = np.zeros((per_req, 16, 14)), (C.c_int32 * per_req)(), (C.c_uint8 * per_req)()
                rc = L.ccmp_geodesic_host_ex(ctx.handle, C.byref(c.problem), fa.ctypes.data_as(dp), ta.ctypes.data_as(dp), per_req, 16,
                                             st.ctypes.data_as(dp), n1, ok1, None, None, 0, 1)
                same = same and rc == 0
                for j, e in enumerate(es):
                    n = min(int(exp_n[e]), 16)
                    same = same and int(n1[j]) == int(exp_n[e]) and int(ok1[j]) == int(exp_ok[e]) and st[j, :n].tobytes() == exp_st[e, :n].tobytes()
            bad += not same
            if k % 997 == 0:
                time.sleep(0.004)  # idle exit: the next call starts the service again
                restarts += 1
            if k % 4001 == 0:  # a batch and a growing workspace on the same context under the live service
                grow += 7000
                c.project_batch(c.ambient_uniform_batch(0x50E, k, grow))
        dt = time.perf_counter() - t0
        gave_up, served = ctx.get_option("resident_gave_up"), ctx.get_option("resident_served") - served0
        ctx.set_option("resident", 0)
        print("%s%s: %d states x (project, function, isSatisfied, jointValid) + %d checkMotion requests of %d edge(s) through the resident service "
              "(%d requests served), %d idle exits, %d batch calls in between: differing from the batched kernels %d; gave up %d; %.1f s" %
              (obj, " (analytic)" if analytic else "", xs_h.shape[0], len(edges), per_req, served, restarts, xs_h.shape[0] // 4001 + 1, bad, gave_up, dt), flush=True)
        assert bad == 0 and gave_up == 0


def scout(argv):
    ctx = Context(0)
    L = _lib.lib()
    L.ccmp_ctx_debug_lpt_pred.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    for obj in ("Wine_Bottle", "stefan"):
        c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        B = 262144
        q = c.ambient_uniform_batch(0xC3, 0, B)
        ctx.set_lpt(1, 0)
        _, _, it = c.project_batch(q)
        pred = np.zeros(B, dtype=np.uint16)
        assert L.ccmp_ctx_debug_lpt_pred(ctx.handle, pred.ctypes.data, B) == 0
        it, p = it.cpu().numpy().astype(np.int32), pred.astype(np.int32)
        big = it > 80
        print("%s scout vs FD iterations: equal %.3f  |d|<=2 %.3f  corr %.4f; of the %d samples with > 80 iterations the scout says > 60 for %.3f"
              % (obj, (p == it).mean(), (np.abs(p - it) <= 2).mean(), np.corrcoef(p, it)[0, 1], big.sum(), (p[big] > 60).mean()))


def clearance(argv):
    """proxy clearance: run time against batch size for both kernels (one block per state / 64-state tiles) + single-state call"""
    from closed_chain_motion_planner_amd.scene import ProxyValidityChecker

    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % (argv[0] if argv else "Wine_Bottle"), ctx=ctx)
    sc = ProxyValidityChecker(c).scene
    print("spheres %d pairs %d" % (len(sc.spheres), sc.num_pairs))
    for B in (1, 64, 1024, 4096, 8192, 16384, 32768, 65536, 262144, 1048576):
        q = c.ambient_uniform_batch(0xC3, 0, B)
        row = []
        for name, lim in (("per_state", 1 << 30), ("tiles", 0)):
            if name == "per_state" and B > 65536:
                row.append(float("nan"))
                continue
            ctx.set_option("clearance_per_state_max", lim)
            row.append(timed(lambda: sc.clearance_batch(q, 0.0), 10))
        print("B %8d  per-state %8.4f ms   tiles %8.4f ms" % (B, row[0], row[1]))
    ctx.set_option("clearance_per_state_max", 8192)
    x = c.ambient_uniform_batch(0xC1, 0, 8).cpu().numpy()
    ts = []
    for i in range(200):
        t0 = time.perf_counter()
        sc.clearance(x[i % 8])
        ts.append(time.perf_counter() - t0)
    print("single-state host call: median %.1f us" % (np.median(ts[20:]) * 1e6))


def valid_states(c, n, seed=0x4E4E):
    """n valid projected states (sampleUniform, the rows project() accepted)"""
    rows, have, first = [], 0, 0
    while have < n:
        B = min(1 << 20, max(4 * (n - have), 4096))
        q, ok, _, _ = c.sample_project_batch(seed, first, B, want_iters=False)
        rows.append(q[ok != 0])
        have += rows[-1].shape[0]
        first += B
    return torch.cat(rows)[:n].contiguous()


def torch_knn_mm(nodes, queries, k):
    """the fastest thing torch offers: |q|^2 + |n|^2 - 2 q n^T through the FP64 matrix product, then topk (inexact distances)"""
    d2 = (queries * queries).sum(1)[:, None] + (nodes * nodes).sum(1)[None, :] - 2.0 * (queries @ nodes.T)
    return torch.topk(d2, k, dim=1, largest=False, sorted=True)


def torch_knn_diff(nodes, queries, k, chunk=256):
    """squared differences summed per pair (the distance's own operations), in chunks of queries, then topk"""
    vals, idxs = [], []
    for s in range(0, queries.shape[0], chunk):
        d2 = torch.cdist(queries[s: s + chunk], nodes, compute_mode="donot_use_mm_for_euclid_dist")
        v, i = torch.topk(d2, k, dim=1, largest=False, sorted=True)
        vals.append(v)
        idxs.append(i)
    return torch.cat(vals), torch.cat(idxs)


def alternate(fns, reps):
    """{name: [ms per call]} — every contender warmed up, then `reps` rounds in which each runs once, device events around each call"""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def _stat(ms):
    a = np.sort(np.asarray(ms))
    return "median %.4f ms (min %.4f, max %.4f, n %d)" % (np.median(a), a[0], a[-1], len(a))


def connect(argv):
    """the connection step against what a user does without it; every line states the median and the spread of both contenders"""
    reps = max(20, int(argv[0])) if argv else 20
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    big = valid_states(c, (1 << 20) + 4096)
    k = 5
    verdicts = []

    def compare(title, ours, theirs):
        t = alternate({"ours": ours, **theirs}, reps)
        best = min(theirs, key=lambda n: np.median(t[n]))
        mo, mt = np.median(t["ours"]), np.median(t[best])
        spread = max(np.max(t["ours"]) - np.min(t["ours"]), np.max(t[best]) - np.min(t[best]))
        print("%s" % title)
        for name, ms in t.items():
            print("    %-28s %s" % (name, _stat(ms)))
        ok = mo <= mt + spread
        verdicts.append((title, ok))
        print("    -> ours / best torch = %.3f  (%s)" % (mo / mt, "not slower" if ok else "SLOWER beyond the spread"), flush=True)
        return mo

    # k-NN throughput
    nodes, queries = big[:65536].contiguous(), big[1 << 20:].contiguous()
    N, Q = nodes.shape[0], queries.shape[0]
    i0, d0 = c.nearest_k_batch(nodes, queries, k)
    ref = torch_knn_diff(nodes, queries, k)
    print("agreement with torch (exact-difference form): %d of %d neighbour slots equal" % (int((i0.long() == ref[1]).sum()), Q * k))
    print(_lib.describe(ctx.handle, _lib.CALL_KNN, Q))
    ms = compare("k-NN  N=%d Q=%d k=%d" % (N, Q, k), lambda: c.nearest_k_batch(nodes, queries, k),
                 {"torch mm + topk": lambda: torch_knn_mm(nodes, queries, k), "torch cdist(exact) + topk": lambda: torch_knn_diff(nodes, queries, k)})
    flops = 42.0 * Q * N / (ms * 1e-3)
    print("    achieved %.2f TFLOP/s FP64 (42 Q N flop per call) = %.1f %% of the 78.6 TFLOP/s vector peak" % (flops / 1e12, 100 * flops / 78.6e12))
    # single-query latency
    for Nn in (65536, 1 << 20):
        nd, q1 = big[:Nn].contiguous(), queries[:1].contiguous()
        print(_lib.describe(ctx.handle, _lib.CALL_KNN, 1))
        compare("k-NN  N=%d Q=1 k=%d" % (Nn, k), lambda: c.nearest_k_batch(nd, q1, k),
                {"torch diff + topk": lambda: torch.topk(((nd - q1) ** 2).sum(1), k, largest=False), "torch mv + topk": lambda: torch_knn_mm(nd, q1, k)})
    # connect
    nodes, queries = big[:16384].contiguous(), big[1 << 20: (1 << 20) + 3277].contiguous()
    for mode in (0, 1):
        c.setJacobianMode(mode)
        idx, _ = c.nearest_k_batch(nodes, queries, k)
        frm = nodes[idx.reshape(-1).long()].contiguous()
        to = queries.repeat_interleave(k, dim=0).contiguous()

        def parent():
            _, i = torch_knn_mm(nodes, queries, k)
            f = nodes[i.reshape(-1)]
            t_ = queries.repeat_interleave(k, dim=0)
            return c.discrete_geodesic_batch(f, t_, 16, check_target=True, want_carry=True, round_budget=128)

        t = alternate({"traversal alone": lambda: c.discrete_geodesic_batch(frm, to, 16, check_target=True, want_carry=True, round_budget=128)}, reps)
        print("connect (%s)  N=%d Q=%d k=%d: %d edges, lists of 16, round budget 128" % ("analytic" if mode else "FD", nodes.shape[0], queries.shape[0], k, frm.shape[0]))
        print("    %-28s %s" % ("traversal alone", _stat(t["traversal alone"])))
        mo = compare("  connect call against torch k-NN + gather + ccmp_geodesic_batch_ex",
                     lambda: c.connect_batch(nodes, queries, k, check_target=True, max_states=16, round_budget=128), {"torch k-NN + gather + ex": parent})
        print("    choosing the pairs costs %.4f ms (connect call - traversal alone, medians)" % (mo - np.median(t["traversal alone"])))
    c.setJacobianMode(0)
    print("VERDICT " + ("all not slower" if all(ok for _, ok in verdicts) else "SLOWER: " + "; ".join(t for t, ok in verdicts if not ok)))


def roadmap(argv):
    """the device-resident roadmap store: host-form single-query k-NN against ccmp_knn_host (which uploads the nodes per call), the
    object metric's many-query kernel against the joint metric's, appends and pose derivation.  Contenders alternate in one process,
    `reps` rounds behind warm-ups; device events around device forms, the wall clock around host forms; every line states the spread"""
    from closed_chain_motion_planner_amd import Roadmap
    from closed_chain_motion_planner_amd._lib import METRIC_JOINT, METRIC_OBJECT

    reps = max(20, int(argv[0])) if argv else 20
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    big = valid_states(c, 65536 + 16384)
    k = 5

    def wall(fns):
        for fn in fns.values():
            for _ in range(3):
                fn()
        out = {name: [] for name in fns}
        for _ in range(reps):
            for name, fn in fns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                out[name].append((time.perf_counter() - t0) * 1e3)
        return out

    def show(title, t):
        print(title)
        for name, ms in t.items():
            print("    %-44s %s" % (name, _stat(ms)))
        sys.stdout.flush()

    # 1. the planner's query: one state, host pointers, k = 5
    verdict = []
    L, dp, ip = _lib.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for N in (4096, 65536):
        nodes = big[:N].contiguous()
        nodes_h, q_h = nodes.cpu().numpy(), big[65536:65537].cpu().numpy()
        rm = Roadmap(c, N)
        rm.append(nodes)
        qp_h = Roadmap(c, 4)
        qp_h.append(big[65536:65537].contiguous())
        qpose = qp_h.read(host=True)[1]
        idx, dist = np.zeros((1, k), np.int32), np.zeros((1, k))
        t = wall({
            "ccmp_knn_host (uploads the nodes)": lambda: _lib.check(L.ccmp_knn_host(ctx.handle, nodes_h.ctypes.data_as(dp), N, q_h.ctypes.data_as(dp), 1, k, 0, 0,
                                                                                    idx.ctypes.data_as(ip), dist.ctypes.data_as(dp)), "ccmp_knn_host"),
            "ccmp_roadmap_knn_host, joint metric": lambda: rm.nearest_k(q_h, k, METRIC_JOINT),
            "ccmp_roadmap_knn_host, object metric": lambda: rm.nearest_k(qpose, k, METRIC_OBJECT),
        })
        show("host-form single-query k-NN  N=%d k=%d (wall clock)" % (N, k), t)
        names = list(t)
        base, spread = np.median(t[names[0]]), np.max(t[names[0]]) - np.min(t[names[0]])
        for n in names[1:]:
            ok = np.median(t[n]) <= base + spread
            verdict.append(ok)
            print("    -> %s / ccmp_knn_host = %.3f (%s)" % (n, np.median(t[n]) / base, "not slower" if ok else "SLOWER beyond the spread"))
    # 2. the many-query kernels, both metrics, k = 5 and k = 16 (does the cheap pre-filter hold up with long lists?)
    N, Q = 65536, 16384
    nodes, queries = big[:N].contiguous(), big[65536:].contiguous()
    rm = Roadmap(c, N)
    rm.append(nodes)
    qrm = Roadmap(c, Q)
    qrm.append(queries)
    qposes = qrm.read()[1]
    print(_lib.describe(ctx.handle, _lib.CALL_ROADMAP_KNN, Q))
    print(_lib.describe(ctx.handle, _lib.CALL_KNN, Q))
    for kk in (5, 16):
        t = alternate({"knn_pose_many (object metric)": lambda: rm.nearest_k(qposes, kk, METRIC_OBJECT),
                       "knn_many (joint metric, same store)": lambda: rm.nearest_k(queries, kk, METRIC_JOINT),
                       "ccmp_knn_batch (joint metric, caller's nodes)": lambda: c.nearest_k_batch(nodes, queries, kk)}, reps)
        show("k-NN  N=%d Q=%d k=%d (device events, scan + merge)" % (N, Q, kk), t)
        mo, mj = np.median(t["knn_pose_many (object metric)"]), np.median(t["knn_many (joint metric, same store)"])
        print("    -> object / joint = %.3f; object metric: %.1f G pairs/s, %.2f TFLOP/s FP64 on the 12 flop of the pre-filter alone" %
              (mo / mj, Q * N / (mo * 1e-3) / 1e9, 12.0 * Q * N / (mo * 1e-3) / 1e12))
    # 3. appends
    row = big[:1].contiguous()
    small = Roadmap(c, 1 << 16)
    small.append(big[:4096].contiguous())

    def append_no_growth():
        small.truncate(4096)
        small.append(row)

    def append_growth():
        g = Roadmap(c, 4096)
        g.append(big[:4096].contiguous())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.append(row)  # 4096 -> 8192 rows: allocation, device-to-device copy, one stream synchronisation
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        g.close()
        return dt

    t = wall({"append of 1 row, capacity holds (host time, incl. sync)": lambda: (append_no_growth(), torch.cuda.synchronize())})
    show("append (wall clock)", t)
    grow = [append_growth() for _ in range(reps + 3)][3:]
    print("    %-44s %s" % ("append of 1 row that doubles 4096 rows", _stat(grow)))
    many = valid_states(c, 262144, seed=0x77)
    bulk = Roadmap(c, 262144)
    t = alternate({"append of 262144 rows (copy + pose_from_joints)": lambda: (bulk.truncate(0), bulk.append(many))}, reps)
    show("pose derivation (device events)", t)
    print("VERDICT host-form k-NN on the resident store: " + ("not slower" if all(verdict) else "SLOWER in at least one case"))


def mirror(argv):
    """host wall time per call of the mirror's own wrappers in the planner's per-vertex loop, on a store of 1 024 vertices: the numpy
    forms of append (one vertex, truncated again outside the clock), nearest_k (Q = 1, k = 5) and read (one row), the device form of
    connect (Q = 1, k = 5; the clock stops when the call returns, the stream is drained outside it).  `warm` rounds of all four, then the
    median of `calls` calls each, one JSON line.  Run from the root of the tree to be measured; CCMP_LIBRARY names the library."""
    import json

    from closed_chain_motion_planner_amd import Roadmap

    calls, warm = (int(argv[0]) if argv else 2000), (int(argv[1]) if len(argv) > 1 else 200)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=Context(0))
    q = valid_states(c, 1024 + 1)
    rm = Roadmap(c, 2048)
    rm.append(q[:1024])
    one_d = q[1024:].contiguous()
    one = one_d.cpu().numpy()
    pose = rm.read(5, 1, host=True)[1]

    def append():
        rm.append(one)

    fns = {"append (numpy, 1 vertex)": (append, lambda: rm.truncate(1024)), "nearest_k (numpy, Q=1, k=5)": (lambda: rm.nearest_k(pose, 5), None),
           "read (host=True, 1 row)": (lambda: rm.read(7, 1, host=True), None),
           "connect (device, Q=1, k=5)": (lambda: rm.connect(one_d, 5, max_states=16), torch.cuda.synchronize)}
    for _ in range(warm):
        for fn, after in fns.values():
            fn()
            if after:
                after()
    out = {}
    for name, (fn, after) in fns.items():
        us = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            us.append((time.perf_counter() - t0) * 1e6)
            if after:
                after()
        out[name] = round(float(np.median(us)), 2)
    print("MIRROR_US " + json.dumps({"calls": calls, "warmup_rounds": warm, "median_us": out}))


def ik(argv):
    """ccmp_pose_ik_host / ccmp_pose_ik_batch against ccmp_pose_ik_ref (the same text on one host thread) on the same inputs; the outputs are
    compared bit for bit while they are timed.  Targets: poses of valid projected states; seeds: their five pose-nearest other states."""
    from closed_chain_motion_planner_amd import Roadmap, pose_ik_ref

    if "--scene" in argv:
        return ik_scene([a for a in argv if a != "--scene"])
    reps_a = int(argv[0]) if len(argv) > 0 else 30
    reps_b = int(argv[1]) if len(argv) > 1 else 2
    Tb = int(argv[2]) if len(argv) > 2 else 4096
    S, R = 5, 14
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    q, ok, _, _ = c.sample_project_batch(0x1C, 0, 16 * Tb + 4096, want_iters=False)
    states = q[(ok != 0) & (c.joint_valid_batch(q) != 0)][:Tb + 1024].contiguous()
    rm = Roadmap(c, states.shape[0])
    rm.append(joints=states)
    poses = rm.read()[1]
    T = min(Tb, states.shape[0])
    idx, _ = rm.nearest_k(poses[:T].contiguous(), S, mode=_lib.KNN_NOT_SELF)
    seeds = states[idx.long()].contiguous()
    tp, sd = poses[:T].contiguous(), seeds
    tph, sdh = tp.cpu().numpy(), sd.cpu().numpy()
    print("%d valid states; %d targets x %d seeds x %d restarts" % (states.shape[0], T, S, R))

    def same(a, b):
        return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in ("q", "ok", "which"))

    # (a) the planner's shape: one pose per call, host pointers, host clock around the synchronous calls
    ta = {"host form (device)": [], "ccmp_pose_ik_ref (one thread)": []}
    agree = True
    for i in range(reps_a + 3):
        t = i % T
        t0 = time.perf_counter()
        dev = c.pose_ik_batch(tph[t:t + 1], sdh[t:t + 1], rng_seed=0x1C, first_index=t)
        t1 = time.perf_counter()
        ref = pose_ik_ref(c.problem, tph[t:t + 1], sdh[t:t + 1], rng_seed=0x1C, first_index=t)
        t2 = time.perf_counter()
        agree = agree and same(dev, ref)
        if i >= 3:
            ta["host form (device)"].append((t1 - t0) * 1e3)
            ta["ccmp_pose_ik_ref (one thread)"].append((t2 - t1) * 1e3)
    print("(a) 1 pose x %d x %d, host form, wall clock; outputs identical: %s" % (S, R, agree))
    for name, ms in ta.items():
        print("    %-34s %s" % (name, _stat(ms)))

    # (b) the batch: device pointers, device events; the contender once per round on the host clock
    tb = {"device form": [], "ccmp_pose_ik_ref (one thread)": []}
    out = c.pose_ik_batch(tp, sd, rng_seed=0x1C, want_candidates=True)
    torch.cuda.synchronize()
    for _ in range(reps_b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev = c.pose_ik_batch(tp, sd, rng_seed=0x1C)
        e1.record()
        torch.cuda.synchronize()
        tb["device form"].append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        ref = pose_ik_ref(c.problem, tph, sdh, rng_seed=0x1C)
        tb["ccmp_pose_ik_ref (one thread)"].append((time.perf_counter() - t0) * 1e3)
        agree = agree and same({k: v.cpu().numpy() for k, v in dev.items()}, ref)
    print("(b) %d poses x %d x %d, device form, device events; outputs identical: %s" % (T, S, R, agree))
    for name, ms in tb.items():
        print("    %-34s %s" % (name, _stat(ms)))
    print("    solved %d of %d; by the first slot %d" % (int(out["ok"].sum()), T, int((out["which"] == 0).sum())))
    # rounds and idle lanes: lane n of an arm is candidate (n // (1 + R), n % (1 + R)); a wavefront is 64 consecutive lanes and runs as
    # many loop passes as its slowest lane (a converged lane took rounds + 1 passes, an unconverged one max_rounds + 1)
    rounds = out["cand_rounds"].cpu().numpy()
    conv = rounds[rounds >= 0]
    hist, edges = np.histogram(conv, bins=[0, 1, 2, 4, 8, 16, 32, 48, 65])
    print("    rounds of the converged candidates (%.1f %% of all; %.1f %% did not converge): median %d, 95th percentile %d"
          % (100.0 * len(conv) / rounds.size, 100.0 * (rounds == -1).mean(), np.median(conv), np.percentile(conv, 95)))
    print("    histogram " + ", ".join("[%d,%d): %d" % (edges[i], edges[i + 1], hist[i]) for i in range(len(hist))))
    passes = np.where(rounds >= 0, rounds + 1, np.where(rounds == -1, 65, 0))  # (T, S, 2, 1 + R)
    busy = wave = 0
    for a in (0, 1):
        lanes = passes[:, :, a, :].reshape(-1)
        pad = (-len(lanes)) % 64
        w = np.concatenate([lanes, np.zeros(pad, dtype=lanes.dtype)]).reshape(-1, 64)
        busy += int(w.sum())
        wave += 64 * int(w.max(axis=1).sum())
    print("    lane-passes spent idle (a finished lane waiting for its wavefront's slowest): %.1f %% of %d" % (100.0 * (1.0 - busy / wave), wave))
    print("VERDICT pose_ik device forms against one host thread: (a) %.2fx, (b) %.1fx"
          % (np.median(ta["ccmp_pose_ik_ref (one thread)"]) / np.median(ta["host form (device)"]),
             np.median(tb["ccmp_pose_ik_ref (one thread)"]) / np.median(tb["device form"])))


def ik_scene(argv):
    """ik --scene: the vetted call (ccmp_pose_ik_vetted_*) against today's route — ccmp_pose_ik_* and one ccmp_clearance_* call on the answers —
    on the default skeleton scene at -0.03: time, targets solved by each route, the vet kernel's share of the call and its resources."""
    from closed_chain_motion_planner_amd import ProxyValidityChecker, Roadmap
    from closed_chain_motion_planner_amd.build import resource_report

    reps_a = int(argv[0]) if len(argv) > 0 else 30
    reps_b = int(argv[1]) if len(argv) > 1 else 10
    Tb = int(argv[2]) if len(argv) > 2 else 4096
    S, R, seed = 5, 14, 0x1C
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    chk = ProxyValidityChecker(c)
    scene, margin = chk.scene, chk.margin
    q, ok, _, _ = c.sample_project_batch(seed, 0, 16 * Tb + 4096, want_iters=False)
    states = q[(ok != 0) & (c.joint_valid_batch(q) != 0)][:Tb + 1024].contiguous()
    rm = Roadmap(c, states.shape[0])
    rm.append(joints=states)
    poses = rm.read()[1]
    T = min(Tb, states.shape[0])
    idx, _ = rm.nearest_k(poses[:T].contiguous(), S, mode=_lib.KNN_NOT_SELF)
    tp, sd = poses[:T].contiguous(), states[idx.long()].contiguous()
    tph, sdh = tp.cpu().numpy(), sd.cpu().numpy()
    print("seed 0x%X; %d valid states; %d targets x %d seeds x %d restarts; default skeleton scene (%d tested pairs), margin %g"
          % (seed, states.shape[0], T, S, R, scene.num_pairs, margin))

    def today_host(t):
        out = c.pose_ik_batch(tph[t:t + 1], sdh[t:t + 1], rng_seed=seed, first_index=t)
        return bool(out["ok"][0]) and bool(scene.clearance(np.nan_to_num(out["q"]), margin)[2][0])

    def vetted_host(t):
        return bool(c.pose_ik_batch(tph[t:t + 1], sdh[t:t + 1], rng_seed=seed, first_index=t, scene=scene, margin=margin)["ok"][0])

    # (a) the planner's shape: one pose per call, host pointers, host clock around the synchronous calls
    ta = {"today: pose_ik_host + clearance_host": [], "ccmp_pose_ik_vetted_host": []}
    solved = [0, 0]
    for i in range(reps_a + 3):
        t = i % T
        t0 = time.perf_counter()
        a = today_host(t)
        t1 = time.perf_counter()
        b = vetted_host(t)
        t2 = time.perf_counter()
        if i >= 3:
            ta["today: pose_ik_host + clearance_host"].append((t1 - t0) * 1e3)
            ta["ccmp_pose_ik_vetted_host"].append((t2 - t1) * 1e3)
            solved[0] += a
            solved[1] += b
    print("(a) 1 pose x %d x %d, host forms, wall clock; solved and clear: today %d, vetted %d of %d" % (S, R, solved[0], solved[1], reps_a))
    for name, ms in ta.items():
        print("    %-40s %s" % (name, _stat(ms)))

    # (b) the batch: device pointers, device events, the contenders alternating
    def today():
        out = c.pose_ik_batch(tp, sd, rng_seed=seed)
        free = scene.clearance_batch(torch.nan_to_num(out["q"]), margin, ok=out["ok"], want_pair=False)[2]
        return out, free

    full = c.pose_ik_batch(tp, sd, rng_seed=seed, want_candidates=True, scene=scene, margin=margin)
    rounds = full["cand_rounds"]
    conv = rounds >= 0
    rows = [full["cand_q"][:, :, a].reshape(-1, 7).contiguous() for a in (0, 1)]
    packed = [full["cand_q"][:, :, a][conv[:, :, a]].contiguous() for a in (0, 1)]
    tb = alternate({"today: pose_ik_batch + clearance_batch": today,
                    "ccmp_pose_ik_vetted_batch": lambda: c.pose_ik_batch(tp, sd, rng_seed=seed, scene=scene, margin=margin),
                    "ccmp_pose_ik_batch alone": lambda: c.pose_ik_batch(tp, sd, rng_seed=seed),
                    "ik_vet_kernel on every candidate row": lambda: [scene.arm_clearance_batch(a, rows[a], margin) for a in (0, 1)],
                    "ik_vet_kernel on the converged rows, packed": lambda: [scene.arm_clearance_batch(a, packed[a], margin) for a in (0, 1)]}, reps_b)
    out, free = today()
    torch.cuda.synchronize()
    n_today, n_vet = int((out["ok"].bool() & free.bool()).sum()), int(full["ok"].sum())
    print("(b) %d poses x %d x %d, device forms, device events" % (T, S, R))
    for name, ms in tb.items():
        print("    %-44s %s" % (name, _stat(ms)))
    print("    targets solved and clear: today's route %d, vetted call %d of %d (%d recovered); plain call solves %d" % (n_today, n_vet, T, n_vet - n_today, int(out["ok"].sum())))
    med = {k: float(np.median(v)) for k, v in tb.items()}
    print("    the vet kernel's share of the vetted call: between %.1f %% (converged rows only, packed) and %.1f %% (every row computed); in the call a row that did "
          "not converge idles: %.1f %% of the rows, what a compaction ahead of the kernel would save"
          % (100.0 * med["ik_vet_kernel on the converged rows, packed"] / med["ccmp_pose_ik_vetted_batch"],
             100.0 * med["ik_vet_kernel on every candidate row"] / med["ccmp_pose_ik_vetted_batch"], 100.0 * (1.0 - float(conv.float().mean()))))
    for k in resource_report().get("ccmp_kernels_ik_vet.hip", []):
        print("    %-20s %d VGPRs, %d SGPRs, %d B LDS per block, %d B scratch, occupancy %d waves per SIMD"
              % (k["name"], k.get("vgprs", -1), k.get("sgprs", -1), k.get("lds", -1), k.get("scratch", -1), k.get("occupancy", -1)))
    print("VERDICT vetted call against today's route: (a) %.2fx the time, (b) %.2fx the time; targets solved and clear %d -> %d"
          % (np.median(ta["ccmp_pose_ik_vetted_host"]) / np.median(ta["today: pose_ik_host + clearance_host"]),
             med["ccmp_pose_ik_vetted_batch"] / med["today: pose_ik_batch + clearance_batch"], n_today, n_vet))


def object_(argv):
    """ccmp_object_propose_host / _batch and ccmp_object_valid_batch against the *_ref forms (the same text on one host thread) on the same
    inputs; the outputs are compared bit for bit while they are timed.  Meshes are procedural (tests/object_cases.py), the workspace is
    the fixture tests/golden/object_workspace.json."""
    sys.path.insert(0, "tests")
    from object_cases import big_sphere, dumbbell, random_poses, workspace

    from closed_chain_motion_planner_amd import ObjectChecker, object_propose_ref, object_valid_ref

    reps_a = int(argv[0]) if len(argv) > 0 else 30
    reps_b = int(argv[1]) if len(argv) > 1 else 3
    Gb = int(argv[2]) if len(argv) > 2 else 4096
    ctx = Context(0)
    boxes, mesh, big = workspace(), dumbbell(), big_sphere()
    chk, chk_big = ObjectChecker(ctx, mesh, boxes), ObjectChecker(ctx, big, boxes)
    rng = np.random.default_rng(0x0B)
    lo, hi = (0.1, -0.5, 1.25), (1.2, 0.5, 1.8)
    frm = random_poses(rng, Gb, lo=(0.2, -0.45, 1.25), hi=(1.1, 0.45, 1.8))
    goal = random_poses(rng, 1, lo=(0.4, -0.2, 1.4), hi=(0.9, 0.2, 1.7))
    kw = dict(t=0.3, sigma=0.2, lo=lo, hi=hi, attempts=2, rng_seed=0x0B)
    print("meshes: %d and %d triangles; %d boxes" % (len(mesh), len(big), len(boxes)))

    def same(a, b, keys):
        return all(np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) for k in keys)

    # (a) the planner's shape: one nearest pose per call, host pointers, host clock around the synchronous calls
    ta = {"host form (device)": [], "ccmp_object_propose_ref (one thread)": []}
    agree = True
    for i in range(reps_a + 3):
        g = i % Gb
        t0 = time.perf_counter()
        dev = chk.propose(frm[g:g + 1], goal, first_index=g, **kw)
        t1 = time.perf_counter()
        ref = object_propose_ref(mesh, boxes, frm[g:g + 1], goal, first_index=g, **kw)
        t2 = time.perf_counter()
        agree = agree and same(dev, ref, ("pose", "which"))
        if i >= 3:
            ta["host form (device)"].append((t1 - t0) * 1e3)
            ta["ccmp_object_propose_ref (one thread)"].append((t2 - t1) * 1e3)
    print("(a) propose G = 1, 2 attempts, %d triangles, host form, wall clock; outputs identical: %s" % (len(mesh), agree))
    for name, ms in ta.items():
        print("    %-40s %s" % (name, _stat(ms)))

    # (b) the batch, (c) valid on the large mesh: device pointers, device events; the contender once per round on the host clock
    frm_d, goal_d = torch.from_numpy(frm).cuda(), torch.from_numpy(goal).cuda()
    poses = random_poses(rng, 4096)
    poses_d = torch.from_numpy(poses).cuda()
    tb = {"device form": [], "ccmp_object_propose_ref (one thread)": []}
    tc = {"device form, mask": [], "device form, early exit": [], "ccmp_object_valid_ref (one thread)": []}
    chk.propose(frm_d, goal_d, **kw), chk_big.valid(poses_d, want_mask=True), chk_big.valid(poses_d)
    torch.cuda.synchronize()
    for _ in range(reps_b):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        dev = chk.propose(frm_d, goal_d, **kw)
        e[1].record()
        dv = chk_big.valid(poses_d, want_mask=True)
        e[2].record()
        dq = chk_big.valid(poses_d)
        e[3].record()
        torch.cuda.synchronize()
        tb["device form"].append(e[0].elapsed_time(e[1]))
        tc["device form, mask"].append(e[1].elapsed_time(e[2]))
        tc["device form, early exit"].append(e[2].elapsed_time(e[3]))
        t0 = time.perf_counter()
        ref = object_propose_ref(mesh, boxes, frm, goal, **kw)
        t1 = time.perf_counter()
        rv = object_valid_ref(big, boxes, poses, want_mask=True)
        t2 = time.perf_counter()
        tb["ccmp_object_propose_ref (one thread)"].append((t1 - t0) * 1e3)
        tc["ccmp_object_valid_ref (one thread)"].append((t2 - t1) * 1e3)
        agree = agree and same({k: v.cpu().numpy() for k, v in dev.items()}, ref, ("pose", "which"))
        agree = agree and np.array_equal(dv[0].cpu().numpy(), rv[0]) and np.array_equal(dv[1].cpu().numpy().view(np.uint32), rv[1]) and np.array_equal(dq.cpu().numpy(), rv[0])
    print("(b) propose G = %d, 2 attempts, %d triangles, device form, device events; outputs identical: %s" % (Gb, len(mesh), agree))
    for name, ms in tb.items():
        print("    %-40s %s" % (name, _stat(ms)))
    print("    found %d of %d; by the first attempt %d" % (int((ref["which"] >= 0).sum()), Gb, int((ref["which"] == 0).sum())))
    print("(c) valid on 4096 poses, %d triangles; %d valid" % (len(big), int(rv[0].sum())))
    for name, ms in tc.items():
        print("    %-40s %s" % (name, _stat(ms)))
    print("VERDICT object device forms against one host thread: (a) %.2fx, (b) %.1fx, (c) %.1fx with the mask, %.1fx with the early exit"
          % (np.median(ta["ccmp_object_propose_ref (one thread)"]) / np.median(ta["host form (device)"]),
             np.median(tb["ccmp_object_propose_ref (one thread)"]) / np.median(tb["device form"]),
             np.median(tc["ccmp_object_valid_ref (one thread)"]) / np.median(tc["device form, mask"]),
             np.median(tc["ccmp_object_valid_ref (one thread)"]) / np.median(tc["device form, early exit"])))


def graph(argv):
    """ccmp_roadmap_commit / _closest / a one-edge label update against their *_ref forms (the same text on one host thread) on the same
    inputs; outputs compared while they are timed.  Writes profiles/roadmap_graph.md.  Inputs: tests/graph_cases.py."""
    import os

    sys.path.insert(0, "tests")
    from graph_cases import Graph, base_store, commit_args, initial_edges, make_case, union_find_labels

    from closed_chain_motion_planner_amd import Roadmap, closest_ref, commit_ref, graph_labels_ref

    reps = int(argv[0]) if len(argv) > 0 else 30
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    joints, poses, fresh, fresh_poses, goal = base_store()
    e0 = initial_edges(len(joints))
    lines = []

    def store():
        rm = Roadmap(c, capacity_hint=1 << 17)
        rm.append(torch.from_numpy(np.array(joints)).cuda(), torch.from_numpy(np.array(poses)).cuda())
        rm.add_edges(torch.from_numpy(e0).cuda())
        return rm

    def report(title, times, agree):
        print("%s; outputs identical: %s" % (title, agree))
        lines.append("%s; outputs identical: %s" % (title, agree))
        for name, ms in times.items():
            print("    %-44s %s" % (name, _stat(ms)))
            lines.append("    %-44s %s" % (name, _stat(ms)))

    # (a) the planner's shape: Q = 1, k = 5, lists of 64 states, host pointers, wall clock around the synchronous call
    rm = store()
    labels = union_find_labels(e0, len(joints))
    ta = {"ccmp_roadmap_commit_host (device)": [], "ccmp_roadmap_commit_ref (one thread)": []}
    agree = True
    for i in range(reps + 3):
        case = make_case(joints, poses, 1, 5, 900 + i, goal, fresh[i % 40:i % 40 + 1], fresh_poses[i % 40:i % 40 + 1], with_vertex_ok=False)
        wide = np.zeros((5, 64, 14))
        wide[:, :case["states"].shape[1]] = case["states"]
        case["states"], case["max_states"] = wide, 64
        kw = commit_args(case)
        n0, ne0 = len(rm), rm.num_edges
        t0 = time.perf_counter()
        dev = rm.commit(**kw)
        t1 = time.perf_counter()
        ref = commit_ref(c.problem, joints, poses, labels, **kw)
        t2 = time.perf_counter()
        agree = agree and all(np.array_equal(dev[k], ref[k]) for k in ("new_index", "mid_index", "grow_state")) and dev["edges_added"] == len(ref["edges_uv"])
        rm.close()
        rm = store()  # every call starts from the same store
        if i >= 3:
            ta["ccmp_roadmap_commit_host (device)"].append((t1 - t0) * 1e3)
            ta["ccmp_roadmap_commit_ref (one thread)"].append((t2 - t1) * 1e3)
    report("(a) commit Q = 1, k = 5, lists of 64, host form, wall clock", ta, agree)

    # (b) Q = 4096, k = 5: device pointers, wall clock to the end of the call (it ends with its own read-back)
    Q = 4096
    case = make_case(joints, poses, Q, 5, 77, goal, fresh, fresh_poses)
    kw = commit_args(case)
    kd = dict(kw)
    for name in ("nbr_idx", "edge_ok", "n_states", "new_joints", "new_poses", "states", "vertex_ok"):
        kd[name] = torch.from_numpy(np.ascontiguousarray(kw[name])).cuda()
    tb = {"ccmp_roadmap_commit (device)": [], "ccmp_roadmap_commit_ref (one thread)": []}
    agree = True
    for i in range(3 + 3):
        rm.close()
        rm = store()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = rm.commit(**kd)
        t1 = time.perf_counter()
        ref = commit_ref(c.problem, joints, poses, labels, **kw)
        t2 = time.perf_counter()
        agree = agree and all(np.array_equal(dev[k].cpu().numpy(), ref[k]) for k in ("new_index", "mid_index", "grow_state"))
        uv, w = rm.edges(len(e0), host=True)
        agree = agree and np.array_equal(uv, ref["edges_uv"]) and np.array_equal(w.view(np.uint8), ref["edges_w"].view(np.uint8))
        if i >= 3:
            tb["ccmp_roadmap_commit (device)"].append((t1 - t0) * 1e3)
            tb["ccmp_roadmap_commit_ref (one thread)"].append((t2 - t1) * 1e3)
    report("(b) commit Q = %d, k = 5, device form, wall clock to its read-back; %d vertices and %d edges added" % (Q, dev["vertices_added"], dev["edges_added"]), tb, agree)
    rm.close()

    # (c) closest and (d) a one-edge label update at N = 65536 (pose-only vertices; random edges: components of every size)
    N = 65536
    rng = np.random.default_rng(0x6A)
    big = np.zeros((N, 8))
    big[:, :3] = rng.uniform(-1, 1, (N, 3))
    quat = rng.normal(size=(N, 4))
    big[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    uv = rng.integers(0, N, size=(N, 2)).astype(np.int32)
    uv = np.ascontiguousarray(uv[uv[:, 0] != uv[:, 1]])
    rm = Roadmap(c, capacity_hint=N + 64)
    rm.append(None, torch.from_numpy(big).cuda())
    rm.add_edges(torch.from_numpy(uv).cuda())
    lab = rm.labels(host=True)
    agree = np.array_equal(lab, graph_labels_ref(uv, N))
    froms = np.array([int(np.argmax(np.bincount(lab)))], dtype=np.int32)  # a vertex of the largest component (its label is its smallest index)
    froms_d, tgt_d = torch.from_numpy(froms).cuda(), torch.from_numpy(big[7].copy()).cuda()
    tc = {"ccmp_roadmap_closest (device, events)": [], "ccmp_roadmap_closest_host (wall clock)": [], "ccmp_roadmap_closest_ref (one thread)": []}
    for i in range(reps + 3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        dev = rm.closest(froms_d, tgt_d)
        e[1].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = rm.closest(froms, big[7])
        t1 = time.perf_counter()
        ref = closest_ref(big, lab, froms, big[7])
        t2 = time.perf_counter()
        agree = agree and all(np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8)) and np.array_equal(h.view(np.uint8), b.view(np.uint8))
                              for a, h, b in zip(dev, host, ref))
        if i >= 3:
            tc["ccmp_roadmap_closest (device, events)"].append(e[0].elapsed_time(e[1]))
            tc["ccmp_roadmap_closest_host (wall clock)"].append((t1 - t0) * 1e3)
            tc["ccmp_roadmap_closest_ref (one thread)"].append((t2 - t1) * 1e3)
    report("(c) closest F = 1 at N = %d (from's component: %d vertices)" % (N, int((lab == lab[froms[0]]).sum())), tc, agree)
    td = {"ccmp_roadmap_add_edges_host, one edge (device)": [], "ccmp_graph_labels_ref, all edges (one thread)": []}
    done = uv
    for i in range(reps + 3):
        one = rng.integers(0, N, size=(1, 2)).astype(np.int32)
        if one[0, 0] == one[0, 1]:
            continue
        t0 = time.perf_counter()
        rm.add_edges(one)
        t1 = time.perf_counter()
        done = np.concatenate([done, one])
        want = graph_labels_ref(done, N)
        t2 = time.perf_counter()
        agree = agree and np.array_equal(rm.labels(host=True), want)
        if i >= 3:
            td["ccmp_roadmap_add_edges_host, one edge (device)"].append((t1 - t0) * 1e3)
            td["ccmp_graph_labels_ref, all edges (one thread)"].append((t2 - t1) * 1e3)
    report("(d) one-edge label update at N = %d, %d edges, host form, wall clock (the host contender has no incremental form: it rebuilds)" % (N, len(done)), td, agree)
    rm.close()
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "roadmap_graph.md"), "w") as f:
        f.write("# Roadmap graph on the device: `tools/measure.py graph`\n\n1 x MI355X, one run; every device form against its `_ref` form on one host thread on the "
                "same inputs, the outputs compared while they are timed.  No speed threshold gates this feature.\n\n```\n" + "\n".join(lines) + "\n```\n")


def path(argv):
    """ccmp_roadmap_shortest_paths (device form: events; host form: wall clock) against ccmp_graph_shortest_paths_ref (heap Dijkstra, one
    host thread) on the same inputs; outputs compared while they are timed.  Writes profiles/roadmap_path.md."""
    import os

    from closed_chain_motion_planner_amd import Roadmap, shortest_paths_ref

    reps = int(argv[0]) if len(argv) > 0 else 15
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    def same(a, b):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))

    for N, E in ((65536, 65536), (2000, 5000)):
        rng = np.random.default_rng(0x9A7 + N)
        joints = rng.uniform(-2.8, 2.8, (N, 14))
        poses = np.zeros((N, 8))
        poses[:, :3] = joints[:, :3]
        poses[:, 6] = 1.0
        uv = rng.integers(0, N, size=(E, 2)).astype(np.int32)
        uv = np.ascontiguousarray(uv[uv[:, 0] != uv[:, 1]])
        rm = Roadmap(c, capacity_hint=N + 64)
        rm.append(torch.from_numpy(joints).cuda(), torch.from_numpy(poses).cuda())
        rm.add_edges(torch.from_numpy(uv).cuda())
        lab = rm.labels(host=True)
        comp = np.flatnonzero(lab == np.bincount(lab).argmax())  # the largest component
        _, w = rm.edges(host=True)
        for F in (1, 64):
            pick = rng.choice(comp, size=(F, 2))
            src, dst = np.ascontiguousarray(pick[:, 0].astype(np.int32)), np.ascontiguousarray(pick[:, 1].astype(np.int32))
            src_d, dst_d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            ref = shortest_paths_ref(uv, w, N, src, dst)
            L = int(ref[1].max())
            t = {"ccmp_roadmap_shortest_paths (device, events)": [], "ccmp_roadmap_shortest_paths_host (wall clock)": [],
                 "ccmp_graph_shortest_paths_ref (one thread)": [], "round trip on the host: read_edges_host + _ref + rows re-uploaded": [],
                 "round trip on the device: shortest_paths, rows stay": []}
            agree = True
            for i in range(reps + 3):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                dev = rm.shortest_paths(src_d, dst_d, max_len=L)
                e[1].record()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = rm.shortest_paths(src, dst, max_len=L, host=True)
                t1 = time.perf_counter()
                ref = shortest_paths_ref(uv, w, N, src, dst)
                t2 = time.perf_counter()
                # the full round trip, as a caller without this call has it: the edge list down, the search, the chosen rows up again
                uv_h, w_h = rm.edges(host=True)
                r2 = shortest_paths_ref(uv_h, w_h, N, src, dst)
                rows = [torch.from_numpy(joints[p]).cuda() for p in r2[2]]
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                d2 = rm.shortest_paths(src_d, dst_d, max_len=L)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                dl, dp = dev["path_len"].cpu().numpy(), dev["path"].cpu().numpy()
                agree = agree and same(dev["cost"].cpu().numpy(), ref[0]) and same(host["cost"], ref[0]) and np.array_equal(dl, ref[1]) and np.array_equal(host["path_len"], ref[1])
                agree = agree and all(np.array_equal(dp[f, :dl[f]], ref[2][f]) and np.array_equal(host["path"][f, :dl[f]], ref[2][f]) for f in range(F))
                agree = agree and all(same(d2["joints"][f, :dl[f]].cpu().numpy(), rows[f].cpu().numpy()) for f in range(F))
                if i >= 3:
                    for name, ms in zip(t, (e[0].elapsed_time(e[1]), (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3)):
                        t[name].append(ms)
            rounds = rm.path_rounds(F)
            say("N = %d, %d edges, F = %d (largest component: %d vertices; longest path %d vertices); outputs identical: %s" % (N, len(uv), F, len(comp), L, agree))
            say("    rounds per pair: relaxation %d .. %d (median %d), hops %d .. %d (median %d)"
                % (rounds[:, 0].min(), rounds[:, 0].max(), int(np.median(rounds[:, 0])), rounds[:, 1].min(), rounds[:, 1].max(), int(np.median(rounds[:, 1]))))
            for name, ms in t.items():
                say("    %-68s %s" % (name, _stat(ms)))
        rm.close()
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "roadmap_path.md"), "w") as f:
        f.write("# Shortest paths on the device roadmap: `tools/measure.py path`\n\n1 x MI355X, one run; the device forms against `ccmp_graph_shortest_paths_ref` "
                "(heap Dijkstra on one host thread) on the same inputs, the outputs compared while they are timed.  No speed threshold gates this feature.\n\n```\n"
                + "\n".join(lines) + "\n```\n")


def dense(argv):
    """ccmp_path_densify (KinematicChainConstraint.densify_paths: the continuation loop in the library, the lists stay on the device) against
    the route a caller had before it on the same waypoints: discrete_geodesic_batch + continue_geodesics (every open list downloaded), the
    join of the lists on the host by the rule, and the upload of the joined rows.  Near-sampling chains of 32 waypoints, one path and 64
    paths, both Jacobian modes, lists of 16 and a round budget of 128 on both routes; wall clock around each synchronous route, medians;
    the outputs compared while they are timed.  Writes profiles/dense_path.md."""
    import os

    reps = int(argv[0]) if len(argv) > 0 else 15
    Lw, cs, budget = 32, 16, 128
    ctx = Context(0)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    for mode in (0, 1):
        c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
        cols = [c.sample_project_batch(0xDE5, 0, 64, want_iters=False)[0]]
        for j in range(1, Lw):
            cols.append(c.sample_near_project_batch(0xDE5 + j, 0, cols[-1], 0.6, 64, want_iters=False)[0])
        chains = torch.stack(cols, dim=1).contiguous()  # the FD constraint's samples for both modes
        c.setJacobianMode(mode)
        extend_sizes = []  # edges of every extend call the old route makes: what it brings to the host is a function of them
        plain = c.discrete_geodesic_batch

        def logged(frm, to, *a, **k):
            extend_sizes.append(frm.shape[0])
            return plain(frm, to, *a, **k)

        for F in (1, 64):
            pj = chains[:F].contiguous()
            pl = torch.full((F,), Lw, dtype=torch.int32, device=pj.device)
            frm, to = pj[:, :-1].reshape(-1, 14).contiguous(), pj[:, 1:].reshape(-1, 14).contiguous()
            S = frm.shape[0]

            def old_route():
                c.discrete_geodesic_batch = logged
                try:
                    s, n, ok, its, carry = c.discrete_geodesic_batch(frm, to, cs, want_carry=True, round_budget=budget)
                    cont = c.continue_geodesics(to, s, n, ok, its, carry, cs, round_budget=budget)
                finally:
                    del c.discrete_geodesic_batch
                s_h, n_h, wp = s.cpu().numpy(), n.cpu().numpy(), pj.cpu().numpy()
                rows = []
                for f in range(F):  # the rule, on the host: w_i, G_i, .., the last waypoint
                    for i in range(Lw - 1):
                        e = f * (Lw - 1) + i
                        rows.append(wp[f, i][None])
                        rows.append(cont[e][0] if e in cont else s_h[e, : n_h[e]])
                    rows.append(wp[f, Lw - 1][None])
                joined = np.concatenate(rows, axis=0)
                up = torch.from_numpy(joined).cuda()  # ... and back up for whatever runs on the dense path next
                torch.cuda.synchronize()
                return joined, up

            t_new, t_old, agree, calls = [], [], True, 0
            for i in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                new = c.densify_paths(pj, pl, chunk_states=cs, round_budget=budget)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                extend_sizes.clear()
                joined, up = old_route()
                t2 = time.perf_counter()
                calls = new["calls"]
                agree = agree and np.array_equal(new["joints"].cpu().numpy().view(np.uint64), joined.view(np.uint64)) and len(extend_sizes) == calls
                if i >= 3:
                    t_new.append((t1 - t0) * 1e3)
                    t_old.append((t2 - t1) * 1e3)
            # bytes to the host.  new: path_len once, then n_states and ok of every open segment of every extend call.  old: the first
            # call's lists whole with their counts, the open subset's lists again, every continuation call's lists, counts, flags and iterations
            per_list = cs * 14 * 8
            new_bytes = 4 * F + 5 * sum(extend_sizes)
            old_bytes = S * (per_list + 4) + (extend_sizes[1] if len(extend_sizes) > 1 else 0) * (per_list + 8) + sum(extend_sizes[1:]) * (per_list + 9)
            say("%s mode, F = %d paths x %d waypoints (%d segments, %d dense rows); outputs identical: %s" % ("analytic" if mode else "FD", F, Lw, S, new["rows"], agree))
            say("    extend calls %d (open segments per call: %s); bytes to the host: densify %d, old route %d" % (calls, extend_sizes[:8] + (["..."] if len(extend_sizes) > 8 else []), new_bytes, old_bytes))
            say("    %-72s %s" % ("ccmp_path_densify (rows stay on the device)", _stat(t_new)))
            say("    %-72s %s" % ("discrete_geodesic_batch + continue_geodesics + host join + upload", _stat(t_old)))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "dense_path.md"), "w") as f:
        f.write("# Dense solution paths on the device: `tools/measure.py dense`\n\n1 x MI355X, one run; `ccmp_path_densify` against the route a caller had before it "
                "(extend call, continuation with every open list downloaded, join on the host, upload of the joined rows) on the same waypoints, wall clock around each "
                "synchronous route, the outputs compared while they are timed.  No speed threshold gates this feature.\n\n```\n" + "\n".join(lines) + "\n```\n")


def shortcut(argv):
    """ccmp_path_shortcut (KinematicChainConstraint.shortcut_paths: every pair of a path's waypoints put to checkMotion in one batch inside
    the library, then the DAG search on the device) against the same work through the calls a caller had before it: the pairs enumerated on
    the host, discrete_geodesic_batch(check_target=True) + continue_geodesics over all of them, the flags and the waypoints brought to the
    host, the joint distances and the selection in numpy.  Paths of 32 waypoints out of a roadmap store: 64 chains of near-sampled
    milestones appended with their chain edges, each path the store's shortest path between a chain's ends (seed 0x5C7); one path and 64
    paths, both Jacobian modes, lists of 16 and a round budget of 128 on both routes; wall clock around each synchronous route, medians;
    the outputs compared while they are timed.  Writes profiles/shortcut.md."""
    import os

    from closed_chain_motion_planner_amd import Roadmap

    reps = int(argv[0]) if len(argv) > 0 else 15
    Lw, cs, budget, seed = 32, 16, 128, 0x5C7
    ctx = Context(0)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    for mode in (0, 1):
        c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
        cols = [c.sample_project_batch(seed, 0, 64, want_iters=False)[0]]
        for j in range(1, Lw):
            cols.append(c.sample_near_project_batch(seed + j, 0, cols[-1], 0.6, 64, want_iters=False)[0])
        chains = torch.stack(cols, dim=1).contiguous()  # the FD constraint's samples for both modes
        rm = Roadmap(c, capacity_hint=64 * Lw)
        rm.append(chains.reshape(-1, 14).contiguous())
        uv = np.array([(f * Lw + i, f * Lw + i + 1) for f in range(64) for i in range(Lw - 1)], dtype=np.int32)
        rm.add_edges(torch.from_numpy(uv).cuda())
        c.setJacobianMode(mode)
        extend_sizes = []
        plain = c.discrete_geodesic_batch

        def logged(frm, to, *a, **k):
            extend_sizes.append(frm.shape[0])
            return plain(frm, to, *a, **k)

        for F in (1, 64):
            src = np.arange(F, dtype=np.int32) * Lw
            sp = rm.shortest_paths(torch.from_numpy(src).cuda(), torch.from_numpy(src + Lw - 1).cuda(), max_len=Lw)
            pj, pl = sp["joints"].contiguous(), sp["path_len"].contiguous()
            assert pj.shape[1] == Lw and int(pl.min()) == Lw
            ii, jj = np.triu_indices(Lw, 2)
            E = F * len(ii)

            def old_route():
                wp = pj.cpu().numpy()  # the waypoints cross once: the weights are computed on the host
                sel_f = np.repeat(np.arange(F), len(ii))
                frm = pj[torch.from_numpy(sel_f).cuda(), torch.from_numpy(np.tile(ii, F)).cuda()].contiguous()
                to = pj[torch.from_numpy(sel_f).cuda(), torch.from_numpy(np.tile(jj, F)).cuda()].contiguous()
                c.discrete_geodesic_batch = logged
                try:
                    s, n, ok, its, carry = c.discrete_geodesic_batch(frm, to, cs, check_target=True, want_carry=True, round_budget=budget)
                    cont = c.continue_geodesics(to, s, n, ok, its, carry, cs, round_budget=budget)
                finally:
                    del c.discrete_geodesic_batch
                flag = ok.cpu().numpy().copy()
                for e, v in cont.items():
                    flag[e] = v[1]
                okm = np.zeros((F, Lw, Lw), dtype=np.uint8)
                okm[sel_f, np.tile(ii, F), np.tile(jj, F)] = flag
                kept, cost = [], []
                for f in range(F):  # the selection in numpy: one forward sweep, (cost, hops, index) lexicographic
                    W = np.sqrt(((wp[f][:, None, :] - wp[f][None, :, :]) ** 2).sum(-1))
                    d, h, pr = np.full(Lw, np.inf), np.zeros(Lw, dtype=np.int64), np.full(Lw, -1)
                    d[0] = 0.0
                    for j in range(1, Lw):
                        adm = (okm[f, :j, j] == 1) | (np.arange(j) == j - 1)
                        cnd = np.where(adm & np.isfinite(d[:j]), d[:j] + W[:j, j], np.inf)
                        best = cnd.min()
                        if np.isfinite(best):
                            t = np.nonzero(cnd == best)[0]
                            i = t[np.argmin(h[t])]
                            d[j], h[j], pr[j] = best, h[i] + 1, i
                    k, v = [], Lw - 1
                    while v >= 0:
                        k.append(v)
                        v = pr[v]
                    kept.append(k[::-1])
                    cost.append(d[Lw - 1])
                return okm, kept, cost

            t_new, t_old, agree = [], [], True
            for i in range(reps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                new = c.shortcut_paths(pj, pl, chunk_states=cs, round_budget=budget, pairs=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                extend_sizes.clear()
                okm, kept, cost = old_route()
                t2 = time.perf_counter()
                nk, nl = new["kept"].cpu().numpy(), new["out_len"].cpu().numpy()
                agree = agree and np.array_equal(new["pair_ok"].cpu().numpy(), okm) and all(nk[f, : nl[f]].tolist() == kept[f] for f in range(F))
                if i >= 3:
                    t_new.append((t1 - t0) * 1e3)
                    t_old.append((t2 - t1) * 1e3)
            # bytes to the host.  new: path_len once, then n_states and ok of every open pair of every extend call.  old: the waypoints, the
            # first call's flags, the open subset's lists, and every continuation call's lists, counts, flags and iterations
            per_list = cs * 14 * 8
            new_bytes = 4 * F + 5 * sum(extend_sizes)
            old_bytes = F * Lw * 14 * 8 + E + (extend_sizes[1] if len(extend_sizes) > 1 else 0) * (per_list + 8) + sum(extend_sizes[1:]) * (per_list + 9)
            say("%s mode, F = %d paths x %d waypoints (%d pairs tested, %d passed; %.1f waypoints kept per path); pair flags and kept vertices identical: %s"
                % ("analytic" if mode else "FD", F, Lw, E, int(okm.sum()), float(np.mean([len(k) for k in kept])), agree))
            say("    extend calls %d (open pairs per call: %s); bytes to the host: shortcut %d, old route %d"
                % (len(extend_sizes), extend_sizes[:8] + (["..."] if len(extend_sizes) > 8 else []), new_bytes, old_bytes))
            say("    %-84s %s" % ("ccmp_path_shortcut (pairs, flags and the search stay on the device)", _stat(t_new)))
            say("    %-84s %s" % ("discrete_geodesic_batch(check_target) + continue_geodesics + selection in numpy", _stat(t_old)))
        rm.close()
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "shortcut.md"), "w") as f:
        f.write("# Shortcut solution paths on the device: `tools/measure.py shortcut`\n\n1 x MI355X, one run, seed 0x5C7; `ccmp_path_shortcut` against the same work through "
                "the calls a caller had before it (pairs enumerated on the host, `discrete_geodesic_batch(check_target=True)` and its continuation over all pairs, "
                "the selection in numpy) on the same waypoints, wall clock around each synchronous route, the outputs compared while they are timed.  "
                "No speed threshold gates this feature.\n\n```\n" + "\n".join(lines) + "\n```\n")


def _smooth_paths(c, F, Lw, seed):
    """F chains of Lw near-sampled milestones (the shortcut measurement's chains): (F,Lw,14) and (F,) int32 on the device"""
    cols = [c.sample_project_batch(seed, 0, F, want_iters=False)[0]]
    for j in range(1, Lw):
        cols.append(c.sample_near_project_batch(seed + j, 0, cols[-1], 0.6, F, want_iters=False)[0])
    return torch.stack(cols, dim=1).contiguous(), torch.full((F,), Lw, dtype=torch.int32, device="cuda")


def smooth(argv):
    """ccmp_path_smooth (KinematicChainConstraint.smooth_paths): three passes on 1 and 64 paths of 32 waypoints (chains of near-sampled
    milestones of the FD constraint, seed 0x5C7), both Jacobian modes, lists of 16 and a round budget of 128; wall clock around the
    synchronous call, medians; the extend calls, projector calls and bytes read on the host as the library counts them
    (ccmp_smooth_last_counts).  With a second argument the inputs and results are written there (.npz) for `smooth_restate`.  Writes
    profiles/smooth.md."""
    import os

    reps = int(argv[0]) if len(argv) > 0 else 9
    dump = argv[1] if len(argv) > 1 else None
    Lw, seed, steps = 32, 0x5C7, 3
    ctx = Context(0)
    lines, saved = [], {}

    def say(text):
        print(text)
        lines.append(text)

    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    pj, pl = _smooth_paths(c, 64, Lw, seed)  # the FD constraint's samples for both modes
    saved["path_joints"] = pj.cpu().numpy()
    for mode in (0, 1):
        c.setJacobianMode(mode)
        for F in (1, 64):
            a, b = pj[:F].contiguous(), pl[:F].contiguous()
            t = []
            for i in range(reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = c.smooth_paths(a, b, max_steps=steps, stats=True)
                torch.cuda.synchronize()
                if i >= 2:
                    t.append((time.perf_counter() - t0) * 1e3)
            calls, projects, nbytes = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
            _lib.lib().ccmp_smooth_last_counts(C.byref(calls), C.byref(projects), C.byref(nbytes))
            o = {k: v.cpu().numpy() for k, v in out.items()}
            for k, v in o.items():
                saved["mode%d_F%d_%s" % (mode, F, k)] = v
            say("%s mode, F = %d paths x %d waypoints, %d passes: %d -> %d vertices, moved %d, length %.3f -> %.3f per path, stop %s, stats (projected, fallback, "
                "degenerate, refused, below) %s" % ("analytic" if mode else "FD", F, Lw, steps, F * Lw, int(o["out_len"].sum()), int(o["moved"].sum()),
                                                  float(o["length_in"].mean()), float(o["length_out"].mean()), sorted(set(o["stop"].tolist())), o["stats"].sum(0).tolist()))
            say("    extend calls %d, projector calls %d, bytes read on the host %d" % (calls.value, projects.value, nbytes.value))
            say("    %-84s %s" % ("ccmp_path_smooth (every state stays on the device)", _stat(t)))
    if dump:
        np.savez(dump, **saved)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "smooth.md"), "w") as f:
        f.write("# Smooth solution paths on the device: `tools/measure.py smooth`\n\n1 x MI355X, one run, seed 0x5C7; `ccmp_path_smooth`, three passes, lists of 16, round "
                "budget 128, wall clock around the synchronous call.  No speed threshold gates this feature.\n\n```\n" + "\n".join(lines) + "\n```\n")


def retime(argv):
    """ccmp_path_resample and ccmp_path_timestamps (KinematicChainConstraint.resample_paths / timestamp_paths) on the smooth measurement's
    inputs, continued: 1 and 64 paths of 32 waypoints, three smoothing passes, densified, then resampled at the problem's delta and stamped
    under the Panda's limits, both Jacobian modes; wall clock around each call (resample is synchronous; the stamps are followed by a
    synchronize), medians; the kind counts.  Then, on the CPU _ref form, the reference's two recorded path files: the duration under the
    Panda's limits beside the 2.5 s of scripts/execute_path.py, and the largest finite-difference joint acceleration of the stamped
    trajectory as a multiple of amax (reported, not asserted: the rule bounds the profile, not finite differences).  Writes
    profiles/retime.md."""
    import os

    from closed_chain_motion_planner_amd import PANDA_ACCELERATION_LIMITS, PANDA_VELOCITY_LIMITS, RETIME_STATUS, timestamps_ref

    reps = int(argv[0]) if len(argv) > 0 else 9
    Lw, seed, steps = 32, 0x5C7, 3
    vmax, amax = PANDA_VELOCITY_LIMITS * 2, PANDA_ACCELERATION_LIMITS * 2
    ctx = Context(0)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    pj, pl = _smooth_paths(c, 64, Lw, seed)  # the FD constraint's samples for both modes
    for mode in (0, 1):
        c.setJacobianMode(mode)
        for F in (1, 64):
            sm = c.smooth_paths(pj[:F].contiguous(), pl[:F].contiguous(), max_steps=steps)
            dense = c.densify_paths(sm["joints"], sm["out_len"], distinct=True, keep_handle=True)
            t_rs, t_ts = [], []
            for i in range(reps + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rs = c.resample_paths(dense)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ts = c.timestamp_paths(rs["joints"], rs["path_first"], vmax, amax)
                torch.cuda.synchronize()
                if i >= 2:
                    t_rs.append((t1 - t0) * 1e3)
                    t_ts.append((time.perf_counter() - t1) * 1e3)
            dense["handle"].close()
            status = rs["status"].cpu().numpy()
            dur = ts["duration"].cpu().numpy()[status == 0]
            say("%s mode, F = %d smoothed paths, %d dense rows -> %d rows at spacing %.3g; status %s; kinds (projected, fallback, degenerate, copied) %s; "
                "duration %.2f s per path (median over the OK paths)"
                % ("analytic" if mode else "FD", F, dense["rows"], rs["rows"], c.problem.delta, {RETIME_STATUS[k]: int((status == k).sum()) for k in sorted(set(status.tolist()))},
                   rs["counts"].sum(0).cpu().tolist(), float(np.median(dur)) if len(dur) else float("nan")))
            say("    %-84s %s" % ("ccmp_path_resample (one projector call for all paths; the mirror's copy-out included)", _stat(t_rs)))
            say("    %-84s %s" % ("ccmp_path_timestamps (four launches, no host read)", _stat(t_ts)))
    say("")
    say("the reference's recorded paths, stamped on the CPU (ccmp_path_timestamps_ref) under the Panda's limits, beta 0.5:")
    for obj in ("Wine_Bottle", "dumbbell"):
        rows = np.loadtxt(os.path.join("tests", "golden", "paths", obj + "_path.txt"))
        out = timestamps_ref(rows, np.array([0, len(rows)], dtype=np.int32), vmax, amax)
        t = out["time"]
        keep = np.concatenate([[True], np.diff(t) > 0])  # a repeated waypoint row at the same time is one sample
        q, tt = rows[keep], t[keep]
        v = np.diff(q, axis=0) / np.diff(tt)[:, None]
        acc = np.diff(v, axis=0) / (0.5 * (tt[2:] - tt[:-2]))[:, None]
        say("    %-12s %2d rows: duration %.3f s (scripts/execute_path.py: 2.5 s for every path); largest finite-difference speed %.2f x vmax, acceleration %.2f x amax"
            % (obj, len(rows), float(out["duration"][0]), float((np.abs(v) / np.array(vmax)).max()), float((np.abs(acc) / np.array(amax)).max())))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "retime.md"), "w") as f:
        f.write("# Resample and time stamps on the device: `tools/measure.py retime`\n\n1 x MI355X, one run, seed 0x5C7; the smooth measurement's inputs, continued: "
                "three smoothing passes, densified (distinct layout), `ccmp_path_resample` at the problem's delta, `ccmp_path_timestamps` under the Panda's data-sheet "
                "limits; wall clock around each call, no GPU time measured.  No speed threshold gates this feature.  The finite-difference figures are reported, not "
                "asserted: the rule bounds the speed profile at the rows, not finite differences of the sampled trajectory.\n\n```\n" + "\n".join(lines) + "\n```\n")


def setpoints(argv):
    """ccmp_path_setpoints (KinematicChainConstraint.setpoint_paths) on the retime measurement's inputs, continued: 1 and 64 paths of 32
    waypoints, three smoothing passes, densified, resampled at the problem's delta and stamped under the Panda's limits, then the
    setpoints at 1 ms with their audit; wall clock around the synchronous call (the mirror's copy-out included), medians; the ticks, the
    statuses and the medians of the peaks.  Then the reference's two recorded path files, stamped on the CPU (ccmp_path_timestamps_ref)
    and put through the device call at 1 ms: the audit's five peaks, where they occur, and the stretch — the library's own figures for
    what the time stamps leave open.  Writes profiles/setpoints.md."""
    import os

    from closed_chain_motion_planner_amd import PANDA_ACCELERATION_LIMITS, PANDA_VELOCITY_LIMITS, SETPOINT_STATUS, timestamps_ref

    reps = int(argv[0]) if len(argv) > 0 else 9
    Lw, seed, steps = 32, 0x5C7, 3
    vmax, amax = PANDA_VELOCITY_LIMITS * 2, PANDA_ACCELERATION_LIMITS * 2
    ctx = Context(0)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    pj, pl = _smooth_paths(c, 64, Lw, seed)
    c.setJacobianMode(1)  # the setpoints do not depend on the mode; the path that feeds them is made in analytic mode
    for F in (1, 64):
        sm = c.smooth_paths(pj[:F].contiguous(), pl[:F].contiguous(), max_steps=steps)
        dense = c.densify_paths(sm["joints"], sm["out_len"], distinct=True, keep_handle=True)
        rs = c.resample_paths(dense)
        dense["handle"].close()
        ts = c.timestamp_paths(rs["joints"], rs["path_first"], vmax, amax)
        t_sp = []
        for i in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp = c.setpoint_paths(rs["joints"], rs["path_first"], ts["time"], vmax, amax)
            torch.cuda.synchronize()
            if i >= 2:
                t_sp.append((time.perf_counter() - t0) * 1e3)
        status = sp["status"].cpu().numpy()
        ok = status == 0
        peak = sp["peak"].cpu().numpy()[ok]
        say("F = %d paths, %d rows at spacing %.3g -> %d ticks at 1 ms; status %s; medians over the OK paths: speed %.2f x vmax, acceleration %.2f x amax, "
            "max |dp| %.2e m, max angle %.2e rad, stretch %.2f; %d of the ticks refused by isSatisfied"
            % (F, rs["rows"], c.problem.delta, sp["ticks"], {SETPOINT_STATUS[k]: int((status == k).sum()) for k in sorted(set(status.tolist()))},
               *([float(np.median(peak[:, k])) for k in range(4)] if len(peak) else [float("nan")] * 4),
               float(np.median(sp["stretch"].cpu().numpy()[ok])) if ok.any() else float("nan"), int(sp["counts"][:, 0].sum())))
        say("    %-84s %s" % ("ccmp_path_setpoints (status read, four launches, function + isSatisfied over all ticks; copy-out included)", _stat(t_sp)))
    say("")
    say("the reference's recorded paths, stamped on the CPU (ccmp_path_timestamps_ref) under the Panda's limits, beta 0.5, then ccmp_path_setpoints at 1 ms:")
    for obj in ("Wine_Bottle", "dumbbell"):
        rows = np.loadtxt(os.path.join("tests", "golden", "paths", obj + "_path.txt"))
        first = np.array([0, len(rows)], dtype=np.int32)
        t = timestamps_ref(rows, first, vmax, amax)["time"]
        c2 = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        sp = c2.setpoint_paths(rows, first, t, vmax, amax)
        p, j = sp["peak"][0], sp["peak_tick"][0]
        say("    %-12s %2d rows, %.3f s, status %s: %d ticks; speed %.3f x vmax at tick %d; mean tick-interval acceleration %.3f x amax at tick %d; max |dp| %.3e m at "
            "tick %d; max angle %.3e rad at tick %d; clearance %s (no scene); %d ticks refused by isSatisfied; stretch %.3f"
            % (obj, len(rows), float(t[-1]), SETPOINT_STATUS[int(sp["status"][0])], sp["ticks"], p[0], j[0], p[1], j[1], p[2], j[2], p[3], j[3], p[4], int(sp["counts"][0, 0]),
               float(sp["stretch"][0])))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "setpoints.md"), "w") as f:
        f.write("# Setpoints and the execution audit on the device: `tools/measure.py setpoints`\n\n1 x MI355X, one run, seed 0x5C7; the retime measurement's inputs, "
                "continued: three smoothing passes, densified (distinct layout), resampled at the problem's delta, stamped under the Panda's data-sheet limits, then "
                "`ccmp_path_setpoints` at a period of 1 ms; wall clock around the synchronous call, no GPU time measured.  No speed threshold gates this feature.  "
                "The audit's figures are measurements of the executed motion, not bounds: the time stamps bound their profile at the rows, and these are what the "
                "commanded trajectory does between them.  The setpoints are not projected; `max |dp|` and `max angle` are the gap that leaves (the projector's "
                "tolerances are 1e-3 m and 5e-3 rad: at a spacing of the problem's delta most ticks are outside them, which is what the audit is for).  A path "
                "the resampling refused (`profiles/retime.md`: 59 of the 64 are broken, a segment that stops short) arrives without rows and answers EMPTY.\n\n```\n"
                + "\n".join(lines) + "\n```\n")


def _fit_by_hand(c, rows, first, time_dev, vmax, amax, period=0.001, max_ticks=65536, aim=0.95, max_passes=8):
    """the loop a caller would write without ccmp_path_fit_timestamps, on the rule of csrc/ccmp_fit.h: ccmp_path_setpoints per trial (it
    materialises every tick and runs the gap and isSatisfied over them: that is the call there is), qd, tau, tick_first and status copied to
    the host, S and A per row interval and the dilation in numpy, the stamps uploaded again.  -> (stamps (R,) numpy, passes [F], status [F])"""
    pf = first.cpu().numpy()
    F = len(pf) - 1
    t = time_dev.cpu().numpy().copy()
    v, a = np.array(vmax), np.array(amax)
    passes, status, open_ = [0] * F, [-1] * F, set(range(F))
    while open_:
        sp = c.setpoint_paths(rows, first, torch.from_numpy(t).cuda(), vmax, amax, period=period, max_ticks=max_ticks)
        qd, tau, tf, st = (sp[k].cpu().numpy() for k in ("qd", "tau", "tick_first", "status"))
        for f in sorted(open_):
            if st[f] != 0:
                status[f] = int(st[f])
                open_.discard(f)
                continue
            r0, r1, g0, g1 = pf[f], pf[f + 1], tf[f], tf[f + 1]
            tt, ta, w = t[r0:r1], tau[g0:g1], qd[g0:g1]
            k = np.searchsorted(tt, ta, side="left")  # the smallest k with t_k >= tau (>= 1 for tau > 0)
            k[0] = k[1]
            S, A = np.zeros(r1 - r0), np.zeros(r1 - r0)
            np.maximum.at(S, k, (np.abs(w) / v).max(axis=1))
            width = ta[1:] - ta[:-1]
            with np.errstate(all="ignore"):  # (an interval of no width is masked below)
                acc = ((np.abs(w[1:] - w[:-1]) / width[:, None]) / a).max(axis=1)
            for span in range(int((k[1:] - k[:-1]).max()) + 1):  # a tick interval owns every row interval from k_j to k_{j+1}
                on = (k[1:] - k[:-1] >= span) & (width > 0.0)
                np.maximum.at(A, k[:-1][on] + span, acc[on])
            if S[1:].max() <= 1.0 and A[1:].max() <= 1.0:
                status[f] = 0
                open_.discard(f)
            elif passes[f] == max_passes:
                status[f] = 6
                open_.discard(f)
            else:
                fk = np.maximum(1.0, np.maximum(S[1:] / aim, np.sqrt(A[1:] / aim)))
                t[r0] = 0.0
                t[r0 + 1:r1] = np.cumsum((tt[1:] - tt[:-1]) * fk)
                passes[f] += 1
    return t, passes, status


def fit(argv):
    """ccmp_path_fit_timestamps (KinematicChainConstraint.fit_timestamps) at 1 ms on the retime measurement's inputs, continued: 1 and 64 paths
    of 32 waypoints, three smoothing passes, densified, resampled at the problem's delta and stamped under the Panda's limits; beside it the
    loop a caller would write today (_fit_by_hand).  The two must give the same stamps bit for bit before either is timed; wall clock around
    each, medians.  Then the reference's two recorded path files, stamped on the CPU (ccmp_path_timestamps_ref): passes, the duration
    before and after, and the duration a uniform stretch by ccmp_path_setpoints' factor would give, at 1 ms and 4 ms.  Writes
    profiles/fit.md."""
    import os

    from closed_chain_motion_planner_amd import FIT_STATUS, PANDA_ACCELERATION_LIMITS, PANDA_VELOCITY_LIMITS, timestamps_ref

    reps = int(argv[0]) if len(argv) > 0 else 9
    Lw, seed, steps = 32, 0x5C7, 3
    vmax, amax = PANDA_VELOCITY_LIMITS * 2, PANDA_ACCELERATION_LIMITS * 2
    ctx = Context(0)
    lines = []

    def say(text):
        print(text)
        lines.append(text)

    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    pj, pl = _smooth_paths(c, 64, Lw, seed)
    c.setJacobianMode(1)  # the fit does not depend on the mode; the path that feeds it is made in analytic mode
    for F in (1, 64):
        sm = c.smooth_paths(pj[:F].contiguous(), pl[:F].contiguous(), max_steps=steps)
        dense = c.densify_paths(sm["joints"], sm["out_len"], distinct=True, keep_handle=True)
        rs = c.resample_paths(dense)
        dense["handle"].close()
        ts = c.timestamp_paths(rs["joints"], rs["path_first"], vmax, amax)
        out = c.fit_timestamps(rs["joints"], rs["path_first"], ts["time"], vmax, amax)
        by_hand, hand_passes, hand_status = _fit_by_hand(c, rs["joints"], rs["path_first"], ts["time"], vmax, amax)
        got = out["time"].cpu().numpy()
        same = np.array_equal(got.view(np.uint64), by_hand.view(np.uint64)) and out["passes"].cpu().tolist() == hand_passes and out["status"].cpu().tolist() == hand_status
        if not same:
            raise SystemExit("the fused call and the loop by hand disagree: nothing is timed")
        t_fit, t_hand = [], []
        for i in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.fit_timestamps(rs["joints"], rs["path_first"], ts["time"], vmax, amax)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _fit_by_hand(c, rs["joints"], rs["path_first"], ts["time"], vmax, amax)
            torch.cuda.synchronize()
            if i >= 2:
                t_fit.append((t1 - t0) * 1e3)
                t_hand.append((time.perf_counter() - t1) * 1e3)
        status, passes = out["status"].cpu().numpy(), out["passes"].cpu().numpy()
        ran = np.isin(status, (0, 6))
        d0, d1 = ts["duration"].cpu().numpy()[ran], out["duration"].cpu().numpy()[ran]
        sp = c.setpoint_paths(rs["joints"], rs["path_first"], ts["time"], vmax, amax)
        stretch = sp["stretch"].cpu().numpy()[ran]
        say("F = %d paths, %d rows at spacing %.3g, %d ticks at 1 ms before the fit; status %s; dilations %s; durations %s -> %s s (a uniform stretch: %s s); the stamps of "
            "both ways agree bit for bit" % (F, rs["rows"], c.problem.delta, sp["ticks"], {FIT_STATUS[k]: int((status == k).sum()) for k in sorted(set(status.tolist()))},
                                            passes[ran].tolist(), np.round(d0, 3).tolist(), np.round(d1, 3).tolist(), np.round(stretch * d0, 3).tolist()))
        say("    %-100s %s" % ("ccmp_path_fit_timestamps (per pass: status read, tangent, measure, dilate; no tick array)", _stat(t_fit)))
        say("    %-100s %s" % ("the loop by hand (per pass: ccmp_path_setpoints, qd / tau / tick_first / status copied out, numpy, stamps uploaded)", _stat(t_hand)))
    say("")
    say("the reference's recorded paths, stamped on the CPU (ccmp_path_timestamps_ref) under the Panda's limits, beta 0.5, then ccmp_path_fit_timestamps, aim 0.95, 8 passes:")
    for obj in ("Wine_Bottle", "dumbbell"):
        rows = np.loadtxt(os.path.join("tests", "golden", "paths", obj + "_path.txt"))
        first = np.array([0, len(rows)], dtype=np.int32)
        t = timestamps_ref(rows, first, vmax, amax)["time"]
        c2 = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        for period in (0.001, 0.004):
            before = c2.setpoint_paths(rows, first, t, vmax, amax, period=period)
            out = c2.fit_timestamps(rows, first, t, vmax, amax, period=period)
            after = c2.setpoint_paths(rows, first, out["time"], vmax, amax, period=period)
            say("    %-12s %2d rows at %g ms: %s after %d dilations; %.3f -> %.3f s (uniform stretch %.3f: %.3f s); peaks %.3f x vmax, %.3f x amax -> %.4f, %.4f (the audit of "
                "the fitted stamps: %.4f, %.4f); largest factor %.2f, %d of %d intervals dilated"
                % (obj, len(rows), period * 1e3, FIT_STATUS[int(out["status"][0])], int(out["passes"][0]), float(t[-1]), float(out["duration"][0]), float(before["stretch"][0]),
                   float(before["stretch"][0]) * float(t[-1]), before["peak"][0, 0], before["peak"][0, 1], out["peak"][0, 0], out["peak"][0, 1], after["peak"][0, 0],
                   after["peak"][0, 1], float(out["factor"].max()), int((out["factor"] > 1.0).sum()), len(rows) - 1))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "fit.md"), "w") as f:
        f.write("# Time stamps fitted to the limits at the controller's rate: `tools/measure.py fit`\n\n1 x MI355X, one run, seed 0x5C7; the retime measurement's inputs, "
                "continued: three smoothing passes, densified (distinct layout), resampled at the problem's delta, stamped under the Panda's data-sheet limits, then "
                "`ccmp_path_fit_timestamps` at a period of 1 ms, aim 0.95, at most 8 dilations; wall clock around the synchronous call, no GPU time measured.  No speed "
                "threshold gates this feature.  Beside it the loop a caller had to write before: `ccmp_path_setpoints` per trial (which materialises every tick and runs "
                "the constraint gap and isSatisfied over them), `qd`, `tau`, `tick_first` and `status` copied to the host, the rule of `csrc/ccmp_fit.h` in numpy, the "
                "stamps uploaded again; the two give the same stamps bit for bit before either is timed.  A path the resampling refused (`profiles/retime.md`) arrives "
                "without rows and answers EMPTY.  What the step is not: it is not TOPP-RA, it has no jerk limit, it bounds the motion only at the ticks of the stated "
                "period, and its convergence is observed on these inputs, not proven; with aim = 1 it is observed not to terminate.\n\n```\n" + "\n".join(lines) + "\n```\n")


def _jerk_by_hand(c, rows, first, time_dev, vmax, amax, jmax, period=0.001, max_window=64, aim=0.95):
    """the loop a caller would write without ccmp_path_jerk_setpoints: ccmp_path_setpoints once, qd, tau and tick_first copied to the host, a
    numpy moving window over every OK path's ticks (held at both ends) and the jerk ratio, the window grown by the update of
    csrc/ccmp_jerk.h until it passes.  The velocities only: the positions, the gap and the clearance of the filtered ticks would be one more
    upload and three more calls.  numpy's sums are not the rule's rounding sequence and the last tick of ccmp_path_setpoints sits at D, not
    on the grid: the windows agree with the library's, the last digits need not.  -> windows of the OK paths"""
    sp = c.setpoint_paths(rows, first, time_dev, vmax, amax, period=period)
    qd, tf, status = sp["qd"].cpu().numpy(), sp["tick_first"].cpu().numpy(), sp["status"].cpu().numpy()
    j = np.asarray(jmax)
    windows = []
    for f in np.flatnonzero(status == 0):
        v = qd[tf[f]:tf[f + 1]]
        W = 1
        while True:
            pad = np.vstack([np.zeros((W - 1, 14)), v, np.zeros((W - 1, 14))]) if W > 1 else v
            filt = np.lib.stride_tricks.sliding_window_view(pad, W, axis=0).mean(axis=2) if W > 1 else v
            P = float((np.abs(np.diff(filt, 2, axis=0)) / (period * period) / j).max()) if len(filt) > 2 else 0.0
            if P <= 1.0 or W >= max_window:
                break
            W = min(max_window, max(W + 1, int(np.ceil(W * P / aim))))
        windows.append(W)
    return windows


def jerk(argv):
    """ccmp_path_jerk_setpoints (KinematicChainConstraint.jerk_setpoint_paths) at 1 ms.  First, on one host core and without a device, the
    figures the unit was asked for with: the plain-Python restatement (tests/jerk_cases.py on tests/setpoint_cases.py and the stamp rule
    of tests/retime_cases.py) on the two recorded paths with repeated rows dropped — the unfiltered jerk ratio, the chosen window and the
    ratio behind it at 1 ms and 4 ms, and dumbbell under doubled stamps.  Then on the device: the setpoints measurement's inputs (1 and 64
    paths) through the call, beside the loop a caller would write today (_jerk_by_hand), wall clock around each, medians; and the two
    recorded paths through the call, stamped by ccmp_path_timestamps_ref, without and behind the fit.  Writes profiles/jerk.md."""
    import os

    from closed_chain_motion_planner_amd import JERK_STATUS, PANDA_ACCELERATION_LIMITS, PANDA_JERK_LIMITS, PANDA_VELOCITY_LIMITS, timestamps_ref

    sys.path.insert(0, "tests")
    import jerk_cases as jc
    import setpoint_cases as sc
    from retime_cases import stamp_path_py

    reps = int(argv[0]) if len(argv) > 0 else 9
    Lw, seed, steps = 32, 0x5C7, 3
    vmax, amax, jmax = PANDA_VELOCITY_LIMITS * 2, PANDA_ACCELERATION_LIMITS * 2, PANDA_JERK_LIMITS * 2
    cpu, lines = [], []

    def say(text, to=None):
        print(text)
        (lines if to is None else to).append(text)

    for obj, scale in (("Wine_Bottle", 1.0), ("dumbbell", 1.0), ("dumbbell", 2.0)):
        g = np.loadtxt(os.path.join("tests", "golden", "paths", obj + "_path.txt"))
        g = g[np.concatenate([[True], (np.diff(g, axis=0) != 0.0).any(axis=1)])]  # repeated rows dropped
        t = [v * scale for v in stamp_path_py(g, vmax, amax, 0.5)[0]]
        for period in ((0.001, 0.004) if scale == 1.0 else (0.001,)):
            n, xq, xd = jc.inputs_py(g, t, period)
            st, W, passes, trace = jc.search_py(xd, n, jmax, period, 65536, 0, 64, 0.95)
            q, qd, tau = jc.window_py(xq, xd, n, W, period)
            q1, qd1, tau1 = jc.window_py(xq, xd, n, 1, period)
            nan, one = np.full((len(tau), 2), np.nan), np.ones(len(tau), dtype=np.uint8)
            pk = jc.audit_py(qd, tau, nan, one, nan[:, 0], vmax, amax, jmax, period, 0.0)[0]
            pk1 = jc.audit_py(qd1, tau1, nan[:len(tau1)], one[:len(tau1)], nan[:len(tau1), 0], vmax, amax, jmax, period, 0.0)[0]
            say("    %-12s %2d rows%s at %g ms: %s, W = %d after %d passes, %d -> %d ticks; jerk ratio %.2f -> %.2f; speed %.4f -> %.4f x vmax, acceleration %.4f -> %.4f x amax"
                % (obj, len(g), "" if scale == 1.0 else ", stamps x %g" % scale, period * 1e3, JERK_STATUS[st], W, passes, n + 1, n + W, trace[0][1], trace[-1][1], pk1[0],
                   pk[0], pk1[1], pk[1]), cpu)

    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
    pj, pl = _smooth_paths(c, 64, Lw, seed)
    c.setJacobianMode(1)  # the setpoints do not depend on the mode; the path that feeds them is made in analytic mode
    for F in (1, 64):
        sm = c.smooth_paths(pj[:F].contiguous(), pl[:F].contiguous(), max_steps=steps)
        dense = c.densify_paths(sm["joints"], sm["out_len"], distinct=True, keep_handle=True)
        rs = c.resample_paths(dense)
        dense["handle"].close()
        ts = c.timestamp_paths(rs["joints"], rs["path_first"], vmax, amax)
        out = c.jerk_setpoint_paths(rs["joints"], rs["path_first"], ts["time"], vmax, amax, jmax)
        status, window, passes = (out[k].cpu().numpy() for k in ("status", "window", "passes"))
        ran = np.isin(status, (0, 6))
        by_hand = _jerk_by_hand(c, rs["joints"], rs["path_first"], ts["time"], vmax, amax, jmax)
        t_call, t_hand = [], []
        for i in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.jerk_setpoint_paths(rs["joints"], rs["path_first"], ts["time"], vmax, amax, jmax)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _jerk_by_hand(c, rs["joints"], rs["path_first"], ts["time"], vmax, amax, jmax)
            torch.cuda.synchronize()
            if i >= 2:
                t_call.append((t1 - t0) * 1e3)
                t_hand.append((time.perf_counter() - t1) * 1e3)
        peak = out["peak"].cpu().numpy()[ran]
        say("F = %d paths, %d rows at spacing %.3g -> %d ticks at 1 ms; status %s; windows %s after %s passes (the loop by hand: %s); speed / acceleration / jerk ratios "
            "of the delivered ticks, medians: %s; %d of the ticks refused by isSatisfied"
            % (F, rs["rows"], c.problem.delta, out["ticks"], {JERK_STATUS[k]: int((status == k).sum()) for k in sorted(set(status.tolist()))}, window[ran].tolist(),
               passes[ran].tolist(), by_hand, np.round(np.median(peak[:, :3], axis=0), 3).tolist() if len(peak) else [], int(out["counts"][:, 0].sum())))
        say("    %-110s %s" % ("ccmp_path_jerk_setpoints (status, tangents, per pass measure + decide + one read; sample, function + isSatisfied, peak; copy-out)", _stat(t_call)))
        say("    %-110s %s" % ("the loop by hand (ccmp_path_setpoints, qd / tick_first / status copied out, numpy windows of the velocities alone)", _stat(t_hand)))
    say("")
    say("the reference's recorded paths, stamped on the CPU (ccmp_path_timestamps_ref) under the Panda's limits, beta 0.5, then ccmp_path_jerk_setpoints at 1 ms, "
        "without and behind ccmp_path_fit_timestamps:")
    for obj in ("Wine_Bottle", "dumbbell"):
        rows = np.loadtxt(os.path.join("tests", "golden", "paths", obj + "_path.txt"))
        first = np.array([0, len(rows)], dtype=np.int32)
        t = timestamps_ref(rows, first, vmax, amax)["time"]
        c2 = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        fitted = c2.fit_timestamps(rows, first, t, vmax, amax)["time"]
        for what, stamps in (("as stamped", t), ("fitted", fitted)):
            plain = c2.jerk_setpoint_paths(rows, first, stamps, vmax, amax, jmax, window=1)
            out = c2.jerk_setpoint_paths(rows, first, stamps, vmax, amax, jmax)
            p0, p = plain["peak"][0], out["peak"][0]
            say("    %-12s %2d rows, %s, %.3f s: %s, W = %d after %d passes, %d -> %d ticks; speed %.4f -> %.4f x vmax, acceleration %.4f -> %.4f x amax, jerk %.3f -> %.3f x "
                "jmax at tick %d; max |dp| %.3e -> %.3e m, max angle %.3e -> %.3e rad; %d -> %d ticks refused by isSatisfied"
                % (obj, len(rows), what, float(stamps[-1]), JERK_STATUS[int(out["status"][0])], int(out["window"][0]), int(out["passes"][0]), plain["ticks"], out["ticks"], p0[0],
                   p[0], p0[1], p[1], p0[2], p[2], int(out["peak_tick"][0, 2]), p0[3], p[3], p0[4], p[4], int(plain["counts"][0, 0]), int(out["counts"][0, 0])))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "jerk.md"), "w") as f:
        f.write("# Jerk-bounded setpoints on the device: `tools/measure.py jerk`\n\n1 x MI355X, one run, seed 0x5C7; the setpoints measurement's inputs: three smoothing "
                "passes, densified (distinct layout), resampled at the problem's delta, stamped under the Panda's data-sheet limits, then `ccmp_path_jerk_setpoints` at a "
                "period of 1 ms, max_window 64, aim 0.95, under the data-sheet jerk limits.  Wall clock only, around the synchronous call (the mirror's copy-out "
                "included): no GPU time was measured and no speed threshold gates this feature.  Beside it the loop a caller has to write today: `ccmp_path_setpoints`, "
                "`qd`, `tick_first` and `status` copied to the host, numpy windows over the velocities and the same update of the window — the velocities alone; the "
                "filtered positions, their gap and their clearance would be one more upload and three more calls.  numpy's sums are another rounding sequence and "
                "`ccmp_path_setpoints` ends at D, not on the grid, so only the windows are compared.  A path the resampling refused (`profiles/retime.md`) arrives "
                "without rows and answers EMPTY.  What the unit is not: a bound at the ticks of the stated period on the qd sequence, not a third difference of "
                "positions; the filtered ticks lag by (W - 1) / 2 ticks and cut corners (the gap and isSatisfied columns below say by how much); it is not a "
                "jerk-optimal profile.  The paths as stamped exceed amax between their rows (`profiles/fit.md`); the window leaves that as it is, which is why the "
                "order of use is time stamps -> fit -> jerk-bounded setpoints.\n\n```\n" + "\n".join(lines) + "\n```\n\n"
                "## The gap the unit closes, on one host core\n\nNot a GPU measurement: the plain-Python restatement of the rule (`tests/jerk_cases.py` on "
                "`tests/setpoint_cases.py: path_py` and `tests/retime_cases.py: stamp_path_py`) on the two recorded paths with repeated rows dropped, stamped under the "
                "Panda's limits with beta 0.5.  The jerk ratio is taken from the `qd` sequence as the audit takes acceleration.  A path whose stamps pass speed and "
                "acceleration can still command more than jmax (dumbbell under doubled stamps).\n\n```\n" + "\n".join(cpu) + "\n```\n")


def plan(argv):
    """the planner's loop (ccmp_plan_*): python tools/measure.py plan [cycles]; writes profiles/plan.md"""
    sys.path.insert(0, "tests")
    from arm_model_cases import default_scene_host
    from object_cases import box_mesh, workspace
    from plan_cases import HandPlan, state_bits
    from closed_chain_motion_planner_amd import PLAN_STATUS, ObjectChecker, ProxyScene, Roadmap

    cycles = int(argv[0]) if argv else 64
    ctx = Context(0)
    MS, MARGIN = 16, -0.03
    names = ("proposals", "valid_proposals", "ik_successes", "vertices_kept", "mid_stones", "unsettled", "checks", "goal_pushes", "start_pushes", "ladder_vertices",
             "push_refused")

    def world(obj, scene, far=False, mode=0):
        c = KinematicChainConstraint.from_yaml(CFG % obj, ctx=ctx)
        c.setJacobianMode(mode)
        chk = ObjectChecker(c, box_mesh(0.04, 0.04, 0.1), workspace())
        sc = None
        if scene:
            hs = default_scene_host(c.problem)
            sc = ProxyScene(c, hs.spheres, hs.boxes, hs.allowed)
        return c, chk, sc, (far_goal_state(c, chk, MS) if far else None)

    def line(tag, r, ms, extra=""):
        return "%-34s %-12s cycles %3d  V %5d  E %5d  d_goal %.4f  d_start %.4f  %s  %8.1f ms%s" % (
            tag, PLAN_STATUS[r["status"]] + ("" if r["solved"] is None else " %s" % (r["solved"],)), r["cycles_total"], r["size"], r["edges"], r["prev_from_goal"],
            r["prev_from_start"], " ".join("%s %d" % (n[:3] + n[-2:], r["counters"][n]) for n in names), ms, extra)

    from plan_cases import far_goal_state

    def store(c, far):
        return Roadmap(c)

    rows, hard, hand, cover = [], [], [], []
    for far, out in ((False, rows), (True, hard)):
        for obj in ("Wine_Bottle", "dumbbell", "stefan"):
            c, chk, _, gj = world(obj, False, far)
            for W in (1, 8, 32, 128):
                rm = store(c, far)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pl = rm.plan(c, chk, goal_joints=gj, width=W, k=5, max_states=MS, rng_seed=0x91A)
                r = pl.run(cycles)
                ms = (time.perf_counter() - t0) * 1e3
                out.append(line("%s width %d" % (obj, W), r, ms, "  (%.2f ms / cycle)" % (ms / max(r["cycles_total"], 1))))
                print(out[-1], flush=True)
                final = pl.state()
                pl.close()
                rm.close()
                if W == 32 and far:  # the same cycles by hand: the same bits, and what they cost a caller
                    rm = store(c, far)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hp = HandPlan(rm, c, chk, goal_joints=gj, width=W, k=5, max_states=MS, rng_seed=0x91A)
                    n = hp.run(cycles)
                    hms = (time.perf_counter() - t0) * 1e3
                    hand.append("%-12s by hand: %3d cycles %8.1f ms (%.2f ms / cycle), %d mirror calls, %d host reads (%.1f / cycle); Plan.run: %.2f ms / cycle; same state bits: %s"
                                % (obj, n, hms, hms / max(n, 1), hp.calls, hp.reads, hp.reads / max(n, 1), ms / max(r["cycles_total"], 1), state_bits(hp.state) == state_bits(final)))
                    print(hand[-1], flush=True)
                    rm.close()
    for scene in (False, True):
        for mode in (0, 1):
            c, chk, sc, gj = world("Wine_Bottle", scene, True, mode)
            for W in (1, 5, 64, 65):
                rm = store(c, True)
                pl = rm.plan(c, chk, goal_joints=gj, scene=sc, margin=MARGIN, width=W, k=5, max_states=MS, rng_seed=0x91A)
                r = pl.run(6)
                cover.append(line("width %d%s%s, 6 cycles" % (W, " scene" if scene else "", " analytic" if mode else ""), r, 0.0))
                print(cover[-1], flush=True)
                pl.close()
                rm.close()
    with open("profiles/plan.md", "w") as f:
        f.write("# The planner's loop on the store (`ccmp_plan_*`, `Roadmap.plan`)\n\nWritten by `python tools/measure.py plan`.  One MI355X, one process.  "
                "**Wall clock only, measured on one card**: `time.perf_counter` around open plus `Plan.run(%d)`; no GPU time was measured and no speed threshold gates "
                "this feature.  Object: a box mesh (0.04, 0.04, 0.1) against the fixture workspace; k = 5, lists of 16 states, rng_seed 0x91A, no scene unless "
                "stated.  Whether and when a config solves is a measurement, not a property the unit promises.\n\n"
                "Counter columns: proposals, valid proposals, IK successes, vertices kept, mid-stones, unsettled queries, checks run, goal pushes, start pushes, "
                "ladder vertices, pushes refused at the cap.\n\n## The shipped problems, %d cycles\n\n```\n" % (cycles, cycles) + "\n".join(rows) + "\n```\n\n"
                "On all three shipped configs checkMotion reaches the goal state from the start state: open connects them and no cycle runs.  That is the "
                "finding for these problems at every width; the rule was not tuned.\n\n## Towards a goal that one motion does not reach\n\nThe same runs with "
                "another goal (`tests/plan_cases.py: far_goal_state`): of 2 048 sampled states the one nearest to the start pose whose mesh is free and which "
                "checkMotion from the start does not reach within 16 states; its object pose is the goal pose, the state itself `goal_joints`.\n\n```\n"
                + "\n".join(hard) + "\n```\n\n"
                "## The same cycles by hand (width 32, towards that goal)\n\n`tests/plan_cases.py: HandPlan` runs the loop over the mirror's calls that exist without the unit (propose, grow, "
                "commit, closest, valid, pose_ik_batch, connect, labels), every decision on the host.  That is what a caller could do on the parent commit.  The first by-hand run of a process also pays the one-time growth of the library's workspaces (Wine_Bottle's single cycle below), so only the rows with more than one cycle compare the two routes; what the unit removes for certain is the count of host reads per cycle.\n\n```\n"
                + "\n".join(hand) + "\n```\n\n## What a cycle of `Plan.run` costs the host\n\nBranches that did not fire are SKIPPED after a read, not launched on NaN "
                "rows (the rows are NaN on the device either way, so the bits are the same).  A cycle without a check: 3 launches of the plan unit (front, tally, "
                "solution test) between 3 calls of the store's entries (propose, grow, commit), and 2 host reads (the commit's own 16-byte count read-back and the "
                "240-byte state block).  A cycle whose check ran adds 2 closest calls, the check kernel, the mesh test of the nine ladder poses, one IK call over the "
                "eleven targets, the prefix kernel and one 16-byte read; each branch that has a vertex to add (goal, ladder prefix, start) adds one connect, one commit "
                "(with its read-back) and one push or tally launch.  The store, the edge list, the labels and the state lists never cross to the host.\n\n"
                "## Which branches six cycles reach (Wine_Bottle towards that goal; FD and analytic mode, without and with the skeleton scene at -0.03)\n\n```\n" + "\n".join(cover) + "\n```\n")


def rrtc_first_step_share(pairs=1024):
    """difference (a) of include/ccmp.h on the CPU: with the oracle's traversal (oracle/ccmp_oracle.c, delta 0.25), of `pairs` pairs of valid
    sampled states, how many list a first step at all and how many first steps exceed 0.2 = 2 range — where OMPL's nearer-state rule gives `from`"""
    sys.path.insert(0, "tests")
    import yaml
    from oracle_binding import Oracle

    O, lines = Oracle("det"), []
    for obj in ("Wine_Bottle", "dumbbell", "stefan"):
        P = O.problem(yaml.safe_load(open(CFG % obj)))
        q, ok, _ = O.sample_project_batch(P, 0x77C, 0, 16 * pairs)
        good = q[(ok != 0) & np.array([O.joint_valid(P, x) for x in q], dtype=bool)]
        frm, to = good[:pairs], good[pairs:2 * pairs]
        st, n, _, _ = O.discrete_geodesic_batch(P, frm, to, max_states=4)
        first = np.array([O.distance(st[e, 0], st[e, 1]) for e in range(len(to)) if n[e] >= 2])
        d = np.array([O.distance(a, b) for a, b in zip(frm, to)])
        lines.append("%-12s valid draws %5d of %5d  pairs %4d  with a first step %4d  first step > 0.2: %4d (%.1f %% of all pairs, %.1f %% of those with a step)  "
                     "first step min / median / max %.4f / %.4f / %.4f  distance of a pair min / median %.3f / %.3f"
                     % (obj, len(good), len(q), len(to), len(first), int((first > 0.2).sum()), 100.0 * (first > 0.2).sum() / len(to), 100.0 * (first > 0.2).mean(),
                        first.min(), np.median(first), first.max(), d.min(), np.median(d)))
        print(lines[-1], flush=True)
    return lines


def rrtc(argv):
    """RRT-Connect on the store (ccmp_rrtc_*): python tools/measure.py rrtc [cpu]; writes profiles/rrtc.md.  `cpu`: the CPU figure alone
    (no device), every GPU figure marked as not measured"""
    cpu_only = "cpu" in argv
    argv = [""] + [a for a in argv if a.endswith(".md")]
    share = rrtc_first_step_share()
    nearest, cycles_, solved, dens, cover = [], [], [], [], []
    if not cpu_only:
        sys.path.insert(0, "tests")
        from object_cases import box_mesh, workspace
        from plan_cases import far_goal_state, problem_poses
        from rrtc_cases import HandRRTConnect, state_bits
        from closed_chain_motion_planner_amd import PLAN_STATUS, RRTC_STATUS, ObjectChecker, Roadmap
        from closed_chain_motion_planner_amd._lib import METRIC_JOINT

        ctx = Context(0)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        c = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
        c.setJacobianMode(1)
        # 1. nearest-in-tree beside the joint-metric k-NN with k = 1 on the same rows; every vertex in the tree (a star on vertex 0)
        r = np.random.default_rng(11)
        for N in (10**3, 10**5, 10**6):
            rm = Roadmap(c, capacity_hint=N)
            rm.append(joints=dev(r.uniform(-2, 2, size=(N, 14))), poses=dev(np.zeros((N, 8))))
            rm.add_edges(dev(np.stack([np.zeros(N - 1, dtype=np.int32), np.arange(1, N, dtype=np.int32)], axis=1)))
            roots = dev(np.zeros(1, dtype=np.int32))
            for Q in (1, 32, 256):
                q = dev(r.uniform(-2, 2, size=(Q, 14)))
                a = rm.nearest_in_tree(roots, q)
                b = rm.nearest_k(q, 1, metric=METRIC_JOINT)
                same = a[0].tolist() == b[0][:, 0].tolist()
                t_a, t_b = timed(lambda: rm.nearest_in_tree(roots, q), 5), timed(lambda: rm.nearest_k(q, 1, metric=METRIC_JOINT), 5)
                nearest.append("N %8d  Q %4d  partitions %3d  nearest_in_tree %8.3f ms  roadmap knn k=1 %8.3f ms  ratio %5.2f  same answer: %s"
                               % (N, Q, _lib_shape(ctx, Q, N), t_a, t_b, t_a / t_b, same))
                print(nearest[-1], flush=True)
            rm.close()
        # 2. the far goal: time per cycle against the loop by hand, cycles and vertices to SOLVED per range, beside Plan
        chk = ObjectChecker(c, box_mesh(0.04, 0.04, 0.1), workspace())
        start = np.array(c.problem.start_joint[:])
        _, shipped_pose = problem_poses(c.problem)
        ik = c.pose_ik_batch(dev(shipped_pose.reshape(1, 8)), dev(start.reshape(1, 1, 14)), rng_seed=0x77C)
        shipped = ik["q"][0].cpu().numpy() if int(ik["ok"][0]) else None
        goal = far_goal_state(c, chk, 16)

        def opened(g):
            rm = Roadmap(c)
            rm.append(joints=dev(np.stack([start, g])))
            return rm

        for W in (1, 32, 256):
            rm = opened(goal)
            pl = rm.rrt_connect(c, starts=[0], goals=[1], width=W, max_states=16, rng_seed=0x77C)
            pl.run(1)  # the workspaces' one-time growth
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = pl.run(8)
            ms = (time.perf_counter() - t0) * 1e3 / max(rep["cycles_run"], 1)
            rmh = opened(goal)
            hp = HandRRTConnect(rmh, c, [0], [1], width=W, rng_seed=0x77C, max_states=16)
            hp.run(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = hp.run(8)
            hms = (time.perf_counter() - t0) * 1e3 / max(n, 1)
            cycles_.append("width %3d  RRTConnect.run %7.2f ms / cycle (%d cycles)   by hand %7.2f ms / cycle (%d cycles)   same state bits: %s   V %d E %d"
                           % (W, ms, rep["cycles_run"], hms, n, state_bits(pl.state()) == state_bits(hp.state), rep["size"], rep["edges"]))
            print(cycles_[-1], flush=True)
            for h in (pl, rm, rmh):
                h.close()
        for name, g in (("far goal", goal), ("shipped goal", shipped)):
            if g is None:
                continue
            for rng in (0.1, 0.5, 1.0, 2.0):
                rm = opened(g)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pl = rm.rrt_connect(c, starts=[0], goals=[1], width=32, range=rng, max_states=64, rng_seed=0x77C)
                rep = pl.run(64)
                ms = (time.perf_counter() - t0) * 1e3
                cnt = rep["counters"]
                line = "%-12s range %.1f  %-7s cycles %3d  V %5d  E %5d  best_gap %.3f  trapped %d advanced %d reached %d unsettled %d | joined %d added %d nothing %d  %8.1f ms" % (
                    name, rng, RRTC_STATUS[rep["status"]], rep["cycles_total"], rep["size"], rep["edges"], rep["best_gap"], cnt["trapped"], cnt["advanced"], cnt["reached"],
                    cnt["unsettled"], cnt["connect_reached"], cnt["connect_added"], cnt["connect_nothing"], ms)
                if rep["solved"] is not None:  # the densify share: the solution path's segments whose fresh traversal arrives
                    d = rm.dense_solution(c, [rep["solved"][0]], [rep["solved"][1]], max_len=256)
                    ok = d[2]["seg_ok"].cpu().numpy().reshape(-1)[:len(d[1]) - 1]
                    dens.append("%-12s range %.1f  path of %3d vertices, cost %.3f: %d of %d segments seg_ok" % (name, rng, len(d[1]), d[0], int((ok == 1).sum()), len(ok)))
                    print(dens[-1], flush=True)
                solved.append(line)
                print(line, flush=True)
                pl.close()
                rm.close()
            rm = Roadmap(c)
            if name == "shipped goal":  # Plan takes its goal pose from the problem: the far goal moved it, so the shipped problem is loaded again
                c2 = KinematicChainConstraint.from_yaml(CFG % "Wine_Bottle", ctx=ctx)
                c2.setJacobianMode(1)
            else:
                c2 = c
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pp = rm.plan(c2, chk, goal_joints=g, width=32, k=5, max_states=16, rng_seed=0x91A)
            rep = pp.run(64)
            solved.append("%-12s Plan (width 32, k 5)  %-7s cycles %3d  V %5d  E %5d  %8.1f ms" % (name, PLAN_STATUS[rep["status"]], rep["cycles_total"], rep["size"], rep["edges"],
                                                                                                  (time.perf_counter() - t0) * 1e3))
            print(solved[-1], flush=True)
            pp.close()
            rm.close()
    na = ["NOT MEASURED (written without a device: `python tools/measure.py rrtc cpu`)"]
    out = argv[1] if len(argv) > 1 else "profiles/rrtc.md"
    with open(out, "w") as f:
        f.write("# RRT-Connect on the store (`ccmp_rrtc_*`, `Roadmap.rrt_connect`, `Roadmap.nearest_in_tree`)\n\nWritten by `python tools/measure.py rrtc`.  One MI355X, one "
                "process, Wine_Bottle in analytic mode unless stated.  **Figures, not gates**: wall clock (`time.perf_counter`) around the synchronous runs, HIP events "
                "(best of 5) around the nearest-vertex calls; whether and when a run solves is a measurement, not a property the unit promises.\n\n"
                "## Difference (a) on the CPU: how often OMPL's nearer-state rule would return `from`\n\nThe oracle's traversal (delta 0.25) between pairs of valid sampled "
                "states (a draw is valid when its projection converged and it is within the joint limits).  With range 0.1 OMPL's constrained `interpolate` returns the "
                "listed state nearer to arc 0.1, which is `from` whenever the first listed step is longer than 0.2, and `checkMotion(from, from)` then adds nothing.  A "
                "pair without a first step is TRAPPED under either rule.\n\n```\n" + "\n".join(share) + "\n```\n\n"
                "So the claim \"nearly every extension\" does not hold as derived: about a fifth to a quarter of all pairs (a quarter to a third of those that move at "
                "all) would be lost to the nearer-state rule, and the median first step (0.17 to 0.18) is below 0.2.  The clip at an absolute arc with at least one "
                "step keeps those extensions; it also makes every ADVANCED vertex one listed step (about 0.17) from its parent instead of 0.1.\n\n"
                "## Nearest vertex of a tree beside the joint-metric k-NN with k = 1 (every vertex in the tree)\n\n```\n" + "\n".join(nearest or na) + "\n```\n\n"
                "`rrtc_nearest_kernel` runs one block per (query, partition) and does not tile over the queries: every query reads its partition's rows and labels "
                "again, where `knn_many_kernel` stages a tile of rows in LDS for 256 queries.  Where the ratio above exceeds 1 at large Q and N that is the reason, not "
                "the label filter (one 4-byte load and eight compares per row beside 112 bytes of joints).  The planner's own calls are Q = width <= 256 on stores of "
                "thousands of rows.\n\n"
                "## Time per cycle against the loop by hand (far goal, lists of 16, range 0.1)\n\n`tests/rrtc_cases.py: HandRRTConnect` runs the cycle over the mirror's "
                "calls with the commit on the host: what a caller could write without the unit.\n\n```\n" + "\n".join(cycles_ or na) + "\n```\n\n"
                "## Cycles and vertices to SOLVED (width 32, lists of 64, at most 64 cycles), beside `Plan`\n\n```\n" + "\n".join(solved or na) + "\n```\n\n"
                "## The densify share: solution-path segments whose fresh traversal arrives\n\nAn edge (parent, child) was validated as a prefix of a traversal towards "
                "something else; `ccmp_path_densify` runs parent -> child (or child -> parent) afresh.\n\n```\n" + "\n".join(dens or na) + "\n```\n\n"
                "## Outcomes the far goal's six-cycle test runs do not reach\n\n`tests/test_gpu_rrtc.py::test_the_runs_cover_the_outcomes` takes, from the hand loop, the "
                "union over widths 1, 5 and 64 at range 0.1 and width 5 at range 3 (six cycles, lists of 16).  It holds NONE, TRAPPED, ADVANCED and UNSETTLED of step 2 "
                "and NOTHING and ADDED of step 3.  It does not hold **REACHED** — the distance between two valid states is never below 2.2 in the pairs above, so no "
                "sample lies within range 3 of a tree vertex — nor **JOINED**, the trees being far apart by the construction of that goal.  JOINED is asserted in the "
                "solved run on the shipped goal, REACHED on real traversals in the pick kernel's test (range 4).\n")


def _lib_shape(ctx, Q, N):
    from closed_chain_motion_planner_amd import rrtc_nearest_shape

    return rrtc_nearest_shape(ctx.handle, Q, N)[1]


def smooth_restate(argv):
    """the plain-Python restatement of the smoothing rule (tests/smooth_cases.py on the det oracle) on one host core, on the inputs `smooth`
    wrote, compared bit for bit with the results it wrote: python tools/measure.py smooth_restate <file.npz> [paths]"""
    sys.path.insert(0, "tests")
    from conftest import load_cfg
    from oracle_binding import Oracle
    from smooth_cases import Restatement, bits

    d = np.load(argv[0])
    n_max = int(argv[1]) if len(argv) > 1 else 64
    O = Oracle("det")
    pj = d["path_joints"]
    for mode in (0, 1):
        P = O.problem(load_cfg("Wine_Bottle"))  # the oracle's own set-up: byte for byte the product's problem (tests/test_gpu_parity.py)
        P.jacobian_mode = mode
        for F in (1, 64):
            F = min(F, n_max)
            t0 = time.perf_counter()
            same = True
            for f in range(F):
                r = Restatement(O, P).smooth(pj[f], 3, 0.005, 249)
                n = len(r["rows"])
                same = same and n == int(d["mode%d_F%d_out_len" % (mode, F)][f]) and np.array_equal(bits(r["rows"]), bits(d["mode%d_F%d_joints" % (mode, F)][f, :n])) \
                    and r["stats"] == d["mode%d_F%d_stats" % (mode, F)][f].tolist()
            print("%s mode, F = %d: restatement on one host core %.1f ms; rows, lengths and stats identical to the device's: %s"
                  % ("analytic" if mode else "FD", F, (time.perf_counter() - t0) * 1e3, same))


def run(argv):
    """fixed workloads for the profiler: one kernel family each, `reps` launches"""
    what = argv[0]
    reps = int(argv[1]) if len(argv) > 1 else 12
    ctx = Context(0)
    c = KinematicChainConstraint.from_yaml(CFG % ("stefan" if what.startswith("stefan") else "Wine_Bottle"), ctx=ctx)
    if what == "stefan_tight":  # BASELINE configs[3] read as "tighter loop tol": half the reference's tolerances
        c.setTolerance(5e-4, 2.5e-3)
    if what == "calibrated":  # C3 on calibrated arms (PandaModel::initModel(dh), offsets differing per arm): the general instantiations
        for arm in (0, 1):
            dh = (C.c_double * 28)(*[(1e-3 if arm == 0 else -7e-4) * ((5 * i + 3 * arm) % 7 - 3) for i in range(28)])
            assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    if what in ("c3", "stefan", "stefan_tight", "calibrated"):
        q = c.ambient_uniform_batch(0xC3, 0, 262144)
        fn = lambda: c.project_batch(q)
    elif what.startswith("flat") and what[4:].isdigit() and int(what[4:]) > 1:  # flat4096 (C2), flat14336 ...: the latency kernel alone
        q = c.ambient_uniform_batch(0xC2, 0, int(what[4:]))
        fn = lambda: c.project_batch(q)
    elif what.startswith("mid"):  # mid32768, mid65536 ...: scout + throughput kernel + hand-over to the latency kernel
        q = c.ambient_uniform_batch(0xC3, 0, int(what[3:]))
        fn = lambda: c.project_batch(q)
    elif what == "flat1":
        x = c.ambient_uniform_batch(0xC1, 0, 64).cpu().numpy()
        fn = lambda: [c.project(x[i].copy()) for i in range(64)]
    elif what.startswith("geodesic_analytic"):  # the same first pass in analytic mode (geodesic_row16_kernel)
        frm, to = near_edges(c, int(what[17:] or 16384))
        c.setJacobianMode(1)
        fn = lambda: c.discrete_geodesic_batch(frm, to, 16, want_carry=True, round_budget=128)
    elif what.startswith("geodesic"):  # geodesic (16384 edges: bench.py's first pass), geodesic65536 (a bulk call) ...
        frm, to = near_edges(c, int(what[8:] or 16384))
        fn = lambda: c.discrete_geodesic_batch(frm, to, 16, want_carry=True, round_budget=128)  # bench.py's first pass
    elif what.startswith("analytic"):  # analytic (C3's batch), analytic4096, analytic2097152 ...
        c.setJacobianMode(1)
        q = c.ambient_uniform_batch(0xC3, 0, int(what[8:] or 262144))
        fn = lambda: c.project_batch(q)
    elif what == "clearance":
        from closed_chain_motion_planner_amd.scene import ProxyValidityChecker

        sc = ProxyValidityChecker(c).scene
        q = c.ambient_uniform_batch(0xC3, 0, 262144)
        fn = lambda: sc.clearance_batch(q, 0.0)
    else:
        raise SystemExit(__doc__)
    import os

    for kv in filter(None, os.environ.get("CCMP_OPTS", "").split(",")):  # CCMP_OPTS=name=value,...: options of the context for this run
        ctx.set_option(kv.split("=")[0], int(kv.split("=")[1]))
    # >= 3 warm-up calls (the profile's summary drops their dispatches), then `reps` calls, each bracketed by HIP events on the
    # launch stream (a call that forks to the context's side stream joins it back before it returns, so the second event is behind
    # everything) and followed by a synchronise — the idle gap that tells two calls apart in the kernel trace.  The per-call times
    # are printed as JSON: under `--kernel-trace` alone they are the call's wall time with its kernels overlapping as they do in
    # production; under `--pmc` they show what counter collection does to that overlap.
    import json

    warm = int(argv[2]) if len(argv) > 2 else 3
    for _ in range(warm):
        fn()
        torch.cuda.synchronize()
    calls = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        calls.append(e0.elapsed_time(e1))
    print("CALL_MS " + json.dumps({"workload": what, "warmup_calls": warm, "call_ms": calls}))


if __name__ == "__main__":
    cmds = {f.__name__: f for f in (sizes, single, geodesic, analytic, host, sharded, afterload, sampler, soak, soak_resident, scout, clearance, connect, roadmap, mirror, ik, graph, path, dense, shortcut, smooth, smooth_restate, retime, setpoints, fit, jerk, plan, rrtc, run)}
    cmds["object"] = object_
    if len(sys.argv) < 2 or sys.argv[1] not in cmds:
        raise SystemExit(__doc__)
    cmds[sys.argv[1]](sys.argv[2:])

"""Builds libccmp.so (HIP kernels for gfx950 + the C-ABI host code) in-tree with hipcc.

Translation units with deliberately different flags:
  ccmp_kernels_fd.hip    -ffp-contract=off -DCCMP_USE_FMA   canonical, bit-reproducible arithmetic (throughput kernel);
                         -DCCMP_LEAN_SQRT: ccmp_detmath.h's wave-uniform fast path of the IEEE square root (same bits, -1.9 %);
                         -DCCMP_ATAN_UNIFORM: atan's first interval without its division when the whole wavefront is in it (same bits, -2.0 %)
  ccmp_kernels_wave.hip  -ffp-contract=off -DCCMP_USE_FMA   same arithmetic, one-wave-per-sample kernels
  ccmp_kernels_flat.hip  -ffp-contract=off -DCCMP_USE_FMA   same arithmetic, one 128-thread block per sample (latency kernel)
  ccmp_kernels_geo.hip   -ffp-contract=off -DCCMP_USE_FMA   the extend step on the same Newton routine (ccmp_flat_newton.h), built twice:
                         like the flat unit (throughput flavour) and -DCCMP_GEO_LATENCY with machine LICM and a 256-register
                         budget (latency flavour)
  ccmp_kernels_geo_scene.hip  the latency flavour's flags   the extend step with a proxy scene's clearance test (geodesic_scene_kernel)
  ccmp_problem.cpp       -ffp-contract=off -DCCMP_USE_FMA   host set-up (problem, constants) in the same rounding model
  ccmp_api.cpp           -ffp-contract=off -DCCMP_USE_FMA   context, launches            } compiled a second time with -DCCMP_DEBUG_HOOKS for
  ccmp_policy.cpp                                           option table, plans, describe } lib/libccmp_debug.so (include/ccmp_debug.h)
  ccmp_resident.cpp                                         opt-in resident service kernel for single-state calls (host side)
  ccmp_kernels_resident.hip -ffp-contract=off -DCCMP_USE_FMA  ... its device side for the reference arithmetic, on the latency flavour's Newton routine
                         (its device side for analytic mode, resident_row16_kernel, is part of ccmp_kernels_fast.hip: the same flags, the same bits)
  ccmp_host_io.cpp                                          *_host conveniences (staging, pinned block, page-locked caller buffers), sharded host calls
  ccmp_comm.cpp                                             one process / several GPUs: RCCL communicator and sharded entry points
  ccmp_kernels_fast.hip  -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   analytic fast mode (lane-pair and row16 projectors, the row16 extend step, the row16 resident service kernel), bit-identical to the oracle's analytic mode
  ccmp_kernels_scout.hip -ffast-math                        FP32 iteration-count predictor + ordering (never touches results)
  ccmp_kernels_scene.hip -ffp-contract=off -DCCMP_USE_FMA   proxy-geometry clearance (pre-filter ahead of the host's MoveIt test); its arithmetic — frames, placement,
                         pair distance — is ccmp_scene_math.h, one text shared with ccmp_clearance.h (the extend step's scene variants), ccmp_kernels_ik_vet.hip and ccmp_ik.cpp
  ccmp_scene.cpp                                            proxy scenes: validation, pair list, launches
  ccmp_kernels_knn.hip   -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   the connection step: FP64 brute-force k nearest neighbours on the joint metric and on the
                         object metric (ccmp_pose.h), the gather of ccmp_connect_batch, the roadmap store's pose_from_joints_kernel
  ccmp_roadmap.cpp       -ffp-contract=off -DCCMP_USE_FMA   the device-resident roadmap store; ccmp_pose_distance / ccmp_pose_from_t_wo on the host (same bits as the kernels)
  ccmp_kernels_ik.hip    -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   growTree's sampleCalibGoal step: pose-targeted IK (ccmp_ik.h), one candidate per lane, and its selection rule;
                         without machine LICM (two wavefronts per SIMD instead of one)
  ccmp_ik.cpp            -ffp-contract=off -DCCMP_USE_FMA   ccmp_pose_ik_*: checks, launches, and the same solver text on the host (ccmp_pose_ik_ref, same bits as the kernels);
                         the vetted forms ccmp_arm_clearance_* / ccmp_pose_ik_vetted_* on ccmp_ik_vet.h (the rule) and ccmp_scene_math.h (the clearances)
  ccmp_kernels_ik_vet.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   the collision gate of sampleCalibGoal on the proxy scene (ccmp_ik_vet.h): the arm clearance of every
                         IK candidate, sixteen lanes per candidate (ik_vet_kernel, on ccmp_scene_math.h), and the vetted selection (ik_assemble_kernel, ik_pick_kernel)
  ccmp_kernels_object.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   the head of growTree: object-pose proposal (interpolate, SE3 Gaussian draw) and the
                         mesh-against-workspace test (ccmp_object.h), one 256-lane block per pose, the triangles strided over the lanes
  ccmp_kernels_graph.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   the roadmap graph (ccmp_graph.h): growTree's tail (commit), explicit edges, the component labels
                         (hooking rounds in one block, then a compress launch) and closestFromGoal's vertex scan; ccmp_roadmap.cpp compiles the same header for the *_ref forms;
                         and the planner's solution step, shortest paths on that graph (ccmp_path.h: graph_path_*, relaxation and hop rounds in one block per pair)
  ccmp_object.cpp        -ffp-contract=off -DCCMP_USE_FMA   ccmp_object_*: checks, launches, and the same text on the host (the *_ref forms, same bits as the kernels)
  ccmp_kernels_dense.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   dense solution paths (ccmp_dense.h): the endpoint gather of the continuation loop, the pack of the
                         extend calls' chunks and the waypoint rows, the arc's serial chain (one block per path) and the segmented clearance reduction
  ccmp_dense.cpp         -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_densify: checks, the continuation loop over ccmp_geodesic_batch_ex, the layout; ccmp_dense_*_ref on the host
  ccmp_kernels_shortcut.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   shortcut solution paths (ccmp_shortcut.h): the enumeration of a tile of waypoint pairs, the endpoint gather
                         of a continuation, the scatter of flags and counts into the pair matrices, the DAG search (one block per path) and the gather of the kept rows
  ccmp_shortcut.cpp      -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_shortcut: checks, the tile and continuation loops over the extend step; ccmp_shortcut_select*, ccmp_shortcut_pairs_ref
  ccmp_kernels_smooth.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   smooth solution paths (ccmp_smooth.h): the pair gather of a pass's stages, the bracket of half the arc and
                         the blend, the pick between projected / fallback / degenerate, the accept step into the other path buffer, lengths and the store
  ccmp_smooth.cpp        -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_smooth: checks, the pass loop (midpoint steps on the dense unit's loop, the test step on the shortcut unit's); ccmp_smooth_mid_ref
  ccmp_kernels_retime.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   resample and time stamps (ccmp_retime.h): the status scan, the bracket of a target arc (ccmp_dense.h: arc_bracket, the smooth unit's too) and the blend, the pick,
                         the ceilings and the minimum of A, the envelope and the stamps' serial sum (one wavefront per path)
  ccmp_retime.cpp        -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_resample, ccmp_sampled_paths_*, ccmp_path_timestamps*: checks, launches; ccmp_path_timestamps_ref, ccmp_arc_bracket_ref, ccmp_resample_targets_ref
  ccmp_kernels_setpoints.hip -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   controller-rate setpoints and the execution audit (ccmp_setpoints.h, which holds no fused operation): the status scan, the row
                         tangents, the bracket of a tick on the stamps and the cubic's q and qd, the per-path peaks (one block per path)
  ccmp_setpoints.cpp     -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_setpoints*, ccmp_setpoints_*: checks, launches, the function / is-satisfied / clearance calls over all ticks; ccmp_setpoints_ref, ccmp_setpoint_tangents_ref
  ccmp_kernels_fit.hip   -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   time stamps fitted to the limits at the controller's rate (ccmp_fit.h, which holds no fused operation): the measure kernel (sixteen lanes
                         per tick interval, no tick array, atomic maxima per row interval), the dilation's serial sum (one wavefront per path), the factors
  ccmp_fit.cpp           -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_fit_timestamps*: checks, the pass loop over the setpoints unit's status and tangent launches and this unit's; ccmp_path_fit_timestamps_ref
  ccmp_kernels_jerk.hip  -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   jerk-bounded setpoints (ccmp_jerk.h, which holds no fused operation): the window search's measure kernel (one block per tile of
                         ticks, the inputs staged in LDS, no tick array, one atomic maximum per block), its decide kernel, the sample kernel and the per-path peaks
  ccmp_jerk.cpp          -ffp-contract=off -DCCMP_USE_FMA   ccmp_path_jerk_setpoints*, ccmp_jerk_setpoints_*: checks, the window search's pass loop, the launches; ccmp_jerk_setpoints_ref
  ccmp_kernels_plan.hip  -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   the planner's loop on the store (ccmp_plan.h): the front's broadcast, the tally of a growth step, the check
                         (one wavefront: the carry rule's serial fold, the thresholds, the IK targets of the ladder), the prefix, the push and the solution test (a ballot over the
                         pairs; a template over the state type, instantiated for ccmp_plan_state and for ccmp_rrtc_state: both under the plan_ line of _SCRATCH_RULES)
  ccmp_plan.cpp          -ffp-contract=off -DCCMP_USE_FMA   ccmp_plan_*: checks, open, the cycle's body over the store's own entry points; ccmp_plan_check_ref / _prefix_ref / _connected_ref
  ccmp_kernels_rrtc.hip  -ffp-contract=off -DCCMP_USE_FMA -DCCMP_LEAN_SQRT   RRT-Connect on the store (ccmp_rrtc.h): nearest vertex within a tree (blocks over (partition, query), a
                         (distance, index) pair reduction), the traversal's endpoints, the pick (sixteen lanes per edge, the arc's serial fold), the commit (one block: a scan
                         gives the total order); its solution test is the plan unit's kernel
  ccmp_rrtc.cpp          -ffp-contract=off -DCCMP_USE_FMA   ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree*: checks, the cycle's body over the library's own entry points; the *_ref forms
  (ccmp_plan.cpp and ccmp_rrtc.cpp share ccmp_planner.h on the host — the state block's reads, open's upload, the run loop with the solution test, the report's head — and
  ccmp_plan.h's solution test on host and device)
  (the three units ccmp_kernels_setpoints / _fit / _jerk share ccmp_lanes.h on the device — the DPP row folds and the audit fold of the two peak kernels — and ccmp_timed.h on the
  host — the checks, the _host staging, the tick ranges, the delivery tail and the _ref loops; a tick of the interpolant is setpoint_bracket and
  setpoint_joint of ccmp_setpoints.h everywhere)
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
# CCMP_LIBRARY: another build of the same library (tools/sanitize_cpu.py: host code under ASan/UBSan); never set in production
LIBPATH = os.environ.get("CCMP_LIBRARY") or os.path.join(LIBDIR, "libccmp.so")
# the same sources with the test / tool hooks of include/ccmp_debug.h (-DCCMP_DEBUG_HOOKS on the two host units that carry them)
DEBUG_LIBPATH = os.path.join(LIBDIR, "libccmp_debug.so")
_DEBUG_UNITS = ("ccmp_api.cpp", "ccmp_policy.cpp")
_DEBUG_ONLY_UNITS = [("ccmp_kernels_debug.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT", "-DCCMP_LEAN_DIV", "-mllvm", "-disable-machine-licm"])]  # the device probe of ccmp_detmath.h
ARCH = "gfx950"

_UNITS = [
    # -disable-machine-licm: LLVM's machine LICM hoists ~35 FP64 polynomial/literal constants out of the Newton
    # loop into VGPR pairs and then spills them to scratch (168 VGPRs + 30 spilled dwords); without it the
    # throughput kernel needed 133 VGPRs and no scratch (measured +3.3 %, in-process A/B; today's kernel: 167, no scratch,
    # three wavefronts per SIMD).  The wave kernels are
    # 2.7 % slower with the option, hence their own unit.
    # the two detmath flavours of this unit: CCMP_ATAN_UNIFORM (-2.0 %, in-process A/B) and CCMP_LEAN_SQRT; CCMP_LEAN_DIV (quotients
    # without scaling and fixup) measured +1.0 % here and stays off.  What the kernel's own text does for the stock Panda's structure
    # and how each piece measured: DESIGN.md §5.1, DESIGN_experiments.md §5.6
    ("ccmp_kernels_fd.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT", "-DCCMP_ATAN_UNIFORM",
                             "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]
     + os.environ.get("CCMP_FD_EXTRA_FLAGS", "").split()),
    ("ccmp_kernels_wave.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA"]),
    # max-ilp scheduling: -0.6 % (throughput kernel) ... -1.5 % (latency kernel, single state), in-process A/B
    ("ccmp_kernels_flat.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    # the extend step, built twice from one source.  Throughput flavour (the projector's latency kernel's flags: eight blocks
    # per CU) for calls that bound the Newton rounds per edge; latency flavour (machine LICM on, 256-register budget, four
    # blocks per CU: the ~60 FP64 literals of a Newton round stay in registers instead of being re-materialised every
    # round) for calls whose end is one edge's serial chain: 16 384 edges without a round budget -16 %, with one +23 %.
    ("ccmp_kernels_geo.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-mllvm", "-disable-machine-licm", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    ("ccmp_kernels_geo.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_GEO_LATENCY", "-DCCMP_SUMS_IN_LANE", "-DCCMP_FLAT_MIN_WAVES=2", "-mllvm", "-amdgpu-sched-strategy=max-ilp"],
     "ccmp_kernels_geo_lat.hip.o"),
    # the extend step with a proxy scene (FD mode): the latency flavour's flags — its 256-register budget holds the clearance without scratch
    ("ccmp_kernels_geo_scene.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_SUMS_IN_LANE", "-DCCMP_FLAT_MIN_WAVES=2", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    # the resident service kernel: one block alone on its SIMDs — the latency flavour's flags (registers are free, fewest instructions per round)
    ("ccmp_kernels_resident.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_SUMS_IN_LANE", "-DCCMP_FLAT_MIN_WAVES=2", "-mllvm", "-amdgpu-sched-strategy=max-ilp"]),
    # the analytic mode's lane-pair kernel: without machine LICM (the ~35 FP64 literals of sincos / atan would be held in
    # registers across the Newton loop and spilled: 168 registers + 36 B of scratch instead of 142 and none)
    ("ccmp_kernels_fast.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT", "-mllvm", "-disable-machine-licm"]),
    ("ccmp_kernels_scout.hip", ["-O3", "-ffp-contract=fast", "-ffast-math", "-fno-slp-vectorize"]),  # SLP packs into v_pk_* and spills 310 dwords
    ("ccmp_problem.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    ("ccmp_api.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    ("ccmp_policy.cpp", ["-O2", "-x", "hip"]),
    ("ccmp_resident.cpp", ["-O2", "-x", "hip"]),
    ("ccmp_host_io.cpp", ["-O2", "-x", "hip"]),
    ("ccmp_comm.cpp", ["-O2", "-x", "hip"]),
    ("ccmp_kernels_scene.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # the connection step (k nearest neighbours, gather): the scene unit's flags; its lists live in registers and LDS, never in scratch
    ("ccmp_kernels_knn.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # growTree's sampleCalibGoal step (ccmp_ik.h): one candidate per lane; the k-NN unit's flags, and without machine LICM (the ~35 FP64
    # literals of sincos / atan would be held in registers across the round loop: 256 + 65 registers, one wavefront per SIMD, instead
    # of 190 and two); registers only, never scratch
    ("ccmp_kernels_ik.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT", "-mllvm", "-disable-machine-licm"]),
    # the collision gate of that step (ccmp_ik_vet.h, ccmp_scene_math.h): sixteen lanes per candidate, frames and centres in LDS; the IK unit's flags; registers and LDS only
    ("ccmp_kernels_ik_vet.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT", "-mllvm", "-disable-machine-licm"]),
    # the head of growTree (ccmp_object.h): one block per pose, one triangle per lane and chunk; the k-NN unit's flags; registers only, never scratch
    ("ccmp_kernels_object.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # the roadmap graph (ccmp_graph.h): commit, explicit edges, component labels, closest; the k-NN unit's flags; registers and LDS only
    ("ccmp_kernels_graph.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    ("ccmp_scene.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # the roadmap store and the host side of the object metric (ccmp_pose.h in the rounding model of the kernels)
    ("ccmp_roadmap.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # ccmp_pose_ik_*: the checks and launches, and ccmp_ik.h compiled for the host (ccmp_pose_ik_ref: the kernels' bits without a device)
    ("ccmp_ik.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # ccmp_object_*: the checks and launches, and ccmp_object.h compiled for the host (the *_ref forms: the kernels' bits without a device)
    ("ccmp_object.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # dense solution paths (ccmp_dense.h): gather, pack, arc and the clearance summary; the k-NN unit's flags; registers and LDS only
    ("ccmp_kernels_dense.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_densify: the checks, the continuation loop and the layout rule on the host (ccmp_dense_layout_ref, ccmp_dense_arc_ref)
    ("ccmp_dense.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # shortcut solution paths (ccmp_shortcut.h): enumerate, regather, scatter, select and the kept rows; the dense unit's flags; registers and LDS only
    ("ccmp_kernels_shortcut.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_shortcut: the checks, the tile and continuation loops, and the rule on the host (ccmp_shortcut_select_ref, ccmp_shortcut_pairs_ref)
    ("ccmp_shortcut.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # smooth solution paths (ccmp_smooth.h): load, gather, bracket, pick, accept, length and store; the shortcut unit's flags; registers and LDS only
    ("ccmp_kernels_smooth.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_smooth: the checks, the pass loop over the dense and shortcut units' loops, and the rule on the host (ccmp_smooth_mid_ref, ccmp_smooth_len_after)
    ("ccmp_smooth.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # resample and time stamps (ccmp_retime.h): status, bracket, pick, ceiling, envelope and stamp; the smooth unit's flags; registers and LDS only
    ("ccmp_kernels_retime.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_resample / ccmp_path_timestamps: the checks, the launches and the rule on the host (the *_ref forms)
    ("ccmp_retime.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # controller-rate setpoints and the execution audit (ccmp_setpoints.h): status, tangent, sample and peak; the retime unit's flags; registers and LDS only
    ("ccmp_kernels_setpoints.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_setpoints: the checks, the launches and the rule on the host (ccmp_setpoints_ref, ccmp_setpoint_tangents_ref)
    ("ccmp_setpoints.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # time stamps fitted to the limits at the controller's rate (ccmp_fit.h): begin, measure, dilate and factor; the setpoints unit's flags; registers and LDS only
    ("ccmp_kernels_fit.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_fit_timestamps: the checks, the pass loop and the rule on the host (ccmp_path_fit_timestamps_ref)
    ("ccmp_fit.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # jerk-bounded setpoints (ccmp_jerk.h): measure, decide, sample and peak; the setpoints unit's flags; registers and LDS only
    ("ccmp_kernels_jerk.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_path_jerk_setpoints: the checks, the window search's pass loop and the rule on the host (ccmp_jerk_setpoints_ref)
    ("ccmp_jerk.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # the planner's loop on the store (ccmp_plan.h): front, tally, check, prefix, push and the solution test (both planners' instantiations); the graph unit's flags; registers and LDS only
    ("ccmp_kernels_plan.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_plan_*: the checks, open and the cycle over the store's entry points, and the rule on the host (ccmp_plan_check_ref, _prefix_ref, _connected_ref)
    ("ccmp_plan.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
    # RRT-Connect on the store (ccmp_rrtc.h): nearest-in-tree, edges, pick and commit (its solution test is the plan unit's kernel); the graph unit's flags; registers and LDS only
    ("ccmp_kernels_rrtc.hip", ["-O3", "-ffp-contract=off", "-DCCMP_USE_FMA", "-DCCMP_LEAN_SQRT"]),
    # ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree*: the checks and the cycle over the library's entry points, and the rule on the host (the *_ref forms)
    ("ccmp_rrtc.cpp", ["-O2", "-ffp-contract=off", "-DCCMP_USE_FMA", "-x", "hip"]),
]
_HEADERS = ["ccmp_detmath.h", "ccmp_kin.h", "ccmp_solve.h", "ccmp_fd_common.h", "ccmp_flat_newton.h", "ccmp_host.h", "ccmp_ctx.h", "ccmp_launch.h", "ccmp_policy.h", "ccmp_resident.h", "ccmp_resident_proto.h", "ccmp_fd_newton_phase1.inc", "ccmp_fd_newton_phase2.inc", "ccmp_fd_project_finish.inc", "ccmp_geo_edge.h", "ccmp_geo_edge_body.inc", "ccmp_scene.h", "ccmp_scene_math.h", "ccmp_clearance.h", "ccmp_pose.h", "ccmp_ik.h", "ccmp_ik_vet.h", "ccmp_object.h", "ccmp_graph.h", "ccmp_path.h", "ccmp_dense.h", "ccmp_shortcut.h", "ccmp_smooth.h", "ccmp_retime.h", "ccmp_setpoints.h", "ccmp_fit.h", "ccmp_jerk.h", "ccmp_plan.h", "ccmp_rrtc.h", "ccmp_planner.h", "ccmp_lanes.h", "ccmp_timed.h", "ccmp_pair_tests.h", "ccmp_stage.h", "ccmp_row16_eval.inc", "ccmp_row16_step.inc", "ccmp_row16_geo_body.inc", os.path.join("..", "..", "include", "ccmp.h")]


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libccmp.so cannot be built (no CPU fallback exists)")


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


# ---- build-time check of the kernels' register allocation (round 5) ------------------------------------------------------------
# Every device unit is compiled with -Rpass-analysis=kernel-resource-usage; the remarks are kept beside the object
# (build/<unit>.resources.json) and checked against the bounds below — a build whose hot kernels have started to spill FAILS
# instead of shipping a silently slower library.  Scratch is in bytes per lane.
#   * the STOCK instantiations (template argument `true`: both arms carry the uncalibrated Panda's exact zeros — what the
#     reference ships, ConstrainedPlanningCommon.cpp:97 has the calibration commented out) of the projector kernels, of the extend
#     step's kernels (geodesic_flat_kernel both builds, geodesic_group_kernel) and of the resident service kernel: NO scratch.
#     (geodesic_group_kernel<true> had 64-76 B until round 5: ten loop-invariant per-lane values the allocator parked in scratch
#     under the bound of three wavefronts per SIMD; they are now recomputed where they are used or kept in LDS.  Without the bound
#     the kernel takes 181 registers, no scratch, and is 5 % SLOWER at 16 384 - 32 768 edges — profiles/r05_bulk_live_ab.log, B/r4
#     of version 1: the front's latency blocks lose the register space.)
#   * the general instantiations (calibrated arms, tilted bases): at most 136 B of PRIVATE SEGMENT and not one scratch
#     instruction — the 96-132 B that project_fd_kernel<0,false>, geodesic_group_kernel<false> and geodesic_flat_kernel<false>
#     declare are stack slots of SGPR spills that the allocator then kept in VGPR lanes (v_writelane / v_readlane; the ISA of
#     those kernels contains no scratch_load / scratch_store: tests/test_host_cabi.py checks the objects).  The fused-sampler
#     general instantiation project_fd_kernel<1,false> (2.3 KB of real spills) was removed in round 6: sampleUniform on
#     calibrated arms runs unfused (ccmp_api.cpp: project_common);
#   * everything else (scouts, small per-lane kernels, analytic mode, scene): at most 64 B unless listed.
_SCRATCH_RULES = [  # (regex on the demangled name, bound); first match wins
    (r"(project_fd_kernel|project_fd_flat_kernel|project_fd_wave_kernel|geodesic_flat_kernel(_lat)?|geodesic_scene_kernel|geodesic_group_kernel|resident_service_kernel)<(\d+, )?true>", 0),
    (r"(project_fd_kernel|project_fd_flat_kernel|project_fd_wave_kernel|geodesic_flat_kernel(_lat)?|geodesic_scene_kernel|geodesic_group_kernel|resident_service_kernel)<(\d+, )?false>", 136),
    (r"project_pair_kernel|project_row16_kernel", 0),  # analytic mode, every instantiation (stock twin arms, stock, calibrated)
    (r"resident_row16_kernel", 0),  # the resident service kernel of analytic mode, both instantiations
    (r"geodesic_row16_(scene_)?kernel", 0),  # analytic mode's extend step and its scene variant, both instantiations (diagonal and general base frames)
    (r"knn_|connect_(gather|fix)_kernel", 0),  # the connection step: per-thread lists of up to 16 (distance, index) pairs in registers, every instantiation
    (r"ik_", 0),  # pose-targeted IK: the 6x6 system, the kept sines and cosines and the iterate live in registers, both instantiations
    (r"object_", 0),  # the head of growTree: a lane's triangle, the pose's frame and one box at a time live in registers, every kernel of the unit
    (r"graph_", 0),  # the roadmap graph: a slot's FK and distances, a lane's best candidate and the scan's sums live in registers and LDS, every kernel of the unit
    (r"dense_", 0),  # dense solution paths: a chunk's descriptor, a lane's distance and a lane's best (value, row) live in registers and LDS, every kernel of the unit
    (r"shortcut_", 0),  # shortcut solution paths: a slot's decode, a lane's best parent and the search's d / hops / pred live in registers and LDS, every kernel of the unit
    (r"smooth_", 0),  # smooth solution paths: a pair's decode, its bracket and a lane's row element live in registers, the length's 64 distances in LDS, every kernel of the unit
    (r"resample_|retime_", 0),  # resample and time stamps: a row's bracket, a lane's joint quotients and the limits (kernel arguments) live in registers, the stamps' 64 intervals in LDS
    (r"setpoints_", 0),  # setpoints and audit: a tick's bracket, a lane's joint and a lane's five peaks live in registers, the block's fold of the peaks in LDS
    (r"fit_", 0),  # fitted time stamps: a tick interval's two brackets, a lane's joint at both ticks and the merged maxima live in registers, the dilation's 64 widths in LDS
    (r"jerk_", 0),  # jerk-bounded setpoints: a tick's bracket, a lane's joint, its window's sum and its six peaks live in registers, the staged inputs and the folds in LDS
    (r"plan_", 0),  # the planner's loop: the state block's fields, a lane's ladder pose and a lane's counts live in registers, the check's triggers in LDS
    (r"rrtc_", 0),  # RRT-Connect: a query row and the eight root labels live in scalar registers, a lane's best pair and a group's arc in registers, the folds and the scan in LDS
    (r"scout_|clearance", 400),
    (r".", 64),
]


def _demangle(names):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", shutil.which("c++filt")):
        if tool and os.path.exists(tool):
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
            return dict(zip(names, out))
    return {n: n for n in names}


def parse_resource_remarks(stderr_text):
    """[{name, vgprs, agprs, sgprs, scratch, occupancy, lds, vgpr_spill, sgpr_spill}] from -Rpass-analysis=kernel-resource-usage"""
    import re

    kernels, cur = [], None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
            "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}
    for line in stderr_text.splitlines():
        m = re.search(r"remark: (?:\s*)([A-Za-z \[\]/]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = {"mangled": v}
            kernels.append(cur)
        elif cur is not None and k in keys:
            cur[keys[k]] = int(v)
    dm = _demangle([k["mangled"] for k in kernels])
    for k in kernels:
        k["name"] = dm[k["mangled"]].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
    return kernels


def check_resources(kernels, unit):
    """raises RuntimeError when a kernel of `unit` exceeds its scratch bound"""
    import re

    bad = []
    for k in kernels:
        bound = next(b for rx, b in _SCRATCH_RULES if re.search(rx, k["name"]))
        k["scratch_bound"] = bound
        if k.get("scratch", 0) > bound:
            bad.append("%s: %d B/lane of scratch (bound %d), %d VGPRs, %d spilled" % (k["name"], k["scratch"], bound, k.get("vgprs", -1), k.get("vgpr_spill", -1)))
    if bad and not os.environ.get("CCMP_ALLOW_SPILLS"):
        raise RuntimeError("register allocation of %s regressed (closed_chain_motion_planner_amd/build.py: _SCRATCH_RULES; CCMP_ALLOW_SPILLS=1 "
                           "builds anyway):\n  " % unit + "\n  ".join(bad))


def resource_report():
    """{unit object: [kernel records]} of the last build (build/*.resources.json)"""
    import glob
    import json

    return {os.path.basename(f)[:-len(".resources.json")]: json.load(open(f)) for f in sorted(glob.glob(os.path.join(HERE, "build", "*.resources.json")))}


def build_library(force=False, verbose=False):
    """Compile (if stale) and return the path of libccmp.so."""
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hipcc = hipcc_path()
    headers = [os.path.join(CSRC, h) for h in _HEADERS]
    objs, dbg_objs, jobs = [], [], []
    relink = force
    for src, flags, *obj in _UNITS:  # optional third entry: object name (a source built twice)
        sp = os.path.join(CSRC, src)
        op = os.path.join(objdir, obj[0] if obj else src + ".o")
        objs.append(op)
        variants = [(op, [])]
        if src in _DEBUG_UNITS:  # the debug library's copy of the unit
            dp = os.path.join(objdir, src + ".dbg.o")
            dbg_objs.append(dp)
            variants.append((dp, ["-DCCMP_DEBUG_HOOKS"]))
        else:
            dbg_objs.append(op)
        for target, extra in variants:
            if force or _stale(target, [sp] + headers):
                jobs.append([hipcc, "--offload-arch=" + ARCH, "-fPIC", "-std=c++17"] + flags + extra +
                            (["-Rpass-analysis=kernel-resource-usage"] if src.endswith(".hip") else []) + ["-c", sp, "-o", target])
    for src, flags in _DEBUG_ONLY_UNITS:
        sp, op = os.path.join(CSRC, src), os.path.join(objdir, src + ".o")
        dbg_objs.append(op)
        if force or _stale(op, [sp] + headers):
            jobs.append([hipcc, "--offload-arch=" + ARCH, "-fPIC", "-std=c++17"] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", sp, "-o", op])
    if jobs:  # the units are independent: compile them side by side (hipcc is one process per unit)
        import json
        from concurrent.futures import ThreadPoolExecutor

        def run(cmd):
            if verbose:
                print(" ".join(cmd))
            r = subprocess.run(cmd, capture_output=True, text=True)
            rest = "\n".join(ln for ln in r.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in ln)
            if rest.strip():
                print(rest)
            if r.returncode != 0:
                raise subprocess.CalledProcessError(r.returncode, cmd)
            if "-Rpass-analysis=kernel-resource-usage" in cmd:
                kernels = parse_resource_remarks(r.stderr)
                try:
                    check_resources(kernels, os.path.basename(cmd[-1]))
                except RuntimeError:
                    os.remove(cmd[-1])  # a failed check must not leave an object that looks up to date
                    raise
                json.dump(kernels, open(cmd[-1][:-2] + ".resources.json", "w"), indent=1)

        workers = max(1, min(len(jobs), int(os.environ.get("CCMP_BUILD_JOBS", "0")) or min(4, os.cpu_count() or 1)))
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(run, jobs))
        relink = True
    default_lib = os.path.join(LIBDIR, "libccmp.so")
    for target, members in ((default_lib, objs), (DEBUG_LIBPATH, dbg_objs)):
        if relink or _stale(target, members):
            cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", target] + members
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
    return LIBPATH


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))

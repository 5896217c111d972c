"""The two cuts of the throughput kernel's STOCK instantiations, checked on the host against the functions they replace
(closed_chain_motion_planner_amd/csrc/ccmp_kin.h: rot_sc_x0, tool_pose_fold).  tests/cpp/rot_x0_check.cpp is compiled
with the det oracle's flags (-ffp-contract=off -DCCMP_USE_FMA, hardware FMA where the host has it) against ccmp_kin.h and takes
the stock constants from libccmp's own set-up code:

  * rot_sc_x0 gives rot_sc's nine doubles — all 72 bytes — for every angle the guard rot_x0_admits lets through: over a million
    angles per general joint (1, 3, 5, 6) and arm, among them 0, +-pi/2, +-pi, subnormal and tiny angles, the guard's edge near
    2^-26.5 with its neighbours, the joints' ranges; and the guard refuses nothing but angles within 2^-26 of zero;
  * an iterate that passes rot_x0_round_ok — the test the kernels make once per Newton round and wavefront — has all six points
    of its finite-difference stencil inside that guard (iterates beside multiples of 2 pi up to +-512 among them);
  * chain_residual fed with tool_pose_fold and a pose scaled once by fold_other_pose gives both components of
    chain_residual(tool_pose_t<true>(...), To) bit for bit: both orientations, the eight sign patterns of diag(+-1), random frames.

The set-up raises the flag the kernels test (ccmp_consts::rot_x0) for the stock constants only: the checker reports it for
calibrated arms and for an axis whose x component is 1e-300."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc")
ANGLES = 1 << 21   # per general joint and arm; an eighth of them lie below the guard on purpose, > 10^6 pass it
FRAMES = 200_000   # per sign pattern and orientation: 3.2 million residual pairs


@pytest.fixture(scope="module")
def checker(ccmp_built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rot_x0") / "rot_x0_check")
    libdir = os.path.dirname(ccmp_built)
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read().split() else []
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCCMP_USE_FMA"] + fma + ["-Wall", "-I", CSRC,
           os.path.join(ROOT, "tests", "cpp", "rot_x0_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan"])
def test_short_rotation_and_folded_base_frame_are_bit_identical(checker, obj):
    r = subprocess.run([checker, os.path.join(ROOT, "tests", "golden", "config", obj + ".yaml"), str(ANGLES), str(FRAMES)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode in (0, 1), r.stderr[-2000:]
    n = json.loads(r.stdout.strip().splitlines()[-1])
    print(n)
    assert n["admitted"] >= 8 * 10 ** 6 and n["refused"] > 1000, n   # both sides of the guard were exercised
    assert n["refused_far"] == 0, (n, r.stderr[-2000:])
    # the kernels ask once per Newton round (rot_x0_round_ok on the iterate): the six stencil points of a column then pass the guard
    assert n["round_ok"] > 10 ** 6 and n["round_refused"] > 10 ** 5 and n["stencil_refused"] == 0, n
    assert n["rot_differ"] == 0, (n, r.stderr[-2000:])
    assert n["fold_cases"] == 16 * FRAMES and n["fold_differ"] == 0, (n, r.stderr[-2000:])
    # ccmp_consts::rot_x0: set for the shipped arms (the checker refuses to start otherwise), clear for calibrated arms and for
    # twin arms whose axis has an x component that is tiny but not zero
    assert n["flag_calibrated"] == 0 and n["flag_tilted"] == 0, n
    assert r.returncode == 0

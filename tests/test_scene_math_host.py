"""The proxy scene's shared arithmetic (closed_chain_motion_planner_amd/csrc/ccmp_scene_math.h), checked on the host.  Two kernels build
an arm's frames row by row (state_clearance<NT> of the extend step, ik_vet_kernel of the vetted IK); until now only GPU tests ran that
form.  tests/cpp/scene_math_check.cpp is compiled with the det oracle's flags (-ffp-contract=off -DCCMP_USE_FMA, hardware FMA where the
host has it) against the header and takes its constants from libccmp's own set-up code, for the stock arms, a calibrated pair
(ccmp_set_calibration) and a tilted base (ccmp_set_base_frame), both arms:

  * scene_joint_rot + scene_chain_row (rows 0, 1, 2 in turn) write the eight frames of the one-thread joint_step walk — all 96 doubles,
    byte for byte — over 10^5 joint vectors per model and arm, among them the all-zero vector, the joint limits, +-pi/2 and +-pi;
  * scene_place on those frames equals frame -> base followed by base -> world applied by hand, for every slot kind (the eight frames,
    the base, the world), with one arm's frames and with both arms' frames."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc")
VECTORS = 100_000   # random joint vectors per arm model and arm, on top of the corners
CORNERS = 7 * 8     # zero, +-pi/2, +-pi, both limits: on all joints and on each joint alone


@pytest.fixture(scope="module")
def checker(ccmp_built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_math") / "scene_math_check")
    libdir = os.path.dirname(ccmp_built)
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read().split() else []
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCCMP_USE_FMA"] + fma + ["-Wall", "-I", CSRC,
           os.path.join(ROOT, "tests", "cpp", "scene_math_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_row_wise_chain_and_placement_equal_the_joint_step_walk(checker):
    r = subprocess.run([checker, os.path.join(ROOT, "tests", "golden", "config", "Wine_Bottle.yaml"), str(VECTORS)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stderr[-2000:]
    n = json.loads(r.stdout.strip().splitlines()[-1])
    print(n)
    assert n["vectors"] == 3 * 2 * (VECTORS + CORNERS), n       # three arm models, both arms
    assert n["places"] == 10 * n["vectors"], n                  # eight frames, the base, the world
    assert n["frames_differ"] == 0, (n, r.stderr[-2000:])
    assert n["place_differ"] == 0, (n, r.stderr[-2000:])
    assert r.returncode == 0

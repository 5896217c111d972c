"""The quaternion's case bodies of the throughput kernel's in-range rounds, checked on the host against the function they stand in
for (closed_chain_motion_planner_amd/csrc/ccmp_kin.h: quat_case, quat_of_t against quat_of).  tests/cpp/quat_case_check.cpp is
compiled with the det oracle's flags (-ffp-contract=off -DCCMP_USE_FMA, hardware FMA where the host has it) against ccmp_kin.h and
takes the constants from libccmp's own set-up code:

  * each case body gives quat_of's four doubles — all 32 bytes — on rotations of every case, on matrices at and beside every case
    boundary (trace 0 and its neighbours, two and three equal largest diagonal entries), on the fixture's own relative rotation at
    its initial pose, and on 10^5 relative rotations that the two chains produce at random states (half inside the joint limits,
    half anywhere in |x_j| <= 512, the range of an in-range round);
  * on the same matrices the radicand that quat_of selects is at least 1 - 2^-40 and its root lies in [1, 2] up to 2^-40: what lets
    the kernels take the root and the quotient 0.5 / root without their guards."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc")
ROTATIONS = 400_000
CHAIN = 100_000


@pytest.fixture(scope="module")
def checker(ccmp_built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("quat_case") / "quat_case_check")
    libdir = os.path.dirname(ccmp_built)
    fma = ["-mfma"] if "fma" in open("/proc/cpuinfo").read().split() else []
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-DCCMP_USE_FMA"] + fma + ["-Wall", "-I", CSRC,
           os.path.join(ROOT, "tests", "cpp", "quat_case_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan", "dumbbell"])
def test_case_bodies_are_bit_identical_and_the_radicand_is_at_least_one(checker, obj):
    r = subprocess.run([checker, os.path.join(ROOT, "tests", "golden", "config", obj + ".yaml"), str(ROTATIONS), str(CHAIN)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stderr[-2000:]
    n = json.loads(r.stdout.strip().splitlines()[-1])
    print(n)
    # every case was exercised: by random rotations, at the boundaries, and by the chains
    assert min(n["random_cases"]) > 10_000, n
    assert min(n["boundary_cases"]) > 1_000, n
    assert n["tr_zero"] > 10_000 and n["tr_pos"] > 10_000 and n["tr_neg"] > 10_000, n
    assert n["ties2"] > 10_000 and n["ties3"] > 10_000, n
    assert n["chain"] == CHAIN and min(n["chain_cases"]) > 100, n
    assert n["init_case"] in (0, 1, 2, 3)
    assert n["differ"] == 0 and n["form_differ"] == 0, (n, r.stderr[-2000:])
    # the lemma: selected radicand >= 1 - 2^-40, root in [1, 2] up to 2^-40
    assert n["radicand_low"] == 0 and n["root_out"] == 0, (n, r.stderr[-2000:])
    assert n["radicand_min_minus_1"] >= -2.0 ** -40 and n["radicand_max"] <= 4.0 + 2.0 ** -40, n
    assert r.returncode == 0

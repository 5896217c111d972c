"""The connection step through the C++ adapter (include/ccmp_ompl_adapter.hpp, part 2, against the interface mock in tests/cpp/mock_ompl):
jy_ProjectedStateSpace::connectMilestone must return the neighbours, bools and lists of the reference's loop — nearestK, then checkMotion
per neighbour — and ask the StateValidityChecker about the same states in the same order."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_connect_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_connect_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_connect_path_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_connect_milestone_equals_the_neighbour_loop(ccmp_built, oracle_det):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    P = oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle")))
    start = np.array(P.start_joint[:])
    out = subprocess.run([exe] + ["%.17g" % v for v in start], check=True, capture_output=True, text=True).stdout.splitlines()
    one = [ln.split(" ", 1)[1] for ln in out if ln.startswith("connect ")]
    loop = [ln.split(" ", 1)[1] for ln in out if ln.startswith("loop ")]
    lists = [ln for ln in out if ln.startswith("lists ")]
    print("edges %d, reached %d, off-manifold target edges %d" % (len(one) - 1, sum(" ok 1" in ln for ln in one), sum(" target 0" in ln for ln in lists)))
    # neighbours and bools, edge by edge; the last line: how often and about which states (hash, in order) the checker was asked
    assert len(one) == len(loop) > 100
    assert one == loop
    # the ranking against (distance, index) computed beside it; no call failed
    assert out[-1] == "rank mismatches 0 errors 0"
    # every list is the list of a single discreteGeodesic call; an unsatisfied target leaves `from` alone
    assert len(lists) == len(one) - 1 and all(" same 1" in ln for ln in lists)
    assert any(" target 0" in ln for ln in lists)
    # fewer nodes than k: three and four neighbours for the first two vertices
    assert sum(ln.startswith("v 3 ") for ln in one) == 3 and sum(ln.startswith("v 4 ") for ln in one) == 4

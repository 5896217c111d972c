"""ccmp::Roadmap's solution step (include/ccmp_ompl_adapter.hpp: shortestPath, constructSolution, against the interface mock in
tests/cpp/mock_ompl): the adapter's answers line by line against ccmp_graph_shortest_paths_ref on the edges read back from the store,
the returned joint rows bit for bit inside the program, and the sticky error on deliberate bad calls; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "path_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "path_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_path_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_adapter_paths_equal_the_ref_form(ccmp_built, oracle_det):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    P = oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle")))
    start = np.array(P.start_joint[:])
    out = subprocess.run([exe] + ["%.17g" % v for v in start], check=True, capture_output=True, text=True).stdout.splitlines()
    got = [ln.split(" ", 1)[1] for ln in out if ln.startswith("adapter ")]
    ref = [ln.split(" ", 1)[1] for ln in out if ln.startswith("ref ")]
    assert len(got) == len(ref) == 10 + 1 and got == ref, [(a, b) for a, b in zip(got, ref) if a != b]
    assert sum(" found 1 " in ln for ln in got) >= 8 and sum(" found 0 cost inf" in ln for ln in got) == 3
    # no mismatch, no failed call before the deliberate ones; those two return false (00) with an empty path and cost +inf, leave
    # CCMP_EINVAL (-1) and clear; the store answers afterwards
    assert out[-1] == "summary mismatches 0 errors 0 before 0 failed 00 shape 1 sticky -1 cleared 0 again 1", out[-1]

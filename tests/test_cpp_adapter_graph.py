"""ccmp::Roadmap's graph verbs (include/ccmp_ompl_adapter.hpp: commit, addEdges, closest, numEdges, against the interface mock in
tests/cpp/mock_ompl): the adapter's answers line by line against the *_ref forms on the arrays read back from the store, the rows,
edges and labels bit for bit inside the program, and the sticky error on deliberate bad calls; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "graph_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "graph_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_graph_path_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_adapter_graph_equals_the_ref_forms(ccmp_built, oracle_det):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    P = oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle")))
    start = np.array(P.start_joint[:])
    out = subprocess.run([exe] + ["%.17g" % v for v in start], check=True, capture_output=True, text=True).stdout.splitlines()
    got = [ln.split(" ", 1)[1] for ln in out if ln.startswith("adapter ")]
    ref = [ln.split(" ", 1)[1] for ln in out if ln.startswith("ref ")]
    assert len(got) == len(ref) == 12 + 5 and got == ref, [(a, b) for a, b in zip(got, ref) if a != b]
    assert any(" state 1 " in ln or " state 2 " in ln for ln in got)  # a vertex was kept with an edge
    # no mismatch, no failed call before the deliberate ones; those three return false (000), leave CCMP_EINVAL (-1) and clear
    assert out[-1] == "summary mismatches 0 errors 0 before 0 failed 000 sticky -1 cleared 0", out[-1]

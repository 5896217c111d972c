"""The adapter's resampled and time-stamped paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::resamplePath / timePath,
ccmp::Roadmap::constructTimedSolution, ccmp::printTrajectory, against the interface mock in tests/cpp/mock_ompl): the rows and times the
program prints, bit for bit against the mirror's host forms on the five waypoints of retime_cases.long_path (every segment traversable: the
recorded Wine_Bottle waypoints have a segment that stops short, which resampling refuses; the mirror itself is compared with the
oracle-backed restatement in tests/test_gpu_retime.py) and on the smooth solution of the recorded roadmap; inside the program printTrajectory's first 14 columns equal printAsMatrix's; a library error returns the unchanged
path / untouched times / the smooth solution without times with lastError() set; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path
from dense_path_cases import RECORDED, recorded_roadmap
import retime_cases as rc
from retime_cases import PANDA_AMAX, PANDA_VMAX, bits

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_retime_check")
EINVAL = -1


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_retime_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_retime_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _rows(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " rows ")][0].split()
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    times = np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(tag + " time")][0].split()[2:]])
    assert len(rows) == int(head[2]) and len(times) == int(head[4])
    return rows, times


def _mirror(c, waypoints, beta, **kw):
    """the mirror's host forms on one path of waypoints: (rows, times)"""
    dense = c.densify_paths(waypoints[None].copy(), np.array([len(waypoints)], dtype=np.int32), distinct=True, keep_handle=True)
    try:
        got = c.resample_paths(dense, **kw)
    finally:
        dense["handle"].close()
    return got["joints"], c.timestamp_paths(got["joints"], got["path_first"], PANDA_VMAX, PANDA_AMAX, beta=beta)["time"]


@pytest.mark.gpu
def test_adapter_rows_and_times_equal_the_mirrors_host_form(ccmp_built, gpu_ctx, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config
    from test_gpu_parity import _constraint

    exe = _build(ccmp_built)
    O = oracle_det
    start = np.array(O.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    pj = rc.reference(0)["long"]["case"]["pj"]
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "retime_input.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (pj.shape[1], len(nodes), len(uv)))
        for r in list(pj[0]) + list(nodes):
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    out = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    c = _constraint("Wine_Bottle", gpu_ctx, 0)
    c.problem.delta = rec["delta"]
    for tag, beta, kw in (("count", 0.5, dict(count=17)), ("spacing", 0.2, dict(spacing=0.125))):
        rows, times = _rows(out, tag)
        want_rows, want_times = _mirror(c, pj[0], beta, **kw)
        assert np.array_equal(bits(rows), bits(want_rows)) and np.array_equal(bits(times), bits(want_times)), tag
    assert _rows(out, "count")[0].shape == (17, 14)
    # constructTimedSolution: the smooth solution (two passes) of the pairs (0|1) x (9|6), resampled at the space's delta, stamped
    smooth, none = _rows(out, "smooth")
    rows, times = _rows(out, "solution")
    want_rows, want_times = _mirror(c, smooth, 0.5)
    assert len(none) == 0 and len(smooth) >= 2 and len(rows) > len(smooth) and np.array_equal(bits(rows), bits(want_rows)) and np.array_equal(bits(times), bits(want_times))
    # nothing mismatched inside the program, no error before the deliberate cases; every refused call keeps CCMP_EINVAL: resamplePath false,
    # timePath false, constructTimedSolution true (the smooth solution without times)
    assert out[-1] == "summary mismatches 0 before 0 0 bad 0 0 %d roadmap 1 %d" % (EINVAL, EINVAL), out[-1]

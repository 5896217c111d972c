"""The adapter's jerk-bounded setpoints (include/ccmp_ompl_adapter.hpp: ccmp::jerkSetpointPath, jy_ProjectedStateSpace::jerkSetpointPath, the
overload of ccmp::Roadmap::constructExecutableSolution that takes jmax and ccmp::JerkOptions, printSetpoints for ccmp::JerkSetpoints, against
the interface mock in tests/cpp/mock_ompl): the ticks and answers the program prints, bit for bit against the mirror's host form on the
three-row path of jerk_cases.ragged_batch (the mirror itself is compared with the restatement in tests/test_gpu_jerk.py) and on the timed
solution of the recorded roadmap, without and with the fit; inside the program window 1 equals the plain setpoints, a path out of order is
an answer with its status, a library error returns *out untouched / the timed solution with empty setpoints with lastError() set; nothing
throws."""
import os
import subprocess

import numpy as np
import pytest

import jerk_cases as jc
from conftest import ROOT, config_path
from dense_path_cases import RECORDED, recorded_roadmap
from jerk_cases import PANDA_AMAX, PANDA_JMAX, PANDA_VMAX, bits

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_jerk_check")
EINVAL = -1
PERIOD = 0.001


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_jerk_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_jerk_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _jerk(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " jerk ")][0].split()[2:]
    ticks = np.array([[float.fromhex(v) for v in ln.split()[3:-1]] for ln in lines if ln.startswith(tag + " tick ")]).reshape(-1, 31)
    sat = np.array([int(ln.split()[-1]) for ln in lines if ln.startswith(tag + " tick ")], dtype=np.uint8)
    assert len(ticks) == int(head[3])
    return dict(status=np.array([int(head[0])], dtype=np.int32), window=np.array([int(head[1])], dtype=np.int32), passes=np.array([int(head[2])], dtype=np.int32),
                counts=np.array([[int(head[4]), int(head[5])]], dtype=np.int32), peak=np.array([[float.fromhex(v) for v in head[6:12]]]),
                peak_tick=np.array([[int(v) for v in head[12:18]]], dtype=np.int32), tau=ticks[:, 0], q=ticks[:, 1:15], qd=ticks[:, 15:29], f=ticks[:, 29:31],
                satisfied=sat)


def _rows(lines, tag):
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    times = np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(tag + " time")][0].split()[2:]])
    return rows, times


@pytest.mark.gpu
def test_adapter_jerk_equals_the_mirrors_host_form(ccmp_built, gpu_ctx, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config
    from test_gpu_parity import _constraint

    exe = _build(ccmp_built)
    start = np.array(oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    one = jc.one_path(jc.reference()["case"], "three")
    path, stamps = one["rows"], one["time"]
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "jerk_input.txt"
    with open(inp, "w") as out:
        out.write("%d %d %d\n" % (len(path), len(nodes), len(uv)))
        for r in path:
            out.write(" ".join(float(v).hex() for v in r) + "\n")
        out.write(" ".join(float(v).hex() for v in stamps) + "\n")
        for r in nodes:
            out.write(" ".join(float(v).hex() for v in r) + "\n")
        out.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    lines = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], "%.17g" % PERIOD, str(inp)], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    c = _constraint("Wine_Bottle", gpu_ctx, 0)
    c.problem.delta = rec["delta"]
    keys = ("q", "qd", "tau", "f", "satisfied", "status", "window", "passes", "peak", "peak_tick", "counts")
    want = c.jerk_setpoint_paths(path, np.array([0, len(path)], dtype=np.int32), stamps, PANDA_VMAX, PANDA_AMAX, PANDA_JMAX, period=PERIOD)
    got = _jerk(lines, "path")
    jc.same_jerk(got, want, "path", keys=keys)
    assert got["status"].tolist() == [jc.OK] and got["window"][0] >= 2
    # the overload of constructExecutableSolution: the timed solution (two smoothing passes) of the pairs (0|1) x (9|6), its ticks filtered
    rows, times = _rows(lines, "timed")
    first = np.array([0, len(rows)], dtype=np.int32)
    want = c.jerk_setpoint_paths(rows, first, times, PANDA_VMAX, PANDA_AMAX, PANDA_JMAX, period=PERIOD)
    jc.same_jerk(_jerk(lines, "executable"), want, "executable", keys=keys)
    # ... and behind the fit: the rows are the same, the stamps the fitted ones
    rows_fit, times_fit = _rows(lines, "fitted")
    fit = c.fit_timestamps(rows, first, times, PANDA_VMAX, PANDA_AMAX, period=PERIOD)
    assert np.array_equal(bits(rows_fit), bits(rows)) and np.array_equal(bits(times_fit), bits(fit["time"])) and fit["status"].tolist() == [0]
    want = c.jerk_setpoint_paths(rows, first, fit["time"], PANDA_VMAX, PANDA_AMAX, PANDA_JMAX, period=PERIOD)
    got = _jerk(lines, "executable_fit")
    jc.same_jerk(got, want, "executable behind the fit", keys=keys)
    assert (got["peak"][0, :3] <= 1.0).all() and len(rows) >= 2
    # nothing mismatched inside the program, no error before the deliberate cases; the refused calls keep CCMP_EINVAL: jerkSetpointPath false,
    # constructExecutableSolution true (the timed solution with empty setpoints)
    assert lines[-1] == "summary mismatches 0 before 0 0 bad 0 %d roadmap 1 %d" % (EINVAL, EINVAL), lines[-1]

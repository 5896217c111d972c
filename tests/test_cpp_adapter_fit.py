"""The adapter's fitted time stamps (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::fitPath and the overload of
ccmp::Roadmap::constructExecutableSolution that takes fit options, against the interface mock in tests/cpp/mock_ompl): the stamps, factors
and answers the program prints, bit for bit against the mirror's host form on the 17-row path of fit_cases.ragged_batch (the mirror itself
is compared with the restatement in tests/test_gpu_fit.py) and on the timed solution of the recorded roadmap; inside the program the audit of
the fitted stamps reports the fit's peaks, fitted stamps come back untouched, a spent pass budget and a path out of order are answers with
their status; a library error returns *out untouched / the time-stamp rule's stamps with lastError() set; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

import fit_cases as fc
from conftest import ROOT, config_path
from dense_path_cases import RECORDED, recorded_roadmap
from fit_cases import NAMES, PANDA_AMAX, PANDA_VMAX, bits

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_fit_check")
EINVAL = -1


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_fit_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_fit_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _fit(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " fit ")][0].split()[2:]
    vals = lambda key: np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(tag + " " + key)][0].split()[2:]])
    return dict(status=np.array([int(head[0])], dtype=np.int32), passes=np.array([int(head[1])], dtype=np.int32),
                peak=np.array([[float.fromhex(head[2]), float.fromhex(head[3])]]), duration=np.array([float.fromhex(head[4])]), time=vals("fitted"),
                factor=vals("factor"))


def _rows(lines, tag):
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    times = np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(tag + " time")][0].split()[2:]])
    return rows, times


@pytest.mark.gpu
def test_adapter_fit_equals_the_mirrors_host_form(ccmp_built, gpu_ctx, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config
    from test_gpu_parity import _constraint

    exe = _build(ccmp_built)
    start = np.array(oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    case = fc.reference()["case"]
    pf, f = case["path_first"], NAMES.index("seventeen")
    path, stamps = case["rows"][pf[f]:pf[f + 1]], case["time"][pf[f]:pf[f + 1]]
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "fit_input.txt"
    with open(inp, "w") as out:
        out.write("%d %d %d\n" % (len(path), len(nodes), len(uv)))
        for r in path:
            out.write(" ".join(float(v).hex() for v in r) + "\n")
        out.write(" ".join(float(v).hex() for v in stamps) + "\n")
        for r in nodes:
            out.write(" ".join(float(v).hex() for v in r) + "\n")
        out.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    lines = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], "%.17g" % case["period"], str(inp)], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    c = _constraint("Wine_Bottle", gpu_ctx, 0)
    c.problem.delta = rec["delta"]
    want = c.fit_timestamps(path, np.array([0, len(path)], dtype=np.int32), stamps, PANDA_VMAX, PANDA_AMAX, period=case["period"])
    got = _fit(lines, "path")
    fc.same_fit(got, want, "path")
    assert got["status"].tolist() == [fc.FITTED] and got["passes"][0] >= 2
    # the overload of constructExecutableSolution: the timed solution (two smoothing passes) of the pairs (0|1) x (9|6), its stamps fitted
    rows, times = _rows(lines, "timed")
    first = np.array([0, len(rows)], dtype=np.int32)
    want = c.fit_timestamps(rows, first, times, PANDA_VMAX, PANDA_AMAX, period=case["period"])
    got = _fit(lines, "executable")
    fc.same_fit(got, want, "executable")
    audit = [ln for ln in lines if ln.startswith("executable audit")][0].split()[2:]
    sp = c.setpoint_paths(rows, first, want["time"], PANDA_VMAX, PANDA_AMAX, period=case["period"])
    assert int(audit[0]) == sp["ticks"] and np.array_equal(bits(np.array([float.fromhex(v) for v in audit[1:3]])), bits(sp["peak"][0, :2]))
    assert float.fromhex(audit[3]) == 1.0 and len(rows) >= 2
    # nothing mismatched inside the program, no error before the deliberate cases; the refused calls keep CCMP_EINVAL: fitPath false,
    # constructExecutableSolution true (the time-stamp rule's stamps and their setpoints)
    assert lines[-1] == "summary mismatches 0 before 0 0 bad 0 %d roadmap 1 %d" % (EINVAL, EINVAL), lines[-1]

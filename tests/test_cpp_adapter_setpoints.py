"""The adapter's setpoints and execution audit (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::setpointPath,
ccmp::Roadmap::constructExecutableSolution, ccmp::printSetpoints, against the interface mock in tests/cpp/mock_ompl): the ticks and audits
the program prints, bit for bit against the mirror's host form on the 17-row path of setpoint_cases.ragged_batch (the mirror itself is
compared with the restatement and the oracle in tests/test_gpu_setpoints.py) and on the timed solution of the recorded roadmap; inside the
program printSetpoints writes one line of 29 columns per tick; a path out of order is an answer with its status; a library error returns
*out untouched / the timed solution without setpoints with lastError() set; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

import setpoint_cases as sc
from conftest import ROOT, config_path
from dense_path_cases import RECORDED, recorded_roadmap
from setpoint_cases import PANDA_AMAX, PANDA_VMAX, bits

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_setpoints_check")
EINVAL = -1


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_setpoints_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_setpoints_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _setpoints(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " ticks ")][0].split()
    ticks = [ln.split()[3:] for ln in lines if ln.startswith(tag + " tick ")]
    vals = np.array([[float.fromhex(v) for v in t[:32]] for t in ticks]).reshape(-1, 32)
    audit = [ln for ln in lines if ln.startswith(tag + " audit")][0].split()[2:]
    assert len(vals) == int(head[2])
    return dict(status=np.array([int(head[4])], dtype=np.int32), tau=vals[:, 0], q=vals[:, 1:15], qd=vals[:, 15:29], f=vals[:, 29:31], clearance=vals[:, 31],
                satisfied=np.array([int(t[32]) for t in ticks], dtype=np.uint8), peak=np.array([[float.fromhex(v) for v in audit[:5]]]),
                stretch=np.array([float.fromhex(audit[5])]), peak_tick=np.array([[int(v) for v in audit[6:11]]], dtype=np.int32),
                counts=np.array([[int(v) for v in audit[11:13]]], dtype=np.int32))


def _rows(lines, tag):
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    times = np.array([float.fromhex(v) for v in [ln for ln in lines if ln.startswith(tag + " time")][0].split()[2:]])
    return rows, times


@pytest.mark.gpu
def test_adapter_setpoints_equal_the_mirrors_host_form(ccmp_built, gpu_ctx, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config
    from test_gpu_parity import _constraint

    exe = _build(ccmp_built)
    start = np.array(oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    case = sc.reference()["ragged"]["case"]
    pf = case["path_first"]
    path, stamps = case["rows"][pf[4]:pf[5]], case["time"][pf[4]:pf[5]]
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "setpoints_input.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (len(path), len(nodes), len(uv)))
        for r in path:
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(float(v).hex() for v in stamps) + "\n")
        for r in nodes:
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    out = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], "%.17g" % case["period"], str(inp)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    c = _constraint("Wine_Bottle", gpu_ctx, 0)
    c.problem.delta = rec["delta"]
    first = np.array([0, len(path)], dtype=np.int32)
    want = c.setpoint_paths(path, first, stamps, PANDA_VMAX, PANDA_AMAX, period=case["period"])
    got = _setpoints(out, "path")
    sc.same_setpoints(got, want, "path")
    assert len(got["tau"]) == 257
    # constructExecutableSolution: the timed solution (two smoothing passes) of the pairs (0|1) x (9|6), then its setpoints
    rows, times = _rows(out, "solution")
    want = c.setpoint_paths(rows, np.array([0, len(rows)], dtype=np.int32), times, PANDA_VMAX, PANDA_AMAX, period=case["period"])
    got = _setpoints(out, "executable")
    sc.same_setpoints(got, want, "executable")
    assert len(rows) >= 2 and np.array_equal(bits(got["tau"][-1:]), bits(times[-1:]))
    # nothing mismatched inside the program, no error before the deliberate cases; the refused calls keep CCMP_EINVAL: setpointPath false,
    # constructExecutableSolution true (the timed solution without setpoints)
    assert out[-1] == "summary mismatches 0 before 0 0 bad 0 %d roadmap 1 %d" % (EINVAL, EINVAL), out[-1]

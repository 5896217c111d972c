"""The adapter's smooth solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::smoothPath,
ccmp::Roadmap::constructSmoothSolution, against the interface mock in tests/cpp/mock_ompl): the rows the program prints, bit for bit
against the mirror's host form on the recorded Wine_Bottle waypoints (projected by the oracle, so that the traversals run; the mirror
itself is compared with the oracle-backed restatement in tests/test_gpu_smooth.py) and on the shortcut cheapest path of the recorded
roadmap; inside the program every answer is compared with the C ABI called directly under another cut; a library error returns the
unchanged path with lastError() set; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path
from dense_path_cases import RECORDED, recorded_roadmap
from shortcut_cases import bits, recorded_waypoints

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_smooth_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_smooth_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_smooth_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _rows(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " rows ")][0].split()
    n, passes, moved = int(head[2]), int(head[4]), int(head[6])
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    assert len(rows) == n
    return rows, passes, moved


@pytest.mark.gpu
def test_adapter_rows_equal_the_mirrors_host_form(ccmp_built, gpu_ctx, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config
    from test_gpu_parity import _constraint

    exe = _build(ccmp_built)
    O = oracle_det
    start = np.array(O.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    P, pj, pl = recorded_waypoints(O, "Wine_Bottle", 0, projected=True)
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "smooth_input.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (pj.shape[1], len(nodes), len(uv)))
        for r in list(pj[0]) + list(nodes):
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    out = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    c = _constraint("Wine_Bottle", gpu_ctx, 0)
    c.problem.delta = rec["delta"]
    for tag, steps in (("three", 3), ("five", 5)):
        want = c.smooth_paths(pj, pl, max_steps=steps)
        n = int(want["out_len"][0])
        rows, passes, moved = _rows(out, tag)
        assert np.array_equal(bits(rows), bits(want["joints"][0, :n])) and (passes, moved) == (int(want["passes"][0]), int(want["moved"][0])), tag
    assert _rows(out, "three")[0].shape == (33, 14) and _rows(out, "five")[0].shape == (129, 14)
    # constructSmoothSolution: the shortcut solution of the pairs (0|1) x (9|6), then two passes
    head = [ln for ln in out if ln.startswith("solution found ")][0].split()
    kept = [int(v) for v in head[6:]]
    assert head[2] == "1" and len(kept) >= 2
    spj, spl = nodes[kept][None].copy(), np.array([len(kept)], dtype=np.int32)
    want = c.smooth_paths(spj, spl, max_steps=2)
    n = int(want["out_len"][0])
    rows, passes, moved = _rows(out, "solution")
    assert np.array_equal(bits(rows), bits(want["joints"][0, :n])) and (passes, moved) == (int(want["passes"][0]), int(want["moved"][0]))
    assert float.fromhex(head[4]) == want["length_out"][0]
    # nothing mismatched inside the program, no error before the deliberate cases; a refused call comes back unchanged with EINVAL kept
    assert out[-1] == "summary mismatches 0 before 0 0 bad 0 -1 roadmap 1 -1", out[-1]

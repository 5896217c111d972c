"""The adapter's dense solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::interpolatePath,
ccmp::Roadmap::constructDenseSolution, against the interface mock in tests/cpp/mock_ompl): the rows the program prints, bit for bit
against the det oracle's segments joined by the rule of tests/dense_path_cases.py — the 30 rows of Wine_Bottle_path.txt from its five
waypoints, and the dense cheapest path on the recorded roadmap; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path
from dense_path_cases import RECORDED, bits, cheapest_pair, join, oracle_segments, recorded_case, recorded_roadmap

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_dense_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_dense_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_dense_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _rows(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " rows ")][0].split()
    n, ok = int(head[2]), [int(v) for v in head[4:]]
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    assert len(rows) == n
    return rows, ok


@pytest.mark.gpu
def test_adapter_rows_equal_the_oracle_joined_by_the_rule(ccmp_built, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    O = oracle_det
    start = np.array(O.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    P, pj, pl, segs, file_rows = recorded_case(O, "Wine_Bottle")
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "dense_input.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (pj.shape[1], len(nodes), len(uv)))
        for r in list(pj[0]) + list(nodes):
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    out = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    # interpolatePath: the 30 rows of the recorded file, the distinct layout's 26
    for tag, distinct in (("reference", False), ("distinct", True)):
        want = join(pj, pl, pj.shape[1], segs, distinct=distinct)
        rows, ok = _rows(out, tag)
        assert rows.shape == want["rows"].shape and np.array_equal(bits(rows), bits(want["rows"])), tag
        assert ok == want["seg_ok"][0].tolist() == [1, 0, 1, 1]
    rows, _ = _rows(out, "reference")
    assert len(rows) == rec["rows"] and np.abs(rows - file_rows).max() <= rec["bound"]
    assert "matrix lines %d" % (rec["rows"] + 1) in out  # printAsMatrix: one line per row and the empty line behind them
    # constructDenseSolution: the cheapest of the pairs (0|1) x (9|6), dense
    cost, path = cheapest_pair(nodes, uv, [0, 1], [9, 6])
    head = [ln for ln in out if ln.startswith("solution found ")][0].split()
    assert head[2] == "1" and float.fromhex(head[4]) == cost and [int(v) for v in head[6:]] == path.tolist()
    spj, spl = nodes[path][None], np.array([len(path)], dtype=np.int32)
    want = join(spj, spl, len(path), oracle_segments(O, P, spj, spl))
    rows, ok = _rows(out, "solution")
    assert rows.shape == want["rows"].shape and np.array_equal(bits(rows), bits(want["rows"])) and ok == want["seg_ok"][0].tolist()
    # nothing mismatched inside the program, no error before the deliberate case; a roadmap without vertices answers "no" without an error
    assert out[-1] == "summary mismatches 0 before 0 0 empty 0 0", out[-1]

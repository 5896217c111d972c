"""The adapter's shortcut solution paths (include/ccmp_ompl_adapter.hpp: jy_ProjectedStateSpace::shortcutPath,
ccmp::Roadmap::constructShortcutSolution, against the interface mock in tests/cpp/mock_ompl): the kept waypoints the program prints, bit
for bit against the det oracle's verdicts under the rule restated in tests/shortcut_cases.py — the recorded Wine_Bottle waypoints
(projected by the oracle, so that the traversals run) shrink to their two ends — and the shortcut cheapest path on the recorded roadmap;
inside the program every answer is compared with the C ABI called directly; nothing throws."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path
from dense_path_cases import RECORDED, cheapest_pair, recorded_roadmap
from shortcut_cases import bits, expect, oracle_pairs, recorded_waypoints

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_shortcut_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_shortcut_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_adapter_shortcut_check_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _rows(lines, tag):
    head = [ln for ln in lines if ln.startswith(tag + " rows ")][0].split()
    n, kept = int(head[2]), [int(v) for v in head[4:]]
    rows = np.array([[float.fromhex(v) for v in ln.split()[3:]] for ln in lines if ln.startswith(tag + " row ")]).reshape(-1, 14)
    assert len(rows) == n == len(kept)
    return rows, kept


@pytest.mark.gpu
def test_adapter_kept_rows_equal_the_oracle_under_the_rule(ccmp_built, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    O = oracle_det
    start = np.array(O.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle"))).start_joint[:])
    rec = RECORDED["Wine_Bottle"]
    P, pj, pl = recorded_waypoints(O, "Wine_Bottle", 0, projected=True)
    nodes, uv = recorded_roadmap()
    inp = tmp_path / "shortcut_input.txt"
    with open(inp, "w") as f:
        f.write("%d %d %d\n" % (pj.shape[1], len(nodes), len(uv)))
        for r in list(pj[0]) + list(nodes):
            f.write(" ".join(float(v).hex() for v in r) + "\n")
        f.write(" ".join(str(int(v)) for v in uv.reshape(-1)) + "\n")
    out = subprocess.run([exe] + ["%.17g" % v for v in start] + ["%.17g" % rec["delta"], str(inp)], check=True, capture_output=True, text=True).stdout.splitlines()
    for tag, span in (("every", 0), ("span2", 2)):
        want = expect(pj, pl, oracle_pairs(O, P, pj, pl, max_span=span)[0])
        n = int(want["out_len"][0])
        rows, kept = _rows(out, tag)
        assert kept == want["kept"][0, :n].tolist() and np.array_equal(bits(rows), bits(want["joints"][0, :n])), tag
        if span == 0:
            assert kept == [0, 4]
    # constructShortcutSolution: the cheapest of the pairs (0|1) x (9|6), then its interior vertices removed
    cost, path = cheapest_pair(nodes, uv, [0, 1], [9, 6])
    head = [ln for ln in out if ln.startswith("solution found ")][0].split()
    assert head[2] == "1" and [int(v) for v in head[6:]] == path.tolist()
    spj, spl = nodes[path][None], np.array([len(path)], dtype=np.int32)
    want = expect(spj, spl, oracle_pairs(O, P, spj, spl)[0])
    n = int(want["out_len"][0])
    rows, idx = _rows(out, "solution")
    assert idx == path[want["kept"][0, :n]].tolist() and np.array_equal(bits(rows), bits(want["joints"][0, :n]))
    assert float.fromhex(head[4]) == want["cost_out"][0] <= cost
    # nothing mismatched inside the program, no error before the deliberate case; a path beyond the limit comes back unchanged with EINVAL kept
    assert out[-1] == "summary mismatches 0 before 0 0 long 0 -1", out[-1]

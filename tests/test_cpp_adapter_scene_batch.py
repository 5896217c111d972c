"""ccmp::discreteGeodesicBatch with a proxy scene (include/ccmp_ompl_adapter.hpp, part 1, plain C++14) at every shape its host loop
treats differently — lists too short for an edge, the 1024-edge first pass, no scene — must give the same edges, bit for bit, and ask the
host checker the same questions in the same order (tests/cpp/adapter_scene_batch_check.cpp).  24 vertices from RefSampleBuffer::Near with
seed 2 and spacing 0.5, delta 0.05, lambda 2.0.  With these, over the margins 0.02 / 0.12: 10 / 0 edges of (a) are continued, 4 / 12
blocked, 4 / 0 cut by the checker, and 93 / 0 edges of (b) have more than 16 states."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_scene_batch_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_scene_batch_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_scene_batch_compiles_as_plain_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


def _runs(out, case):
    """{run tag: its lines, edge lines first, then the checker's log} of one case, in the order printed"""
    runs = {}
    for ln in out:
        if ln.startswith(case + " "):
            tag, body = ln.split(" | ", 1)
            runs.setdefault(tag, []).append(body)
    return runs


@pytest.mark.gpu
def test_scene_batch_is_the_same_at_every_shape(ccmp_built, oracle_det):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    P = oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle")))
    start = np.array(P.start_joint[:])
    conditions = np.zeros(4, dtype=int)
    for margin in (0.02, 0.12):
        out = subprocess.run([exe, "%.17g" % margin] + ["%.17g" % v for v in start], check=True, capture_output=True, text=True).stdout.splitlines()
        # (a) lists of 2, 3 and 64 states: the same six edges and the same log, with and without the target test
        a = _runs(out, "a")
        assert len(a) == 6
        for ct in (0, 1):
            small, three, long = (a["a ct %d max_states %d" % (ct, m)] for m in (1, 3, 64))
            assert len(long) == 7 and long[-1].startswith("log ")
            assert small == long and three == long, (margin, ct)
        # (b) 1024 edges in one call and in two calls of 512: the same edges, the same concatenated log
        b = _runs(out, "b")
        one, two = b["b calls 1"], b["b calls 2"]
        assert len(one) == 1025 and [ln.split()[1] for ln in one[:-1]] == [str(e) for e in range(1024)]
        assert one == two, margin
        # (c) no scene: what the plain overload prints
        c = _runs(out, "c")
        assert len(c) == 8
        for ct in (0, 1):
            for m in (3, 64):
                plain, noscene = (c["c ct %d max_states %d %s" % (ct, m, which)] for which in ("plain", "noscene"))
                assert len(plain) == 7 and plain == noscene, (margin, ct, m)
        assert c["c ct 0 max_states 3 plain"] == c["c ct 0 max_states 64 plain"]
        # (d) a small batch with room for every list is ONE library call (counted by the resident service), although some of its edges
        # are longer than the 16 states a large batch's first pass lists
        d = [ln.split() for ln in out if ln.startswith("d served ")]
        assert len(d) == 1 and d[0][2] == "1" and int(d[0][4]) > 0 and d[0][6] == "0", d
        cond = out[-1].split()
        assert cond[0] == "conditions" and cond[1::2] == ["continued", "blocked", "cut", "over16"], out[-1]
        print("margin %g: %s" % (margin, out[-1]))
        conditions += np.array([int(v) for v in cond[2::2]])
    # the comparisons were not empty: over the two margins an edge of (a) was continued, one was blocked by the proxies, one was cut
    # by the checker, and an edge of (b) went on past the first pass's 16 states
    assert (conditions > 0).all(), conditions

"""The resident service for analytic mode, as far as a machine without a GPU can check it: the read-only option "resident_served",
the build's account of the new service kernel (resident_row16_kernel, both instantiations, no scratch), and the mailbox protocol
of the several-edge request — packed with the code the library's host side uses and judged by the rule the kernel applies
(csrc/ccmp_resident_proto.h; tests/cpp/resident_proto_check.cpp)."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc")


def test_resident_served_reads_zero_without_a_context(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    assert _lib.get_option(None, "resident_served") == 0
    assert "resident_served" not in {o["name"] for o in _lib.option_table()}  # read-only: not a knob


def test_analytic_service_kernel_has_no_scratch(ccmp_built):
    from closed_chain_motion_planner_amd.build import _SCRATCH_RULES, resource_report

    rep = resource_report()["ccmp_kernels_fast.hip"]
    inst = [k for k in rep if re.search(r"\bresident_row16_kernel<(true|false)>", k["name"])]
    assert sorted(k["name"] for k in inst) == ["resident_row16_kernel<false>", "resident_row16_kernel<true>"], sorted(k["name"] for k in rep)
    for k in inst:
        assert k["scratch"] == 0 and k["scratch_bound"] == 0 and k.get("vgpr_spill", 0) == 0, k
        assert k["lds"] <= 65536, k
        # the rule that binds it is its own (first match wins), not the catch-all's 64 B
        assert next(b for rx, b in _SCRATCH_RULES if re.search(rx, k["name"])) == 0


@pytest.fixture(scope="module")
def proto_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_proto") / "resident_proto_check")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "resident_proto_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_several_edge_requests_are_accepted_whole_and_refused_torn(proto_check):
    r = subprocess.run([proto_check], capture_output=True, text=True, timeout=120)
    n = json.loads(r.stdout.strip().splitlines()[-1])
    print(n)
    assert n["failures"] == 0
    assert n["accepted"] == 6  # E = 1, 5, 8, each with and without carry_in
    assert n["words_back"] == 2 * (3 * 7 + 30 * (1 + 5 + 8))
    assert n["stale_cases"] > 0 and n["stale_refused"] == n["stale_cases"]
    assert n["flip_cases"] > 0 and n["flip_refused"] == n["flip_cases"]
    assert r.returncode == 0

"""ccmp::ProxyScene::ikValid, the vetted ccmp::Projector::sampleCalibGoal and the vetted ccmp::Roadmap::grow
(include/ccmp_ompl_adapter.hpp, against the interface mock in tests/cpp/mock_ompl): the adapter's verbs give the bits of the rule's host
forms (ccmp_arm_clearance_ref, ccmp_pose_ik_vetted_ref) and advance the restarts' stream by one index per call; a failing call answers
false, fills NaN and keeps the first error until clearError(); nothing throws."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_ik_vet_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_ik_vet_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_vetted_path_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_adapter_agrees_with_the_host_forms(ccmp_built):
    exe = _build(ccmp_built)
    out = subprocess.run([exe, config_path("Wine_Bottle")], check=True, capture_output=True, text=True).stdout.splitlines()
    valids = [ln for ln in out if ln.startswith("valid t=")]
    goals = [ln for ln in out if ln.startswith("goal t=")]
    grows = [ln for ln in out if ln.startswith("grow t=")]
    assert len(valids) == 16 and len(goals) == 8 and len(grows) == 3
    assert all(ln.endswith("agree=1") for ln in valids + goals + grows), out
    assert grows[2].startswith("grow t=2 ok=0 which=-1 reached=0 ")  # the pose 10 m away: no state, empty slots
    m = re.match(r"summary solved (\d+) free (\d+) refused (\d+) (.*)$", out[-1])
    assert m, out[-1]
    # agreement is what is checked here; some target must have a state and some arm must be free for it to mean something
    assert int(m.group(1)) >= 1 and int(m.group(2)) >= 1, out[-1]
    # no mismatch, no error before the deliberate failures; those return false (00000), fill NaN (1111), leave CCMP_EINVAL (-1), keep it, clear
    assert m.group(4) == "mismatches 0 before 0 failed 00000 nan 1111 sticky -1 -1 kept 11 cleared 0 0 roadmap -1 cleared 0", out[-1]

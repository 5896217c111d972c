"""ccmp::Projector::sampleCalibGoal and ccmp::Roadmap::grow (include/ccmp_ompl_adapter.hpp, against the interface mock in
tests/cpp/mock_ompl): the adapter's verbs give the bits of the C calls they stand on and advance the restarts' stream by one index per
call; a pose out of reach answers false with NaN joints and no error; a failing call answers false, fills NaN and keeps the first
error until clearError(); nothing throws."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_ik_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_ik_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_ik_path_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_adapter_agrees_with_the_c_calls(ccmp_built):
    exe = _build(ccmp_built)
    out = subprocess.run([exe, config_path("Wine_Bottle")], check=True, capture_output=True, text=True).stdout.splitlines()
    goals = [ln for ln in out if ln.startswith("goal t=")]
    grows = [ln for ln in out if ln.startswith("grow t=")]
    assert len(goals) == 8 and len(grows) == 3
    assert all(ln.endswith("agree=1") for ln in goals + grows), out
    assert "goal own-state ok=1 same=1" in out and "goal unreachable ok=0 nan=1 error=0" in out
    assert grows[2].startswith("grow t=2 ok=0 which=-1 reached=0 ")  # the pose 10 m away: no state, empty slots
    m = re.match(r"summary solved (\d+) (.*)$", out[-1])
    assert m and int(m.group(1)) >= 2, out[-1]  # agreement is what is checked here; some target must have a state for it to mean something
    # no mismatch, no error before the deliberate failures; those return false (000), fill NaN (111), leave CCMP_EINVAL (-1), keep it, clear
    assert m.group(2) == "mismatches 0 before 0 failed 000 nan 111 sticky -1 kept 1 cleared 0 roadmap -1 cleared 0", out[-1]

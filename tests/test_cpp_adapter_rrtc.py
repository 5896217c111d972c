"""ccmp::RRTConnectOptions / ccmp::RRTConnectPlanner / ccmp::Roadmap::solveRRTConnect (include/ccmp_ompl_adapter.hpp, against the
interface mock in tests/cpp/mock_ompl): the planner's verbs compile as C++14 with the flags of the other adapter tests; a planner that
could not be opened answers "no" to every verb, throws nothing and keeps the library's first error until clearError()."""
import os
import subprocess

from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_rrtc_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_rrtc_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_every_verb_answers_no_with_a_sticky_error_without_a_planner(ccmp_built):
    import torch

    exe = _build(ccmp_built)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    code = -1 if torch.cuda.is_available() else -5  # a NULL store: CCMP_EINVAL with a device, CCMP_ENODEV without one
    assert out[0] == "defaults width 32 max_states 64 round_budget 0 range 0.1 max_vertices 2147483647", out
    assert out[1] == "none create 0 run 0 state 0 solved 0 status -1 first %d message 1" % code, out
    assert out[2] == "none kept 1", out
    assert out[3] == "none cleared 0 then -1", out  # after clearError the next verb records its own refusal: there is no planner
    assert out[4] == "solve 1", out

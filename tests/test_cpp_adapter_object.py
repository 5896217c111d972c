"""ccmp::ObjectChecker (include/ccmp_ompl_adapter.hpp, against the interface mock in tests/cpp/mock_ompl): stefanFCL's questions compile on
an Eigen::Isometry3d, an SE3 state pointer and (pos, quat); a checker that could not be created answers "no" to every one, throws
nothing and keeps its first error until clearError(); on a device its answers are those of the *_ref calls."""
import os
import re
import subprocess

import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_object_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_object_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_every_question_answers_no_with_a_sticky_error_without_a_checker(ccmp_built):
    import torch

    exe = _build(ccmp_built)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    code = -1 if torch.cuda.is_available() else -5  # a NULL context: CCMP_EINVAL with a device, CCMP_ENODEV without one
    assert out[0] == "none answers 00000 ladder 0 which -1 nan 1 rows 72 triangles 0 first %d kept 1 message 1" % code, out
    assert out[1] == "none cleared 0 then -1", out  # after clearError the next question records its own refusal: there is no object
    assert out[2] == "bad first -1 answers 0", out


@pytest.mark.gpu
def test_adapter_agrees_with_the_ref_calls(ccmp_built):
    exe = _build(ccmp_built)
    out = subprocess.run([exe, config_path("Wine_Bottle")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert "device free 111 table 00 triangles 12" in out, out
    props = [ln for ln in out if ln.startswith("propose n=")]
    assert len(props) == 12 and all(ln.endswith("agree=1") for ln in props), out
    assert any(re.match(r"ladder (\d) ref \1 next 112$", ln) and 0 < int(ln.split()[1]) < 9 for ln in out), out
    m = re.match(r"summary found (\d+) mismatches 0 failed 0 nan 1 sticky -1$", out[-1])
    assert m and 0 < int(m.group(1)), out[-1]

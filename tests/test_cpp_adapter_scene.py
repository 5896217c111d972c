"""The extend step with the proxy pre-filter on the device through the C++ adapter (include/ccmp_ompl_adapter.hpp, part 2, against the
interface mock in tests/cpp/mock_ompl): with a PrefilteredValidityChecker installed, jy_ProjectedStateSpace runs the proxies inside the
traversal; the lists, bools and the exact checker's questions must be those of the host path (the same checker behind a wrapper)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, config_path

EXE = os.path.join(ROOT, "tests", "cpp", "adapter_scene_check")


def _build(ccmp_built):
    libdir = os.path.dirname(ccmp_built)
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "cpp", "mock_ompl"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "adapter_scene_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_scene_path_compiles_as_cxx14(ccmp_built):
    assert os.path.exists(_build(ccmp_built))


@pytest.mark.gpu
def test_device_prefilter_equals_host_path(ccmp_built, oracle_det):
    from closed_chain_motion_planner_amd import load_config

    exe = _build(ccmp_built)
    P = oracle_det.checker_problem(config_path("Wine_Bottle"), load_config(config_path("Wine_Bottle")))
    start = np.array(P.start_joint[:])
    rejected = exact_refusals = 0
    for margin in (0.02, 0.12):
        out = subprocess.run([exe, "%.17g" % margin] + ["%.17g" % v for v in start], check=True, capture_output=True, text=True).stdout.splitlines()
        dev = [ln.split(" ", 1)[1] for ln in out if ln.startswith("device ")]
        host = [ln.split(" ", 1)[1] for ln in out if ln.startswith("host ")]
        assert len(dev) == len(host) > 100
        # every list, bool and checkMotion answer
        assert dev[:-1] == host[:-1]
        cd, ch = dev[-1].split(), host[-1].split()
        # counters: the exact checker was asked about the same states in the same order (count and hash of its questions)
        assert cd[:3] == ch[:3] and cd[6:] == ch[6:], (dev[-1], host[-1])
        # proxy refusals: the device path counts one per edge that ended at a refused state (the reference's order: the proxies
        # run before the step test); the host path sees the refused state only when the unfiltered traversal listed it
        assert int(cd[4]) >= int(ch[4]), (dev[-1], host[-1])
        rejected += int(cd[4])
        exact_refusals += sum(1 for ln in dev if " ok 0" in ln)
    assert rejected > 0 and exact_refusals > 0

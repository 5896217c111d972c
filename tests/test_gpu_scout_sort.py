"""The scouts' counting sort and the cut of its order: the cases of tests/scout_sort_cases.py, run ONCE in a process of their own against
lib/libccmp_debug.so, which exports the probes that feed the sort synthetic keys and the read-back of a call's order
(ccmp_debug_sort_probe, ccmp_debug_split_probe, ccmp_ctx_debug_lpt_order; the default library, which every other test loads, does not)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scout_sort_cases_pass_on_the_debug_library(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    assert os.path.exists(_lib.DEBUG_LIBPATH), "lib/libccmp_debug.so is built beside lib/libccmp.so (closed_chain_motion_planner_amd/build.py)"
    env = dict(os.environ, CCMP_LIBRARY=_lib.DEBUG_LIBPATH)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "scout_sort_cases.py"), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-500:]

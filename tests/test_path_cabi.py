"""The C ABI of the shortest paths on the roadmap graph (include/ccmp.h: ccmp_roadmap_shortest_paths, its _host form,
ccmp_graph_shortest_paths_ref, ccmp_roadmap_path_rounds_host): declarations and exports, the documented answers to a NULL store, and the
argument checks of the _ref form.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_roadmap_shortest_paths", "ccmp_roadmap_shortest_paths_host", "ccmp_graph_shortest_paths_ref", "ccmp_roadmap_path_rounds_host"]


@pytest.fixture(scope="module")
def L(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    return _lib.lib()


def test_header_declares_and_the_library_exports(L):
    import closed_chain_motion_planner_amd as pkg
    from closed_chain_motion_planner_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ccmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert "#define CCMP_PATH_MAX_PAIRS 64" in code and _lib.PATH_MAX_PAIRS == 64
    assert L.ccmp_version() == 600
    assert "capturable once the workspace holds" in hdr  # the header says when the call may be captured
    assert "stays with the caller's graph" not in hdr    # the path search is no longer left to the caller
    assert callable(pkg.shortest_paths_ref) and all(hasattr(pkg.Roadmap, m) for m in ("shortest_paths", "solution", "approximate_solution"))


def test_a_null_store_answers_the_documented_codes(L):
    """no quiet host path behind the device and host forms: without a device (no store can exist) they say CCMP_ENODEV; with one a
    NULL store is CCMP_EINVAL — before any other check, F == 0 included"""
    import torch

    want = EINVAL if torch.cuda.is_available() else ENODEV
    i32 = (C.c_int32 * 64)()
    d = (C.c_double * 64)()
    assert L.ccmp_roadmap_shortest_paths(None, None, None, 1, 8, None, None, None, None, None, None, None, None) == want
    assert L.ccmp_roadmap_shortest_paths(None, None, None, 0, 8, None, None, None, None, None, None, None, None) == want
    assert L.ccmp_roadmap_shortest_paths_host(None, i32, i32, 1, 8, d, i32, i32, None, None, None, None) == want
    assert L.ccmp_roadmap_shortest_paths_host(None, i32, i32, 65, 0, d, i32, i32, None, None, None, None) == want
    assert L.ccmp_roadmap_path_rounds_host(None, 1, i32) == want


def test_the_ref_form_checks_its_arguments(L):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    N = 5
    uv = np.array([[0, 1], [1, 2], [3, 2]], np.int32)
    w = np.array([1.0, 2.0, 4.0])
    src, dst = np.zeros(70, np.int32), np.full(70, 3, np.int32)
    cost, plen, path = np.full(70, -1.0), np.full(70, -1, np.int32), np.full((70, 8), -1, np.int32)
    dist, pred = np.zeros((70, N)), np.zeros((70, N), np.int32)

    def call(uv=uv, w=w, E=3, N=N, src=src, dst=dst, F=1, ml=8, cost=cost, plen=plen, path=path, dist=dist, pred=pred):
        return L.ccmp_graph_shortest_paths_ref(p(uv, ip), p(w, dp), E, N, p(src, ip), p(dst, ip), F, ml, p(cost, dp), p(plen, ip), p(path, ip), p(dist, dp), p(pred, ip))

    assert call() == 0 and cost[0] == 7.0 and plen[0] == 4 and path[0, :4].tolist() == [0, 1, 2, 3] and pred[0].tolist() == [-1, 0, 1, 2, -1]
    assert call(dist=None, pred=None) == 0           # the optional outputs
    assert call(F=64) == 0 and call(F=65) == EINVAL  # CCMP_PATH_MAX_PAIRS
    assert call(ml=0) == EINVAL and call(ml=-3) == EINVAL and call(ml=1) == 0
    for name in ("src", "dst", "cost", "plen", "path", "uv", "w"):
        assert call(**{name: None}) == EINVAL, name
    assert call(E=0, uv=None, w=None) == 0 and np.isinf(cost[0]) and plen[0] == 0  # no edges: nothing is reached
    for bad in (np.array([N], np.int32), np.array([-1], np.int32)):
        assert call(src=bad) == EINVAL and call(dst=bad) == EINVAL  # a pair's vertex is a vertex
    assert call(uv=np.array([[0, 1], [2, 2], [3, 2]], np.int32)) == EINVAL  # u == v, as add_edges_host
    assert call(uv=np.array([[0, 1], [1, N], [3, 2]], np.int32)) == EINVAL and call(uv=np.array([[0, 1], [-1, 2], [3, 2]], np.int32)) == EINVAL
    # F == 0 returns CCMP_OK and touches nothing, whatever else is wrong
    cost[:], plen[:] = -2.0, -2
    assert call(F=0, src=None, dst=None, ml=0, uv=None, path=None) == 0 and (cost == -2.0).all() and (plen == -2).all()
    assert call(N=0, E=0, uv=None, w=None) == EINVAL  # no vertex: no pair


def test_the_path_search_is_no_longer_left_to_the_caller():
    """README, DESIGN, INTEGRATION and the header once said that the path search stays with the caller's graph library"""
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "ccmp.h")):
        text = open(os.path.join(ROOT, name)).read()
        assert "stays with the caller's graph" not in text and "(A*) stays on the host" not in text, name
    assert "5.13" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "roadmap_path.md"))

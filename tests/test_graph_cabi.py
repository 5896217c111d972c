"""The C ABI of the roadmap graph (include/ccmp.h: ccmp_roadmap_commit / _add_edges / _closest / reads, ccmp_graph_labels_ref,
ccmp_joint_distance): declarations and exports, CCMP_ENODEV from every device and host form on a machine without a device, and the
argument checks of the *_ref forms.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import config_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_joint_distance", "ccmp_graph_labels_ref", "ccmp_roadmap_commit", "ccmp_roadmap_commit_host", "ccmp_roadmap_commit_ref", "ccmp_roadmap_add_edges",
         "ccmp_roadmap_add_edges_host", "ccmp_roadmap_num_edges", "ccmp_roadmap_read_edges", "ccmp_roadmap_read_edges_host", "ccmp_roadmap_read_labels",
         "ccmp_roadmap_read_labels_host", "ccmp_roadmap_closest", "ccmp_roadmap_closest_host", "ccmp_roadmap_closest_ref"]


@pytest.fixture(scope="module")
def L(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    return _lib.lib()


def test_header_declares_and_the_library_exports(L):
    from closed_chain_motion_planner_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ccmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for text in ("#define CCMP_GRAPH_MAX_ROOTS 32", "#define CCMP_CLOSEST_MAX_FROM 64", "CCMP_GROW_TRAPPED = 0", "CCMP_GROW_SREACHED = 1", "CCMP_GROW_GREACHED = 2",
                 "CCMP_GROW_UNSETTLED = 3", "CCMP_COMMIT_KEEP_ISOLATED = 1"):
        assert text in code, text
    assert (_lib.GROW_TRAPPED, _lib.GROW_SREACHED, _lib.GROW_GREACHED, _lib.GROW_UNSETTLED, _lib.COMMIT_KEEP_ISOLATED) == (0, 1, 2, 3, 1)
    assert L.ccmp_version() == 600
    assert "SYNCHRONOUS AT ITS END AND NOT CAPTURABLE" in hdr  # the header says what commit's read-back means


def test_device_and_host_forms_answer_enodev_here(L):
    """no quiet host path behind the device entry points: without a device (no store can exist) they say CCMP_ENODEV; with one a NULL
    store is CCMP_EINVAL"""
    import torch

    want = EINVAL if torch.cuda.is_available() else ENODEV
    n = C.c_size_t()
    i32 = (C.c_int32 * 32)()
    u8 = (C.c_uint8 * 8)()
    d = (C.c_double * 64)()
    assert L.ccmp_roadmap_commit(None, None, i32, u8, i32, None, 4, d, d, None, 1, 5, None, None, 0, 0, i32, i32, i32, C.byref(n), C.byref(n), None) == want
    assert L.ccmp_roadmap_commit_host(None, None, i32, u8, i32, None, 4, d, d, None, 1, 5, None, None, 0, 0, i32, i32, i32, C.byref(n), C.byref(n)) == want
    assert L.ccmp_roadmap_add_edges(None, i32, 1, C.byref(n), None) == want
    assert L.ccmp_roadmap_add_edges_host(None, i32, 1) == want
    assert L.ccmp_roadmap_read_edges(None, 0, 0, None, None, None) == want
    assert L.ccmp_roadmap_read_edges_host(None, 0, 0, i32, d) == want
    assert L.ccmp_roadmap_read_labels(None, 0, 0, None, None) == want
    assert L.ccmp_roadmap_read_labels_host(None, 0, 0, i32) == want
    assert L.ccmp_roadmap_closest(None, None, 1, None, None, None, None, None) == want
    assert L.ccmp_roadmap_closest_host(None, i32, 1, d, i32, d, d) == want
    assert L.ccmp_roadmap_num_edges(None) == 0


def test_ref_forms_refuse_bad_arguments(L):
    from closed_chain_motion_planner_amd import load_config

    P = load_config(config_path("Wine_Bottle"))
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    N, Q, k, ms = 6, 2, 3, 4
    sj, sp, lab = np.zeros((N, 14)), np.zeros((N, 8)), np.arange(N, dtype=np.int32)
    nbr, ok, ns = np.zeros((Q, k), np.int32), np.zeros(Q * k, np.uint8), np.zeros(Q * k, np.int32)
    st, nj, npo = np.zeros((Q * k, ms, 14)), np.zeros((Q, 14)), np.zeros((Q, 8))
    goal = np.zeros(8)
    roots = np.zeros(40, np.int32)
    ni, mi, gs = np.zeros(Q, np.int32), np.zeros(Q * k, np.int32), np.zeros(Q, np.int32)
    rj, rp, euv, ew = np.zeros((Q * (1 + k), 14)), np.zeros((Q * (1 + k), 8)), np.zeros((Q * k, 2), np.int32), np.zeros(Q * k)
    nv, ne = C.c_size_t(), C.c_size_t()
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None

    def call(problem=P, sj=sj, lab=lab, nbr=nbr, ok=ok, ns=ns, st=st, ms=ms, nj=nj, npo=npo, Q=Q, k=k, goal=goal, roots=roots, n_roots=1, flags=0, ni=ni, rj=rj):
        return L.ccmp_roadmap_commit_ref(C.byref(problem) if problem is not None else None, p(sj, dp), p(sp, dp), p(lab, ip), N, p(nbr, ip), p(ok, up), p(ns, ip),
                                         p(st, dp), ms, p(nj, dp), p(npo, dp), None, Q, k, p(goal, dp), p(roots, ip), n_roots, flags, p(ni, ip), p(mi, ip), p(gs, ip),
                                         p(rj, dp), p(rp, dp), p(euv, ip), p(ew, dp), C.byref(nv), C.byref(ne))

    assert call() == 0
    assert call(n_roots=33) == EINVAL and call(n_roots=32, roots=np.zeros(32, np.int32)) == 0 and call(n_roots=-1) == EINVAL
    assert call(k=0) == EINVAL and call(k=17) == EINVAL
    for name in ("sj", "lab", "nbr", "ok", "ns", "nj", "npo", "ni", "rj"):
        assert call(**{name: None}) == EINVAL, name
    assert call(n_roots=1, roots=None) == EINVAL
    assert call(roots=np.array([N], np.int32)) == EINVAL and call(roots=np.array([-1], np.int32)) == EINVAL  # a root is a vertex
    assert call(flags=2) == EINVAL and call(ms=0) == EINVAL
    assert call(problem=None) == EINVAL          # mid-stones need the problem ...
    assert call(problem=None, goal=None) == 0    # ... a call without a goal or without lists does not
    assert call(problem=None, st=None) == 0
    assert call(Q=0, nbr=None, ok=None, ns=None, nj=None, npo=None, ni=None, rj=None) == 0  # zero counts touch nothing

    labels = np.zeros(4, np.int32)
    uv = np.array([[0, 1], [3, 2]], np.int32)
    assert L.ccmp_graph_labels_ref(p(uv, ip), 2, 4, p(labels, ip)) == 0 and labels.tolist() == [0, 0, 2, 2]
    assert L.ccmp_graph_labels_ref(p(np.array([[0, 1], [2, 2]], np.int32), ip), 2, 4, p(labels, ip)) == EINVAL  # u == v
    assert L.ccmp_graph_labels_ref(p(np.array([[0, 4]], np.int32), ip), 1, 4, p(labels, ip)) == EINVAL
    assert L.ccmp_graph_labels_ref(p(np.array([[-1, 0]], np.int32), ip), 1, 4, p(labels, ip)) == EINVAL
    assert L.ccmp_graph_labels_ref(None, 1, 4, p(labels, ip)) == EINVAL and L.ccmp_graph_labels_ref(p(uv, ip), 1, 4, None) == EINVAL
    assert L.ccmp_graph_labels_ref(None, 0, 0, None) == 0

    fr, idx, dist, fd = np.zeros(70, np.int32), np.zeros(70, np.int32), np.zeros(70), np.zeros(70)
    cl = lambda F=1, poses=sp, labels=lab, fr=fr, tgt=goal, idx=idx: L.ccmp_roadmap_closest_ref(p(poses, dp), p(labels, ip), N, p(fr, ip), F, p(tgt, dp), p(idx, ip),
                                                                                                  p(dist, dp), p(fd, dp))
    assert cl() == 0 and cl(F=64) == 0 and cl(F=65) == EINVAL and cl(F=0, poses=None) == 0
    for name in ("poses", "labels", "fr", "tgt", "idx"):
        assert cl(**{name: None}) == EINVAL, name
    assert cl(fr=np.array([N], np.int32)) == EINVAL and cl(fr=np.array([-1], np.int32)) == EINVAL


def test_u_equals_v_and_out_of_range_edges_are_refused_on_the_host(L):
    """ccmp_roadmap_add_edges_host checks its edges before it touches a device; without a store that check cannot be reached here, so this
    pins the order of the answers: the store comes first"""
    import torch

    uv = (C.c_int32 * 2)(3, 3)
    assert L.ccmp_roadmap_add_edges_host(None, uv, 1) == (EINVAL if torch.cuda.is_available() else ENODEV)

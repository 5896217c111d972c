"""The extend step in analytic mode, host side (no GPU): the policy's description of the call and the build's register record of
its kernel (geodesic_row16_kernel, ccmp_kernels_fast.hip) and of the projector whose Newton round it shares."""
import re


def test_describe_names_the_analytic_extend_kernel(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    assert _lib.CALL_GEODESIC_ANALYTIC == 5
    for E, waves in ((1, 1), (5, 2), (700, 175), (16384, 2048), (65536, 2048)):  # ceil(E / 4), at most 8 per CU of the assumed 256
        line = _lib.describe(None, _lib.CALL_GEODESIC_ANALYTIC, E)
        assert "geodesic_row16_kernel" in line and "E=%d" % E in line, line
        assert "x %d wavefronts" % waves in line and "four edges per wavefront, ticket queue" in line, line
    # the existing kinds are unchanged
    assert "geodesic_row16_kernel" not in _lib.describe(None, _lib.CALL_GEODESIC, 16384)


def test_analytic_extend_kernel_has_no_scratch(ccmp_built):
    from closed_chain_motion_planner_amd.build import resource_report

    rep = resource_report()["ccmp_kernels_fast.hip"]
    names = {k["name"]: k for k in rep}
    for kernel in ("geodesic_row16_kernel", "project_row16_kernel"):
        inst = [k for n, k in names.items() if re.search(r"\b%s<(true|false)>" % kernel, n)]
        assert len(inst) == 2, (kernel, sorted(names))
        for k in inst:
            assert k["scratch"] == 0 and k["agprs"] == 0 and k["occupancy"] >= 2, k
    assert not [n for n in names if n.startswith("geo_an_")]  # the step loop's kernels are gone

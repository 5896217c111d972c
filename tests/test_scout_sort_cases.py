"""The integer model and the case builders of tests/scout_sort_cases.py, proven without a GPU: the model against a sort written out
the slow way, and every case against what it is named for (`heavy` both ways, the equalities hit, `limit` binding, the stale-bin pair
differing above bin 64)."""
import numpy as np
import pytest

import scout_sort_cases as ss


def _slow_ge(pred):
    keys = [min(int(v), 1023) for v in pred]
    return [sum(1 for v in keys if v >= k) for k in range(1024)]


def test_model_against_the_definitions_written_out():
    pred = np.array([0, 3, 3, 1023, 1024, 65535, 7, 0, 96], dtype=np.uint16)
    ge = ss.ge_of(pred)
    assert ge == _slow_ge(pred) and ge[0] == 9 and ge[1023] == 3 and ge[8] == 4 and all(isinstance(v, int) for v in ge)
    # a valid order: any permutation with non-increasing clamped keys; ties in any order, the three clamped keys too
    assert ss.order_defects([5, 3, 4, 8, 6, 1, 2, 7, 0], pred) == "" and ss.order_defects([3, 4, 5, 8, 6, 2, 1, 0, 7], pred) == ""
    assert "rise" in ss.order_defects([3, 4, 5, 8, 6, 1, 2, 0, 7][::-1], pred)
    assert "permutation" in ss.order_defects([3, 4, 5, 8, 6, 1, 1, 0, 7], pred)
    assert "range" in ss.order_defects([3, 4, 5, 8, 6, 1, 2, 0, 9], pred) and "range" in ss.order_defects(np.array([0xFFFFFFFF] * 9, dtype=np.uint32), pred)
    assert "shape" in ss.order_defects([0, 1], pred)
    assert ss.order_defects([], np.zeros(0, dtype=np.uint16)) == ""
    # the cuts, by hand: keys >= 3 are seven, keys >= 4 five, keys >= 8 four
    assert ss.front_kind1(ge, 3, 9) == 7 and ss.front_kind1(ge, 3, 4) == 4 and ss.front_kind1(ge, 4000, 9) == 3 and ss.front_kind1(ge, 3, 0) == 0
    total = 3 + 3 + 3 * 1023 + 7 + 96
    assert sum(ge[1:]) == total
    assert ss.kind2_sides(ge, 96, 10) == ((96 * 4 + 3 * (1023 - 96)) * 1000, total * 10)
    assert ss.front_kind2(ge, 3, 96, 10) == 4 and ss.front_kind2(ge, 3, 96, 999) == 7 and ss.front_kind2(ge, 4, 5000, 1000) == 5
    assert ss.geo_cut(ge, 2, 96, 10) == 96 and ss.geo_cut(ge, 2, 5000, 900) == 1023
    assert ss.geo_cut(ge, 2, 96, 1000) == 3 and ss.geo_cut(ge, 4, 96, 1000) == 4  # all of the work: every key >= 3; no P above p_min = 4
    assert ss.front_geo(ge, 2, 96, 1000) == ge[3] == 7 and ss.front_geo(ge, 4, 96, 1000) == ge[4] == 5
    # the queue block
    fill = ss.QUEUE_FILL
    assert len(set(fill)) == 16 and min(fill) > 2 ** 40
    assert ss.queue_after(fill, 5, 0) == [5, fill[1], fill[2], 5, 5] + fill[5:]
    assert ss.queue_after(fill, 5, 3) == [5, 0, 0, 5, 5] + fill[5:]
    assert ss.queue_after(fill, 5, 8) == [5, 0, 0, 5, 5, 0, 0, 0] + fill[8:]
    assert ss.queue_after(fill, 5, None) == ss.queue_after(fill, 5, 0)


def test_sizes_and_bin_counts_are_the_ones_that_change_a_path():
    assert max(ss.FUSED_SIZES) == ss.FUSED_MAX and min(ss.THREE_SIZES) == ss.FUSED_MAX + 1
    assert {1, 2, 63, 64, 1023, 1024, 1025, 16383} <= set(ss.FUSED_SIZES)
    assert ss.THREE_SIZES[0] % 1024 == 1 and ss.THREE_SIZES[1] == 17 * 1024 and ss.THREE_SIZES[2] == 17 * 1024 + 1  # scatter blocks of 1 024 keys
    assert ss.THREE_SIZES[3] == 256 * 256 + 1 and ss.THREE_SIZES[4] > 256 * 256 and ss.THREE_SIZES[4] % 256  # the histogram grid's second stride
    assert ss.NBINS == [1, 2, 9, 63, 64, 65, 97, 128, 129, 1023, 1024]
    for nbins in (65, 129):  # idle lanes, and a lane whose run of `per` bins ends below bin 0
        per = -(-nbins // 64)
        runs = [[nbins - 1 - (lane * per + i) for i in range(per)] for lane in range(64)]
        assert any(r[0] < 0 for r in runs) and (nbins != 65 or any(r[0] >= 0 > r[-1] for r in runs))
    assert all(n > ss.FUSED_MAX for n in ss.NBINS_SIZES + [ss.STALE_N, ss.CUT_SIZES[1], ss.GEO_E, ss.SPLIT_SIZES[1]]) and ss.CUT_SIZES[0] <= ss.FUSED_MAX >= ss.SPLIT_SIZES[0]


@pytest.mark.parametrize("nbins", ss.NBINS)
def test_key_sets(nbins):
    n, top = 17409, nbins - 1
    ks = {kind: ss.make_keys(kind, n, nbins).astype(np.int64) for kind in ss.KEYSETS}
    assert all(k.shape == (n,) and k.min() >= 0 and k.max() <= top for k in ks.values())
    assert not ks["all_zero"].any() and (ks["all_top"] == top).all() and (ks["all_mid"] == top // 2).all()
    assert set(ks["uniform"]) == set(range(nbins))
    assert set(ks["two_point"]) == {0, top} and (nbins == 1 or 0.4 * n < (ks["two_point"] == top).sum() < 0.6 * n)
    assert ks["lone_top"].sum() == top and np.count_nonzero(ks["lone_top"]) == (top > 0)
    assert (np.diff(ks["ascending"]) >= 0).all() and (np.diff(ks["descending"]) <= 0).all()
    if nbins > 1:
        assert ks["ascending"][0] < ks["ascending"][-1] and ks["descending"][0] > ks["descending"][-1]
        assert ss.front_kind1(ss.ge_of(ks["lone_top"]), top, ss.NO_LIMIT) == 1
    g = ks["geometric"]
    assert g.max() == min(96, top) and (nbins < 64 or (np.median(g) < 16 and len(np.unique(g)) > 40))
    assert np.array_equal(ss.make_keys("uniform", n, nbins), ss.make_keys("uniform", n, nbins))  # seeded


def test_clamp_keys_reach_past_the_bins():
    for n in (4, 1025, 70001):
        k = ss.make_keys("clamp", n, 1024).astype(np.int64)
        assert {0, 1023, 1024, 65535} <= set(k) and (n < 100 or 0.4 * n < (k >= 1024).sum() < 0.6 * n)
        assert ss.ge_of(k)[1023] == (k >= 1023).sum()


def test_sweeps_cover_every_cut_shape():
    cases = [c for n in ss.FUSED_SIZES + ss.THREE_SIZES for c in ss.size_cases(n)] + [c for b in ss.NBINS for c in ss.nbins_cases(b)]
    assert len(cases) == 14 * 10 + 11 * 2 * 9
    for fused in (True, False):
        mine = [c for c in cases if (c["n"] <= ss.FUSED_MAX) == fused]
        assert {(c["split"]["kind"], c["split"]["clear"]) if c["split"] else None for c in mine} == {None, (1, 0), (2, 8), (1, 3), (2, 3), (1, 8), (2, 0)}
    heavy = set()
    for c in cases:
        s = c["split"]
        assert c["keys"] in ss.KEYSETS + ["clamp"] and (c["keys"] != "clamp" or c["nbins"] == 1024)
        assert c["hist_blocks"] == (256 if c["nbins"] == 1024 and c["name"].find("nbins=") < 0 else 64)
        if s:
            assert 0 <= s["p_low"] <= 1023 and s["p_high"] >= 0 and 0 <= s["permille"] <= 1000 and 0 <= s["clear"] <= 16
            if s["kind"] == 2:
                lhs, rhs = ss.kind2_sides(ss.ge_of(ss.make_keys(c["keys"], c["n"], c["nbins"])), s["p_high"], s["permille"])
                heavy.add(lhs >= rhs)
    assert heavy == {True, False}


def test_cut_key_multiset():
    for n in ss.CUT_SIZES:
        k = ss.cut_keys("M", n).astype(np.int64)
        ge = ss.ge_of(k)
        assert len(k) == n and k.sum() == 10000 == sum(ge[1:]) and np.count_nonzero(k) == 870
        work = lambda P: sum(int(v) for v in k if v >= P)
        assert [work(P) for P in (96, 65, 64, 41, 40, 21, 20, 10, 9, 8, 6, 5)] == [960, 960, 2240, 2240, 4240, 4240, 6240, 6240, 6600, 7000, 7000, 10000]
        assert all(ss.kind2_sides(ge, P, 1)[0] == 1000 * work(P) for P in (96, 64, 40, 9, 8, 1))
        assert (ge[8], ge[9], ge[20], ge[40], ge[41], ge[64], ge[65], ge[96], ge[97]) == (270, 220, 180, 80, 30, 30, 10, 10, 0)
        assert not np.array_equal(k, np.sort(k)) and not np.array_equal(k, np.sort(k)[::-1])
        kc, k64, kz = (ss.cut_keys(w, n).astype(np.int64) for w in ("Mc", "M64", "zero"))
        assert (kc == 3000).sum() == 7 and ss.ge_of(kc)[1023] == 7 and ss.ge_of(kc)[40] == 87 and ss.ge_of(kc)[97] == 7
        assert k64.max() == 64 and ss.ge_of(k64)[64] == 30 and ss.ge_of(k64)[65] == 0 and not kz.any()


@pytest.mark.parametrize("case", ss.KIND1_CASES, ids=lambda c: c["name"])
def test_kind1_cases_are_what_they_say(case):
    s = case["split"]
    for n in ss.CUT_SIZES:
        keys = ss.cut_keys(case["keys"], n).astype(np.int64)
        assert keys.max() < case["nbins"] or case["nbins"] == 1024
        ge = ss.ge_of(keys)
        count = ge[min(s["p_low"], 1023)]
        front = ss.front_kind1(ge, s["p_low"], s["limit"])
        assert front == (n if case["front"] is None else case["front"])
        name = case["name"]
        if "limit below" in name or "limit binds" in name:
            assert s["limit"] < count and front == s["limit"]
        if "limit equal" in name:
            assert s["limit"] == count
        if "limit above" in name or "no limit" in name:
            assert s["limit"] > count == front
        if "limit 0" in name:
            assert s["limit"] == 0 == front < count
        if "1024" in name or "5000" in name:
            assert s["p_low"] >= 1024 and count == ge[1023] > 0
        if "beyond the bins" in name:
            assert s["p_low"] >= case["nbins"] and count == 0
    # an off-by-one bin changes the kind 1 front wherever the limit does not hide it
    assert any(c["split"]["p_low"] < 1023 and ss.ge_of(ss.cut_keys(c["keys"], 2048))[c["split"]["p_low"] + 1] < c["front"] for c in ss.KIND1_CASES if c["front"])


@pytest.mark.parametrize("case", ss.KIND2_CASES, ids=lambda c: c["name"])
def test_kind2_cases_are_what_they_say(case):
    s = case["split"]
    for n in ss.CUT_SIZES:
        keys = ss.cut_keys(case["keys"], n).astype(np.int64)
        assert keys.max() < case["nbins"] or case["nbins"] == 1024
        ge = ss.ge_of(keys)
        lhs, rhs = ss.kind2_sides(ge, s["p_high"], s["permille"])
        assert (lhs >= rhs) == case["heavy"] and ss.front_kind2(ge, s["p_low"], s["p_high"], s["permille"]) == case["front"]
        assert ge[min(s["p_high"], 1023)] != ge[s["p_low"]] or not keys.any()  # the two answers differ: a wrong `heavy` shows
        name = case["name"]
        if "equal" in name:
            assert (lhs == rhs) == ("both sides" in name) and abs(lhs - rhs) <= sum(ge[1:])  # at, or one permille past
            P = s["p_high"]
            assert ((P * ge[P] + sum(ge[P:])) * 1000 >= rhs) and not (lhs >= (sum(ge[1:]) + ge[0]) * s["permille"])  # `above` from P on / `all` from bin 0 on flip it
        if ">= nbins" in name:
            assert s["p_high"] >= case["nbins"] and ge[s["p_high"]] == 0 and lhs == 0
        if "> 1023" in name:
            assert s["p_high"] > 1023 and ge[1023] > 0
        if "every key 0" in name:
            assert rhs == 0 == lhs and s["permille"] > 0
    both = {c["heavy"] for c in ss.KIND2_CASES}
    assert both == {True, False}


def test_equal_sides_flip_under_either_off_by_one():
    """the pair of cases around equality: `above` summed from p_high on makes the one past equal heavy, `all` summed from bin 0 on
    makes the equal one not heavy"""
    ge = ss.ge_of(ss.cut_keys("M", 2048))
    eq, past = (c["split"] for c in ss.KIND2_CASES if "equal" in c["name"])
    assert ss.kind2_sides(ge, 64, eq["permille"]) == (2240000, 2240000)
    lhs, rhs = ss.kind2_sides(ge, 64, past["permille"])
    assert lhs < rhs <= lhs + ge[64] * 1000
    assert 2240000 < (sum(ge[1:]) + ge[0]) * eq["permille"]


@pytest.mark.parametrize("case", ss.GEO_CASES, ids=lambda c: c["name"])
def test_geo_cases_are_what_they_say(case):
    ge = ss.ge_of(ss.cut_keys(case["keys"], 2048))
    p_min, p_max, pm = case["p_min"], case["p_max"], case["permille"]
    P = ss.geo_cut(ge, p_min, p_max, pm)
    assert P == case["P"] and ss.front_geo(ge, p_min, p_max, pm) == ge[P] == case["front"]
    side = lambda Q: (Q * ge[Q] + sum(ge[Q + 1:])) * 1000
    rhs = sum(ge[1:]) * pm
    top = min(p_max, 1023)
    assert all(side(Q) < rhs for Q in range(P + 1, top + 1)) and (P == p_min or side(P) >= rhs)
    name = case["name"]
    if "at p_max" in name:
        assert P == p_max
    if "between" in name:
        assert p_min + 1 < P < p_max
    if "within 1 %" in name:  # a front whose `above` stops growing falls short here
        assert side(P) - rhs < rhs // 100 and P * ge[P] * 1000 + sum(ge[p_max + 1:]) * 1000 < rhs
    if "both sides equal" in name:
        assert side(P) == rhs
    if "one permille past" in name:
        assert side(40) < rhs <= side(40) + sum(ge[1:])
    if "p_min + 1" in name:
        assert P == p_min + 1
    if "no P qualifies" in name:
        assert P == p_min and side(p_min + 1) < rhs and ge[p_min + 1] != ge[p_min]  # a loop that stops one bin early shows
    if "> 1023" in name:
        assert p_max > 1023 and (("last bin" in name) == (P == 1023))


def test_stale_pair_differs_above_bin_64():
    for n in (ss.STALE_N, ss.FUSED_MAX + 1):
        first, second = ss.stale_pair(n)
        a, b = ss.ge_of(first["keys"]), ss.ge_of(second["keys"])
        assert first["nbins"] == 1024 and second["nbins"] == 65 and len(first["keys"]) == len(second["keys"]) == n > ss.FUSED_MAX
        assert first["keys"].max() == 96 and second["keys"].max() == 64
        assert min(a[65:97]) > 0 and not any(b[65:])
        s = second["split"]
        assert s["kind"] == 2 and s["clear"] == 8
        # bins 65 .. 96 of the first sort would change the second's cut: `all` and `above` both read them
        stale = b[:65] + a[65:]
        assert ss.front_kind2(b, s["p_low"], s["p_high"], s["permille"]) == b[40] == 300 and ss.front_kind2(stale, s["p_low"], s["p_high"], s["permille"]) == b[64] == 100
        assert ss.front_geo(stale, 8, 64, s["permille"]) != ss.front_geo(b, 8, 64, s["permille"])


def test_queue_word_places_are_the_launch_header_s():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "closed_chain_motion_planner_amd", "csrc", "ccmp_launch.h")).read()
    assert re.search(r"kQFrontLen = 4,", text) and re.search(r"kBFrontLen = 4,", text) and re.search(r"kFastQueues = 64;", text)
    assert re.search(r"kQAnalytic = 8,", text) and "kQGeoAnalytic = kQAnalytic + kFastQueues + 2," in text and "kQBulk = kQGeoAnalytic + 1," in text
    assert "kQueueWords = kQBulk + 8," in text
    assert (ss.Q_FRONT_LEN, ss.B_FRONT_LEN, ss.Q_BULK, ss.QUEUE_WORDS) == (4, 4, 8 + 64 + 2 + 1, 8 + 64 + 2 + 1 + 8)

"""The scouts' descending counting sort and the cut of its order (closed_chain_motion_planner_amd/csrc/ccmp_kernels_scout.hip: hist_kernel,
scan_desc_kernel, scatter_kernel, sort_fused_kernel, apply_split, fd_split_kernel, geo_split_kernel) against an integer model.

Two halves.  The MODEL and the CASE BUILDERS need no device: plain Python ints and numpy, no text shared with the kernels;
tests/test_scout_sort_cases.py proves on them alone that every case holds what it is named for.  The gpu-marked tests below drive the
kernels through ccmp_debug_sort_probe / ccmp_debug_split_probe (synthetic keys: the shapes that break a counting sort are reached at a
few thousand keys, natural predictions only span 0 .. 96) and read the order of real calls back through ccmp_ctx_debug_lpt_order.  They
are NOT collected by the suite directly (the default library exports no such symbol): tests/test_gpu_scout_sort.py runs this file once,
in a process of its own, with CCMP_LIBRARY = lib/libccmp_debug.so.  Everything is integers: every comparison is exact.

The model.  key = min(pred, 1023); ge[k] = #{key >= k}, k < 1024 — what hist holds behind either form of the sort; a valid order is
ANY permutation of range(n) with key[order] non-increasing (ranks come from atomics: no stability, no order inside a bin); the cuts
are front_kind1 / front_kind2 / front_geo below; words 0, 3 and 4 of the queue block hold the front, the other words below `clear`
hold 0, every other word keeps what the caller put there.

Mutants.  Each was applied to a copy of ccmp_kernels_scout.hip and this file run against the debug library built from it; the
unmutated library passes all 89 tests.  Mutants 1 - 12 ran the probe tests only (an order that is no permutation, or a finished count
that starts wrong, must not reach the projector's persistent kernels), mutant 13 everything.  What failed:

   1  scan_desc_kernel: ascending bins (k = lane * per + i)          test_sizes (all 5 three-kernel sizes), test_bin_counts (all 11),
                                                                      test_cut_by_the_sort (20), test_bins_of_the_last_sort... (both)
   2  sort_fused_kernel: ascending bins (k = t)                      test_sizes (all 9 fused sizes), test_cut_by_the_sort (20),
                                                                      test_bins_of_the_last_sort... (both: its fused sort)
   3  scan_desc_kernel: `if (lane > off)` in the wave scan           test_sizes (5 three-kernel sizes), test_bin_counts (all but 1 bin),
                                                                      test_cut_by_the_sort (9), test_bins_of_the_last_sort... (both)
   4  sort_fused_kernel: the `above` loop skips wave 0's sum         test_sizes (all 9 fused sizes: all_top, two_point, uniform, clamp),
                                                                      test_cut_by_the_sort (the 5 cases with keys in bin 1023, at 2 048)
   5  scatter_kernel: stores i0, not i0 + k                          test_sizes (5 three-kernel sizes), test_bin_counts (all 11),
                                                                      test_cut_by_the_sort (20), test_bins_of_the_last_sort... (both)
   6  apply_split kind 1: `limit` ignored                            test_cut_by_the_sort (limit below the count, limit 0, limit binds; both
                                                                      sizes), test_sizes (13), test_bin_counts (all 11)
   7  apply_split kind 1: ge[p_low + 1]                              test_cut_by_the_sort (10), test_sizes (5), test_bin_counts (8)
   8  apply_split kind 2: `j >= p_high` for `above`                  test_cut_by_the_sort[one permille past equal] (both sizes),
                                                                      test_bins_of_the_last_sort... (both)
   9  apply_split kind 2: `all` summed from j >= 0                   test_cut_by_the_sort[both sides equal] (both sizes), [heavy-16385],
                                                                      [p_high at the last of 65 bins-16385], test_bin_counts[1], [2]
  10  apply_split: lane 3 not written                                67 of the 80 probe tests (every one with a cut)
  11  geo_split_kernel: `above += n[P]` dropped                      test_cut_by_geo_split_kernel (5, among them `within 1 % of the share`),
                                                                      test_sizes (12), test_bin_counts (9), test_bins_of_the_last_sort... (both)
  12  geo_split_kernel: loop bound `P > p_min + 1`                   test_cut_by_geo_split_kernel[no P qualifies], test_bin_counts[2]
  13  geodesic_scout_order clears nbins words, not 1 024             test_bulk_extend_call_behind_a_projector_call (all three cut forms)
  14  the clear's rule and the sort's form disagree at 16 385 keys   NOT RUN.  The fused kernel at 16 385 keys behind a clear is a correct sort
                                                                      (nothing to find); the three-kernel form WITHOUT the clear adds its
                                                                      counts to the last sort's and scatters from bases beyond n — stores
                                                                      outside `order`, which no mutant here may make.  Both decisions now
                                                                      stand side by side in one unit and test one constant (sort_needs_clear,
                                                                      sort_desc); the probe refuses an uncleared histogram
                                                                      (test_probe_refuses_what_would_leave_the_buffers), and 16 385 keys on a
                                                                      used histogram are test_bins_of_the_last_sort...[16385], the split
                                                                      launch's second size and the bulk extend call.
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BINS = 1024
FUSED_MAX = 16384  # up to here the sort is one launch (sort_fused_kernel)
FUSED_SIZES = [1, 2, 63, 64, 1023, 1024, 1025, 16383, 16384]
THREE_SIZES = [16385, 17408, 17409, 65537, 70001]  # last scatter block of 1 key; 17 scatter blocks exactly, and one key more; the 256-block histogram's second, ragged stride
NBINS = [1, 2, 9, 63, 64, 65, 97, 128, 129, 1023, 1024]  # ceil(nbins / 64) leaves idle lanes and a negative k at 65 and 129
NBINS_SIZES = [16385, 17409]
KEYSETS = ["all_zero", "all_top", "all_mid", "uniform", "two_point", "geometric", "lone_top", "ascending", "descending"]
QUEUE_WORDS, Q_FRONT_LEN, Q_BULK, B_FRONT_LEN = 83, 4, 75, 4  # ccmp_launch.h: kQueueWords, kQFrontLen, kQBulk, kBFrontLen
QUEUE_FILL = [0xA5A5000000000007 + 0x0101 * i for i in range(16)]  # what the caller's queue block holds: distinct, non-zero, none a plausible front
NO_LIMIT = 0xFFFFFFFF


# ---- the model --------------------------------------------------------------------------------------------------------------------
def clamp_keys(pred):
    return np.minimum(np.asarray(pred).astype(np.int64), BINS - 1)


def ge_of(pred):
    """ge[k] = number of keys >= k, as Python ints"""
    counts = np.bincount(clamp_keys(pred), minlength=BINS)
    return [int(v) for v in counts[::-1].cumsum()[::-1]]


def order_defects(order, pred):
    """why `order` is no descending permutation of the keys ('' = it is one)"""
    n = len(pred)
    order = np.asarray(order).astype(np.int64)
    if order.shape != (n,):
        return "shape %s" % (order.shape,)
    if n and (order.min() < 0 or order.max() >= n):
        return "index out of range: %s" % order[(order < 0) | (order >= n)][:4]
    if not np.array_equal(np.sort(order), np.arange(n)):
        return "not a permutation: %d distinct of %d" % (len(np.unique(order)), n)
    k = clamp_keys(pred)[order]
    up = np.flatnonzero(k[1:] > k[:-1])
    return "" if len(up) == 0 else "keys rise at place %d: %d -> %d" % (up[0], k[up[0]], k[up[0] + 1])


def front_kind1(ge, p_low, limit):
    """fd_split_kernel's rule and apply_split's kind 1"""
    return min(ge[min(p_low, BINS - 1)], limit)


def kind2_sides(ge, p_high, permille):
    P = min(p_high, BINS - 1)
    return (P * ge[P] + sum(ge[P + 1:])) * 1000, sum(ge[1:]) * permille


def front_kind2(ge, p_low, p_high, permille):
    lhs, rhs = kind2_sides(ge, p_high, permille)
    return ge[min(p_high, BINS - 1) if lhs >= rhs else p_low]


def geo_cut(ge, p_min, p_max, permille):
    """the P geo_split_kernel settles on"""
    total = sum(ge[1:])
    for P in range(min(p_max, BINS - 1), p_min, -1):
        if (P * ge[P] + sum(ge[P + 1:])) * 1000 >= total * permille:
            return P
    return p_min


def front_geo(ge, p_min, p_max, permille):
    return ge[geo_cut(ge, p_min, p_max, permille)]


def queue_after(fill, front, clear):
    """the queue block behind a cut: clear = None for the two stand-alone kernels (words 0, 3, 4 and nothing else)"""
    out = list(fill)
    for i in range(clear or 0):
        out[i] = 0
    for i in (0, 3, 4):
        out[i] = front
    return out


def front_of(ge, split):
    if split["kind"] == 1:
        return front_kind1(ge, split["p_low"], split["limit"])
    return front_kind2(ge, split["p_low"], split["p_high"], split["permille"])


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def make_keys(kind, n, nbins, seed=0):
    """n uint16 keys below nbins ('clamp': 1024 bins, half the values beyond them)"""
    rng = np.random.default_rng([seed, n, nbins, KEYSETS.index(kind) if kind in KEYSETS else 99])
    top = nbins - 1
    if kind == "all_zero":
        k = np.zeros(n, dtype=np.int64)
    elif kind == "all_top":
        k = np.full(n, top)
    elif kind == "all_mid":
        k = np.full(n, top // 2)
    elif kind in ("uniform", "ascending", "descending"):
        k = rng.integers(0, nbins, n)
        if n >= nbins:
            k[rng.permutation(n)[:nbins]] = np.arange(nbins)  # every bin at least once
        if kind != "uniform":
            k = np.sort(k)[::1 if kind == "ascending" else -1]
    elif kind == "two_point":
        k = rng.integers(0, 2, n) * top
        if n >= 2:
            k[:2] = (0, top)
    elif kind == "geometric":  # like real predictions: most short, a tail, the scout's cap of 96
        k = np.minimum(rng.geometric(0.06, n) - 1, min(96, top))
    elif kind == "lone_top":
        k = np.zeros(n, dtype=np.int64)
        k[n // 3] = top
    elif kind == "clamp":
        assert nbins == BINS
        k = np.where(rng.integers(0, 2, n) == 1, rng.integers(1024, 65536, n), rng.integers(0, 1024, n))
        if n >= 4:
            k[rng.permutation(n)[:4]] = (1023, 1024, 65535, 0)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(k).astype(np.uint16)


_SPLITS = [None, (1, 0), (2, 8), (1, 3), (2, 3), (1, 8), (2, 0)]  # (kind, clear): production clears 0 (projector) and 8 (bulk)


def sweep_split(i, n, nbins):
    """the cut request the i-th case of a sweep carries (None: no cut, the queue block must stay as it was)"""
    s = _SPLITS[i % len(_SPLITS)]
    if s is None:
        return None
    top = nbins - 1
    return dict(kind=s[0], clear=s[1], p_low=top // 4, p_high=top // 2 + (i % 3), permille=(50, 100, 400)[i % 3], limit=(n // 3, NO_LIMIT, 0)[(i // 7) % 3])


def size_cases(n):
    """1024 bins, the projector's 256 histogram blocks: every key set at n keys"""
    return [dict(name="%s n=%d" % (ks, n), n=n, nbins=BINS, hist_blocks=256, keys=ks, split=sweep_split(i + n, n, BINS)) for i, ks in enumerate(KEYSETS + ["clamp"])]


def nbins_cases(nbins):
    """the three-kernel form at nbins bins on the extend step's 64 histogram blocks, keys < nbins"""
    return [dict(name="%s nbins=%d n=%d" % (ks, nbins, n), n=n, nbins=nbins, hist_blocks=64, keys=ks, split=sweep_split(i + j + nbins, n, nbins))
            for j, n in enumerate(NBINS_SIZES) for i, ks in enumerate(KEYSETS)]


# The key multiset of the cut cases: value -> count, the rest zeros.  sum of the keys 10 000; the keys >= P carry
# 960 (64 < P <= 96), 2 240 (40 < P <= 64), 4 240 (20 < P <= 40), 6 240 (9 < P <= 20), 6 600 (P = 9), 7 000 (5 < P <= 8), 10 000 (P <= 5).
CUT_COUNTS = {5: 600, 8: 50, 9: 40, 20: 100, 40: 50, 64: 20, 96: 10}
CUT_SIZES = [2048, 16385]  # either form of the sort


def cut_keys(which, n):
    """'M': CUT_COUNTS; 'Mc': M and seven keys of 3000 (bin 1023); 'M64': M cut off at 64 (fits 65 bins); 'zero': all keys 0"""
    vals = [] if which == "zero" else [v for v, c in CUT_COUNTS.items() for _ in range(c)]
    if which == "Mc":
        vals += [3000] * 7
    k = np.zeros(n, dtype=np.int64)
    k[:len(vals)] = vals
    if which == "M64":
        k = np.minimum(k, 64)
    return np.random.default_rng(len(vals) + n).permutation(k).astype(np.uint16)


def _k1(name, keys, p_low, limit, front, nbins=BINS):
    return dict(name="kind 1: " + name, keys=keys, nbins=nbins, split=dict(kind=1, p_low=p_low, p_high=0, permille=0, limit=limit), front=front)


def _k2(name, keys, p_low, p_high, permille, heavy, front, nbins=BINS):
    return dict(name="kind 2: " + name, keys=keys, nbins=nbins, split=dict(kind=2, p_low=p_low, p_high=p_high, permille=permille, limit=0), heavy=heavy, front=front)


# `front` and `heavy` are what the case is NAMED for, written down by hand from CUT_COUNTS; tests/test_scout_sort_cases.py proves that
# the model gives them, the gpu tests compare the kernels with the model
KIND1_CASES = [
    _k1("limit below the count", "M", 40, 79, 79),
    _k1("limit equal to the count", "M", 40, 80, 80),
    _k1("limit above the count", "M", 40, 81, 80),
    _k1("no limit", "M", 40, NO_LIMIT, 80),
    _k1("limit 0", "M", 40, 0, 0),
    _k1("p_low 0", "M", 0, NO_LIMIT, None),  # every key
    _k1("p_low 1023", "Mc", 1023, NO_LIMIT, 7),
    _k1("p_low 1024", "Mc", 1024, NO_LIMIT, 7),
    _k1("p_low 5000, limit binds", "Mc", 5000, 3, 3),
    _k1("p_low beyond the bins of a 65-bin sort", "M64", 65, NO_LIMIT, 0, nbins=65),
]
KIND2_CASES = [
    _k2("heavy", "M", 40, 64, 100, True, 30),
    _k2("not heavy", "M", 40, 64, 300, False, 80),
    _k2("both sides equal", "M", 40, 64, 224, True, 30),
    _k2("one permille past equal", "M", 40, 64, 225, False, 80),
    _k2("p_high >= nbins: a ge of 0", "M64", 40, 80, 100, False, 80, nbins=65),
    _k2("p_high >= nbins, permille 0", "M64", 40, 80, 0, True, 0, nbins=65),
    _k2("p_high at the last of 65 bins", "M64", 40, 64, 100, True, 30, nbins=65),
    _k2("p_high > 1023, heavy", "Mc", 40, 2000, 100, True, 7),
    _k2("p_high > 1023, not heavy", "Mc", 40, 2000, 500, False, 87),
    _k2("every key 0", "zero", 40, 64, 100, True, 0),
]
CUT_CLEARS = [0, 3, 8]


def _geo(name, keys, p_min, p_max, permille, P, front):
    return dict(name="geo: " + name, keys=keys, p_min=p_min, p_max=p_max, permille=permille, P=P, front=front)


GEO_CASES = [
    _geo("break at p_max", "M", 8, 64, 200, 64, 30),
    _geo("break strictly between", "M", 8, 64, 400, 40, 80),
    _geo("break between, the front's work within 1 % of the share", "M", 8, 64, 420, 40, 80),
    _geo("both sides equal", "M", 8, 64, 424, 40, 80),
    _geo("one permille past equal", "M", 8, 64, 425, 20, 180),
    _geo("break at p_min + 1", "M", 8, 64, 660, 9, 220),
    _geo("no P qualifies", "M", 8, 64, 800, 8, 270),
    _geo("p_max > 1023", "M", 8, 5000, 50, 96, 10),
    _geo("p_max > 1023, the last bin qualifies", "Mc", 8, 5000, 400, 1023, 7),
    _geo("every key 0", "zero", 8, 64, 100, 64, 0),
    _geo("permille 0", "M", 8, 64, 0, 64, 30),
]

# stale bins: two sorts on ONE hist buffer, the second of fewer bins — what a bulk extend call behind a projector call is
STALE_N = 20001


def stale_pair(n=STALE_N):
    first = dict(n=n, nbins=BINS, hist_blocks=256, keys=make_keys("geometric", n, BINS, seed=11), split=None)
    # the second key set is just short of heavy (64 * 100 = 6 400 of 29 400 * 0.22 = 6 468): anything left above bin 64 tips the cut
    k = np.zeros(n, dtype=np.int64)
    k[:15000], k[15000:15200], k[15200:15300] = 1, 40, 64
    second = dict(n=n, nbins=65, hist_blocks=64, keys=np.random.default_rng(12).permutation(k).astype(np.uint16),
                  split=dict(kind=2, clear=8, p_low=40, p_high=64, permille=220, limit=0))
    return first, second


# ---- the device side --------------------------------------------------------------------------------------------------------------
def _lib():
    from closed_chain_motion_planner_amd import _lib as L

    return L


def _dev(a, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


GUARD = 1024


def run_sort(ctx, keys, nbins, hist_blocks=256, split=None, hist_dev=None, clear_first=1, fill=QUEUE_FILL):
    """ccmp_debug_sort_probe on fresh buffers (order pre-filled with 0xFFFFFFFF and a guard of 1024 words behind it, hist — unless the
    caller brings one — with a pattern, the queue block with `fill`) -> order[n], guard, hist[1024], queue[16], the hist buffer"""
    import torch

    L = _lib()
    n = len(keys)
    keys_d = _dev(np.asarray(keys, dtype=np.uint16), np.int16)
    order_d = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    if hist_dev is None:
        hist_dev = torch.full((BINS,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    queue_d = _dev(np.array(fill, dtype=np.uint64), np.int64)
    s = split or dict(kind=0, p_low=0, p_high=0, permille=0, limit=0, clear=0)
    torch.cuda.synchronize()
    L.check(L.lib().ccmp_debug_sort_probe(ctx.handle, keys_d.data_ptr(), n, nbins, hist_blocks, clear_first, order_d.data_ptr(), hist_dev.data_ptr(),
                                          queue_d.data_ptr(), s["kind"], s["p_low"], s["p_high"], s["permille"], s["limit"], s.get("clear", 0), None),
            "ccmp_debug_sort_probe")
    torch.cuda.synchronize()
    o = order_d.cpu().numpy().view(np.uint32)
    return o[:n], o[n:], hist_dev.cpu().numpy().view(np.uint32), [int(v) for v in queue_d.cpu().numpy().view(np.uint64)], hist_dev


def run_split(ctx, kernel, hist, p_min, p_max=0, permille=0, limit=0, fill=QUEUE_FILL):
    """ccmp_debug_split_probe: fd_split_kernel (1) / geo_split_kernel (2) on hist[1024] (host array or device tensor) -> queue[16]"""
    import torch

    L = _lib()
    hist_d = hist if isinstance(hist, torch.Tensor) else _dev(np.asarray(hist, dtype=np.uint32), np.int32)
    queue_d = _dev(np.array(fill, dtype=np.uint64), np.int64)
    L.check(L.lib().ccmp_debug_split_probe(ctx.handle, kernel, hist_d.data_ptr(), p_min, p_max, permille, limit, queue_d.data_ptr(), None), "ccmp_debug_split_probe")
    torch.cuda.synchronize()
    return [int(v) for v in queue_d.cpu().numpy().view(np.uint64)]


def check_sort(case, keys, got):
    """order, guard, every word of hist and of the queue block of one probe run against the model"""
    order, guard, hist, queue, _ = got
    what = case.get("name", "")
    assert (guard == 0xFFFFFFFF).all(), (what, "words behind order written", np.flatnonzero(guard != 0xFFFFFFFF)[:4])
    why = order_defects(order, keys)
    assert why == "", (what, why)
    ge = ge_of(keys)
    assert hist.tolist() == ge, (what, "hist", [(k, int(hist[k]), ge[k]) for k in np.flatnonzero(hist != np.array(ge, dtype=np.uint32))[:4]])
    split = case.get("split")
    want = list(QUEUE_FILL) if split is None else queue_after(QUEUE_FILL, front_of(ge, split), split["clear"])
    assert queue == want, (what, "queue", split, [(i, hex(queue[i]), hex(want[i])) for i in range(16) if queue[i] != want[i]])
    return ge


def check_standalone(ctx, what, ge, hist_dev, i=0):
    """fd_split_kernel and geo_split_kernel on the histogram a sort left on the device, against the model"""
    nz = [k for k in range(1, BINS) if ge[k]]
    top = nz[-1] if nz else 0
    for p, lim in ((top // 2, NO_LIMIT), (top, 1 + i % 5), (top + 1, NO_LIMIT), (0, max(ge[0] - 1, 0))):
        want = queue_after(QUEUE_FILL, front_kind1(ge, p, lim), None)
        got = run_split(ctx, 1, hist_dev, p, limit=lim)
        assert got == want, (what, "fd_split_kernel", p, lim, got[:5], want[:5])
    for p_min, p_max, pm in ((min(8, top), max(top, 8), 100 + 150 * (i % 5)), (0, 1023, 900)):
        want = queue_after(QUEUE_FILL, front_geo(ge, p_min, p_max, pm), None)
        got = run_split(ctx, 2, hist_dev, p_min, p_max, pm)
        assert got == want, (what, "geo_split_kernel", p_min, p_max, pm, got[:5], want[:5])


def test_this_process_runs_on_the_debug_library():
    import os

    L = _lib()
    assert os.path.basename(L.LIBPATH).startswith("libccmp_debug") and all(hasattr(L.lib(), n) for n in L.DEBUG_EXPORTS)


def _sweep(ctx, cases):
    for i, case in enumerate(cases):
        keys = make_keys(case["keys"], case["n"], case["nbins"])
        got = run_sort(ctx, keys, case["nbins"], case["hist_blocks"], case["split"])
        ge = check_sort(case, keys, got)
        if i % 3 == 0:
            check_standalone(ctx, case["name"], ge, got[4], i)


@pytest.mark.parametrize("n", FUSED_SIZES + THREE_SIZES)
def test_sizes(gpu_ctx, n):
    """every key set at every size either side of the fused sort's last, of a scatter block and of the histogram grid's stride"""
    _sweep(gpu_ctx, size_cases(n))


@pytest.mark.parametrize("nbins", NBINS)
def test_bin_counts(gpu_ctx, nbins):
    """scan_desc_kernel's runs of ceil(nbins / 64) bins per lane: one bin, fewer bins than lanes, idle lanes, a run that ends below bin 0"""
    _sweep(gpu_ctx, nbins_cases(nbins))


@pytest.mark.parametrize("n", CUT_SIZES)
@pytest.mark.parametrize("case", KIND1_CASES + KIND2_CASES, ids=lambda c: c["name"])
def test_cut_by_the_sort(gpu_ctx, case, n):
    """apply_split in either sort kernel, every `clear` production uses and one between; kind 1 also as fd_split_kernel on the same histogram"""
    keys = cut_keys(case["keys"], n)
    for clear in CUT_CLEARS:
        split = dict(case["split"], clear=clear)
        got = run_sort(gpu_ctx, keys, case["nbins"], 64 if case["nbins"] < BINS else 256, split)
        ge = check_sort(dict(name=case["name"], split=split), keys, got)
        if split["kind"] == 1:
            alone = run_split(gpu_ctx, 1, got[4], split["p_low"], limit=split["limit"])
            assert alone == queue_after(QUEUE_FILL, front_kind1(ge, split["p_low"], split["limit"]), None), (case["name"], alone[:5])
            assert [alone[i] for i in (0, 3, 4)] == [got[3][i] for i in (0, 3, 4)]


@pytest.mark.parametrize("case", GEO_CASES, ids=lambda c: c["name"])
def test_cut_by_geo_split_kernel(gpu_ctx, case):
    ge = ge_of(cut_keys(case["keys"], 2048))
    got = run_split(gpu_ctx, 2, ge, case["p_min"], case["p_max"], case["permille"])
    assert got == queue_after(QUEUE_FILL, front_geo(ge, case["p_min"], case["p_max"], case["permille"]), None), (case["name"], got[:5])


@pytest.mark.parametrize("n", [STALE_N, FUSED_MAX + 1])
def test_bins_of_the_last_sort_do_not_reach_the_next(gpu_ctx, n):
    """a 1024-bin sort of keys up to 96, then a 65-bin sort of other keys on the SAME hist: bins 65 .. 96 are cleared, the histogram and
    the cut are the second key set's alone — for the sort's own cut and for both stand-alone kernels reading the histogram behind it"""
    first, second = stale_pair(n)
    a = run_sort(gpu_ctx, first["keys"], first["nbins"], first["hist_blocks"], first["split"])
    check_sort(first, first["keys"], a)
    assert a[2][65:97].min() > 0
    b = run_sort(gpu_ctx, second["keys"], second["nbins"], second["hist_blocks"], second["split"], hist_dev=a[4])
    ge = check_sort(second, second["keys"], b)
    assert not b[2][65:].any()
    check_standalone(gpu_ctx, "behind a sort of more bins", ge, b[4])
    # and a fused sort on the same buffer leaves nothing of either
    keys = make_keys("two_point", 1025, 9)
    c = run_sort(gpu_ctx, keys, 9, 64, None, hist_dev=b[4])
    check_sort(dict(name="fused sort on a used hist"), keys, c)
    # the three-kernel form without the clear, on a histogram of zeros
    d = run_sort(gpu_ctx, second["keys"], second["nbins"], second["hist_blocks"], second["split"], hist_dev=c[4].zero_(), clear_first=0)
    check_sort(second, second["keys"], d)


def test_probe_refuses_what_would_leave_the_buffers(gpu_ctx):
    """the probe's own argument checks: a key beyond the scanned bins or an uncleared histogram in the three-kernel form, a cut whose bin
    index the kernels do not clamp"""
    import torch

    L = _lib()
    n = FUSED_MAX + 1
    keys = make_keys("uniform", n, 65)
    keys_d = _dev(keys, np.int16)
    order_d = torch.full((n + GUARD,), -1, dtype=torch.int32, device="cuda")
    hist_d = torch.full((BINS,), 7, dtype=torch.int32, device="cuda")
    queue_d = _dev(np.array(QUEUE_FILL, dtype=np.uint64), np.int64)

    def probe(nbins, clear_first, kind=0, p_low=0, p_high=0, clear=0):
        return L.lib().ccmp_debug_sort_probe(gpu_ctx.handle, keys_d.data_ptr(), n, nbins, 64, clear_first, order_d.data_ptr(), hist_d.data_ptr(), queue_d.data_ptr(),
                                             kind, p_low, p_high, 100, 0, clear, None)

    assert probe(64, 1) == -1 and probe(65, 0) == -1 and probe(0, 1) == -1 and probe(1025, 1) == -1
    assert probe(65, 1, kind=2, p_low=1024) == -1 and probe(65, 1, kind=1, p_low=-1) == -1 and probe(65, 1, kind=2, p_high=-1) == -1
    assert probe(65, 1, kind=1, clear=17) == -1 and probe(65, 1, kind=3) == -1
    for bad in ((1, -1, 0, 100), (2, -1, 64, 100), (2, 9, 8, 100), (2, 1024, 2000, 100), (3, 0, 0, 0)):
        assert L.lib().ccmp_debug_split_probe(gpu_ctx.handle, bad[0], hist_d.data_ptr(), bad[1], bad[2], bad[3], 0, queue_d.data_ptr(), None) == -1, bad
    torch.cuda.synchronize()
    assert (order_d.cpu().numpy() == -1).all() and (hist_d.cpu().numpy() == 7).all()
    assert [int(v) for v in queue_d.cpu().numpy().view(np.uint64)] == QUEUE_FILL


# ---- end to end: the order, the histogram and the queue words real calls leave ------------------------------------------------------
def read_back(ctx, n):
    """(pred[n], order[n], hist[1024], queue words) as the context's last call left them"""
    L = _lib()
    pred = np.full(n, 0xFFFF, dtype=np.uint16)
    order = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    hist = np.full(BINS, 0xFFFFFFFF, dtype=np.uint32)
    queue = np.full(QUEUE_WORDS, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    L.check(L.lib().ccmp_ctx_debug_lpt_pred(ctx.handle, pred.ctypes.data, n), "ccmp_ctx_debug_lpt_pred")
    assert L.lib().ccmp_ctx_debug_lpt_order(ctx.handle, order.ctypes.data, n, hist.ctypes.data, queue.ctypes.data, QUEUE_WORDS - 1) == -1  # (the count is the library's)
    L.check(L.lib().ccmp_ctx_debug_lpt_order(ctx.handle, order.ctypes.data, n, hist.ctypes.data, queue.ctypes.data, QUEUE_WORDS), "ccmp_ctx_debug_lpt_order")
    return pred, order, hist, [int(v) for v in queue]


def check_call(ctx, n, what):
    pred, order, hist, queue = read_back(ctx, n)
    why = order_defects(order, pred)
    assert why == "", (what, why)
    ge = ge_of(pred)
    assert hist.tolist() == ge, (what, "hist", [(k, int(hist[k]), ge[k]) for k in np.flatnonzero(hist != np.array(ge, dtype=np.uint32))[:4]])
    return pred, ge, queue


@pytest.fixture(scope="module")
def own_ctx(ccmp_built):
    """a context of this module's own: its scout buffers hold what THESE calls left"""
    from closed_chain_motion_planner_amd import Context

    return Context(0)


@pytest.fixture(scope="module")
def samples(own_ctx):
    from test_gpu_parity import _constraint

    c = _constraint("Wine_Bottle", own_ctx)
    return c, c.ambient_uniform_batch(0x50A7, 0, 2 * (FUSED_MAX + 64))


SPLIT_SIZES = [12001, FUSED_MAX + 1]  # the fused sort; the first size of the three-kernel form


@pytest.mark.parametrize("pred_min,limit", [(30, 600), (80, 0x7FFFFFFF)], ids=["limit binds", "limit does not bind"])
@pytest.mark.parametrize("n", SPLIT_SIZES)
def test_projector_split_launch(own_ctx, samples, n, pred_min, limit):
    """the sort decides the cut (apply_split kind 1, clear 0): behind the call the order is a descending permutation of the predictions,
    hist their ge, and the front's length — the one queue word no kernel of the call counts on — the model's for the options set"""
    L = _lib()
    c, q = samples
    ctx = own_ctx
    ctx.set_option("fd_split_pred", pred_min)
    ctx.set_option("fd_split_samples", limit)
    try:
        text = ctx.describe(L.CALL_PROJECT, n)
        m = re.search(r"split launch: front = samples predicted >= (\d+) iterations \(<= (\d+)\)", text)
        assert m and "FP32 scout + counting sort" in text, text
        assert (int(m.group(1)), int(m.group(2))) == (pred_min, limit) and limit >= 2 * ctx.num_cus, text
        c.project_batch(q[FUSED_MAX + 64:FUSED_MAX + 64 + n].contiguous(), want_iters=False)  # other content first
        other = read_back(ctx, n)[0]
        c.project_batch(q[:n].contiguous(), want_iters=False)
        pred, ge, queue = check_call(ctx, n, ("split launch", n))
    finally:
        ctx.set_option("fd_split_pred", -1)
        ctx.set_option("fd_split_samples", -1)
    assert not np.array_equal(pred, other) and pred.max() <= 96 and len(np.unique(pred)) > 20
    front = front_kind1(ge, pred_min, limit)
    assert queue[Q_FRONT_LEN] == front, (queue[:8], front)
    assert (front == limit) == (limit == 600) and front > 0  # the case is what its id says


@pytest.mark.parametrize("n", [641, FUSED_MAX + 37])
def test_head_and_resume_form(ccmp_built, samples, n):
    """not in place: the sort runs on the caller's stream behind a scout pass on the side stream and the head launch beside it"""
    from closed_chain_motion_planner_amd import Context

    L = _lib()
    c0, q = samples
    ctx = Context(0)
    ctx.set_schedule(0, 0)
    ctx.set_lpt(1, 0)
    ctx.set_option("fd_head_min_batch", 0)
    ctx.set_option("fd_head_rounds", 5)
    from test_gpu_parity import _constraint

    c = _constraint("Wine_Bottle", ctx)
    text = ctx.describe(L.CALL_PROJECT, n)
    assert "(head)" in text and "FP32 scout" in text and "the scout pass beside them on the side stream" in text, text
    c.project_batch(q[FUSED_MAX + 64:FUSED_MAX + 64 + n].contiguous(), want_iters=False)  # other content first
    other = read_back(ctx, n)[0]
    c.project_batch(q[:n].contiguous(), want_iters=False)
    pred, _, _ = check_call(ctx, n, ("head and resume", n))
    assert not np.array_equal(pred, other) and pred.max() <= 96 and len(np.unique(pred)) > 20


GEO_E = FUSED_MAX + 1


@pytest.fixture(scope="module")
def edges(own_ctx, samples):
    """growTree-shaped edges, as tests/debug_hook_cases.py makes its 16 384"""
    c, _ = samples
    qs, oks, _, _ = c.sample_project_batch(0x6F5, 0, 8 * 16384, want_iters=False)
    frm = qs[oks == 1][:GEO_E].contiguous()
    assert frm.shape[0] == GEO_E
    to, _, _, _ = c.sample_near_project_batch(0x6F6, 0, frm, 0.6, GEO_E, want_iters=False)
    return frm, to


@pytest.mark.parametrize("form", ["default cut", "permille", "fixed cut"])
def test_bulk_extend_call_behind_a_projector_call(own_ctx, samples, edges, form):
    """the extend step's sort fills round cap + 1 bins of a histogram in which the projector's sort has just left counts up to bin 96:
    behind the call hist is the edge predictions' ge — zero above the cap — and the front's length the model's, for each of the three
    ways the cut is decided (the sort's own kernel; geo_split_kernel; fd_split_kernel)"""
    L = _lib()
    c, q = samples
    frm, to = edges
    ctx = own_ctx
    cap = ctx.get_option("geodesic_scout_rounds")
    opts = {"default cut": {}, "permille": {"geodesic_group_permille": 300}, "fixed cut": {"geodesic_group_pred": 20}}[form]
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        text = ctx.describe(L.CALL_GEODESIC_BUDGET, GEO_E)
        m = re.search(r"bulk form: front \(predicted >= 64 rounds if those edges carry (\d+) permille of the work, else >= (\d+)\)", text)
        assert m and "FP32 scout" in text and "counting sort" in text, text
        assert ("(cut fixed at 20)" in text) == (form == "fixed cut"), text
        assert "split launch" in ctx.describe(L.CALL_PROJECT, GEO_E)
        c.project_batch(q[:GEO_E].contiguous(), want_iters=False)
        _, ge_p, _ = check_call(ctx, GEO_E, "the projector call in front")
        assert ge_p[cap + 1] > 0  # it leaves counts above the extend step's bins
        c.discrete_geodesic_batch(frm, to, 16, want_carry=True, round_budget=128)
        pred, ge, queue = check_call(ctx, GEO_E, ("bulk extend", form))
    finally:
        ctx.set_option("geodesic_group_permille", 0)
        ctx.set_option("geodesic_group_pred", -1)
    assert pred.max() <= cap and len(np.unique(pred)) > 10 and ge[1] > 0
    if form == "default cut":
        front = front_kind2(ge, int(m.group(2)), 64, int(m.group(1)))
    elif form == "permille":
        front = front_geo(ge, 8, 64, 300)
    else:
        front = front_kind1(ge, 20, NO_LIMIT)
    assert queue[Q_BULK + B_FRONT_LEN] == front, (form, queue[Q_BULK:], front)
    assert 0 < front < GEO_E

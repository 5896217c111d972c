"""The five device forms of the proxy clearance — clearance_kernel<4> and <10> (64-state tiles), clearance_state_kernel (one block
per state), state_clearance<128> and <16> (the extend step, FD and analytic) — at every pair-table shape of tests/scene_cases.py,
on exact ties across wavefronts, around the tile kernel's squared-distance prune and beyond its domain: bit for bit against
oracle/ccmp_oracle.c: orc_clearance on the same rows, NaN equal to NaN, with the pair codes and the flags.

Mutation check: one-token changes of the device and launch code on scratch builds, one run of this file each; all gave wrong
answers, none a fault.  (tests/test_gpu_scene.py and test_gpu_geodesic_scene.py, run once on five of the builds: they too fail under
the two tie-breaks and the box loop — the default skeleton scene has ties and box pairs — and pass under the launch switch; under the
shuffle width test_gpu_geodesic_scene.py does not end — with a finite margin the threads of a block disagree about the state's
validity around the extend step's barriers; the margin -inf of the extend-step test here keeps them agreed.)  What failed here:
  phase 3 of the tile kernel `vp < bestp` -> `>`                   test_twins[tiles-*] (3), test_prune_cases[tiles-*] (2), test_every_shape[tiles-ns64]
  clearance_state_kernel's shuffle tie-break, likewise             test_twins[per_state-19+3 / 256+44], test_prune_cases[per_state-*] (2),
                                                                   test_every_shape[per_state-ns64]
  the launch switch `n_pairs <= 1024` -> `<= 1025`                 test_last_pair_of_the_table_wins[tiles-700+325] alone: in the random 1025-pair
                                                                   scene the pair that falls off the table is never the minimum
  the table load `p < np` -> `p + kTileWaves < np` (both lines)    run on shapes without sphere-box pairs only (with them the changed kernel indexes
                                                                   box -64, before the scene's allocation): test_every_shape[tiles-1+0 / 5+0 / 127+0 /
                                                                   257+0], test_last_pair_of_the_table_wins[tiles-5+0 / 257+0]; [tiles-1024+0] passed
  the box loop `l < end` -> `l + 1 < end`                          test_every_shape[tiles-*] at 13 shapes with sphere-box pairs, test_grid_stride_tile_loop,
                                                                   test_last_pair_of_the_table_wins[tiles-*] at all 5 tables that end in one
  state_clearance's first shuffle width `/ 2` -> `/ 4`             test_extend_step_forms: 21 of 26 (not n_pairs 15..17 in mode 0: lanes 32.. hold no pair;
                                                                   not the twin scene: a copy of the minimum survives)
  the host's guard on the prune's domain disabled                  test_beyond_the_prune_domain[1-tiles], [64-tiles]: pair 0 and 0.42 instead of pair 4"""
import ctypes as C

import numpy as np
import pytest

import scene_cases as SC
from conftest import NCPU
from test_gpu_analytic_extend import _edges
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu

OBJ = "stefan"
B_SHAPES = 130  # two full tiles and two live lanes of a third
OPTIONS = {"tiles": 0, "per_state": 1 << 30, "default": 8192}
GUARD_F, GUARD_I, GUARD_B = 12345.0, 0x7E57, 0xA5
HOST_SHAPES = ("1+0", "257+0", "1920+512")
EXTEND_SHAPES = ("12+3", "13+3", "14+3", "127+0", "128+0", "129+0", "700+325", "1920+512", "ns15", "ns16", "ns17", "ns64", "twin:256+44")


@pytest.fixture(params=["tiles", "per_state"])
def kernel_choice(request, gpu_ctx):
    gpu_ctx.set_option("clearance_per_state_max", OPTIONS[request.param])
    yield request.param
    gpu_ctx.set_option("clearance_per_state_max", 8192)


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


class Bench:
    """what the tests of this module share: the constraint, the checker's problem, the states and the oracle's answers per scene"""

    def __init__(self, ctx, oracle):
        self.ctx, self.o = ctx, oracle
        self.c = _constraint(OBJ, ctx)
        self.P = _oracle_problem(oracle, self.c)
        q = oracle.ambient_uniform_batch(self.P, 0x5CE3, 0, B_SHAPES)  # half ambient, half projected (tests/test_gpu_scene.py: _states)
        proj, _, _ = oracle.project_batch(self.P, q[: B_SHAPES // 2], NCPU)
        self.q = np.concatenate([q[B_SHAPES // 2:], proj])
        self.q[7, 3] = np.nan
        self.q[8, 12] = np.inf
        self.ok = np.random.default_rng(0x5CE4).integers(0, 2, B_SHAPES).astype(np.uint8)
        self.x0 = SC.fixed_state(oracle, self.P)
        self._ref, self._twice, self._edges = {}, {}, {}

    def reference(self, name):
        if name not in self._ref:
            clr, pair = self.o.clearance_batch(self.P, *SC.scene(name), self.q)
            clr.setflags(write=False); pair.setflags(write=False)
            self._ref[name] = (clr, pair)
        return self._ref[name]

    def twice(self, name):
        if name not in self._twice:
            self._twice[name] = SC.min_attained_twice(self.o, self.P, SC.scene(name), self.q)
        return self._twice[name]

    def proxy_scene(self, sc, c=None):
        from closed_chain_motion_planner_amd import scene as S

        return S.ProxyScene(c or self.c, *sc)

    def run(self, ps, q, ok=None, margin=0.0):
        """ccmp_clearance_batch into buffers with one guard element behind each output -> (clearance, pair, free) on the host"""
        import torch
        from closed_chain_motion_planner_amd import _lib

        B = q.shape[0]
        qd = torch.as_tensor(np.ascontiguousarray(q)).cuda()
        okd = None if ok is None else torch.as_tensor(ok).cuda()
        clr = torch.full((B + 1,), GUARD_F, dtype=torch.float64, device="cuda")
        pair = torch.full((B + 1,), GUARD_I, dtype=torch.int32, device="cuda")
        free = torch.full((B + 1,), GUARD_B, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().ccmp_clearance_batch(self.c.ctx.handle, C.byref(self.c.problem), ps._h, qd.data_ptr(),
                                                   okd.data_ptr() if okd is not None else None, B, float(margin), clr.data_ptr(),
                                                   pair.data_ptr(), free.data_ptr(), None), "ccmp_clearance_batch")
        torch.cuda.synchronize()
        clr, pair, free = clr.cpu().numpy(), pair.cpu().numpy(), free.cpu().numpy()
        assert clr[B] == GUARD_F and pair[B] == GUARD_I and free[B] == GUARD_B
        return clr[:B], pair[:B], free[:B]

    def compare(self, got, ref, ok=None, margin=0.0, what=None):
        clr, pair, free = got
        clr_o, pair_o = ref
        bad = np.nonzero(~_bits_equal(clr, clr_o) | (pair != pair_o))[0]
        assert bad.size == 0, (what, bad[:8], clr[bad[:4]], clr_o[bad[:4]], pair[bad[:4]], pair_o[bad[:4]])
        with np.errstate(invalid="ignore"):
            want = (clr_o > margin) if ok is None else ((ok != 0) & (clr_o > margin))
        assert np.array_equal(free, want.astype(np.uint8)), what


@pytest.fixture(scope="module")
def bench(gpu_ctx, oracle_det):
    return Bench(gpu_ctx, oracle_det)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_every_shape(bench, name, kernel_choice):
    ps = bench.proxy_scene(SC.scene(name))
    n_ss, n_sb = (len(v) for v in SC.tested_pairs(*SC.scene(name)))
    assert ps.num_pairs == n_ss + n_sb
    ref = bench.reference(name)
    bench.compare(bench.run(ps, bench.q, bench.ok, 0.02), ref, bench.ok, 0.02, name)
    assert np.isnan(ref[0][7]) and np.isnan(ref[0][8]) and ref[1][7] == -1
    if name in HOST_SHAPES:  # the host entry: one state (the done word) and twenty
        clean = np.delete(bench.q, (7, 8), axis=0)
        clr, pair, free = ps.clearance(clean[0])
        clr_o, pair_o, _ = bench.o.clearance(bench.P, *SC.scene(name), clean[0])
        assert _bits_equal(clr, clr_o).all() and pair == pair_o and free == (clr_o > 0.0)
        clr, pair, free = ps.clearance(clean[:20])
        clr_o, pair_o = bench.o.clearance_batch(bench.P, *SC.scene(name), clean[:20])
        assert _bits_equal(clr, clr_o).all() and np.array_equal(pair, pair_o) and np.array_equal(free, (clr_o > 0.0).astype(np.uint8))
    ps.close()


def test_grid_stride_tile_loop(bench, gpu_ctx):
    """the largest scene (> 64 KB of LDS: one block per CU) on more tiles than blocks, the last one ragged; every state compared"""
    import torch

    name = "1920+512"
    B = 64 * int(gpu_ctx.get_option("num_cus")) + 65
    c = bench.c
    q = torch.cat([c.ambient_uniform_batch(0x5CE9, 0, B - B // 2), c.sample_project_batch(0x5CEA, 0, B // 2, want_iters=False)[0]]).cpu().numpy()
    ps = bench.proxy_scene(SC.scene(name))
    gpu_ctx.set_option("clearance_per_state_max", 0)
    try:
        got = bench.run(ps, q, None, 0.0)
    finally:
        gpu_ctx.set_option("clearance_per_state_max", 8192)
    bench.compare(got, bench.o.clearance_batch(bench.P, *SC.scene(name), q), None, 0.0, B)
    ps.close()


@pytest.mark.parametrize("name", SC.TWINS)
def test_twins(bench, name, kernel_choice):
    """every proxy twice: each minimum is attained by a pair and its copies, which sit in other wavefronts' shares (and register
    sets) — the earliest in the list must be reported"""
    name = "twin:" + name
    twice = bench.twice(name)  # a condition on the inputs, from the oracle's centres
    assert twice.mean() >= 0.25, twice.mean()
    ps = bench.proxy_scene(SC.scene(name))
    bench.compare(bench.run(ps, bench.q, bench.ok, 0.02), bench.reference(name), bench.ok, 0.02, name)
    ps.close()


@pytest.mark.parametrize("name", SC.LAST_WINS)
def test_last_pair_of_the_table_wins(bench, name, kernel_choice):
    """the end of a wavefront's share, of a register set and of the table: the last tested pair is the strict minimum"""
    name = "last:" + name
    clr_o, pair_o = bench.reference(name)
    last = SC.pair_codes(*SC.scene(name))[-1]
    assert (pair_o == last).mean() >= 0.9  # a condition on the inputs: all but the two non-finite rows and a rare near-coincidence
    ps = bench.proxy_scene(SC.scene(name))
    bench.compare(bench.run(ps, bench.q, bench.ok, 0.02), (clr_o, pair_o), bench.ok, 0.02, name)
    ps.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", EXTEND_SHAPES)
def test_extend_step_forms(bench, gpu_ctx, name, mode):
    """state_clearance<128> (mode 0, geodesic_scene_kernel) and <16> (mode 1, geodesic_row16_scene_kernel): the clearances the extend
    step reports for its listed states; margin -inf, so the traversal itself does not depend on the scene"""
    if mode not in bench._edges:
        import torch

        c = _constraint("Wine_Bottle", gpu_ctx, mode=mode)
        frm, to = _edges(c, 256, 0x5CEB)  # growTree-shaped edges list about three states each: the eight longest of 256
        keep = torch.argsort(c.discrete_geodesic_batch(frm, to, 16)[1], descending=True, stable=True)[:8].sort().values
        bench._edges[mode] = (c, _oracle_problem(bench.o, c), frm[keep].contiguous(), to[keep].contiguous())
    c, P, frm, to = bench._edges[mode]
    ms = 16
    ps = bench.proxy_scene(SC.scene(name), c)
    st, n, ok, its, bl, clr = [x.cpu().numpy() for x in c.discrete_geodesic_scene_batch(frm, to, ps, float("-inf"), ms, want_clearance=True)]
    listed = 0
    for e in range(frm.shape[0]):
        m = min(int(n[e]), ms)
        assert np.isnan(clr[e, 0]) and np.isnan(clr[e, m:]).all(), e
        if m > 1:
            clr_o, _ = bench.o.clearance_batch(P, *SC.scene(name), st[e, 1:m])
            assert _bits_equal(clr[e, 1:m], clr_o).all(), (e, clr[e, 1:m], clr_o)
            listed += m - 1
    assert listed >= 40 and not bl.any()
    ps.close()


@pytest.mark.parametrize("B", [1, 64])
def test_prune_cases(bench, kernel_choice, B):
    """pairs a hair apart in rising and falling order, a swallowed hand (best + rsum <= 0), a zero distance: one state, and a
    wavefront of copies of it (the square root runs if any lane needs it)"""
    q = np.repeat(bench.x0[None, :], B, axis=0)
    for name, sc in SC.prune_cases(bench.o, bench.P, bench.x0).items():
        ps = bench.proxy_scene(sc)
        bench.compare(bench.run(ps, q), bench.o.clearance_batch(bench.P, *sc, q), None, 0.0, name)
        ps.close()


@pytest.mark.parametrize("choice", sorted(OPTIONS))
@pytest.mark.parametrize("B", [1, 64])
def test_beyond_the_prune_domain(bench, gpu_ctx, choice, B):
    """A world sphere 2^25 m (2^27 m) away whose pair becomes the minimum by 1.9e-9 (1.3e-8) behind an earlier pair of the same
    wavefront: the tile kernel's prune drops it — without the host's guard the answer is pair 0 and 0.42, not pair 4 — so the scene is
    served by the one-block kernel under every option value.  And a scene just inside the bound still matches with tiles forced."""
    q = np.repeat(bench.x0[None, :], B, axis=0)
    gpu_ctx.set_option("clearance_per_state_max", OPTIONS[choice])
    try:
        for dist in (2.0 ** 25, 2.0 ** 27):
            sph, facts = SC.huge_pair_scene(bench.o, bench.P, bench.x0, dist, True)
            ps = bench.proxy_scene((sph, [], None))
            clr, pair, free = bench.run(ps, q)
            print("%s B=%d dist %g: clearance %.17g pair %d (oracle %.17g pair %d; the pair before %.17g pair %d)"
                  % (choice, B, dist, clr[0], pair[0], facts["clearance"], facts["pair"], facts["best"], facts["first_pair"]))
            bench.compare((clr, pair, free), bench.o.clearance_batch(bench.P, sph, [], None, q), None, 0.0, (choice, dist))
            assert (pair == facts["pair"]).all()
            ps.close()
        sph, facts = SC.huge_pair_scene(bench.o, bench.P, bench.x0, 1.3e6, False)
        assert SC.prune_bound(bench.P, sph, [], None) < SC.PRUNE_LIMIT
        ps = bench.proxy_scene((sph, [], None))
        bench.compare(bench.run(ps, q), bench.o.clearance_batch(bench.P, sph, [], None, q), None, 0.0, (choice, "inside"))
        ps.close()
    finally:
        gpu_ctx.set_option("clearance_per_state_max", 8192)

"""Proxy scenes for the clearance tests (tests/test_scene_cases.py, tests/test_gpu_scene_shapes.py).  Host only.

  * `tested_pairs`: the pair rule of include/ccmp.h restated in plain Python, in the public numbering;
  * `scene_with`: a seeded scene with EXACTLY the asked numbers of tested sphere-sphere and sphere-box pairs.  Sphere i rides on
    moving frame MOVING[i % 16]; the first eight spheres sit alone in groups 0..7, the rest round-robin in groups 8..23, every box
    in a group of its own (24..).  The excess over the asked counts is removed by allowing whole pairs of groups, largest first;
    the singleton groups supply the removals of exactly one pair;
  * `CASES` / `scene`: the table of shapes, by the edges of the five device forms of the clearance (the 64-state tile kernel's
    register sets of 64 entries per wavefront and its two instantiations, its four-at-a-time sphere-sphere loop, the strides 256,
    128 and 16 of the one-block, extend-step and 16-lane-row forms, the row form's placement loop over 16 spheres);
  * `twin`: every proxy twice, so that every minimum is attained by at least two pairs of the list; `last_wins`: the same table with
    the last pair the strict minimum;
  * the prune cases: scenes around one projected state in which the tile kernel's squared-distance prune (ccmp_kernels_scene.hip:
    consider_pair) meets pairs a hair apart, a swallowed hand, a zero distance — and `huge_pair_scene`, the large-magnitude pair
    the prune would drop beyond its domain, found on the host with the kernel's dot3 in exact rationals;
  * `prune_bound`: the host's bound on `best + rsum` (ccmp_scene.cpp) restated."""
import functools
import math
from collections import Counter
from fractions import Fraction

import numpy as np

FRAME_WORLD = -1
MAX_SPHERES, MAX_BOXES = 64, 8
MOVING = tuple(arm * 9 + k for arm in (0, 1) for k in range(8))  # bodies 0..6 and the hand of both arms
PRUNE_LIMIT = 2.0 ** 22  # the tile kernel serves scenes whose bound lies below


def _static(frame):
    return frame < 0 or frame % 9 == 8


def _is_allowed(allowed, g, h):
    return allowed is not None and bool(((allowed[g] >> h) & 1) or ((allowed[h] >> g) & 1))


def tested_pairs(spheres, boxes, allowed):
    """-> ([(i, j)], [(i, b)]): never tested are two proxies on one frame, two static proxies (world or an arm's base; a box is
    static) and pairs whose groups are allowed in either direction; sphere-sphere pairs first in (i, j) order, then (i, b)"""
    ss = [(i, j) for i in range(len(spheres)) for j in range(i + 1, len(spheres))
          if spheres[i][0] != spheres[j][0] and not (_static(spheres[i][0]) and _static(spheres[j][0]))
          and not _is_allowed(allowed, spheres[i][1], spheres[j][1])]
    sb = [(i, b) for i in range(len(spheres)) for b in range(len(boxes))
          if not _static(spheres[i][0]) and not _is_allowed(allowed, spheres[i][1], boxes[b][0])]
    return ss, sb


def pair_codes(spheres, boxes, allowed):
    """the tested pairs as the codes ccmp_clearance_batch reports, in list order"""
    ss, sb = tested_pairs(spheres, boxes, allowed)
    return [i | (j << 8) for i, j in ss] + [i | ((MAX_SPHERES + b) << 8) for i, b in sb]


def _skeleton(m, n_world, n_base):
    """(frame, group) of m moving spheres, then the statics: n_world on the world frame, n_base on each arm's base"""
    frames = [MOVING[i % 16] for i in range(m)] + [FRAME_WORLD] * n_world + [8] * n_base + [17] * n_base
    return [(f, i if i < 8 else 8 + (i - 8) % 16) for i, f in enumerate(frames)]


def _trim(sk, box_groups, allowed, kind, excess):
    """allow whole pairs of groups, the one with the most tested pairs of `kind` that still fits first, until `excess` pairs are gone"""
    while excess > 0:
        pairs = tested_pairs([(f, g, None, None) for f, g in sk], [(g,) for g in box_groups], allowed)[kind]
        other = (lambda j: sk[j][1]) if kind == 0 else (lambda b: box_groups[b])
        counts = Counter((min(sk[i][1], other(j)), max(sk[i][1], other(j))) for i, j in pairs)
        fits = [(c, key) for key, c in counts.items() if c <= excess]
        assert fits, "no pair of groups removes %d or fewer pairs" % excess
        c, (g, h) = max(fits, key=lambda ck: (ck[0], -ck[1][0], -ck[1][1]))
        allowed[g] |= 1 << h
        allowed[h] |= 1 << g
        excess -= c


def scene_with(n_ss, n_sb, *, n_spheres=None, statics=0, seed):
    """(spheres, boxes, allowed) with exactly n_ss tested sphere-sphere and n_sb tested sphere-box pairs.  n_spheres: the number of
    spheres, statics included (default: the fewest that reach the counts).  statics: so many extra spheres on the world frame and
    on both arms' bases (0, or at least 5: five on the world frame — every wavefront of the tile kernel places one, one places two)"""
    assert statics == 0 or statics >= 5
    n_base = max(0, statics - 5) // 2
    n_world = statics - 2 * n_base

    def capacity(m):
        sk = _skeleton(m, n_world, n_base)
        return len(tested_pairs([(f, g, None, None) for f, g in sk], [], None)[0]), m * MAX_BOXES

    if n_spheres is None:
        m = next(m for m in range(1, MAX_SPHERES - statics + 1) if capacity(m)[0] >= n_ss and capacity(m)[1] >= n_sb)
    else:
        m = n_spheres - statics
    nb = -(-n_sb // m)
    assert m >= 1 and m + statics <= MAX_SPHERES and nb <= MAX_BOXES and capacity(m)[0] >= n_ss
    sk = _skeleton(m, n_world, n_base)
    box_groups = [24 + b for b in range(nb)]
    allowed = [0] * 32
    _trim(sk, box_groups, allowed, 0, capacity(m)[0] - n_ss)
    _trim(sk, box_groups, allowed, 1, m * nb - n_sb)
    rng = np.random.default_rng(seed)
    spheres = []
    for i, (f, g) in enumerate(sk):
        c = rng.uniform([-0.2, -0.8, 0.6], [0.9, 0.8, 1.8]) if f == FRAME_WORLD else rng.uniform(-0.15, 0.15, 3)
        r = float(rng.uniform(0.0, 0.08))
        spheres.append((f, g, tuple(float(v) for v in c), 0.0 if i % 7 == 3 else r))
    boxes = []
    for b in range(nb):  # as tests/test_gpu_scene.py: two axis-aligned, the others turned
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        boxes.append((box_groups[b], tuple(float(v) for v in rng.uniform([-0.2, -0.8, 0.6], [0.9, 0.8, 1.8])), np.eye(3) if b < 2 else Q,
                      tuple(float(v) for v in rng.uniform(0.0, 0.3, 3))))
    ss, sb = tested_pairs(spheres, boxes, allowed)
    assert (len(ss), len(sb)) == (n_ss, n_sb), (len(ss), len(sb), n_ss, n_sb)
    assert len(spheres) == (n_spheres if n_spheres is not None else m + statics)
    return spheres, boxes, allowed


# (n_ss, n_sb): what each group of shapes is there for
TINY = [(1, 0), (0, 1), (2, 0), (2, 1), (3, 2), (4, 0), (5, 0)]  # a wavefront's share of the table empty or a single pair
TAILS = [(12, 3), (13, 3), (14, 3), (15, 3), (16, 3), (17, 3), (18, 3), (19, 3)]  # every tail of the four-at-a-time loop; n_pairs 15..22:
#                                                   the 16-lane row's stride
STRIDES = [(127, 0), (128, 0), (129, 0)]  # the extend step's 128 threads
SETS = [(255, 0), (256, 0), (257, 0), (260, 0), (256, 44), (250, 12), (258, 0)]  # register sets of 4 x 64 entries; the one-block stride 256;
#                                                   sphere-box pairs starting on a set boundary (256, 44) and astride one (250, 12)
SWITCH = [(700, 323), (700, 324), (700, 325), (1024, 0)]  # n_pairs 1023 / 1024 / 1025: the two instantiations of the tile kernel
REST = [(0, 512), (1920, 512)]  # boxes only; the largest scene the rule admits (64 spheres four to a moving frame, 8 boxes)
SHAPES = TINY + TAILS + STRIDES + SETS + SWITCH + REST
CASES = {"%d+%d" % s: dict(n_ss=s[0], n_sb=s[1]) for s in SHAPES}
CASES["statics9"] = dict(n_ss=300, n_sb=70, statics=9)  # five world spheres, two on each arm's base
CASES.update({"ns15": dict(n_ss=97, n_sb=21, n_spheres=15), "ns16": dict(n_ss=101, n_sb=37, n_spheres=16),  # the row form places
              "ns17": dict(n_ss=110, n_sb=23, n_spheres=17), "ns64": dict(n_ss=1000, n_sb=300, n_spheres=64)})  # spheres s, s + 16, ...
TWINS = ("19+3", "256+44", "700+325")  # twin() of these: 88, 1200 and 2247 tested pairs


@functools.lru_cache(maxsize=None)
def scene(name):
    if name.startswith("twin:"):
        return twin(scene(name[5:]))
    if name.startswith("last:"):
        return last_wins(scene(name[5:]))
    return scene_with(seed=0x5CE00 + sorted(CASES).index(name), **CASES[name])


def twin(sc):
    """every sphere and every box twice (the copies behind the originals, cut at 64 spheres and 8 boxes): a pair and its copies have
    the same operands, so their distances tie bit for bit; the copies sit elsewhere in the list — other wavefronts' shares, other
    register sets"""
    spheres, boxes, allowed = sc
    return (list(spheres) * 2)[:MAX_SPHERES], (list(boxes) * 2)[:MAX_BOXES], list(allowed)


LAST_WINS = ("5+0", "19+3", "257+0", "256+44", "700+324", "700+325", "1920+512")  # last_wins() of these


def last_wins(sc):
    """the same pair table, with the geometry changed so that the LAST tested pair is the strict minimum of (nearly) every state: the
    end of a wavefront's share, of a register set, of the whole table.  A last sphere-sphere pair gets two radii of 5 m (its distance
    less 10 m lies below every other pair's, none of which has more than 5.08 m of radii); a last sphere-box pair gets a sphere of
    5 m in a box of 50 m (distance 0, clearance -5 m), the other boxes 100 m away (a box the sphere's centre is in would tie earlier
    in the list)"""
    spheres, boxes, allowed = list(sc[0]), list(sc[1]), sc[2]
    ss, sb = tested_pairs(spheres, boxes, allowed)
    grow = lambda s: (s[0], s[1], s[2], 5.0)
    if sb:
        i, b = sb[-1]
        spheres[i] = grow(spheres[i])
        boxes = [(g, (0.0, 0.0, 1.0), R, (50.0, 50.0, 50.0)) if k == b else (g, (c[0] + 100.0, c[1], c[2]), R, h) for k, (g, c, R, h) in enumerate(boxes)]
    else:
        i, j = ss[-1]
        spheres[i], spheres[j] = grow(spheres[i]), grow(spheres[j])
    return spheres, boxes, allowed


def min_attained_twice(oracle, P, sc, q):
    """per state: does more than one tested pair attain the smallest signed distance?  From the oracle's centres, in numpy's own
    rounding: copies of a pair have identical operands, so they tie in any rounding"""
    spheres, boxes, allowed = sc
    ss, sb = tested_pairs(spheres, boxes, allowed)
    r = np.array([s[3] for s in spheres])
    out = np.zeros(len(q), dtype=bool)
    for n, x in enumerate(q):
        if not np.isfinite(x).all():
            continue
        c = oracle.proxy_centres(P, spheres, x)
        v = []
        if ss:
            i, j = np.array(ss).T
            v.append(np.sqrt(((c[i] - c[j]) ** 2).sum(1)) - (r[i] + r[j]))
        if sb:
            i, b = np.array(sb).T
            Rb = np.array([boxes[k][2] for k in range(len(boxes))])
            d = c[i] - np.array([boxes[k][1] for k in range(len(boxes))])[b]
            loc = np.einsum("nji,nj->ni", Rb[b], d)
            e = np.maximum(np.abs(loc) - np.array([boxes[k][3] for k in range(len(boxes))])[b], 0.0)
            v.append(np.sqrt((e ** 2).sum(1)) - r[i])
        v = np.concatenate(v)
        out[n] = (v == v.min()).sum() >= 2
    return out


# ---- the prune of the tile kernel -------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # the exact value, rounded once (tests/graph_cases.py)


def dot3(a0, b0, a1, b1, a2, b2):
    """ccmp_fd_common.h: dot3 in the canonical rounding model, fma(a2, b2, fma(a1, b1, a0 * b0))"""
    return _fma(a2, b2, _fma(a1, b1, a0 * b0))


def prune_skips(best, rsum, d2):
    """consider_pair's predicate: the pair is dropped on its squared distance, without its square root"""
    t = (best + rsum) + 1e-9
    return t <= 0.0 or d2 > t * t


def becomes_minimum(best, rsum, d2):
    """the plain rule (orc_clearance, clearance_state_kernel, state_clearance)"""
    return math.sqrt(d2) - rsum < best


def sqrt_preimages(S):
    """the doubles whose correctly rounded square root is S"""
    d = S * S
    return sorted({v for v in (_step(d, k) for k in range(-3, 4)) if math.sqrt(v) == S})


def _step(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, np.inf if k > 0 else -np.inf))
    return v


def dropped_minima(scale, n, seed):
    """adversarial triples at best + rsum ~ scale: S in {t, pred(t)} and every d2 whose square root rounds to S.  -> (tried, the
    triples (best, rsum, d2) the prune drops although the plain rule makes them the minimum)"""
    rng = np.random.default_rng(seed)
    tried, bad = 0, []
    for _ in range(n):
        best = float(rng.uniform(-0.5, 1.0)) if rng.integers(0, 4) else float(rng.uniform(0.0, 1.0) * scale * 0.25)
        rsum = float(scale * rng.uniform(0.5, 0.999)) - max(best, 0.0)
        if rsum < 0.0:
            continue
        t = (best + rsum) + 1e-9
        for S in (t, _step(t, -1)):
            if not S > 0.0:
                continue
            for d2 in sqrt_preimages(S):
                tried += 1
                if prune_skips(best, rsum, d2) and becomes_minimum(best, rsum, d2):
                    bad.append((best, rsum, d2))
    return tried, bad


def fixed_state(oracle, P):
    """one projected state (on the manifold, within the joint limits): the x0 of every prune case"""
    q = oracle.ambient_uniform_batch(P, 0x5CA5E, 0, 64)
    proj, ok, _ = oracle.project_batch(P, q, 1)
    return proj[np.nonzero(ok == 1)[0][0]].copy()


HAND = 7  # CCMP_FRAME(0, 7)


def _hand_centre(oracle, P, x0):
    return oracle.proxy_centres(P, [(HAND, 0, (0.0, 0.0, 0.0), 0.0)], x0)[0]


def prune_cases(oracle, P, x0):
    """{name: (spheres, boxes, allowed)}: one hand sphere against world spheres.  The pairs are (0, 1), (0, 2), ... in list order, and
    wavefront w of the tile kernel keeps its own running minimum over pairs w, w + 4, ...: whatever must meet in one running minimum is
    listed four times over"""
    a = _hand_centre(oracle, P, x0)
    u = np.array([0.6, 0.0, 0.8])
    gaps = (0.0, 0.0, 1e-10, 1e-9, 1e-8)

    def stacked(order):
        return [(HAND, 0, (0.0, 0.0, 0.0), 0.03)] + [(FRAME_WORLD, 1, tuple(float(v) for v in a + u * (0.5 + g)), 0.05) for g in order for _ in range(4)]

    cases = {"stacked_rising": (stacked(gaps), [], None), "stacked_falling": (stacked(gaps[::-1]), [], None)}
    # a world sphere of radius 10 m swallows the hand: best + rsum <= 0 for the small pairs behind it in wavefront 0 (pairs 4, 8), and a
    # deeper one behind those (pair 12) still has to be found
    far = [(FRAME_WORLD, 1, tuple(float(v) for v in a + [0.0, 1.0 + 0.1 * k, 0.0]), 0.01 * (k % 3)) for k in range(16)]
    sw = [(HAND, 0, (0.0, 0.0, 0.0), 0.03), (FRAME_WORLD, 1, tuple(float(v) for v in a + [0.5, 0.0, 0.0]), 10.0)] + far
    sw[13] = (FRAME_WORLD, 1, tuple(float(v) for v in a + [0.0, 0.0, 0.7]), 20.0)  # pair 12
    cases["swallowed"] = (sw, [], None)
    # a world sphere exactly on the computed centre of the hand sphere, both of radius 0: d2 = 0, clearance 0 — behind a positive
    # pair of the same wavefront (pair 0 -> pair 4), once more behind itself (pair 8: the tie keeps pair 4), small pairs after it
    z = [(HAND, 0, (0.0, 0.0, 0.0), 0.0)] + [(FRAME_WORLD, 1, tuple(float(v) for v in a + [0.3 + 0.01 * k, 0.0, 0.0]), 0.0) for k in range(14)]
    z[5] = z[9] = (FRAME_WORLD, 1, tuple(float(v) for v in a), 0.0)
    z[13] = (FRAME_WORLD, 1, tuple(float(v) for v in a + [0.0, 1e-10, 0.0]), 0.0)  # pair 12: d2 ~ 1e-20 against t = 1e-9
    cases["zero_distance"] = (z, [], None)
    return cases


def huge_pair_scene(oracle, P, x0, dist, want_skip):
    """A hand sphere of radius 0 (centre a), a world sphere 0.5 m from it (pair 0: it leaves `best`), three far fillers (pairs 1..3)
    and a world sphere at a + (dist, e, 0) of radius fl(S - best) + k ulp, S the computed distance (pair 4: wavefront 0's next pair, so
    it meets pair 0's `best`).  (e, k) is the first candidate for which the oracle makes pair 4 the minimum and — want_skip — the tile
    kernel's predicate says skip.  -> (spheres, facts) or None"""
    hand = (HAND, 0, (0.0, 0.0, 0.0), 0.0)
    a = _hand_centre(oracle, P, x0)
    head = [hand, (FRAME_WORLD, 1, (float(a[0] + 0.5), float(a[1]), float(a[2])), 0.08)]
    head += [(FRAME_WORLD, 1, (float(a[0]), float(a[1] + 3.0 + 0.1 * k), float(a[2])), 0.0) for k in range(3)]
    best, first, _ = oracle.clearance(P, head, [], None, x0)
    assert first == (0 | (1 << 8))
    for n in range(41):
        e = 0.1 + 0.37 * n
        cH = (float(a[0] + dist), float(a[1] + e), float(a[2]))
        d0, d1, dz = float(a[0]) - cH[0], float(a[1]) - cH[1], float(a[2]) - cH[2]
        d2 = dot3(d0, d0, d1, d1, dz, dz)
        S = math.sqrt(d2)
        for k in range(-6, 7):
            rH = _step(S - best, k)
            clr = S - rH
            if not clr < best or prune_skips(best, rH, d2) != want_skip:
                continue
            spheres = head + [(FRAME_WORLD, 1, cH, rH)]
            got, pair, np_ = oracle.clearance(P, spheres, [], None, x0)
            assert np_ == 5 and pair == (0 | (5 << 8)) and got == clr, (got, clr, pair)
            return spheres, dict(dist=dist, e=e, k=k, best=best, first_pair=first, clearance=clr, pair=pair, rsum=rH, d2=d2)
    return None


def prune_bound(P, spheres, boxes, allowed):
    """ccmp_scene.cpp's bound on the largest `best + rsum` any state can produce: the largest distance between two tested proxies'
    centres (every centre within its reach of the origin) plus the largest sum of radii in the pair table"""
    def norm(v):
        return float(np.sqrt((np.asarray(v, dtype=np.float64) ** 2).sum()))

    off = np.ctypeslib.as_array(P.offset).reshape(2, 7, 3)
    ee = np.ctypeslib.as_array(P.ee).reshape(2, 3)
    bR = np.ctypeslib.as_array(P.base_R).reshape(2, 9)
    bp = np.ctypeslib.as_array(P.base_p).reshape(2, 3)
    reach = 0.0
    for f, _, c, _ in spheres:
        if f < 0:
            rc = norm(c)
        else:
            arm, k = divmod(f, 9)
            chain = 0.0 if k == 8 else sum(norm(o) for o in off[arm]) + norm(ee[arm])
            rc = norm(bp[arm]) + norm(bR[arm]) * (chain + norm(c))
        reach = max(reach, rc)
    dmax = 2.0 * reach
    if boxes:
        dmax = max(dmax, max([1.0] + [norm(np.asarray(R).reshape(9)) for _, _, R, _ in boxes]) * (reach + max(norm(c) for _, c, _, _ in boxes)))
    ss, sb = tested_pairs(spheres, boxes, allowed)
    rsum = max([spheres[i][3] + spheres[j][3] for i, j in ss] + [spheres[i][3] for i, _ in sb] + [0.0])
    return dmax + rsum

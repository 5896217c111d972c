"""The forms an in-range Newton round of the STOCK throughput kernels runs — quat_of_t<true> (one case body behind a scalar branch
when the wavefront agrees on the case, the lean root and quotient) and ccmp_sincos_inr (no range test) — on the device, through the
debug library's probe (include/ccmp_debug.h: ccmp_detmath_round_facts_probe), against the forms they stand in for on the device
and against the same arithmetic on the host (numpy's IEEE sums, products, square root and quotient for the quaternion, the det
oracle's ccmp_detmath.h for sine and cosine):

  * a wavefront whose 64 matrices share a case, once per case: it takes that case's body;
  * a wavefront with one lane of another case: it takes the branch-free text;
  * a wavefront with NaN matrices and out-of-range angles in lanes that are told not to store: they leave no trace, the other
    lanes' results are right whichever path the wavefront took;
  * angles from 0 to 512 + 1e-5 of either sign, multiples of pi / 2 and their neighbours by one ulp among them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from closed_chain_motion_planner_amd import Context, _lib
ctx = Context(0)
d = np.load(sys.argv[2])
m, y, store = (torch.as_tensor(d[k]).cuda() for k in ("m", "y", "store"))
n = len(d["y"])
out = torch.full((n, 13), -7.0, dtype=torch.float64, device="cuda")
assert _lib.lib().ccmp_detmath_round_facts_probe(ctx.handle, m.data_ptr(), y.data_ptr(), store.data_ptr(), out.data_ptr(), n - 1, None) == -1  # CCMP_EINVAL
_lib.check(_lib.lib().ccmp_detmath_round_facts_probe(ctx.handle, m.data_ptr(), y.data_ptr(), store.data_ptr(), out.data_ptr(), n, None), "probe")
torch.cuda.synchronize()
np.save(sys.argv[3], out.cpu().numpy())
"""


def _rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)


def _kase(m):
    tr = (m[:, 0] + m[:, 4]) + m[:, 8]
    i = np.where(m[:, 4] > m[:, 0], 1, 0)
    mii = np.where(i == 1, m[:, 4], m[:, 0])
    i = np.where(m[:, 8] > mii, 2, i)
    return np.where(tr > 0.0, 3, i)


def _quat_host(m):
    """Eigen's Quaterniond(Matrix3d) as ccmp_kin.h: quat_of writes it: IEEE operations one by one, so numpy gives its bits"""
    tr = (m[:, 0] + m[:, 4]) + m[:, 8]
    k = _kase(m)
    arg = np.select([k == 3, k == 0, k == 1], [tr + 1.0, ((m[:, 0] - m[:, 4]) - m[:, 8]) + 1.0, ((m[:, 4] - m[:, 8]) - m[:, 0]) + 1.0],
                    ((m[:, 8] - m[:, 0]) - m[:, 4]) + 1.0)
    t = np.sqrt(arg)
    h, f = 0.5 * t, 0.5 / t
    d1, d2, d3 = (m[:, 7] - m[:, 5]) * f, (m[:, 2] - m[:, 6]) * f, (m[:, 3] - m[:, 1]) * f
    s1, s2, s3 = (m[:, 3] + m[:, 1]) * f, (m[:, 6] + m[:, 2]) * f, (m[:, 7] + m[:, 5]) * f
    pick = lambda a3, a0, a1, a2: np.select([k == 3, k == 0, k == 1], [a3, a0, a1], a2)
    return np.stack([pick(d1, h, s1, s2), pick(d2, s1, h, s3), pick(d3, s2, s3, h), pick(h, d1, d2, d3)], axis=1)


def _angles(rng, n):
    pi2 = np.pi / 2
    mult = np.arange(0, 327) * pi2  # up to 513.6: cut below
    mult = mult[mult <= 512.0]
    special = np.concatenate([mult, np.nextafter(mult, np.inf), np.nextafter(mult, -np.inf), [0.0, -0.0, 512.0, 512.0 + 1e-5, 1e-300, 5e-324, 1.0]])
    y = np.concatenate([special, -special, rng.uniform(-512.0 - 1e-5, 512.0 + 1e-5, n)])[:n]
    assert len(y) == n and len(special) * 2 < n
    return y


def test_in_range_forms_on_the_device(ccmp_built, oracle_det, tmp_path):
    from closed_chain_motion_planner_amd import _lib

    assert os.path.exists(_lib.DEBUG_LIBPATH)
    rng = np.random.default_rng(0x0FAC75)
    pool = _rotations(rng, 20000)
    kp = _kase(pool)
    by_case = [pool[kp == k] for k in range(4)]
    assert min(len(b) for b in by_case) >= 256
    waves, expect_path = [], []
    for k in range(4):  # uniform wavefronts, two per case
        for rep in range(2):
            waves.append(by_case[k][64 * rep:64 * rep + 64])
            expect_path.append(k)
    for k in range(4):  # one lane of another case: first, last, in the middle
        w = by_case[k][128:192].copy()
        w[(0, 63, 17, 40)[k]] = by_case[(k + 1) % 4][200]
        waves.append(w)
        expect_path.append(4)
    n_plain = len(waves)
    for k in range(4):  # NaN (and an infinity) in lanes that do not store
        w = by_case[k][192:256].copy()
        w[5], w[6, 4], w[63, 0] = np.nan, np.inf, np.nan
        waves.append(w)
        expect_path.append(None)
    for _ in range(96 - len(waves)):  # whatever random rotations give: mixed wavefronts
        waves.append(_rotations(rng, 64))
        expect_path.append(None)
    m = np.ascontiguousarray(np.concatenate(waves))
    n = len(m)
    assert n == 96 * 64
    y = _angles(rng, n)
    store = np.ones(n, dtype=np.uint8)
    silent = []
    for wv in range(n_plain, n_plain + 4):
        for lane in (5, 6, 63):
            store[64 * wv + lane] = 0
            silent.append(64 * wv + lane)
    y[silent[0]], y[silent[1]], y[silent[2]] = np.nan, 1e300, np.inf
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npy"
    np.savez(inp, m=m, y=y, store=store)
    env = dict(os.environ, CCMP_LIBRARY=_lib.DEBUG_LIBPATH)
    r = subprocess.run([sys.executable, "-c", _PROBE, ROOT, str(inp), str(outp)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(outp)
    live = store == 1
    assert (got[~live] == -7.0).all()  # lanes told not to store left no trace
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    # the in-range forms against the forms they stand in for, on the device
    assert np.array_equal(bits(got[live, 0:4]), bits(got[live, 4:8])), np.argwhere(bits(got[:, 0:4]) != bits(got[:, 4:8]))[:5]
    assert np.array_equal(bits(got[live, 8:10]), bits(got[live, 10:12])), np.argwhere(bits(got[:, 8:10]) != bits(got[:, 10:12]))[:5]
    # ... and against the host
    with np.errstate(all="ignore"):
        host = _quat_host(m)
    assert np.array_equal(bits(got[live, 0:4]), bits(host[live]))
    s, c = C.c_double(), C.c_double()
    exp = np.empty((n, 2))
    for i in np.flatnonzero(live):
        oracle_det.lib.orc_sincos(y[i], C.byref(s), C.byref(c))
        exp[i] = s.value, c.value
    assert np.array_equal(bits(got[live, 8:10]), bits(exp[live]))
    # the path each wavefront took, as quat_of_t<true> reports it from inside the branch it entered (-1 would mean: neither)
    path = got[:, 12].reshape(96, 64)
    for wv, want in enumerate(expect_path):
        lanes = store.reshape(96, 64)[wv] == 1
        assert (path[wv][lanes] == path[wv][lanes][0]).all()
        if want is not None:
            assert path[wv][lanes][0] == want, (wv, want, path[wv][0])
    assert set(np.unique(path[live.reshape(96, 64)])) >= {0.0, 1.0, 2.0, 3.0, 4.0}

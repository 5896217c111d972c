"""The wave-uniform fast paths of the residual's tail (in the throughput kernel CCMP_ATAN_UNIFORM and arm 1's term of the residual
once per round, the opt-in CCMP_LEAN_DIV; closed_chain_motion_planner_amd/build.py): a wavefront takes the lean sequence only when every lane qualifies, the general code
otherwise, and both must give the det oracle's bits.  Batches at throughput-kernel size (> 10 240 samples) in which waves are
mixed — samples far from the manifold (atan off its first interval, several quaternion cases) interleaved with near-manifold
ones — and batches of near-manifold samples only; plus the device's lean quotient against the compiler's over the whole
exponent range."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 12288


def _near_and_far(c, oracle, P, seed):
    """B projected states pushed ~1e-3 rad off the manifold (a few Newton rounds, residual angle far inside atan's first
    interval) and B uniform samples (tens of rounds, any quaternion case, atan on every interval)"""
    qs, oks, _, _ = c.sample_project_batch(seed, 0, 8 * B, want_iters=False)
    on = qs.cpu().numpy()[oks.cpu().numpy() == 1]
    assert len(on) >= B, len(on)
    rng = np.random.default_rng(seed)
    near = on[:B] + rng.normal(0.0, 1e-3, (B, 14))
    far = oracle.ambient_uniform_batch(P, seed + 1, 0, B)
    return np.ascontiguousarray(near), far


@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan"])
def test_mixed_and_uniform_waves_bitwise(gpu_ctx, oracle_det, obj):
    import torch

    c = _constraint(obj, gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    near, far = _near_and_far(c, oracle_det, P, 0xFA57)
    mixed = np.empty_like(near)
    mixed[0::2], mixed[1::2] = near[0::2], far[1::2]  # every wavefront of ten samples holds both kinds
    w = B // 20  # whole wavefronts of one kind, in turn
    blocks = np.stack([near[:10 * w].reshape(w, 10, 14), far[:10 * w].reshape(w, 10, 14)], axis=1).reshape(-1, 14)
    assert len(blocks) > 10240
    for q in (near, mixed, blocks):
        q = np.ascontiguousarray(q)
        q_gpu, ok_gpu, it_gpu = c.project_batch(torch.as_tensor(q).cuda())
        q_cpu, ok_cpu, it_cpu = oracle_det.project_batch(P, q, NCPU)
        assert np.array_equal(q_gpu.cpu().numpy().view(np.uint64), q_cpu.view(np.uint64))
        assert np.array_equal(ok_gpu.cpu().numpy(), ok_cpu)
        assert np.array_equal(it_gpu.cpu().numpy().astype(np.int32), it_cpu)


_DIV_PROBE = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from closed_chain_motion_planner_amd import Context, _lib
ctx = Context(0)
d = np.load(sys.argv[2])
n, den = torch.as_tensor(d["n"]).cuda(), torch.as_tensor(d["d"]).cuda()
out = torch.empty((len(d["n"]), 3), dtype=torch.float64, device="cuda")
_lib.check(_lib.lib().ccmp_detmath_div_probe(ctx.handle, n.data_ptr(), den.data_ptr(), out.data_ptr(), len(d["n"]), None), "div probe")
torch.cuda.synchronize()
np.save(sys.argv[3], out.cpu().numpy())
"""


def test_lean_division_is_the_correctly_rounded_quotient(ccmp_built, tmp_path):
    """ccmp_div_steps (forced on every lane) == n / d wherever both operands are in 2^-300 <= |v| < 2^300; ccmp_div_lean ==
    n / d everywhere — subnormals, zeros, infinities and NaN included (those wavefronts take the compiler's expansion)"""
    from closed_chain_motion_planner_amd import _lib

    assert os.path.exists(_lib.DEBUG_LIBPATH)
    rng = np.random.default_rng(11)
    k = 64 * 1024

    def draw(lo, hi, m):
        v = np.ldexp(rng.uniform(1, 2, m), rng.integers(lo, hi, m))
        return np.where(rng.random(m) < 0.5, -v, v)

    # first half: whole wavefronts in the plain range (the lean path); second half: the whole exponent range with
    # specials sprinkled in (every wavefront falls back)
    n = np.concatenate([draw(-300, 300, k), draw(-1074, 1024, k)])
    d = np.concatenate([draw(-300, 300, k), draw(-1074, 1024, k)])
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.0 ** -1022, 1.0, 2.0 ** -300, 2.0 ** 300])
    idx = k + rng.choice(k, 4096, replace=False)
    n[idx[:2048]] = rng.choice(specials, 2048)
    d[idx[2048:]] = rng.choice(specials, 2048)
    # ends of the plain range, wave-uniform: the largest and smallest operands the lean path accepts
    n[:64], d[:64] = np.nextafter(2.0 ** 300, 0), 2.0 ** -300
    n[64:128], d[64:128] = 2.0 ** -300, np.nextafter(2.0 ** 300, 0)
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npy"
    np.savez(inp, n=n, d=d)
    env = dict(os.environ, CCMP_LIBRARY=_lib.DEBUG_LIBPATH)
    r = subprocess.run([sys.executable, "-c", _DIV_PROBE, ROOT, str(inp), str(outp)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(outp)
    with np.errstate(all="ignore"):
        exp = n / d

    def same(a, b):
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))

    plain = (np.abs(n) >= 2.0 ** -300) & (np.abs(n) < 2.0 ** 300) & (np.abs(d) >= 2.0 ** -300) & (np.abs(d) < 2.0 ** 300)
    assert plain[:k].all() and not plain[k:].all()
    assert same(got[:, 2], exp).all(), "the compiler's quotient is not IEEE"
    assert same(got[:, 1], exp).all(), np.argwhere(~same(got[:, 1], exp))[:5]
    assert same(got[plain, 0], exp[plain]).all(), np.argwhere(plain & ~same(got[:, 0], exp))[:5]

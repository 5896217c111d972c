#!/usr/bin/env python3
"""How many Newton rounds a sample spends far from the manifold — the model behind `fd_head_rounds` (DESIGN_experiments.md §5.6),
from the det oracle alone: no GPU.

    python tools/head_rounds_model.py [fixture=Wine_Bottle] [samples=768] [seed=0xC3]

ccmp_atan's wave-uniform first interval (ccmp_detmath.h, CCMP_ATAN_UNIFORM) holds for a wavefront only while the angular residual
f[1] of every sample it iterates on is below 2 atan(0.4375), about 47 degrees.  For k = 0, 1, 2, ... the script projects the
fixture's uniform samples with max_iter = k, evaluates function() on what comes out, and prints the share of the samples still
iterating after k rounds whose f[1] is at or above that bound.  Where the share has fallen to a per cent or less is where a head
launch of that many rounds leaves the persistent kernel wavefronts that take the short path in nearly every round; the column
"mixed" is the hit rate of a wavefront of ten samples of all ages without a head launch, (1 - far share of sample-rounds)^10."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 24)
BOUND = 2.0 * math.atan(0.4375)


def model(obj, n, seed, threads):
    import numpy as np
    from conftest import load_cfg
    from oracle_binding import Oracle

    O = Oracle("det")
    P = O.problem(load_cfg(obj))
    cap = P.max_iter
    q = O.ambient_uniform_batch(P, seed, 0, n)
    rounds = O.project_batch(P, q, threads)[2]
    shares, far_rounds = [], 0
    for k in range(0, max(KS) + 1):
        P.max_iter = k
        x, _, it = O.project_batch(P, q, threads)
        f = O.function_batch(P, x, threads)
        still = (it == k) & ((f[:, 0] > P.tol_pos) | (f[:, 1] > P.tol_rot))  # did k updates and would do another
        far = still & (f[:, 1] >= BOUND)
        far_rounds += int(far.sum())
        if k in KS:
            shares.append((k, int(still.sum()), float(far.sum()) / max(1, int(still.sum()))))
    P.max_iter = cap
    return rounds, shares, far_rounds


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else "Wine_Bottle"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    seed = int(sys.argv[3], 0) if len(sys.argv) > 3 else 0xC3
    rounds, shares, far_rounds = model(obj, n, seed, max(1, min(16, os.cpu_count() or 1)))
    total = int(rounds.sum()) + n  # every sample's last evaluation is a pass of phase 1 too
    print("%s, %d samples, seed 0x%X: mean %.1f rounds; f[1] >= 2 atan(0.4375) = %.4f rad" % (obj, n, seed, rounds.mean(), BOUND))
    print("| k | still iterating | far share |")
    print("|---|---|---|")
    for k, still, share in shares:
        print("| %d | %d | %.3f |" % (k, still, share))
    far = far_rounds / float(total)
    print("far sample-rounds up to k = %d: %.1f %% of all; a wavefront of ten samples of all ages takes the short path in (1 - %.3f)^10 = %.0f %% "
          "of its rounds" % (max(KS), 100 * far, far, 100 * (1 - far) ** 10))


if __name__ == "__main__":
    main()

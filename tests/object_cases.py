"""Procedural meshes, the fixture workspace and pose sets of the object-checker tests (tests/test_object_*.py, tests/test_gpu_object.py).
Meshes are (M, 9) float64: x0 y0 z0 x1 y1 z1 x2 y2 z2 in the object frame."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def workspace():
    """the six static boxes of the reference's object checker (tests/golden/object_workspace.json): [{"c", "half"}], world axes"""
    with open(os.path.join(GOLDEN, "object_workspace.json")) as f:
        return [{"c": b["c"], "half": b["half"]} for b in json.load(f)["boxes"]]


def box_mesh(hx, hy, hz, centre=(0.0, 0.0, 0.0)):
    """12 triangles"""
    c = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) + np.asarray(centre)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, cc, d in quads:
        tris += [(a, b, cc), (a, cc, d)]
    return np.array([np.concatenate([c[i], c[j], c[k]]) for i, j, k in tris])


def uv_sphere(r, n_lat=8, n_lon=12, centre=(0.0, 0.0, 0.0)):
    """2 n_lon (n_lat - 1) triangles"""
    centre = np.asarray(centre, dtype=np.float64)
    pt = lambda i, j: centre + r * np.array([np.sin(np.pi * i / n_lat) * np.cos(2 * np.pi * j / n_lon), np.sin(np.pi * i / n_lat) * np.sin(2 * np.pi * j / n_lon),
                                             np.cos(np.pi * i / n_lat)])
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = pt(i, j), pt(i, j + 1), pt(i + 1, j + 1), pt(i + 1, j)
            if i > 0:
                tris.append(np.concatenate([a, c, b]))
            if i < n_lat - 1:
                tris.append(np.concatenate([a, d, c]))
    return np.array(tris)


def dumbbell():
    """two spheres of radius 0.06 at x = -0.12 and 0.12 and a bar between them: 2 x 496 + 12 = 1004 triangles"""
    return np.concatenate([uv_sphere(0.06, 9, 31, (-0.12, 0, 0)), uv_sphere(0.06, 9, 31, (0.12, 0, 0)), box_mesh(0.12, 0.015, 0.015)])


def big_sphere(m_about=8600):
    """a UV sphere of radius 0.1 with about m_about triangles"""
    n_lat = max(3, int(np.ceil(np.sqrt(m_about / 4.0))))
    return uv_sphere(0.1, n_lat, 2 * n_lat)


def random_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def random_poses(rng, n, lo=(0.0, -0.6, 1.0), hi=(1.3, 0.6, 1.95)):
    """general poses around the free volume of the fixture workspace: some collide, some do not"""
    p = np.zeros((n, 8))
    p[:, :3] = rng.uniform(lo, hi, size=(n, 3))
    p[:, 3:7] = random_quats(rng, n)
    return p


def soup(rng, M, extent=0.15, size=0.05):
    """M random small triangles within `extent` of the origin"""
    c = rng.uniform(-extent, extent, size=(M, 1, 3))
    return (c + rng.uniform(-size, size, size=(M, 3, 3))).reshape(M, 9)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

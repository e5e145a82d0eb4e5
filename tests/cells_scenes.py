"""Scenes for the muffle direction-cell list tests (test_cells_ref_cpu.py, test_cells_lists_gpu.py): the
smallest at which each path of csrc/art_cells.hip runs. Each maker returns (spheres, aabbs, obbs, targets);
positions, radii and extents are exactly representable in half precision, the targets are float32."""
import numpy as np

import bvh_ref
import cells_ref
from art import abi

f16 = bvh_ref._f16


def records(kind, centres, sizes, rng, tid=-1, rot=None):
    """ABI records of one kind: sizes [n] (sphere radii) or [n, 3] (box half extents)."""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    n = len(centres)
    a = np.zeros(n, {0: abi.SPHERE, 1: abi.AABB, 2: abi.OBB}[kind])
    a["center"] = f16(centres).reshape(n, 3)
    if kind == 0:
        a["radius"] = f16(np.asarray(sizes, np.float64).reshape(n))
    else:
        a["size"] = f16(np.asarray(sizes, np.float64).reshape(n, 3)).reshape(n, 3)
    if kind == 2:
        if rot is None:
            q = rng.normal(size=(n, 4))
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            q[q[:, 3] < 0] *= -1
            rot = q[:, :3]
        a["rot"] = f16(rot).reshape(n, 3)
    a["material"] = f16(rng.uniform(0.0, 1.0, (n, 3))).reshape(n, 3)
    a["audio_target_id"] = tid
    return a


def _cat(parts, kind):
    dt = {0: abi.SPHERE, 1: abi.AABB, 2: abi.OBB}[kind]
    parts = [p for p in parts if p.size]
    return np.concatenate(parts) if parts else np.zeros(0, dt)


EDGE_TARGETS = np.array([[0.0, 0.0, 0.0], [2.0, 1.0, -1.5], [-3.0, 0.5, 2.0], [0.25, -40.0, 0.125]], np.float32)
# the 6 axis, 12 cube-edge and 8 cube-corner directions: seen from target 0, the last 20 straddle face boundaries
DIRS26 = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], np.float64)


class _Builder:
    def __init__(self, seed):
        self.rng, self.part = np.random.default_rng(seed), {0: [], 1: [], 2: []}

    def add(self, kind, c, size, tid=-1, rot=None):
        self.part[kind].append(records(kind, [c], [size], self.rng, tid, rot))

    def ring(self, dist, size, k=0, T=0):
        """One collider along each of the 26 directions from the origin, the kinds in turn; with T, every
        seventh is owned by one of the T targets."""
        for d in DIRS26:
            kind = k % 3
            tid = (k // 7) % T if T and k % 7 == 0 else -1
            self.add(kind, d * dist, size if kind == 0 else [size, 0.5 * size, 0.75 * size], tid)
            k += 1
        return k

    def done(self, targets):
        return _cat(self.part[0], 0), _cat(self.part[1], 1), _cat(self.part[2], 2), np.array(targets, np.float32)


# The hand-placed geometry edges are four scenes, not one: a collider that surrounds a target, or nearly, is
# listed in most of its 6144 cells, and a scene's entry capacity is 128 per (target, collider) pair, at least
# 65 536. Each scene below stays within it, so that no target loses its lists.
def edges_directions():
    """Around 4 targets (target 0 at the origin): colliders of the three kinds along every axis, cube-edge and
    cube-corner direction from target 0, from well under one cell wide (D = 48, size 1/8) over a few cells
    (D = 16, 4) to a fifth of a face (D = 2), some owned by each target; and the degenerate shapes: a point
    sphere, a plate and a rod without thickness, a box given with min > max."""
    b = _Builder(101)
    k = 0
    for dist, size in ((48.0, 0.125), (16.0, 1.0), (4.0, 0.75), (2.0, 0.25)):
        k = b.ring(dist, size, k, T=4)
    b.add(0, [5.0, 6.0, -7.0], 0.0)
    b.add(1, [-6.0, 5.0, 7.0], [2.0, 0.0, 2.0])
    b.add(1, [7.0, -5.0, -6.0], [-1.0, -0.5, -2.0])
    b.add(2, [-7.0, -6.0, 5.0], [0.0, 1.5, 0.0])
    return b.done(EDGE_TARGETS)


def edges_wide(far=84.0):
    """Around one target at the origin (segment bound about `far`: the ring at D = 48): cubes of half 2
    along +x stepping through the distances at which their widened sphere (radius about 4.03) reaches the
    enumeration's `wide` case (gamma >= 1.5) and its `all` case (the sphere holds the target); and unit cubes
    and unrotated unit OBBs stepping through the tangency of their cone with a face plane (a_n^2 = sin^2 gamma:
    the rectangle rule's denominator changes sign; on the opposite face a_n = -sin gamma: the cone just
    behind it)."""
    b = _Builder(102)
    b.ring(48.0, 0.125, T=1)
    for x in 4.0 + 0.0117 * np.arange(9):
        b.add(1, [x, 0.0, 0.0], [2.0, 2.0, 2.0])
    xa, xo = _tangent_x(8.0, np.sqrt(3.0), 3.0, 1e-4, far), _tangent_x(8.0, np.sqrt(3.0), 3.0, 1e-3, far)
    for s in range(-6, 7):
        b.add(1, [xa + s * 0.0078, 8.0, 0.0], [1.0, 1.0, 1.0])
        b.add(2, [0.0, -(xo + s * 0.0078), 8.0], [1.0, 1.0, 1.0], rot=[0.0, 0.0, 0.0])
    return b.done(EDGE_TARGETS[:1])


def edges_inside():
    """Around targets 1, 2, 3: colliders centred on a target (D = 0; one owned by another target), and target 2
    = (-3, 0.5, 2) just inside and just outside a sphere, a box and an OBB (by 0.002)."""
    b = _Builder(103)
    b.ring(16.0, 1.0, T=3)
    b.add(0, EDGE_TARGETS[1], 0.25)
    b.add(1, EDGE_TARGETS[2], [0.5, 0.25, 0.125], tid=0)
    b.add(0, [-3.0, 0.5, 4.0], 2.002)
    b.add(0, [-3.0, 0.5, 0.0], 1.998)
    b.add(1, [-3.0, 3.5, 2.0], [1.0, 3.002, 1.0])
    b.add(1, [-3.0, -2.5, 2.0], [1.0, 2.998, 1.0])
    b.add(2, [-6.0, 0.5, 2.0], [3.002, 1.0, 1.0], rot=[0.0, 0.0, 0.0])
    b.add(2, [0.0, 0.5, 2.0], [2.998, 1.0, 1.0], rot=[0.0, 0.0, 0.0])
    return b.done(EDGE_TARGETS[1:])


def edges_far():
    """Colliders at coordinates near 10^4 beside ones near the origin, around targets 0 and 3: every
    segment bound is about 2 * 10^4, so the rounding margins are units wide (a box 3.5, a sphere 70)."""
    b = _Builder(104)
    for d in DIRS26:
        kind = 1 + int(abs(d).sum()) % 2
        b.add(kind, d * 32.0, [1.0, 0.5, 0.75])
    b.add(0, [5.0, 6.0, -7.0], 0.5)
    b.add(0, [-40.0, 24.0, 8.0], 0.0)
    b.add(0, [9984.0, 0.0, 16.0], 16.0)
    b.add(1, [0.0, -9984.0, 9984.0], [8.0, 32.0, 4.0])
    b.add(2, [-9984.0, 9984.0, -9984.0], [16.0, 2.0, 8.0])
    return b.done(EDGE_TARGETS[[0, 3]])


def _tangent_x(y, r, h1, factor, far):
    """x at which a box of bounding radius r at (x, y, 0) has a_n = x / D equal to sin gamma for a target at
    the origin, gamma = ALPHA_MAX + asin(rho / D) + 1e-3 with the documented rho at a segment bound `far`."""
    rho = r + np.sqrt(3.0) * factor * (far + r + h1 + 1.0) + 2.0 * (2e-6 * far + 1e-6) + 1e-6 * y + cells_ref.cell_slack(r)
    lo, hi = 0.0, y
    for _ in range(60):
        x = 0.5 * (lo + hi)
        D = np.hypot(x, y)
        if x / D < np.sin(cells_ref.ALPHA_MAX + np.arcsin(rho / D) + 1e-3):
            lo = x
        else:
            hi = x
    return float(np.float16(x))


def _own(recs, rng, T, every=9):
    for a in recs:
        m = np.arange(a.size) % every == 0
        a["audio_target_id"][m] = rng.integers(0, T, int(m.sum()))
    return recs


def chunk_seams(n):
    """n random colliders of the three kinds (one 256-collider chunk against several) around 3 targets."""
    rng = np.random.default_rng(200 + n)
    sph, box, obb = _own(bvh_ref.random_scene(n, 300 + n, with_obb=True), rng, 3)
    return sph, box, obb, rng.uniform(-30.0, 30.0, (3, 3)).astype(np.float32)


def sort_paths():
    """Clusters of small colliders seen from the targets through a few cells: 700 spheres, 160 boxes, 40 more
    spheres, beside six walls: lists of at most 1, of 2..64, of 65..256 and of more than 256 entries."""
    rng = np.random.default_rng(2024)
    sph = records(0, np.array([12.0, 0.0, 0.0]) + rng.uniform(-1.2, 1.2, (700, 3)), rng.uniform(0.05, 0.15, 700), rng)
    few = records(0, np.array([0.0, 0.0, -13.0]) + rng.uniform(-0.5, 0.5, (40, 3)), rng.uniform(0.05, 0.15, 40), rng)
    box = records(1, np.array([0.0, 14.0, 0.0]) + rng.uniform(-1.0, 1.0, (160, 3)), rng.uniform(0.05, 0.2, (160, 3)), rng)
    walls = records(1, np.array([[30.0, 0, 0], [-30.0, 0, 0], [0, 30.0, 0], [0, -30.0, 0], [0, 0, 30.0], [0, 0, -30.0]]),
                    np.array([[1.0, 40, 40], [1.0, 40, 40], [40, 1.0, 40], [40, 1.0, 40], [40, 40, 1.0], [40, 40, 1.0]]), rng)
    targets = np.array([[-2.0, 0.5, 0.3], [0.5, -3.0, 0.2], [1.0, 1.0, -2.0]], np.float32)
    return np.concatenate([sph, few]), np.concatenate([box, walls]), np.zeros(0, abi.OBB), targets


def tiny_far_spheres(n, T, seed):
    """n spheres of radius 1/16 .. 1/8 in a shell of radius 60 .. 100 around T targets near the origin."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sph = records(0, d * rng.uniform(60.0, 100.0, (n, 1)), rng.uniform(0.0625, 0.125, n), rng)
    sph["audio_target_id"][::97] = rng.integers(0, T, sph[::97].size)
    targets = rng.uniform(-6.0, 6.0, (T, 3)).astype(np.float32)
    return sph, np.zeros(0, abi.AABB), np.zeros(0, abi.OBB), targets


def nonfinite():
    """chunk_seams(255) with one box of infinite extent."""
    sph, box, obb, targets = chunk_seams(255)
    box["size"][3, 1] = 0x7C00
    return sph, box, obb, targets


def small_resident(n=96, T=4, seed=77, owners=None):
    """A small mixed scene for the resident-store tests: n colliders in a 40-unit box, T targets inside it,
    every fifth collider owned by a target (one of `owners`, default any)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20.0, 20.0, (n, 3))
    s = rng.uniform(0.25, 2.0, (n, 3))
    sph, box, obb = _own(bvh_ref.make_records(c, s, rng, n // 3, n // 3), rng, T, every=5)
    if owners is not None:
        for a in (sph, box, obb):
            m = a["audio_target_id"] >= 0
            a["audio_target_id"][m] = np.asarray(owners)[a["audio_target_id"][m] % len(owners)]
    return sph, box, obb, rng.uniform(-10.0, 10.0, (T, 3)).astype(np.float32)


def sole_blockers():
    """The output-level companion: 3 targets, a shell of 48 disjoint small colliders (16 of each kind) at
    varied distances around them, inside one large box that every ray of the fans hits from within. Returns
    (spheres, aabbs, obbs, targets, origins[2, 3])."""
    rng = np.random.default_rng(48)
    d = cells_ref._fibonacci(48)
    dist = 4.0 + 3.0 * ((np.arange(48) * 7) % 11) / 11.0          # 4 .. 7: disjoint at sizes <= 0.5
    c = d * dist[:, None]
    kinds = np.arange(48) % 3
    sph = records(0, c[kinds == 0], np.full(16, 0.5), rng)
    box = records(1, c[kinds == 1], np.tile([0.5, 0.375, 0.25], (16, 1)), rng)
    obb = records(2, c[kinds == 2], np.tile([0.25, 0.5, 0.375], (16, 1)), rng)
    room = records(1, [[0.0, 0.0, 0.0]], [[24.0, 24.0, 24.0]], rng)
    targets = np.array([[0.0, 0.0, 0.0], [0.75, -0.5, 0.25], [-0.5, 0.5, -0.75]], np.float32)
    origins = np.array([[0.5, 0.25, -0.5], [-0.25, -0.75, 0.5]], np.float32)
    return sph, np.concatenate([box, room]), obb, targets, origins


# name -> maker of the build scenes (the reference is checked alone on each, test_cells_ref_cpu.py)
BUILD_SCENES = {
    "edges": edges_directions,
    "edges-wide": edges_wide,
    "edges-inside": edges_inside,
    "edges-far": edges_far,
    "seam-255": lambda: chunk_seams(255),
    "seam-256": lambda: chunk_seams(256),
    "seam-257": lambda: chunk_seams(257),
    "seam-513": lambda: chunk_seams(513),
    "sort-paths": sort_paths,
    "rows": lambda: tiny_far_spheres(11000, 8, 4),
    "wide-entries": lambda: tiny_far_spheres(65536, 1, 5),
    "resident": small_resident,
}
# Python-side sampling of the two large scenes' coverage check: the fraction of (target, collider) pairs
COVERAGE_FRACTION = {"rows": 0.1, "wide-entries": 0.125}

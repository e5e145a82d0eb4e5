"""The float64 reference of the muffle direction-cell lists (tests/cells_ref.py) on its own, before a
GPU is involved: its cell lookup against a float32 restatement of the device's, its two conditions
(`required`: what a build must list; `justified`: what it may list) shown to be compatible on every
scene of test_cells_lists_gpu.py, what `required` asks for in two plain cases, what the coverage
assertion sees of a narrowed enumeration, and the validity of the sole-blocker fixture."""
import numpy as np
import pytest

import art
from art import abi
from art.synth import fibonacci_directions
import cells_ref as cr
import cells_scenes as cs
import oracle

G = cr.G


def cube_cell_f32(v):
    """cube_cell (csrc/art_trace_muffle.hpp) restated in float32, every operation rounded on its own."""
    v = np.asarray(v, np.float32)
    a = np.abs(v)
    m = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
    k = np.arange(len(v))
    n = a[k, m]
    u, w = v[k, (m + 1) % 3] / n, v[k, (m + 2) % 3] / n
    half_g = np.float32(0.5 * G)
    i = np.clip(np.floor((u + np.float32(1)) * half_g).astype(np.int64), 0, G - 1)
    j = np.clip(np.floor((w + np.float32(1)) * half_g).astype(np.int64), 0, G - 1)
    f = 2 * m + (v[k, m] < 0)
    return (f * G + j) * G + i


def test_cell_of_matches_the_float32_lookup():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(130000, 3)).astype(np.float32)
    d = v.astype(np.float64)
    a = np.abs(d)
    s = np.sort(a, axis=1)
    m = a.argmax(1)
    k = np.arange(len(d))
    uw = np.stack([d[k, (m + 1) % 3], d[k, (m + 2) % 3]], 1) / a[k, m][:, None]
    grid = (uw + 1.0) * (0.5 * G)
    # not within 1e-5 of a cell edge (in the gnomonic coordinate) or of a face boundary
    clear = (np.abs(grid - np.round(grid)) > 1e-5 * 0.5 * G).all(1) & (s[:, 2] - s[:, 1] > 1e-5 * s[:, 2])
    v, d = v[clear][:100000], d[clear][:100000]
    assert len(v) == 100000
    got, want = cr.cell_of(d), cube_cell_f32(v)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert got.min() == 0 and got.max() == cr.CELLS - 1 and np.unique(got).size == cr.CELLS
    # the convention at a glance: +x face centre, then one cell towards +y (i) and one towards +z (j)
    assert cr.cell_of([1.0, 0.01, 0.01]) == (0 * G + 16) * G + 16
    assert cr.cell_of([1.0, 0.07, 0.01]) == (0 * G + 16) * G + 17 and cr.cell_of([1.0, 0.01, 0.07]) == (0 * G + 17) * G + 16
    assert cr.cell_of([-1.0, 0.01, 0.01]) == (1 * G + 16) * G + 16 and cr.cell_of([0.01, 0.01, -1.0]) == (5 * G + 16) * G + 16


def test_cones_hold_their_cells():
    """Every direction of a cell lies within the cell's cone (axis, alpha) of the reference's own table."""
    rng = np.random.default_rng(4)
    d = rng.normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = cr.cell_of(d)
    ang = np.arccos(np.clip((d * cr.CONE_AXIS[c]).sum(1), -1.0, 1.0))
    assert (ang <= cr.CONE_ALPHA[c] + 1e-12).all()
    assert 0.03 < cr.ALPHA_MAX < 0.05


def pairs_of(ref, name, t, rng):
    """The colliders whose coverage is checked for target t: every finite one it does not own, or the
    scene's random fraction of them (cells_scenes.COVERAGE_FRACTION)."""
    sh = ref.shapes
    gs = np.nonzero((sh.tid != t) & sh.finite())[0]
    frac = cs.COVERAGE_FRACTION.get(name, 1.0)
    return gs if frac >= 1.0 else gs[rng.random(gs.size) < frac]


@pytest.mark.parametrize("name", list(cs.BUILD_SCENES))
def test_required_is_justified(name):
    """required(t, g) lies within the justified cells, with the segment bound taken as the float64 distance
    to the farthest corner of the colliders' exact box times 1.001 (not above what a build stores) and the
    factor as the build's documented constant: a build can meet both GPU assertions at once."""
    sph, box, obb, targets = cs.BUILD_SCENES[name]()
    ref = cr.Ref(sph, box, obb, targets)
    sh = ref.shapes
    lo, hi = ref.scene_box()
    rng = np.random.default_rng(1)
    checked = 0
    for t in range(len(targets)):
        gs = pairs_of(ref, name, t, rng)
        far = ref.far64(t, lo, hi) * 1.001
        pairs, dmin = ref.required_many(t, gs)
        g, cell = pairs // cr.CELLS, pairs % cr.CELLS
        assert np.array_equal(np.unique(g), gs), "every collider requires at least one cell"
        factor = np.array([cr.FACTOR[0], cr.FACTOR[1], cr.FACTOR[2]])[sh.kind[g]]
        ok = ref.justified(t, cell, g, factor, far)
        assert ok.all(), [(t, int(a), int(b)) for a, b in zip(g[~ok][:8], cell[~ok][:8])]
        # and the near bound a build may store lies below every sample: D - rho_hi <= dmin
        D = np.linalg.norm(sh.centre[gs] - ref.targets[t], axis=1)
        fac = np.array([cr.FACTOR[0], cr.FACTOR[1], cr.FACTOR[2]])[sh.kind[gs]]
        assert (D - ref.rho_hi(gs, fac, far) <= dmin + 1e-9).all()
        # the nearest point is among the samples: dmin is the distance to the shape itself
        assert np.allclose(ref.dmin_many(t, gs), dmin, rtol=1e-12, atol=1e-12)
        checked += pairs.size
    assert checked > 0


def test_the_wide_scene_reaches_its_branches():
    """The sweeps of cells_scenes.edges_wide straddle the thresholds they are placed for, by the documented
    rho (without the 1.001 of rho_hi) at the float64 segment bound: cubes that hold the target (`all`), cubes
    with gamma >= 1.5 that do not (`wide`) and cubes just under it; and, for the +x face (boxes) and the -y
    face (OBBs), cones whose a_n^2 - sin^2 gamma lies above 1e-3, in (0, 1e-3] and below 0."""
    sph, box, obb, targets = cs.edges_wide()
    ref = cr.Ref(sph, box, obb, targets)
    sh = ref.shapes
    far = ref.far64(0, *ref.scene_box()) * 1.001
    assert abs(far - 84.0) < 1.0   # (what the scene's maker assumed)
    factor = np.array([cr.FACTOR[0], cr.FACTOR[1], cr.FACTOR[2]])[sh.kind]
    g = np.arange(sh.n)
    rho = ref.rho_hi(g, factor, far) / 1.001
    w = sh.centre - ref.targets[0]
    D = np.linalg.norm(w, axis=1)
    with np.errstate(invalid="ignore"):
        gamma = cr.ALPHA_MAX + np.arcsin(np.minimum(1.0, rho / D)) + 1e-3
    big = (sh.kind == cr.AABB) & (sh.half[:, 0] == 2.0)
    assert big.sum() == 9
    holds = D <= rho * 1.0001
    assert (big & holds).any() and (big & ~holds & (gamma >= 1.5)).any() and (big & ~holds & (gamma < 1.5) & (gamma > 1.4)).any()
    unit = (sh.half == 1.0).all(1)
    for kind, axis, sign in ((cr.AABB, 0, 1.0), (cr.OBB, 1, -1.0)):
        m = unit & (sh.kind == kind)
        assert m.sum() == 13
        den = (sign * w[m, axis] / D[m]) ** 2 - np.sin(gamma[m]) ** 2
        assert (den > 1e-3).any() and ((den > 0) & (den <= 1e-3)).any() and (den < 0).any(), den


def test_a_small_sphere_requires_one_to_four_cells():
    """A sphere seen under an angular radius well below one cell's: 1 cell, or up to 4 at a cell corner."""
    rng = np.random.default_rng(6)
    d = rng.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[0] = [1.0, 0.0, 0.0]                       # a cell corner of the +x face: 4 cells
    d[1] = [1.0, 1.0, 1.0] / np.sqrt(3.0)        # a cube corner: 3 faces
    sph = cs.records(0, d * 64.0, np.full(300, 0.0625), rng)
    ref = cr.Ref(sph, np.zeros(0, abi.AABB), np.zeros(0, abi.OBB), np.zeros((1, 3), np.float32))
    counts = [ref.required(0, g)[0].size for g in range(300)]
    assert min(counts) == 1 and max(counts) <= 4, (min(counts), max(counts))
    assert counts[0] == 4 and counts[1] == 3
    assert np.bincount(counts)[1] > 150  # most lie inside one cell
    cells, dmin = ref.required(0, 5)
    assert abs(dmin - (np.linalg.norm(ref.shapes.centre[5]) - 0.0625)) < 1e-9


def test_a_target_inside_a_shape_requires_every_cell():
    rng = np.random.default_rng(7)
    t = np.array([[1.0, 2.0, 3.0]], np.float32)
    sph = cs.records(0, [[1.5, 2.0, 3.0], [4.0, 2.0, 3.0]], [1.0, 1.0], rng)
    box = cs.records(1, [[1.0, 2.5, 3.0], [1.0, 6.0, 3.0]], [[0.25, 0.75, 0.25]] * 2, rng)
    obb = cs.records(2, [[1.0, 2.0, 3.5], [1.0, 2.0, 9.0]], [[0.125, 0.125, 1.0]] * 2, rng, rot=[[0.0, 0.3827, 0.0]] * 2)
    ref = cr.Ref(sph, box, obb, t)
    for g in (0, 2):
        cells, dmin = ref.required(0, g)
        assert cells.size == 6 * 32 * 32 and dmin == 0.0 and np.array_equal(cells, np.arange(cr.CELLS))
    for g in (1, 3, 5):
        cells, dmin = ref.required(0, g)
        assert 0 < cells.size < cr.CELLS // 4 and dmin > 0
    # the OBB is turned by 45 degrees about y: its long local z axis points along world (-1, 0, 1) / sqrt 2 or
    # (1, 0, 1) / sqrt 2, and the target (0, 0, -0.5) from its centre lies inside only for the unturned box
    cells, dmin = ref.required(0, 4)
    assert dmin > 0 and cells.size < cr.CELLS


def test_what_the_coverage_assertion_sees_of_a_narrowed_enumeration():
    """The enumeration visits, per face, the cell rectangle of the pair's cone (face_range in art_cells.hip:
    the conic bounds of a cone of half-angle gamma = alpha_max + asin(rho / D) + 1e-3, widened by one cell
    each way), restated here in float64 (cells_ref.face_rects). On the geometry-edge scene:

    the documented rule holds every required cell, with the one-cell margin and, in exact arithmetic, also
    without it: gamma already carries alpha_max (a whole cell's half-diagonal) and rho the motion slack, so
    the margin guards the float rounding of the bounds and nothing else. Deleting it alone is therefore not
    visible to samples of the shapes, here or on the device;

    a cone that is under-wide is visible: with gamma short by one cell (2 / G rad) of the bare shape's
    angular radius, the tangent-rim samples of the wider colliders fall outside the rectangles, and the
    one-cell margin hides that for some pairs but not for all."""
    sph, box, obb, targets = cs.edges_directions()
    ref = cr.Ref(sph, box, obb, targets)
    sh = ref.shapes
    missing = {k: [] for k in ("rule", "rule-no-margin", "narrow", "narrow-no-margin")}
    pairs = 0
    for t in range(len(targets)):
        for g in np.nonzero(sh.tid != t)[0]:
            cells, dmin = ref.required(t, g)
            w = sh.centre[g] - ref.targets[t]
            D = np.linalg.norm(w)
            rho = sh.r[g] + cr.cell_slack(sh.r[g])          # (without the rounding margins: a lower bound)
            if D <= rho:
                continue                                    # listed in every cell
            pairs += 1
            beta, bare = np.arcsin(rho / D), np.arcsin(sh.r[g] / D)
            for key, gamma, margin in (("rule", cr.ALPHA_MAX + beta + 1e-3, 1), ("rule-no-margin", cr.ALPHA_MAX + beta + 1e-3, 0),
                                       ("narrow", bare - 2.0 / G, 1), ("narrow-no-margin", bare - 2.0 / G, 0)):
                if gamma <= 0:
                    continue
                lost = np.setdiff1d(cells, cr.rect_cells(cr.face_rects(w / D, gamma, margin)))
                if lost.size:
                    missing[key].append((t, int(g), int(lost[0])))
    assert pairs > 400
    assert not missing["rule"], missing["rule"][:8]
    assert not missing["rule-no-margin"], missing["rule-no-margin"][:8]
    assert len(missing["narrow-no-margin"]) > len(missing["narrow"]) > 0, {k: len(v) for k, v in missing.items()}


# ------------------------------------------------------------------------------------------------
# The sole-blocker fixture of test_cells_lists_gpu.py::test_sole_blockers_outputs
# ------------------------------------------------------------------------------------------------
def sole_blocker_frame(sph, box, obb, targets, origins, R=512):
    scene = art.Scene(dirs=fibonacci_directions(R), targets=targets, spheres=sph, aabbs=box, obbs=obb)
    params = art.FrameParams(max_hits_per_ray=1, max_ray_life=1e4, max_muffle_hit_distance=1e5,
                             stages=abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_REDUCE)
    return scene, params, origins


def test_every_shell_collider_is_some_rays_sole_blocker():
    """The fixture is valid only if removing any single shell collider changes the oracle's muffle counts:
    each of the 48 then decides at least one muffle ray alone, so a list that misses it, or a walk that
    steps over it, changes the outputs."""
    sph, box, obb, targets, origins = cs.sole_blockers()
    assert (sph.size, box.size, obb.size) == (16, 17, 16)

    def muffle(s, b, o):
        scene, params, org = sole_blocker_frame(s, b, o, targets, origins)
        out = art.FanOutputs(2, 512, 1, scene.T, params.thread_count)
        oracle.run(scene, params, org, out)
        return out.muffle.copy()

    full = muffle(sph, box, obb)
    assert (full != 0).any()
    same = []
    for k in range(16):
        for kind, (s, b, o) in enumerate(((np.delete(sph, k), box, obb), (sph, np.delete(box, k), obb), (sph, box, np.delete(obb, k)))):
            if np.array_equal(muffle(s, b, o), full):
                same.append((kind, k))
    assert not same, same

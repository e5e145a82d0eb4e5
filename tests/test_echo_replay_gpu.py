"""Bounce-0 echo rays decided from the nearest cast's leaf records (DESIGN.md §3, §5 item 8 "replay").

In the one-hit fused plan the bounce-0 cast (nearest_first_kernel<..., LOG>) records the BVH leaves it
tests for each ray, and the echo waves of echo_muffle_kernel test those leaves against the echo
segment instead of traversing the tree. A ray keeps the echo traversal when its record overflowed
(more than K_LOG leaves), when its hit lies past the reach the logging margins were sized for
(best * |d|_1 > CAP_FRAC * the L1 diagonal of the BVH root's box) or when its direction is zero or
non-finite. art_debug_echo_decided reports how many echo rays of the last frame went each way.

Every case compares the echo halves (and every other output) with the oracle byte for byte and
asserts the (replayed, traversed) counts it was built for, so no case can pass on the other path:
exact numbers for the hand-built scenes, "both non-zero" for the seeded sweep. The scene builders
and the oracle's share of each case need no GPU; `reference` asserts on the oracle's output alone
that a case holds what its name says (hits, misses, blocked and returned echoes).
"""
from functools import partial

import numpy as np
import pytest

import art
from art import abi
import oracle
from test_broadphase_gpu import aabbs, f16bits, fib_dirs, spheres
from test_plan_matrix_gpu import check_equal, stale_outputs

pytestmark = pytest.mark.gpu

K_LOG = 15       # kLogK (art_trace_rays.hpp): leaf ids a ray's record holds
CAP_FRAC = 0.3   # kLogCapFrac: share of the root box's L1 diagonal that best * |d|_1 may reach
K_BVH_LEAF = 4   # kBvhLeaf: colliders per leaf

TARGETS = np.array([[3, 2, -4], [-9, 5, 6], [8, -7, 1], [-2, -3, 9]], np.float32)


def params_one_hit():
    return art.FrameParams(max_hits_per_ray=1, max_ray_life=1e4, max_muffle_hit_distance=1e5,
                           stages=abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_REDUCE)


def dirs_of(v):
    """Ray directions as the scene stores them (half3 bits) and as the kernels read them (float32)."""
    bits = f16bits(np.asarray(v, np.float32)).reshape(-1, 3)
    return bits, bits.view(np.float16).astype(np.float32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def xcap_of(scene):
    """CAP_FRAC * the L1 diagonal of the union of the sphere and AABB bounds (the BVH root's box of an
    OBB-free scene)."""
    lo, hi = [], []
    if scene.spheres.size:
        c = scene.spheres["center"].view(np.float16).astype(np.float32).reshape(-1, 3)
        r = np.abs(scene.spheres["radius"].view(np.float16).astype(np.float32)).reshape(-1, 1)
        lo.append(c - r), hi.append(c + r)
    if scene.aabbs.size:
        c = scene.aabbs["center"].view(np.float16).astype(np.float32).reshape(-1, 3)
        h = np.abs(scene.aabbs["size"].view(np.float16).astype(np.float32).reshape(-1, 3))
        lo.append(c - h), hi.append(c + h)
    lo, hi = np.concatenate(lo).min(0), np.concatenate(hi).max(0)
    return CAP_FRAC * float((hi - lo).sum())


# ---- the hand-built scenes: (scene, origins, want) with want = (replayed, traversed) or None when the
# ---- counts follow from the oracle's hits (every hit ray replays)

def grazing_scene(seed):
    """A sphere or a box per ray placed tangent to the primary segment, a hair inside or outside of
    it (the offsets straddle the exact tests' rounding and sit well inside one node margin), in front
    of a wall: rays that hit their collider at a glancing angle or pass it and hit the wall. In exact
    arithmetic nothing blocks a bounce-0 echo; the seeds are two of those (of 300 scanned with the
    oracle) where the float tests do block some: 156 behind grazed spheres, 191 behind a grazed box."""
    rng = np.random.default_rng(seed)
    R = 32
    bits, d = dirs_of(unit(np.concatenate([np.ones((R, 1)), rng.uniform(-0.2, 0.2, (R, 2))], axis=1)))
    du = unit(d)
    s = rng.uniform(4.0, 15.0, R).astype(np.float32)
    P = du * s[:, None]  # a point of each ray of the fan at the origin
    perp = np.cross(du, rng.normal(size=(R, 3)))
    perp = unit(perp)
    f = rng.choice([0.98, 0.995, 0.999, 1.0, 1.001, 1.005, 1.02], R).astype(np.float32)
    r = rng.choice([0.25, 0.5, 1.0], R).astype(np.float32)
    ns = R // 2
    sph_c = P[:ns] + perp[:ns] * (r[:ns] * f[:ns])[:, None]
    # boxes: the ray runs along the face y = c_y -+ h (nearly parallel to x)
    sign = rng.choice([-1.0, 1.0], R - ns).astype(np.float32)
    box_c = P[ns:] + np.stack([np.zeros(R - ns), sign * r[ns:] * f[ns:], np.zeros(R - ns)], axis=1).astype(np.float32)
    wall = aabbs(np.array([[20.0, 0, 0]]), np.array([[1.0, 30, 30]]), rng)
    anchor = spheres(np.array([[-200.0, 0, 0]]), np.array([1.0]), rng)  # a wide root box: no hit is past the cap
    scene = art.Scene(dirs=bits, targets=TARGETS,
                      spheres=np.concatenate([spheres(sph_c, r[:ns], rng), anchor]),
                      aabbs=np.concatenate([aabbs(box_c, np.stack([r[ns:]] * 3, axis=1), rng), wall]))
    org = np.array([[0, 0, 0], [0.0078125, -0.00390625, 0.00390625]], np.float32)
    return scene, org, None


def inside_scene():
    """Fan 0 starts inside an AABB (a room with small spheres and boxes in it), fan 1 inside a sphere:
    every ray leaves its enclosing collider through a far face, and the echo segment starts inside it."""
    rng = np.random.default_rng(6)
    bits = fib_dirs(32)
    room = aabbs(np.array([[0.0, 0, 0]]), np.array([[3.0, 3, 3]]), rng)
    c = rng.uniform(-2.5, 2.5, (20, 3)).astype(np.float32)
    c = c[np.linalg.norm(c - np.array([0.5, 0.25, -0.5]), axis=1) > 1.0][:12]
    inner_s = spheres(c[:6], rng.uniform(0.2, 0.5, 6), rng)
    inner_b = aabbs(c[6:], rng.uniform(0.2, 0.5, (len(c) - 6, 3)), rng)
    ball = spheres(np.array([[10.0, 0, 0]]), np.array([2.0]), rng)
    shell = aabbs(np.array([[10.0, 0, 0]]), np.array([[4.0, 4, 4]]), rng)  # around the ball and fan 1's origin
    anchor = spheres(np.array([[-150.0, 0, 0], [150.0, 0, 0]]), np.array([1.0, 1.0]), rng)
    scene = art.Scene(dirs=bits, targets=TARGETS, spheres=np.concatenate([inner_s, ball, anchor]),
                      aabbs=np.concatenate([room, inner_b, shell]))
    org = np.array([[0.5, 0.25, -0.5], [10.5, 0.25, 0.0]], np.float32)
    return scene, org, None


def overlap_scene():
    """Two overlapping colliders at the hit point (a sphere sunk halfway into a wall's face, a box
    flush with it) and a box that starts one half-precision step (2^-10) behind the face."""
    rng = np.random.default_rng(8)
    R = 16
    bits, _ = dirs_of(unit(np.concatenate([np.ones((R, 1)), rng.uniform(-0.3, 0.3, (R, 2))], axis=1)))
    wall = aabbs(np.array([[1.5, 0, 0]]), np.array([[0.5, 4, 4]]), rng)               # face x = 1
    flush = aabbs(np.array([[1.25, 0.5, 0]]), np.array([[0.25, 0.25, 4]]), rng)       # face x = 1 too
    behind = aabbs(np.array([[1.5 + 2.0 ** -10, -0.5, 0]]), np.array([[0.5, 0.25, 4]]), rng)  # face x = 1 + 2^-10
    sunk = spheres(np.array([[1.0, 0, 0.5], [1.0, 0.125, -0.5]]), np.array([0.125, 0.25]), rng)
    anchor = spheres(np.array([[-60.0, 0, 0]]), np.array([1.0]), rng)
    scene = art.Scene(dirs=bits, targets=TARGETS, spheres=np.concatenate([sunk, anchor]),
                      aabbs=np.concatenate([wall, flush, behind]))
    org = np.array([[0, 0, 0], [0.25, 0.25, -0.25]], np.float32)
    return scene, org, None


def overflow_scene():
    """63 spheres in a row and a wall behind them: 64 colliders, 16 leaves. The +x ray of fan 0 runs
    beside the row through every sphere's bounds and misses every sphere, so its cast tests all 16
    leaves before the wall (one more than a record holds): it keeps the echo traversal. Fan 1 starts
    near the wall: its +x ray tests the last leaves only and replays. The other rays miss."""
    rng = np.random.default_rng(9)
    n = 63
    row = spheres(np.stack([0.5 * np.arange(n), np.zeros(n), np.zeros(n)], axis=1), np.full(n, 0.25), rng)
    wall = aabbs(np.array([[33.0, 0, 0]]), np.array([[1.0, 40, 40]]), rng)
    bits, _ = dirs_of([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 1]])
    scene = art.Scene(dirs=bits, targets=TARGETS + np.array([0, 20, 0], np.float32), spheres=row, aabbs=wall)
    assert scene.C == 64 and scene.C // K_BVH_LEAF == K_LOG + 1
    org = np.array([[-1.0, 0.1875, 0.1875], [29.875, 0.1875, 0.1875]], np.float32)
    return scene, org, (1, 1)


def cap_scene():
    """A near sphere and a far wall: the ray that hits the sphere replays, the one that passes it hits
    the wall at 1.7 times the cap and keeps the echo traversal, the third misses."""
    rng = np.random.default_rng(10)
    bits, _ = dirs_of(np.concatenate([[[1.0, 0, 0]], unit([[0.98, 0.2, 0]]), [[-1.0, 0, 0]]]))
    scene = art.Scene(dirs=bits, targets=TARGETS, spheres=spheres(np.array([[3.0, 0, 0]]), np.array([0.5]), rng),
                      aabbs=aabbs(np.array([[60.0, 0, 0]]), np.array([[1.0, 20, 20]]), rng))
    return scene, np.zeros((1, 3), np.float32), (1, 1)


def degenerate_scene():
    """Rays with an infinite, a zero and a NaN direction from inside a box, beside two ordinary ones.
    The reference's slab test reports the infinite ray as a hit at distance 0 (its echo ray counts,
    and keeps the traversal); the zero and the NaN ray hit nothing."""
    rng = np.random.default_rng(12)
    bits, _ = dirs_of([[0, 1, 0], [np.inf, 0, 0], [0, 0, 0], [np.nan, np.nan, np.nan], [0, 0, -1]])
    scene = art.Scene(dirs=bits, targets=TARGETS, spheres=spheres(np.array([[40.0, 0, 0]]), np.array([1.0]), rng),
                      aabbs=aabbs(np.array([[0.0, 0, 0]]), np.array([[5.0, 5, 5]]), rng))
    return scene, np.array([[0.25, 0.5, -0.25]], np.float32), (2, 1)


def all_miss_scene():
    rng = np.random.default_rng(13)
    bits, _ = dirs_of(unit(-np.abs(rng.normal(size=(16, 3))) - 0.05))
    scene = art.Scene(dirs=bits, targets=TARGETS, spheres=spheres(np.array([[30.0, 30, 30], [50.0, 20, 10]]), np.array([1.0, 2.0]), rng),
                      aabbs=aabbs(np.array([[20.0, 40, 25]]), np.array([[2.0, 2, 2]]), rng))
    return scene, np.array([[0, 0, 0], [-1, -2, -3]], np.float32), (0, 0)


SCENES = {"grazing-spheres": partial(grazing_scene, 156), "grazing-box": partial(grazing_scene, 191), "inside": inside_scene, "overlap": overlap_scene, "overflow": overflow_scene,
          "cap": cap_scene, "degenerate": degenerate_scene, "all-miss": all_miss_scene}
_BUILT = {}


def reference(name, builder):
    """(scene, origins, want, oracle outputs with hit results), built once and left unchanged."""
    if name not in _BUILT:
        scene, org, want = builder()
        assert scene.C <= 64 and org.shape[0] <= 2 and scene.R <= 64
        p = params_one_hit()
        ref = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, True, False)
        oracle.run(scene, p, org, ref, threads=4)
        _BUILT[name] = (scene, org, want, ref)
    return _BUILT[name]


def run_fused(ctx, scene, org, flags=0):
    """The frame without hit outputs (the fused plan): outputs, plan, (replayed, traversed)."""
    p = params_one_hit()
    out = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, False, False)
    ctx.set_flags(flags)
    try:
        ctx.run(art.Frame(scene, p, org, out))
        plan = ctx.debug_last_plan()
        decided = ctx.debug_echo_decided()
    finally:
        ctx.set_flags(0)
    assert plan & abi.ART_PLAN_FUSED, abi.plan_names(plan)
    return out, plan, decided


def hit_mask(ref):
    return np.asarray(ref.hit_counts).reshape(-1) > 0


def hit_param(scene, org, ref):
    """best * |d|_1 of every ray (fan-major), from the oracle's hit points (half precision: a few
    parts in a thousand)."""
    d = scene.dirs.view(np.float16).astype(np.float32).reshape(-1, 3)
    hp = np.asarray(ref.hit_points).view(np.float16).astype(np.float32).reshape(org.shape[0], scene.R, 3)
    dist = np.linalg.norm(hp - org[:, None, :], axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (dist / np.linalg.norm(d, axis=1)[None, :] * np.abs(d).sum(1)[None, :]).reshape(-1)


@pytest.mark.parametrize("name", list(SCENES))
def test_hand_built(ctx, name):
    scene, org, want, ref = reference(name, SCENES[name])
    hit = hit_mask(ref)
    echo = np.asarray(ref.echo).reshape(-1)
    if name == "all-miss":
        assert not hit.any() and not echo.any()
    else:
        assert hit.any() and (echo != 0).any(), f"{name}: the oracle returns no echo"
    if name.startswith("grazing"):  # both sides of blocking, behind the kind of collider the case is named for
        blocked = (echo == 0) & hit
        assert blocked.any() and (echo[hit] != 0).any(), f"{name}: no blocked / no returned echo among the hits"
        assert (blocked.reshape(2, -1)[:, :16] if name == "grazing-spheres" else blocked.reshape(2, -1)[:, 16:]).any()
    if name == "overflow":
        assert hit.reshape(2, -1).tolist() == [[True, False, False, False]] * 2
    if name == "degenerate":
        assert hit.tolist() == [True, True, False, False, True]
    if want is None:  # small trees (at most K_LOG leaves), hits well inside the cap: every hit ray replays
        assert (scene.C + K_BVH_LEAF - 1) // K_BVH_LEAF <= K_LOG
        assert np.nanmax(hit_param(scene, org, ref)[hit]) < 0.7 * xcap_of(scene)
        want = (int(hit.sum()), 0)
    elif name in ("overflow", "cap"):  # the hits' distance from the cap: far on the side the case needs
        t, cap = hit_param(scene, org, ref)[hit], xcap_of(scene)
        assert (t < 0.9 * cap).all() if name == "overflow" else sorted(t > 1.5 * cap) == [False, True], (t, cap)
    out, plan, decided = run_fused(ctx, scene, org)
    assert not plan & (abi.ART_PLAN_EX | abi.ART_PLAN_OBB | abi.ART_PLAN_TAB), abi.plan_names(plan)
    assert np.array_equal(np.asarray(out.echo).view(np.uint16), np.asarray(ref.echo).view(np.uint16)), f"{name}: echo halves"
    check_equal(out, ref, name)
    assert decided == want, f"{name}: (replayed, traversed) = {decided}, built for {want}"


def sweep_case(seed, S=8, R=64, ci=2):
    """256 mixed colliders (config 2: spheres and AABBs) in the benchmark scenes' box: a 64-leaf tree."""
    scene, org, _ = art.synth(art.CONFIGS[ci], S=S, R=R, C_scale=256 / 4096, seed=seed)
    assert 250 <= scene.C <= 260 and (scene.obbs.size > 0) == (ci != 2)
    key = ("sweep", seed, S, R, ci)
    if key not in _BUILT:
        ref = stale_outputs(S, R, 1, scene.T, 1, True, False)
        oracle.run(scene, params_one_hit(), org, ref, threads=8)
        _BUILT[key] = ref
    return scene, org, _BUILT[key]


@pytest.mark.parametrize("seed", range(16))
def test_seeded_sweep(ctx, seed):
    scene, org, ref = sweep_case(7000 + seed)
    out, plan, (rep, trav) = run_fused(ctx, scene, org)
    assert not plan & (abi.ART_PLAN_OBB | abi.ART_PLAN_TAB)
    assert np.array_equal(np.asarray(out.echo).view(np.uint16), np.asarray(ref.echo).view(np.uint16))
    check_equal(out, ref, f"seed {seed}")
    assert rep > 0 and trav > 0, (rep, trav)
    assert rep + trav == int(hit_mask(ref).sum())  # every echo ray is decided once


def test_counts_over_fan_chunks_and_other_plans(ctx, monkeypatch):
    """The counts add up over a frame's fan chunks; the counting instantiations, scenes with OBBs (the
    switch is off for them, by measurement) and the multi-hit plans replay nothing and report (0, 0)."""
    scene, org, ref = sweep_case(7000)
    _, _, whole = run_fused(ctx, scene, org)
    _, plan, counted = run_fused(ctx, scene, org, flags=abi.ART_CTX_COUNT_EXECUTED)
    assert plan & abi.ART_PLAN_EX and counted == (0, 0)
    monkeypatch.setenv("ART_FAST_CHUNK_FANS", "3")
    out, plan, chunked = run_fused(ctx, scene, org)
    assert plan & abi.ART_PLAN_CHUNKED and chunked == whole
    check_equal(out, ref, "chunked")
    monkeypatch.delenv("ART_FAST_CHUNK_FANS")
    obb_scene, obb_org, obb_ref = sweep_case(7000, ci=5)
    out, plan, decided = run_fused(ctx, obb_scene, obb_org)
    assert plan & abi.ART_PLAN_OBB and decided == (0, 0)
    check_equal(out, obb_ref, "OBB scene")
    p = params_one_hit()
    p.max_hits_per_ray = 3
    ctx.run(art.Frame(scene, p, org, stale_outputs(8, 64, 3, scene.T, 1, False, False)))
    assert ctx.debug_last_plan() & abi.ART_PLAN_FOLD and ctx.debug_echo_decided() == (0, 0)

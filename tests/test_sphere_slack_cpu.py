"""The sphere lemma behind every sphere rounding margin, checked on the CPU.

The reference's float sphere test (RayIntersectsSphere :323-355, general quadratic) can report a hit for
a ray whose exact line misses the sphere: the discriminant b^2 - 4ac cancels near tangency. The margins
of the broad phase, of the echo replay and of the muffle cell lists all rest on one bound of how far
outside the sphere the reported point P = o + dist * d can lie, `sphere_report_slack(r, D)`
(art_frame_math.hpp, here through art_debug_sphere_slack): the smaller of the square-root form
4e-3 D and the r-aware form 2 * (E / (2 r) + 16 eps (r + D)), E = 13 eps D^2 + 4 eps r^2, for a segment
start within D of the centre.

This file restates the reference test in numpy float32, one IEEE operation per step as tests/unity32.py
does scalar by scalar (here on arrays), aims rays around tangency and measures |P - c| - r in float64
on the float operands. Every reported hit must lie within half of sphere_report_slack: the helper's
safety factor of 2 stays to spare (measured here: the worst hit reaches 0.27 of the slack). The last
test shows why the `min` and the scene's smallest radius are needed.
"""
import ctypes as C

import numpy as np

import art

F = np.float32
EPS = 2.0 ** -24
SAFETY = 2.0  # kSlackSafety

RADII = [2.0 ** e for e in range(-10, 3)]       # 2^-10 .. 4
REACH = [1.0, 3.0, 10.0, 30.0, 100.0, 300.0]    # |oc|
N = 6000                                        # rays per (radius, reach)


def slack_lib(r, D):
    lib = art.load_library()
    out = C.c_float()
    assert lib.art_debug_sphere_slack(None, C.c_float(r), C.c_float(D), C.byref(out), None) == 0
    return float(out.value)


def slack_forms(r, D):
    """(square-root form, r-aware form) in float64."""
    e = EPS * (13.0 * D * D + 4.0 * r * r)
    return 4e-3 * D, SAFETY * (e / (2.0 * r) + 16.0 * EPS * (r + D))


def dot32(a, b):
    return F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])


def ray_sphere32(o, d, c, r):
    """unity32.ray_sphere on arrays of rays (components as lists of float32 arrays): (hit, dist)."""
    oc = [F(o[k] - c[k]) for k in range(3)]
    a = dot32(d, d)
    b = F(F(2) * dot32(oc, d))
    cc = F(dot32(oc, oc) - F(r * r))
    disc = F(F(b * b) - F(F(F(4) * a) * cc))
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
        t0 = F(F(F(-b) - sq) / F(F(2) * a))
        t1 = F(F(F(-b) + sq) / F(F(2) * a))
    ok = disc >= 0
    dist = np.where(t0 >= 0, t0, t1)
    return ok & ((t0 >= 0) | (t1 >= 0)), dist


def sample(r, reach, rng, n=N):
    """n rays from distance `reach` of a sphere of radius r, aimed at perpendicular distance
    r * (1 +- k 2^-j) of its centre: (excess |P - c| - r of every reported hit, their |oc|)."""
    c = rng.uniform(-100, 100, (n, 3)).astype(np.float32)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c.astype(np.float64) + reach * u).astype(np.float32)
    w = np.cross(u, rng.normal(size=(n, 3)))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    k = rng.integers(0, 4, n)
    j = rng.integers(1, 24, n)
    sign = rng.choice([-1.0, 1.0], n)
    p = r * (1.0 + sign * k * 2.0 ** -j)
    aim = c.astype(np.float64) + p[:, None] * w
    d = aim - o.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # the casts' directions are half3 values of any length, the echo and muffle rays' normalized float32
    d = (d * rng.choice([0.5, 1.0, 1.0, 2.0], n)[:, None]).astype(np.float32)
    rr = np.full(n, r, np.float32)
    hit, dist = ray_sphere32([o[:, i] for i in range(3)], [d[:, i] for i in range(3)], [c[:, i] for i in range(3)], rr)
    hit &= np.isfinite(dist) & (dist >= 0)
    o64, d64, c64 = o.astype(np.float64), d.astype(np.float64), c.astype(np.float64)
    P = o64 + dist.astype(np.float64)[:, None] * d64
    excess = np.linalg.norm(P - c64, axis=1) - float(rr[0])
    D = np.linalg.norm(o64 - c64, axis=1)
    return excess[hit], D[hit]


def test_helper_is_the_documented_formula():
    for r in (2.0 ** -10, 0.25, 1.4, 4.0):
        for D in (1.0, 72.0, 300.0):
            root, aware = slack_forms(r, D)
            assert abs(slack_lib(r, D) - min(root, aware)) <= 1e-5 * min(root, aware)
    # r <= 0 and a non-finite r keep the square-root form
    for r in (0.0, -1.0, float("inf"), float("nan")):
        assert abs(slack_lib(r, 50.0) - 0.2) < 1e-6
    # config 2's smallest sphere at the echo replay's reach, and a typical one
    assert slack_lib(0.25, 72.25) < 0.02 < 0.06 < 4e-3 * 72.25
    assert slack_lib(1.4, 73.4) < 0.004


def test_reported_hits_lie_within_the_slack():
    rng = np.random.default_rng(2024)
    worst = 0.0
    outside = 0
    for r in RADII:
        for reach in REACH:
            excess, D = sample(r, reach, rng)
            assert excess.size > N // 4, (r, reach, excess.size)
            outside += int((excess > 0).sum())
            Dm = float(D.max()) * 1.000001
            bound = slack_lib(r, Dm)
            ratio = float(excess.max()) / bound
            worst = max(worst, ratio)
            print(f"r {r:9.3g} |oc| {reach:5.0f}: {excess.size} hits, max excess {excess.max():.3e}, slack {bound:.3e}, ratio {ratio:.3f}")
            assert ratio <= 1.0 / SAFETY, (r, reach, float(excess.max()), bound)
    print(f"worst excess / slack {worst:.3f}; hits outside their sphere {outside}")
    assert outside > 1000  # the rays do probe the rounding


def test_the_min_and_the_scene_radius_are_needed():
    """Each form is the smaller one somewhere: E / (2 r) grows without bound as r -> 0, the square-root
    form wastes a factor of about sqrt(E) / r once r is not tiny. (r + E / (2 r) >= sqrt(r^2 + E) for
    every r > 0, so the r-aware form at a sphere's own radius cannot be violated; it is violated as
    soon as it is evaluated at a larger radius than the sphere's: hits reported around a sphere of
    radius 2^-10 lie further out than the bound of a sphere of radius 0.25 at the same reach allows.
    Hence the echo replay takes the scene's smallest radius, and the lists each sphere's own.)"""
    r, D = 2.0 ** -10, 100.0
    root, aware = slack_forms(r, D)
    assert aware > 10 * root and abs(slack_lib(r, D) - root) <= 1e-5 * root
    root, aware = slack_forms(1.0, D)
    assert root > 10 * aware and abs(slack_lib(1.0, D) - aware) < 1e-5 * aware
    excess, Dm = sample(r, D, np.random.default_rng(7))
    at_typical_radius = slack_forms(0.25, float(Dm.max()))[1]
    print(f"r 2^-10 |oc| 100: max excess {excess.max():.3e}; r-aware bound at r = 0.25: {at_typical_radius:.3e}")
    assert excess.max() > at_typical_radius
    assert excess.max() <= slack_lib(r, float(Dm.max())) / SAFETY

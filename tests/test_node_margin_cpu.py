"""The per-ray cap of the BVH node margins (the capped node margin), checked on the CPU.

`node_margin_cap(r_min, S_root, om, has_obb, reach)` (art_frame_math.hpp, here through
art_debug_node_margin_cap) bounds a node's margin `fma(factor, om, fscale)` for one ray:

    D = S_root + om
    cap = max(s * sphere_report_slack(r_min, D), 1.01 * kF * D) + kCullSphere * reach,   s = 1,

kF = kCullObb with OBBs in the scene, else kCullBox; +infinity ("no cap") for r_min <= 0 or non-finite
and for a non-finite S_root, om or reach. The tests: the helper is that formula; the degenerate inputs
give "no cap"; it is monotone in om; every hit the float32 restatement of the reference's sphere test
reports outside its sphere lies within cap / s of the sphere, for radii in [r_min, D] and |oc| <= D; and
on seeded scenes no node without a sphere ever sees the cap bind.
"""
import ctypes as C

import numpy as np
import pytest

import art
import bvh_ref
from test_sphere_slack_cpu import sample, slack_forms

EPS = 2.0 ** -24
K_BOX, K_SPHERE, K_OBB = 1e-4, 4e-3, 1e-3   # kCullBox, kCullSphere, kCullObb
S_MULT, GUARD = 1.0, 1.01                   # kNodeCapSlack, kNodeCapGuard

R_MINS = [2.0 ** e for e in range(-10, 3)]  # 2^-10 .. 4
S_ROOTS = [1.0, 7.0, 40.0, 170.0, 600.0]
OMS = [0.0, 0.5, 3.0, 25.0, 100.0, 300.0]


def cap_lib(r_min, s_root, om, has_obb=False, reach=0.0):
    lib = art.load_library()
    out = C.c_float()
    rc = lib.art_debug_node_margin_cap(None, C.c_float(r_min), C.c_float(s_root), C.c_float(om), int(has_obb), C.c_float(reach),
                                       C.byref(out), None)
    assert rc == 0
    return float(out.value)


def cap64(r_min, s_root, om, has_obb=False, reach=0.0):
    """The documented formula in float64."""
    D = s_root + om
    return max(S_MULT * min(slack_forms(r_min, D)), GUARD * (K_OBB if has_obb else K_BOX) * D) + K_SPHERE * reach


def test_helper_is_the_documented_formula():
    for r in R_MINS:
        for s in S_ROOTS:
            for om in OMS:
                for obb in (False, True):
                    for reach in (0.0, 6.2, 90.0):
                        want = cap64(r, s, om, obb, reach)
                        assert abs(cap_lib(r, s, om, obb, reach) - want) <= 1e-5 * want, (r, s, om, obb, reach)
    # config 2's scale: the smallest sphere 0.25 in a box of |x|, |y|, |z| <= ~50, a ray from inside it
    assert 0.05 < cap_lib(0.25, 150.0, 20.0) < 0.2 < K_SPHERE * 100.0


def test_degenerate_inputs_give_no_cap():
    inf, nan = float("inf"), float("nan")
    for r in (0.0, -0.0, -1.0, inf, -inf, nan):
        assert cap_lib(r, 100.0, 10.0) == inf, r
    for bad in (inf, -inf, nan):
        assert cap_lib(0.25, bad, 10.0) == inf     # a non-finite collider makes the root box infinite
        assert cap_lib(0.25, 100.0, bad) == inf    # a non-finite origin
        assert cap_lib(0.25, 100.0, 10.0, False, bad) == inf
    # S_root + om overflowing is a non-finite D as well
    big = float(np.finfo(np.float32).max)
    assert cap_lib(0.25, big, big) == inf
    # and a finite cap is positive
    assert 0.0 < cap_lib(0.25, 100.0, 10.0) < inf


def test_monotone_in_om():
    oms = np.concatenate([[0.0], np.geomspace(1e-3, 300.0, 400)]).astype(np.float32)
    for r in R_MINS:
        for s in S_ROOTS:
            for obb in (False, True):
                caps = np.array([cap_lib(r, s, float(om), obb) for om in oms])
                assert (np.diff(caps) >= 0).all(), (r, s, obb)


@pytest.mark.parametrize("r_min", [2.0 ** -10, 2.0 ** -6, 0.25, 1.0])
def test_reported_hits_lie_within_the_cap(r_min):
    """Spheres of radius r in [r_min, D] tested from |oc| <= D, rays aimed at tangency: the helper's value
    at r_min bounds what every one of them reports (the E / (2 r) part decreases in r, the linear part
    grows and stays under the cap's floor)."""
    rng = np.random.default_rng(int(r_min * 4096) + 5)
    outside = 0
    worst = 0.0
    for D in (10.0, 100.0, 300.0):
        cap = cap_lib(r_min, D, 0.0)
        radii = sorted({r for r in (r_min, 2 * r_min, 8 * r_min, 64 * r_min, 0.5 * D, 0.99 * D) if r_min <= r <= D})
        for r in radii:
            for reach in (0.999 * D, 0.5 * D, 0.1 * D):
                excess, oc = sample(np.float32(r), reach, rng, n=3000)
                assert oc.max() <= D
                if not excess.size:
                    continue
                outside += int((excess > 0).sum())
                worst = max(worst, float(excess.max()) / (cap / S_MULT))
                assert excess.max() <= cap / S_MULT, (r_min, D, r, reach, float(excess.max()), cap)
    print(f"r_min {r_min}: worst excess / (cap / s) {worst:.3f}; hits outside their sphere {outside}")
    assert outside > 1000


# ---------------------------------------------------------------- nodes without a sphere
def _half(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32)


def obb_cull(obbs):
    """Broad-phase bounds of OBB records as prep_obb documents them (float32, each operation rounded; the
    rotated extents need not match the device bit for bit here: the property below is an inequality).
    This is a copy of prep_obb's formulas (art_frame_math.hpp): the library has no host decode that returns
    the records without a device, so a change of prep_obb's scale (|c|_1 + 1.001 |h|_1) or extents has to be
    made here too, or this test checks a stale format."""
    n = obbs.size
    out = np.zeros(n, bvh_ref.REC)
    F = np.float32
    c = _half(obbs["center"]).reshape(n, 3)
    h = np.abs(_half(obbs["size"]).reshape(n, 3))
    q3 = _half(obbs["rot"]).reshape(n, 3).astype(np.float64)
    w = np.sqrt(np.maximum(1.0 - (q3 ** 2).sum(1), 0.0))
    q = np.concatenate([q3, w[:, None]], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)  # [n, i, j]
    A = np.abs(R)
    wext = np.maximum(np.einsum("nij,nj->ni", A, h.astype(np.float64)), np.einsum("nji,nj->ni", A, h.astype(np.float64)))
    h1 = (h[:, 0] + h[:, 1]) + h[:, 2]
    rho = h1 * F(1.001)
    b = np.minimum((wext * 1.0001 + 1e-5 * h1[:, None]).astype(np.float32), rho[:, None])
    a = np.abs(c)
    scale = ((a[:, 0] + a[:, 1]) + a[:, 2]) + rho
    out["lo"], out["hi"] = c - b, c + b
    out["fscale"] = F(K_OBB) * scale
    out["factor"] = F(K_OBB)
    return out


@pytest.mark.parametrize("with_obb", [False, True], ids=["mixed", "obb"])
def test_cap_never_binds_on_nodes_without_a_sphere(with_obb):
    """A seeded 64-collider scene (spheres and AABBs; with OBBs for the OBB factor): every BVH node whose
    factor is below kCullSphere (no sphere under it) keeps its margin, m_old <= cap, for plain operands
    and for the logging cast's (operand b + reach against cap(b) + kCullSphere * reach). The nodes come
    from the host reference of the build (tests/bvh_ref.py): art_debug_bvh_records reads device memory."""
    sph, box, obb = bvh_ref.random_scene(64, 977, with_obb)
    cull = bvh_ref.cull_bounds(sph, box)
    if with_obb:
        assert obb.size > 0
        cull = np.concatenate([cull, obb_cull(obb)])
    order = bvh_ref.kd_order(cull["lo"], cull["hi"])
    nodes = bvh_ref.build_nodes(cull, order)
    nodes = nodes[np.isfinite(nodes["lo"]).all(1)]   # (hollow nodes hold nothing)
    root = nodes[0]
    s_root = float(np.maximum(np.abs(root["lo"]), np.abs(root["hi"])).astype(np.float32).sum(dtype=np.float32))
    r_min = float(np.abs(_half(sph["radius"])).min())
    plain = nodes[nodes["factor"] < np.float32(K_SPHERE)]
    assert 0 < plain.size < nodes.size   # nodes of both kinds
    # (a mixed tree has few nodes without a sphere: the boxes' and OBBs' own records, the one-member case, as well)
    plain = np.concatenate([plain, cull[cull["factor"] < np.float32(K_SPHERE)]])
    checked = 0
    for om in (0.0, 0.37, 12.0, 150.0, 300.0):
        for reach in (0.0, 6.2, 28.8):
            cap = np.float32(cap_lib(r_min, s_root, om, with_obb, reach))
            operand = np.float32(np.float32(om) + np.float32(reach))
            m_old = (plain["factor"].astype(np.float64) * float(operand) + plain["fscale"].astype(np.float64)).astype(np.float32)
            assert (m_old <= cap).all(), (om, reach, float(m_old.max()), float(cap))
            checked += plain.size
    # and with a smallest radius like config 2's (0.25; this scene's is about 0.05, where the r-aware form
    # gains little) the cap does bind on sphere nodes of this scale: the change is not vacuous
    sphere_nodes = nodes[nodes["factor"] >= np.float32(K_SPHERE)]
    m_sph = sphere_nodes["factor"].astype(np.float64) * 12.0 + sphere_nodes["fscale"].astype(np.float64)
    assert (m_sph > cap_lib(0.25, s_root, 12.0, with_obb)).any()
    print(f"{checked} node margins checked, S_root {s_root:.1f}, r_min {r_min}")

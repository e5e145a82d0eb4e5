"""A plain NumPy restatement of the collider BVH build (csrc/art_bvh.hip), for the structural tests.

Sequential host code written from the documented rules (the "kd leaf order ..." comment blocks of
art_bvh.hip): the broad-phase bounds of spheres and AABBs, the kd leaf order and
the heap-ordered node boxes. It shares no code with the kernels. All arithmetic is np.float32 with
every operation rounded on its own: the library is compiled with -ffp-contract=off (the Makefile's
CXXFLAGS apply to every csrc/*.hip, art_bvh.hip included; only the scheduler option is cleared for
that file, and art_frame_math.hpp, where the bounds are computed, also carries `#pragma clang fp
contract(off)`), so the device forms no fused multiply-adds and the results are comparable bit for bit.

Minima and maxima are taken on an order-preserving integer image of the floats (-0.0 below +0.0, as
the device's v_min_f32 / v_max_f32 and its integer atomics order them); the bounds never hold a NaN.

Records are the 32-byte CullRec as it lies in memory: lo.xyz, fscale, hi.xyz, factor (REC).
"""
import numpy as np

REC = np.dtype([("lo", "<f4", 3), ("fscale", "<f4"), ("hi", "<f4", 3), ("factor", "<f4")])
FLT_MAX = np.finfo(np.float32).max
SPHERE_FACTOR = np.float32(4e-3)
BOX_FACTOR = np.float32(1e-4)
LEAF = 4                  # colliders per leaf
SAH_MAX_COLLIDERS = 1 << 14  # the surface-area rule: scenes up to this size ...
SAH_MAX_SEGS = 64            # ... on levels of at most this many segments


def f32_key(v: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 image of float32 values (the radix key: -0.0 sorts before +0.0)."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def f32_unkey(k: np.ndarray) -> np.ndarray:
    k = np.ascontiguousarray(k, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k)
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


def _half(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32)


def _min(a, b):
    return f32_unkey(np.minimum(f32_key(a), f32_key(b)))


def _max(a, b):
    return f32_unkey(np.maximum(f32_key(a), f32_key(b)))


def cull_bounds(spheres: np.ndarray, aabbs: np.ndarray) -> np.ndarray:
    """Broad-phase bounds of the half-precision sphere and AABB records, spheres first (prep_sphere,
    prep_aabb)."""
    ns, na = spheres.size, aabbs.size
    out = np.zeros(ns + na, REC)
    with np.errstate(all="ignore"):
        if ns:
            c = _half(spheres["center"]).reshape(ns, 3)
            ra = np.abs(_half(spheres["radius"]).reshape(ns))
            a = np.abs(c)
            scale = ((a[:, 0] + a[:, 1]) + a[:, 2]) + ra
            fin = np.isfinite(c).all(axis=1) & np.isfinite(ra)
            o = out[:ns]
            o["lo"] = np.where(fin[:, None], c - ra[:, None], -np.inf)
            o["hi"] = np.where(fin[:, None], c + ra[:, None], np.inf)
            o["fscale"] = np.where(fin, SPHERE_FACTOR * scale, np.float32(0))
            o["factor"] = SPHERE_FACTOR
        if na:
            c = _half(aabbs["center"]).reshape(na, 3)
            h = _half(aabbs["size"]).reshape(na, 3)
            mn, mx = c - h, c + h
            a, b = np.abs(c), np.abs(h)
            scale = ((((a[:, 0] + a[:, 1]) + a[:, 2]) + b[:, 0]) + b[:, 1]) + b[:, 2]
            fin = np.isfinite(c).all(axis=1) & np.isfinite(h).all(axis=1)
            o = out[ns:]
            o["lo"] = np.where(fin[:, None], _min(mn, mx), -np.inf)
            o["hi"] = np.where(fin[:, None], _max(mn, mx), np.inf)
            o["fscale"] = np.where(fin, BOX_FACTOR * scale, np.float32(0))
            o["factor"] = BOX_FACTOR
    assert out["lo"].dtype == np.float32
    return out


def capacity(n: int) -> int:
    """Leaf positions of the complete 4-ary tree over n colliders: 4 * 4^(L-1), L the smallest number of
    levels whose 4^(L-1) leaves hold ceil(n / 4) groups."""
    w = 1
    while w < (n + LEAF - 1) // LEAF:
        w *= 4
    return LEAF * w


def centres(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        c = np.float32(0.5) * (np.asarray(lo, np.float32) + np.asarray(hi, np.float32))
    c[~np.isfinite(c)] = FLT_MAX
    return c


def _area(lo_k: np.ndarray, hi_k: np.ndarray) -> np.float32:
    """Half the surface area of the box whose corners are the column-wise min / max of the keys."""
    e = np.fmax(f32_unkey(hi_k.max(axis=0)) - f32_unkey(lo_k.min(axis=0)), np.float32(0))
    return (e[0] * e[1] + e[1] * e[2]) + e[2] * e[0]


def kd_order(lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The leaf order of n colliders with bounds lo, hi ([n, 3] float32): position -> collider index."""
    lo = np.ascontiguousarray(lo, np.float32).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, np.float32).reshape(-1, 3)
    n = lo.shape[0]
    c = centres(lo, hi)
    keys = f32_key(c)
    lo_k, hi_k = f32_key(lo), f32_key(hi)
    P = [np.argsort(keys[:, x], kind="stable") for x in range(3)]  # ties in id order
    pos = np.arange(n)
    lg_cap = capacity(n).bit_length() - 1
    with np.errstate(all="ignore"):
        for lg in range(lg_cap, 2, -1):
            seg, half = 1 << lg, 1 << (lg - 1)
            nseg = (n + seg - 1) >> lg
            a0 = np.arange(nseg) << lg
            cnt = np.minimum(seg, n - a0)
            split = cnt > half
            ax = np.full(nseg, -1)
            if n <= SAH_MAX_COLLIDERS and nseg <= SAH_MAX_SEGS:  # the cheapest halves by surface area
                for s in np.nonzero(split)[0]:
                    best = np.float32(np.inf)
                    for x in range(3):
                        left = P[x][a0[s]:a0[s] + half]
                        right = P[x][a0[s] + half:a0[s] + cnt[s]]
                        cost = (_area(lo_k[left], hi_k[left]) * np.float32(half)
                                + _area(lo_k[right], hi_k[right]) * np.float32(cnt[s] - half))
                        if cost < best:  # (a non-finite cost never wins)
                            best, ax[s] = cost, x
            # otherwise the axis the segment's centres extend furthest on
            ext = [c[P[x][a0 + cnt - 1], x] - c[P[x][a0], x] for x in range(3)]
            wide, best = np.zeros(nseg, int), ext[0].copy()
            for x in (1, 2):
                w = ext[x] > best
                wide[w], best[w] = x, ext[x][w]
            ax = np.where(split & (ax < 0), wide, ax)
            # the chosen array's first half is the left set; segments that fit their left half stay
            s_of, in_left = pos >> lg, (pos & (seg - 1)) < half
            side = np.ones(n, bool)
            for x in range(3):
                m = ax[s_of] == x
                side[P[x][m]] = in_left[m]
            for x in range(3):  # stable partition of every array, segment by segment
                P[x] = P[x][np.argsort(2 * s_of + ~side[P[x]], kind="stable")]
    return P[0]


def build_nodes(cull: np.ndarray, order: np.ndarray) -> np.ndarray:
    """The heap-ordered node records over the colliders' bounds in leaf order (root 0, children of g at
    4g + 1 .. 4g + 4)."""
    order = np.asarray(order, np.int64)
    n = order.size
    rec = np.ascontiguousarray(cull).view(np.float32).reshape(-1, 8)
    cap = capacity(n)
    empty = np.array([np.inf] * 3 + [0.0] + [-np.inf] * 3 + [0.0], np.float32)
    k = np.tile(f32_key(empty), (cap, 1))
    k[:n] = f32_key(rec[order])
    is_min = np.array([1, 1, 1, 0, 0, 0, 0, 0], bool)
    levels = []
    while True:
        g = k.reshape(-1, 4, 8)
        k = np.where(is_min, g.min(axis=1), g.max(axis=1))
        levels.append(k)
        if k.shape[0] == 1:
            break
    nodes = f32_unkey(np.concatenate(levels[::-1])).reshape(-1, 8)
    hollow = nodes[:, 0] > nodes[:, 4]  # no collider below: stored as the box at +infinity, no margin
    nodes[hollow] = np.array([np.inf] * 3 + [0.0] + [np.inf] * 3 + [0.0], np.float32)
    return np.ascontiguousarray(nodes).view(REC).reshape(-1)


def check_tree(cull: np.ndarray, order: np.ndarray, nodes: np.ndarray) -> np.ndarray:
    """Indices of the nodes whose bit patterns differ from build_nodes(cull, order)."""
    want = build_nodes(cull, order).view(np.uint32).reshape(-1, 8)
    got = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.nonzero((got != want).any(axis=1))[0]


# ------------------------------------------------------------------------------------------------
# Test scenes (collider records as the C ABI takes them), shared by the CPU and the GPU module.
# ------------------------------------------------------------------------------------------------
def _f16(x) -> np.ndarray:
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def make_records(centers, sizes, rng, ns: int, na: int):
    """Spheres [0, ns), AABBs [ns, ns + na) and OBBs (the rest) from centres [n, 3] and sizes [n, 3] (a
    sphere's radius is its first size)."""
    from art import abi
    n = len(centers)
    sph, box, obb = np.zeros(ns, abi.SPHERE), np.zeros(na, abi.AABB), np.zeros(n - ns - na, abi.OBB)
    sph["center"] = _f16(centers[:ns]).reshape(ns, 3)
    sph["radius"] = _f16(sizes[:ns, 0])
    box["center"] = _f16(centers[ns:ns + na]).reshape(na, 3)
    box["size"] = _f16(sizes[ns:ns + na]).reshape(na, 3)
    obb["center"] = _f16(centers[ns + na:]).reshape(obb.size, 3)
    obb["size"] = _f16(sizes[ns + na:]).reshape(obb.size, 3)
    q = rng.normal(size=(obb.size, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1
    obb["rot"] = _f16(q[:, :3]).reshape(obb.size, 3)
    for a in (sph, box, obb):
        a["material"] = _f16(rng.uniform(0.0, 1.0, (a.size, 3))).reshape(a.size, 3)
        a["audio_target_id"] = -1
    return sph, box, obb


def _kinds(n: int, with_obb: bool):
    no = n // 3 if with_obb else 0
    ns = (n - no + 1) // 2
    return ns, n - no - ns


def random_scene(n: int, seed: int, with_obb: bool = False):
    """Mixed colliders scattered in a box, a tenth of them large."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-40.0, 40.0, (n, 3))
    s = rng.uniform(0.05, 2.0, (n, 3))
    s[rng.random(n) < 0.1] *= 8.0
    return make_records(c, s, rng, *_kinds(n, with_obb))


def ties_scene(n: int, seed: int):
    """Centres and sizes on a coarse integer lattice: many equal keys and equal costs, zero sizes, and
    -0.0 beside +0.0 in the records. The signed zeros reach the bounds (lo = -0.0 beside lo = +0.0 in
    the unions' minima) but not the sort keys: hi = c + |r|, or max(c - h, c + h), is +0.0 whenever its
    inputs are signed zeros (an OBB's hi = c + b with b >= +0.0 likewise), so lo + hi, and with it a
    centre, is never -0.0 from collider records. Centre keys of -0.0 against +0.0 are covered on the
    host alone (test_bvh_ref_cpu.py, bounds given directly)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-2, 3, (n, 3)).astype(np.float32)
    c[(c == 0) & (rng.random((n, 3)) < 0.5)] = -0.0
    s = rng.integers(0, 3, (n, 3)).astype(np.float32)
    s[(s == 0) & (rng.random((n, 3)) < 0.5)] = -0.0
    return make_records(c, s, rng, *_kinds(n, False))


def line_scene(n: int, seed: int):
    """Every centre on one line along z."""
    rng = np.random.default_rng(seed)
    c = np.empty((n, 3))
    c[:, 0], c[:, 1], c[:, 2] = 1.5, -2.25, rng.uniform(-60.0, 60.0, n)
    return make_records(c, rng.uniform(0.05, 2.0, (n, 3)), rng, *_kinds(n, False))


def nonfinite_scene(n: int, seed: int):
    """A random scene with about 1 % of the colliders given an infinite or NaN centre, radius or size."""
    rng = np.random.default_rng(seed)
    sph, box, obb = random_scene(n, seed)
    bad = np.array([0x7C00, 0xFC00, 0x7E00], np.uint16)  # +inf, -inf, NaN
    for i in rng.choice(n, max(1, n // 100), replace=False):
        a, j = (sph, i) if i < sph.size else (box, i - sph.size)
        field = ("center", "radius" if a is sph else "size")[int(rng.integers(0, 2))]
        if field == "radius":
            a[field][j] = rng.choice(bad)
        else:
            a[field][j, int(rng.integers(0, 3))] = rng.choice(bad)
    return sph, box, obb

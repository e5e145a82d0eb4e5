"""A plain Python/NumPy model of the decisions of the permeation loss pass (csrc/art_permeate.hip), and the
scenes that drive every one of them, shared by test_perm_loss_ref_cpu.py and test_perm_loss_gpu.py.

Written from the comment block at the top of art_permeate.hip and from DESIGN.md §5; it shares no code
with the kernel. The pass takes a frame's T loss rays in chunks (plan), gives each ray P quads that split
the BVH root's children between them (part_of), keeps at most CAP non-zero terms per quad and re-sums a
ray with one list over CAP by the whole wave. Which of these a ray takes is decided here from the leaf
order (bvh_ref.kd_order on the host, art_debug_leaf_order on the device) and from the colliders' float32
loss terms as unity32 evaluates them: a collider's term is kept exactly when it is non-zero and the
ray's target does not own the collider. The expected values are kat_scenes.perm_value's.

Ray classes (kept_counts): 'fit' every part <= CAP; 'fit_wide' fit with a total > CAP (the ranking must
merge the quads' lists); 'edge48' fit with some part exactly CAP; 'overflow' some part > CAP; 'edge49'
some part exactly CAP + 1.
"""
import math

import numpy as np

import art
import bvh_ref
import kat_scenes as K
import unity32 as U
from art import abi

F = np.float32
CAP = 48


# ------------------------------------------------------------------------------------------------
# The pass's decisions
# ------------------------------------------------------------------------------------------------
def leaf0_of(n: int) -> int:
    """Index of the first leaf node of the complete 4-ary tree over n colliders (0: the root is a leaf)."""
    return (bvh_ref.capacity(n) // 4 - 1) // 3


def plan(T: int, leaf0: int):
    """The chunks of T loss rays as (t0, P, rays): P quads per ray, 16 // P rays at most."""
    out, t0 = [], 0
    while t0 < T:
        P = min(4, 16 // min(16, T - t0)) if leaf0 > 0 else 1
        rays = min(T - t0, 16 // P)
        out.append((t0, P, rays))
        t0 += rays
    return out


def chunk_of(T: int, leaf0: int, t: int):
    return next(c for c in plan(T, leaf0) if c[0] <= t < c[0] + c[2])


def part_of(position: int, n: int) -> int:
    """The root child (0..3, node 1 + child) above leaf position `position` of n colliders; quad
    (child % 4) % P of the ray walks it. A tree whose root is a leaf has the one part 0."""
    cap = bvh_ref.capacity(n)
    return 0 if cap == 4 else int(position) // (cap // 4)


def slot_batches(R: int, TC: int, T: int):
    """{batch slot: (first, end) of the last batch that maps to it} (AudioPermeationJobBatched.cs:36-37)."""
    bs = int(max(1.0, math.ceil(F(R) / F(TC))))
    out = {}
    for start in range(0, R, bs):
        n = min(bs, R - start)
        out[start * (TC * T // n // T) // R] = (start, start + n)
    return out


def last_hit_ray(scene, origin, first, end):
    """The highest ray of [first, end) whose permeation first hit exists, with the hit; or (None, None)."""
    o = U.v3(*origin)
    for r in range(end - 1, first - 1, -1):
        hit = K.nearest(scene, o, U.hv3(*[int(x) for x in scene.dirs[r]]), perm=True)
        if hit is not None:
            return r, hit
    return None, None


def loss_segment(scene, origin, ray, t, hit=None):
    """(offset origin, unit direction) of the loss ray of `ray` to target t (:61-78)."""
    o = U.v3(*origin)
    d = U.hv3(*[int(x) for x in scene.dirs[ray]])
    hit = hit or K.nearest(scene, o, d, perm=True)
    off = U.sub(U.add(o, U.muls(d, hit[2])), U.muls(d, U.EPS))
    return off, U.normalize(U.sub(U.v3(*scene.targets[t]), off))


def lengths(dec, off, dt):
    """Per global collider (Sphere, AABB, OBB order): the unity32 loss term at density 1, the density and
    the owner. The term proper is F(length * density): the reference's last multiply."""
    sph, aab, obs = dec
    out = []
    one = F(1)
    for c, r, dens, tid in sph:
        out.append((U.perm_sphere(off, dt, c, r, one), dens, tid))
    for c, hh, dens, tid in aab:
        out.append((U.perm_aabb(off, dt, c, hh, one), dens, tid))
    for c, hh, q, dens, tid in obs:
        out.append((U.perm_aabb(U.qmul(q, U.sub(off, c)), U.qmul(q, dt), U.v3(0, 0, 0), hh, one), dens, tid))
    return out


def classes_of(parts):
    cl = set()
    if max(parts) <= CAP:
        cl.add("fit")
        if sum(parts) > CAP:
            cl.add("fit_wide")
        if max(parts) == CAP:
            cl.add("edge48")
    else:
        cl.add("overflow")
    if CAP + 1 in parts:
        cl.add("edge49")
    return cl


def kept_counts(scene, origin, ray, order, dec=None, hit=None):
    """For the loss rays of `ray`: per target the kept terms of each quad part under `order` (leaf position
    -> global collider), the same count with zero densities and owners ignored (`crossed`), the ray's
    classes, the kinds of excluded and negative-density colliders it crosses (`seen`) and the value summed
    from the kept terms in reference order (at the default strength of 1 per ray)."""
    dec = dec or K.decoded(scene)
    n, T = len(order), scene.T
    child = np.empty(n, int)
    child[np.asarray(order, int)] = [part_of(p, n) for p in range(n)]
    res = []
    for t in range(T):
        P = chunk_of(T, leaf0_of(n), t)[1]
        off, dt = loss_segment(scene, origin, ray, t, hit)
        kept, crossed, total, ids, seen = [0] * P, [0] * P, F(0), [], set()
        for g, (ln, dens, tid) in enumerate(lengths(dec, off, dt)):
            j = (child[g] % 4) % P
            crossed[j] += int(ln != 0)
            term = F(ln * dens)
            if ln != 0:  # what the ray crosses beside plain colliders
                seen |= {"owned"} if tid == t else {"-0" if np.signbit(dens) else "+0"} if dens == 0 else {"negative"} if dens < 0 else set()
            if tid != t and term != 0:
                kept[j] += 1
                total = F(total + term)
                ids.append(g)
        res.append(dict(P=P, parts=kept, crossed=crossed, classes=classes_of(kept), ids=ids, child=child, seen=seen,
                        value=F(F(F(scene.R) * F(1.0)) - total)))
    return res


def value(scene, origin, ray, t, strength=1.0):
    """The expected PermeationPowerRemains of (ray, t): kat_scenes.perm_value."""
    return K.perm_value(scene, origin, ray, t, strength)


# ------------------------------------------------------------------------------------------------
# Broad-phase bounds on the host (spheres and AABBs: bvh_ref.cull_bounds; OBBs: prep_obb's rotated-box
# rule of art_frame_math.hpp, every operation rounded on its own)
# ------------------------------------------------------------------------------------------------
def obb_bounds(obbs):
    lo, hi = np.zeros((obbs.size, 3), F), np.zeros((obbs.size, 3), F)
    for i, b in enumerate(obbs):
        c, h = U.hv3(*b["center"]), tuple(F(abs(x)) for x in U.hv3(*b["size"]))
        q = U.half_quaternion(*[int(x) for x in b["rot"]])
        col = [tuple(F(abs(x)) for x in U.qmul(q, e)) for e in (U.v3(1, 0, 0), U.v3(0, 1, 0), U.v3(0, 0, 1))]
        hs = U.hv3(*b["size"])
        h1 = F(F(F(abs(hs[0])) + F(abs(hs[1]))) + F(abs(hs[2])))
        rho, slack = F(h1 * F(1.001)), F(F(1e-5) * h1)
        for x in range(3):
            by_col = F(F(F(col[x][0] * h[0]) + F(col[x][1] * h[1])) + F(col[x][2] * h[2]))
            by_row = F(F(F(col[0][x] * h[0]) + F(col[1][x] * h[1])) + F(col[2][x] * h[2]))
            w = max(by_col, by_row)
            bx = min(F(F(w * F(1.0001)) + slack), rho)
            lo[i, x], hi[i, x] = F(c[x] - bx), F(c[x] + bx)
    return lo, hi


def host_bounds(scene):
    """(lo, hi) of every collider in global order, as the kd build reads them."""
    cull = bvh_ref.cull_bounds(scene.spheres, scene.aabbs)
    olo, ohi = obb_bounds(scene.obbs)
    return np.concatenate([cull["lo"].reshape(-1, 3), olo]), np.concatenate([cull["hi"].reshape(-1, 3), ohi])


def host_order(scene):
    return bvh_ref.kd_order(*host_bounds(scene))


# ------------------------------------------------------------------------------------------------
# A frame under the model
# ------------------------------------------------------------------------------------------------
class Case:
    """One frame of the matrix: the scene, the parameters, the fan origins and what the model must find in
    it (`require`, a list of (rule, argument...) read by check_classes)."""

    def __init__(self, name, scene, params, org, require):
        self.name, self.scene, self.params, self.org, self.require = name, scene, params, org, require


def analyse(case, order):
    """{(fan, slot): None for a batch without a hit, else {ray, hit, rays: kept_counts}} under `order`."""
    sc, dec = case.scene, K.decoded(case.scene)
    out = {}
    for f, origin in enumerate(case.org):
        for slot, (x, y) in sorted(slot_batches(sc.R, case.params.thread_count, sc.T).items()):
            ray, hit = last_hit_ray(sc, origin, x, y)
            out[(f, slot)] = None if ray is None else dict(ray=ray, hit=hit, batch=(x, y),
                                                           rays=kept_counts(sc, origin, ray, order, dec, hit))
    return out


def expected_perm(case, info, stale):
    """The frame's PermeationPowerRemains [S, TC * T] from the model's values over the stale contents."""
    want = np.array(stale, np.float32, copy=True)
    T = case.scene.T
    for (f, slot), e in info.items():
        for t in range(T):
            want[f, slot * T + t] = F(0) if e is None else value(case.scene, case.org[f], e["ray"], t)
    return want


def _rays(info):
    for (f, slot), e in sorted(info.items()):
        if e is not None:
            for t, r in enumerate(e["rays"]):
                yield f, slot, t, r


def check_classes(case, order):
    """Assert the case's declared classes on the model's counts under `order`; returns the analysis and a
    one-line summary (classes reached, largest part)."""
    info = analyse(case, order)
    n, T = len(order), case.scene.T
    chunks = plan(T, leaf0_of(n))
    rays = list(_rays(info))
    has = lambda cls, ts, P=None: [(f, s, t) for f, s, t, r in rays if t in ts and cls in r["classes"] and (P is None or r["P"] == P)]
    for rule, *arg in case.require:
        what = f"{case.name}: {rule}{tuple(arg)}"
        if rule == "chunk_mix":  # every chunk: an overflow ray and a fit_wide ray (a fit ray at P = 1)
            for t0, P, nr in chunks:
                ts = range(t0, t0 + nr)
                assert has("overflow", ts), f"{what}: no overflow ray in chunk {(t0, P, nr)}"
                assert has("fit_wide" if P > 1 else "fit", ts), f"{what}: no fitting ray in chunk {(t0, P, nr)}"
        elif rule == "same_wave_mix":  # one wave's chunk holds an overflow ray beside a fit_wide ray
            t0, P, nr = chunks[arg[0]]
            ts = range(t0, t0 + nr)
            assert {(f, s) for f, s, _ in has("overflow", ts)} & {(f, s) for f, s, _ in has("fit_wide", ts)}, what
        elif rule == "tail_overflow":  # an overflow ray in the tail chunk, past its first ray where it has more than one
            t0, P, nr = chunks[-1]
            assert t0 > 0 and P == arg[0], f"{what}: tail {(t0, P, nr)}"
            assert has("overflow", range(t0 + (nr > 1), t0 + nr)), what
        elif rule == "edges":  # at P: an edge48 ray (ranked: it fits) and an edge49 ray
            assert has("edge48", range(T), arg[0]) and has("edge49", range(T), arg[0]), what
        elif rule == "excluded_edge":  # an edge48 ray that crosses more than CAP colliders in that part: zero densities
            # of both signs and colliders its target owns took it there, a negative density's term stayed
            assert any("edge48" in r["classes"] and any(k == CAP and c > CAP for k, c in zip(r["parts"], r["crossed"]))
                       and r["seen"] >= {"owned", "+0", "-0", "negative"} for _, _, _, r in rays), what
        elif rule == "multi_overflow":  # three overflow rays of one wave's 16-ray chunk, a fit ray between each pair
            ok = False
            for key, e in info.items():
                if e is None or chunks[0][2] != 16:
                    continue
                cl = ["overflow" in r["classes"] for r in e["rays"][:16]]
                ov = [t for t in range(16) if cl[t]]
                pick = [ov[0]] if ov else []
                for t in ov[1:]:
                    if any(not cl[u] for u in range(pick[-1] + 1, t)):
                        pick.append(t)
                ok = ok or len(pick) >= 3
            assert ok, what
        elif rule == "slot_overflow":  # an overflow ray written in a batch slot above 0
            assert any(s > 0 for _, s, _ in has("overflow", range(T))), what
        elif rule == "stale_slots":  # some slot no batch maps to
            assert len(slot_batches(case.scene.R, case.params.thread_count, T)) < case.params.thread_count, what
        elif rule == "hit_ray":  # (fan, slot) -> the batch's winning ray (None: no hit)
            for key, ray in arg[0].items():
                got = info[key] and info[key]["ray"]
                assert got == ray, f"{what}: {key} found {got}"
        elif rule == "zero_hit":  # the first hit of (fan, slot 0) is collider type arg at distance 0
            for f, ty in arg[0].items():
                hit = info[(f, 0)]["hit"]
                assert hit[0] == ty and hit[2] == 0, f"{what}: fan {f} hit {hit}"
        elif rule == "all_crossed":  # every collider is crossed by every loss ray
            assert all(sum(r["crossed"]) == n for _, _, _, r in rays), what
        elif rule == "P":
            assert [c[1] for c in chunks] == arg[0], f"{what}: {chunks}"
        elif rule == "terms":  # among colliders arg: one zero term and one non-zero term on some loss ray
            zero = nonzero = False
            for f, s, t, r in rays:
                e = info[(f, s)]
                off, dt = loss_segment(case.scene, case.org[f], e["ray"], t, e["hit"])
                assert sum(int(x == 0) for x in dt) == 2, f"{what}: loss direction {dt}"
                ln = lengths(K.decoded(case.scene), off, dt)
                zero = zero or any(ln[g][0] == 0 for g in arg[0])
                nonzero = nonzero or any(ln[g][0] != 0 for g in arg[0])
            assert zero and nonzero, what
        else:
            raise KeyError(rule)
    reached = sorted(set().union(*[r["classes"] for _, _, _, r in rays])) if rays else []
    top = max((max(r["parts"]) for _, _, _, r in rays), default=0)
    return info, f"{case.name}: classes {', '.join(reached) or '-'}; largest part {top}"


# ------------------------------------------------------------------------------------------------
# Scenes
# ------------------------------------------------------------------------------------------------
STAGES = abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_PERMEATE | abi.ART_STAGE_REDUCE


def frame_params(tc=1, stages=STAGES):
    p = art.FrameParams(max_hits_per_ray=1, max_ray_life=1e4, max_muffle_hit_distance=1e5, stages=stages)
    p.thread_count = tc
    return p


def _mat(density):
    return (0.25, density, 1.0)


def _sphere(c, r, density, tid=-1):
    return K.sphere(c, r, *_mat(density), tid=tid)


def _aabb(c, hh, density, tid=-1):
    return K.aabb(c, hh, *_mat(density), tid=tid)


def _obb(c, hh, q, density, tid=-1):
    return K.obb(c, hh, q, *_mat(density), tid=tid)


def _dirs(R, seed, last=(1.0, 0.0, 0.0), spread=None):
    """R directions whose last is `last`; spread: every ray within that of `last` (all hit the wall)."""
    rng = np.random.default_rng(seed)
    if spread is None:
        d = rng.normal(size=(R, 3))
        d[:, 0] = -np.abs(d[:, 0])  # away from the colliders: only the last ray hits
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    else:
        d = np.asarray(last) + np.concatenate([np.zeros((R, 1)), rng.uniform(-spread, spread, (R, 2))], axis=1)
    d[-1] = last
    return K.half3_dirs([tuple(x) for x in d])


# The row scene. Fan 0 looks along +x at wall 1 (hit point P0); three rows of colliders run from P0
# towards three anchors, and the targets sit (jittered) at the anchors: group A's row is dense, B's
# medium, C's light. Along x the scene falls into four blocks of 64 colliders, the root's children, so
# a row's colliders per block are its rays' counts per root child. Fan 1 starts inside a gap of row A
# and hits wall 2 on A's line a quarter of the way along: its rays to A's targets meet the rest of the
# row (fit_wide where fan 0's overflow). Fan 2 hits wall 1 off the rows' common point.
P0 = np.array([4.0, 0.0, 0.0])
ANCHORS = {"A": np.array([100.0, 4.0, 2.0]), "B": np.array([100.0, 16.0, -3.0]), "C": np.array([100.0, -14.0, 5.0])}
BLOCKS = [(10.0, 26.0), (29.0, 45.0), (47.0, 63.0), (65.0, 81.0)]
ROWS = {"A": (52, 20, 15, 15), "B": (8, 10, 17, 17), "C": (2, 2, 2, 2)}
ROW_ORIGINS = np.array([[0.0, 0.0, 0.0], [27.5, 1.0, 0.5], [0.0, 0.25, -0.25]], np.float32)


def _row_colliders(with_obb):
    """[(kind, record, row or None)] of the 256 colliders, in block order."""
    rng = np.random.default_rng(41)
    out = [("aabb", _aabb((4.125, 0, 0), (0.125, 0.5, 0.5), 0.5), None),      # wall 1: face x = 4
           ("aabb", _aabb((28.125, 1, 0.5), (0.125, 0.3, 0.3), 0.75), None)]  # wall 2: face x = 28 on row A's line
    for b, (x0, x1) in enumerate(BLOCKS):
        here = []
        for row, per_block in ROWS.items():
            m = per_block[b]
            for i in range(m):
                x = x0 + (x1 - x0) * (i + 0.5) / m
                c = P0 + (x - P0[0]) / (ANCHORS[row][0] - P0[0]) * (ANCHORS[row] - P0)
                dens = -0.5 if i % 9 == 4 else float(rng.uniform(0.2, 1.0))  # a negative density's term is kept
                if with_obb and i % 5 == 2:
                    q = rng.normal(size=4)
                    q /= np.linalg.norm(q)
                    here.append(("obb", _obb(c, (0.3, 0.35, 0.4), tuple((q[:3] if q[3] > 0 else -q[:3])), dens), row))
                elif i % 3 == 1:
                    here.append(("aabb", _aabb(c, (0.1, 0.4, 0.4), dens), row))
                else:
                    here.append(("sphere", _sphere(c, 0.35, dens), row))
        for i in range(64 - len(here) - (2 if b == 0 else 0)):  # clutter, well off the rows
            c = (rng.uniform(x0, x1), rng.uniform(-3, 3), rng.choice([-1, 1]) * rng.uniform(6, 9))
            here.append(("sphere", _sphere(c, 0.3, 0.5), None) if i % 2 else ("aabb", _aabb(c, (0.3, 0.2, 0.3), 0.5), None))
        out += here
    assert len(out) == 256
    return out


def row_scene(T, groups="ABAC", with_obb=False, R=8, dirs=None):
    """The row scene with T targets, target t in group groups[t % len(groups)]; list positions shuffled."""
    recs = _row_colliders(with_obb)
    rng = np.random.default_rng(43)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    tg = np.array([ANCHORS[groups[t % len(groups)]] + (0.0, ((7 * t) % 5 - 2) * 0.01, ((3 * t) % 7 - 3) * 0.01)
                   for t in range(T)], np.float32)
    sc = art.Scene(dirs=_dirs(R, 5) if dirs is None else dirs, targets=tg,
                   spheres=K.cat(abi.SPHERE, *[r for k, r, _ in recs if k == "sphere"]),
                   aabbs=K.cat(abi.AABB, *[r for k, r, _ in recs if k == "aabb"]),
                   obbs=K.cat(abi.OBB, *[r for k, r, _ in recs if k == "obb"]))
    return sc


def _records(scene, g):
    ns, na = scene.spheres.size, scene.aabbs.size
    return (scene.spheres, g) if g < ns else (scene.aabbs, g - ns) if g < ns + na else (scene.obbs, g - ns - na)


def trim(scene, origin, ray, order, shared, owned):
    """Bring loss rays to the cap's edge without moving a collider (the leaf order stays): for each target t
    of `shared`, zero the density (+0 and -0 in turn) of kept colliders until no part exceeds CAP + 1; then
    let each target t of `owned` own kept colliders until no part exceeds CAP. Every third excluded
    collider of a part is taken from its far end, the rest evenly."""
    zero = [U.f2h(F(0.0)), U.f2h(F(-0.0))]
    k = 0
    for ts, limit in ((shared, CAP + 1), (owned, CAP)):
        for t in ts:
            r = kept_counts(scene, origin, ray, order)[t]
            for j in range(r["P"]):
                ids = [g for g in r["ids"] if (r["child"][g] % 4) % r["P"] == j]
                extra = len(ids) - limit
                if extra <= 0:
                    continue
                for g in [ids[int(i * len(ids) / extra)] for i in range(extra)]:
                    arr, i = _records(scene, g)
                    if limit == CAP:
                        arr["audio_target_id"][i] = t
                    else:
                        arr["material"][i][1] = zero[k % 2]
                        k += 1
    return scene


def row_case(T, name=None, tc=1, R=8, stages=STAGES, with_obb=False, groups="ABAC", require=None, spread=None, fans=3):
    sc = row_scene(T, groups, with_obb, R, None if spread is None else _dirs(R, 5, spread=spread))
    n_chunks = len(plan(T, leaf0_of(256)))
    req = [("chunk_mix",)] if require is None else require
    if require is None and T >= 4 and plan(T, 21)[0][1] > 1:
        req.append(("same_wave_mix", 0))
    if require is None and n_chunks > 1 and plan(T, 21)[-1][1] > 1:
        req.append(("tail_overflow", plan(T, 21)[-1][1]))
    return Case(name or f"rows-T{T}" + ("-obb" if with_obb else ""), sc, frame_params(tc, stages), ROW_ORIGINS[:fans].copy(), req)


EDGE_T = {4: 4, 3: 5, 2: 8, 1: 9}  # P -> a target count whose one chunk has that P


def edge_case(P, with_obb=False):
    """Targets 0 and 2 (group A, fan 0: overflow as built) trimmed to CAP + 1 by zero densities, then
    target 0 to CAP by colliders it owns: an edge49 ray and an edge48 ray in one chunk."""
    c = row_case(EDGE_T[P], name=f"edge-P{P}" + ("-obb" if with_obb else ""), with_obb=with_obb,
                 require=[("P", [P]), ("edges", P), ("excluded_edge",)])
    trim(c.scene, c.org[0], c.scene.R - 1, host_order(c.scene), shared=[2, 0], owned=[0])
    return c


def first_hit_case(name, R, k, decoys=(), tc=1, expect=None):
    """One small box along ray k and one along each lower ray of `decoys`, seen from two fans; nothing else
    in the scene. Target 0 lies behind ray k's box, so the value tells which ray's hit point was used."""
    from art.synth import fibonacci_directions
    dirs = fibonacci_directions(R) if R > 1 else K.half3_dirs([(0.6, 0.0, 0.8)])  # (one Fibonacci ray is 0 / 0)
    unit = lambda r: (lambda d: d / np.linalg.norm(d))(np.array([float(U.h2f(int(x))) for x in dirs[r]]))
    boxes = [_aabb(tuple(unit(r) * 20.0), (1.0, 1.0, 1.0), 0.5 + 0.125 * i) for i, r in enumerate((k,) + tuple(decoys))]
    tg = np.array([unit(k) * 60.0 + (1, 2, 0), [5, 5, 5], [-30, 2, 1]], np.float32)
    sc = art.Scene(dirs=dirs, targets=tg, aabbs=K.cat(abi.AABB, *boxes))
    org = np.array([[0, 0, 0], [0.1, -0.2, 0.05]], np.float32)
    return Case(name, sc, frame_params(tc), org, [("hit_ray", expect or {(0, 0): k, (1, 0): k})])


def first_hit_cases():
    out = []
    # y - 1, y - 2, y - 17, y - 18, x + 1, x of the batch [0, 40): the last ray alone, then 16 at a time
    for k, decoys in ((39, (38, 20)), (38, (37, 23, 22)), (23, (22, 10)), (22, (21, 7, 6)), (1, (0,)), (0, ())):
        out.append(first_hit_case(f"first-hit-40-ray{k}", 40, k, decoys))
    out.append(first_hit_case("first-hit-R1", 1, 0))
    out.append(first_hit_case("first-hit-R17", 17, 0))   # the last ray, then one full round of 16
    out.append(first_hit_case("first-hit-R18", 18, 0))   # ... and a round with one live quad
    # three batches of one ray in three slots, the middle one without a hit
    want = {(f, s): r for f in (0, 1) for s, r in ((0, 0), (1, None), (2, 2))}
    out.append(first_hit_case("first-hit-tc3-gap", 3, 2, (0,), tc=3, expect=want))
    return out


def zero_distance_case():
    """First hits at distance 0, one fan each. The reference's tests report the far root or the exit face
    for an origin strictly inside a collider (fans 0-2: a positive distance) and for one on an AABB's entry
    face (fan 3); the distance is 0 where the ray leaves the collider at its origin: on a sphere's surface
    (fan 4), on an AABB's exit face (fan 5) and on the exit face of an OBB turned half a turn about z
    (fan 6: the rotation is exact in float32). The last ray is (1, 0, 0)."""
    half_turn = (0.0, 0.0, 1.0)
    sc = art.Scene(dirs=_dirs(4, 9), targets=np.array([[30, 3, 1], [-20, 40, 2], [8, -9, 60]], np.float32),
                   spheres=K.cat(abi.SPHERE, _sphere((0, 0, 0), 2.0, 0.5), _sphere((-2, 40, 0), 2.0, 0.75), _sphere((12, 1, 0), 1.0, 0.5)),
                   aabbs=K.cat(abi.AABB, _aabb((0, 10, 0), (1, 2, 3), 0.5), _aabb((1, 50, 0), (1, 1, 1), 0.25),
                               _aabb((-1, 60, 0), (1, 1, 1), 0.5), _aabb((15, 12, 1), (0.5, 3, 3), 0.5)),
                   obbs=K.cat(abi.OBB, _obb((0, 20, 0), (1, 2, 3), (0.1, 0.2, 0.3), 0.5), _obb((0, 30, 0), (1, 2, 3), half_turn, 0.5)))
    org = np.array([[0.5, 0.25, 0], [0.25, 10.5, 1], [0.25, 20.5, 0.5], [0, 50, 0.5], [0, 40, 0], [0, 60, 0.5], [1, 30.5, 0.25]],
                   np.float32)
    S, A, O = abi.ART_COLLIDER_SPHERE, abi.ART_COLLIDER_AABB, abi.ART_COLLIDER_OBB
    return Case("zero-distance", sc, frame_params(), org, [("zero_hit", {4: S, 5: A, 6: O})])


def axis_case():
    """Loss rays along (1, 0, 0) exactly: the wall's face at x = 4, the targets on the fan's own line. Thin
    boxes with a face in the ray's plane (0 * inf in the slab test) and spheres tangent to the ray (a
    discriminant that cancels) are colliders 'on the ray'; boxes and spheres around it give plain terms."""
    on_ray_s = [_sphere((8 + 3 * i, r, 0), r, 0.5) for i, r in enumerate((0.5, 0.75, 1.0, 0.3, 0.7, 1.3))]
    on_ray_s += [_sphere((30 + 3 * i, 0, -r), r, 0.5) for i, r in enumerate((0.1, 0.6, 0.9))]
    on_ray_a = [_aabb((7, 0.25, 0), (0.1, 0.25, 1), 0.5), _aabb((10, -0.25, 0), (0.1, 0.25, 1), 0.5),
                _aabb((13, 0, 0.5), (0.1, 1, 0.5), 0.5), _aabb((16, 0, -0.5), (0.1, 1, 0.5), 0.5),
                _aabb((19, 0.5, 0.5), (0.1, 0.5, 0.5), 0.5), _aabb((22, 0, 0), (0.1, 0, 1), 0.5)]
    plain_s = [_sphere((40 + 2 * i, 0.1, -0.1), 0.5, 0.5) for i in range(3)]
    plain_a = [_aabb((4.125, 0, 0), (0.125, 1, 1), 0.5)] + [_aabb((50 + 2 * i, 0, 0), (0.1, 0.5, 0.5), 0.5) for i in range(3)]
    sc = art.Scene(dirs=_dirs(4, 13), targets=np.array([[200, 0, 0], [90, 0, 0], [1000, 0, 0]], np.float32),
                   spheres=K.cat(abi.SPHERE, *on_ray_s, *plain_s), aabbs=K.cat(abi.AABB, *on_ray_a, *plain_a))
    on_ray = list(range(len(on_ray_s))) + [sc.spheres.size + i for i in range(len(on_ray_a))]
    return Case("axis-aligned", sc, frame_params(), np.zeros((2, 3), np.float32), [("terms", on_ray)])


def tiny_case(n, T=3):
    """n colliders in a line behind the wall (the wall is one of them), every one crossed by every loss ray;
    n <= 4: the root is the one leaf, P = 1 for any T; n = 5: one inner level, P = 4 at T = 3."""
    recs = [("aabb", _aabb((4.125, 0, 0), (0.125, 1, 1), 0.5)), ("sphere", _sphere((8, 0.1, 0), 1.0, 0.75)),
            ("obb", _obb((12, 0, 0.1), (0.5, 1, 1), (0.1, 0.2, 0.3), 0.5)), ("sphere", _sphere((16, 0, -0.1), 1.0, 0.25)),
            ("aabb", _aabb((20, 0.1, 0), (0.5, 1, 1), 1.0))][:n]
    sc = art.Scene(dirs=_dirs(4, 17), targets=np.array([[60 + 9 * t, 0.05 * t, -0.04 * t] for t in range(T)], np.float32),
                   spheres=K.cat(abi.SPHERE, *[r for k, r in recs if k == "sphere"]),
                   aabbs=K.cat(abi.AABB, *[r for k, r in recs if k == "aabb"]),
                   obbs=K.cat(abi.OBB, *[r for k, r in recs if k == "obb"]))
    org = np.array([[0, 0, 0], [1, 0.05, -0.05]], np.float32)
    return Case(f"tiny-{n}-T{T}", sc, frame_params(), org, [("all_crossed",), ("P", [c[1] for c in plan(T, leaf0_of(n))])])


CHUNK_T = (1, 4, 5, 6, 8, 9, 16, 17, 21, 22, 33, 37)
PERMEATE = abi.ART_STAGE_PERMEATE


def cases():
    """{name: builder} of the whole matrix."""
    out = {f"rows-T{T}": (lambda T=T: row_case(T)) for T in CHUNK_T}
    out["rows-T6-obb"] = lambda: row_case(6, with_obb=True)
    out["rows-T21-obb"] = lambda: row_case(21, with_obb=True)
    for P in (4, 3, 2, 1):
        out[f"edge-P{P}"] = lambda P=P: edge_case(P)
    out["edge-P2-obb"] = lambda: edge_case(2, with_obb=True)
    out["multi-overflow"] = lambda: row_case(16, name="multi-overflow", groups="ACCACACC", fans=1,
                                             require=[("P", [1]), ("multi_overflow",)])
    for tc, R in ((3, 64), (5, 64), (3, 9), (5, 9)):
        req = [("chunk_mix",)] + ([("slot_overflow",), ("stale_slots",)] if (tc, R) == (5, 9) else [])
        out[f"slots-tc{tc}-R{R}"] = lambda tc=tc, R=R, req=req: row_case(6, name=f"slots-tc{tc}-R{R}", tc=tc, R=R, fans=2,
                                                                        spread=0.02, require=list(req))
    out["stages-permeate"] = lambda: row_case(6, name="stages-permeate", stages=PERMEATE, fans=2)
    out["stages-permeate-reduce"] = lambda: row_case(6, name="stages-permeate-reduce", stages=PERMEATE | abi.ART_STAGE_REDUCE, fans=2)
    for c in first_hit_cases():
        out[c.name] = lambda c=c: c
    out["zero-distance"] = zero_distance_case
    out["axis-aligned"] = axis_case
    for n, T in ((1, 3), (2, 5), (3, 3), (4, 17), (5, 3)):
        out[f"tiny-{n}-T{T}"] = lambda n=n, T=T: tiny_case(n, T)
    return out

"""The muffle direction-cell lists (csrc/art_cells.hip) read back and pinned to the float64 reference
(tests/cells_ref.py): every list holds every collider a segment through its cell can meet, with a near
bound not above the true distance, sorted, without duplicates, owned colliders or entries the rule
does not justify; after a build, a partial build, a target add / remove and every kind of collider
sync. Output parity is a weak witness of this: a muffle ray is an any-hit OR, so a list
that misses a collider changes a count only where that collider was a ray's sole blocker.

Scenes are bound only (one fan of 8 rays, no frame) unless a test says otherwise; the lists are read back
through art_debug_cells_lists and the colliders' cull records through art_debug_bvh_records."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import art
import cells_ref as cr
import cells_scenes as cs
import oracle
from art import abi
from art.colliders import ColliderStore, resident_frame
from art.synth import fibonacci_directions
from art.targets import TargetStore, resident_targets_frame
from test_cells_ref_cpu import pairs_of, sole_blocker_frame

pytestmark = pytest.mark.gpu

LISTS = cr.CELLS * 3   # lists per target: (cell, collider type)
SPH, BOX, OBB = abi.ART_KIND_SPHERE, abi.ART_KIND_AABB, abi.ART_KIND_OBB


def make_frame(sph, box, obb, targets, S=1, R=8):
    scene = art.Scene(dirs=fibonacci_directions(R), targets=np.ascontiguousarray(targets, np.float32), spheres=sph, aabbs=box,
                      obbs=obb)
    params = art.FrameParams(max_hits_per_ray=2)
    org = np.linspace(-3.0, 3.0, 3 * S, dtype=np.float32).reshape(S, 3)
    return art.Frame(scene, params, org, art.FanOutputs(S, R, params.max_hits_per_ray, scene.T, params.thread_count))


def read_lists(c):
    start, code, key, near, ok, far, info = c.debug_cells_lists()
    raw = c._cells_words(abi.ART_DEBUG_CELLS_ENTRIES)   # the arena's words as they lie in memory
    return SimpleNamespace(start=start, code=code, key=key, near=near, ok=ok, far=far, info=info, raw=raw)


def target_lists(L, t):
    """(s, list id of each entry, arena positions) of target t: s = its LISTS + 1 starts."""
    stride = L.info["kCellStride"]
    s = L.start[t * stride:t * stride + LISTS + 1].astype(np.int64)
    ln = np.diff(s)
    assert (ln >= 0).all(), f"target {t}: starts decrease at lists {np.nonzero(ln < 0)[0][:8]}"
    return s, np.repeat(np.arange(LISTS), ln), np.arange(s[0], s[-1])


def check_lists(c, recs, targets, name=None, full=True, bloat=True, far_bounds=None, mutate=None):
    """Every assertion on the lists of the scene bound on c, whose colliders are recs = (spheres, aabbs,
    obbs) and whose targets are `targets`. full: the arena holds a full build (no garbage). far_bounds: the
    cull records the lists' segment bounds were built from (default: the current ones). mutate: applied to the
    lists as read back, before any check (test_check_lists_notices). Returns the lists."""
    sph, box, obb = recs
    ref = cr.Ref(sph, box, obb, targets)
    sh = ref.shapes
    T, counts = len(ref.targets), np.array(sh.counts)
    first = np.array([0, counts[0], counts[0] + counts[1]])
    L = read_lists(c)
    if mutate:
        mutate(L, ref)
    info, stride = L.info, L.info["kCellStride"]
    assert info["kCellG"] == cr.G and stride >= LISTS and info["cap"] > 0
    assert L.start.size == T * stride + 1 and L.ok.size == T and L.far.size == T
    assert info["tail"] <= info["cap"] and L.code.size == info["tail"]
    bounds = c.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS)
    assert bounds.size == sh.n
    rng = np.random.default_rng(1)
    total = 0
    for t in range(T):
        # ---- structure
        s, lid, pos = target_lists(L, t)
        pads = L.start[t * stride + LISTS:(t + 1) * stride]
        assert (pads == s[-1]).all(), f"target {t}: pad starts differ from its end {s[-1]}"
        assert s[-1] <= info["tail"]
        total += pos.size
        if not L.ok[t]:
            assert pos.size == 0, f"target {t} has no lists (ok 0) but {pos.size} entries"
            continue
        code, key = L.code[pos], L.key[pos].astype(np.int64)
        ty, idx = (code >> 28).astype(np.int64), (code & 0x0fffffff).astype(np.int64)
        assert (ty == lid % 3).all(), f"target {t}: entries in a list of another type"
        assert (idx < counts[ty]).all(), f"target {t}: index past its type's count"
        g, cell = first[ty] + idx, lid // 3
        assert (sh.tid[g] != t).all(), f"target {t} lists colliders it owns: {np.unique(g[sh.tid[g] == t])[:8]}"
        pair = g * cr.CELLS + cell
        assert np.unique(pair).size == pair.size, f"target {t}: a collider twice in one list"
        # ---- order
        same = lid[1:] == lid[:-1]
        d = np.nonzero(same & (key[1:] < key[:-1]))[0]
        assert d.size == 0, f"target {t}: near keys decrease in lists {np.unique(lid[d])[:8]}"
        dmin = ref.dmin_many(t, g)
        if L.near is None:
            nearf = (L.key[pos] << np.uint32(16)).view(np.float32).astype(np.float64)
        else:
            nearf = L.near[pos].astype(np.float64)
            nk = np.where(L.near[pos].view(np.int32) <= 0, 0, L.near[pos].view(np.uint32) >> np.uint32(16))
            assert np.array_equal(nk, key), f"target {t}: a key that is not near_key(near)"
        d = np.nonzero(~(nearf <= dmin))[0]
        assert d.size == 0, (f"target {t}: near bound above the distance to the shape", [(int(g[k]), int(cell[k]), float(nearf[k]),
                                                                                         float(dmin[k])) for k in d[:8]])
        # ---- far
        fb = bounds if far_bounds is None else far_bounds
        far64 = ref.far64(t, fb["lo"].min(0), fb["hi"].max(0))
        assert far64 <= L.far[t] <= far64 * 1.002 + 2e-3, (t, far64, float(L.far[t]))
        # ---- coverage
        gs = pairs_of(ref, name, t, rng)
        need, _ = ref.required_many(t, gs)
        assert need.size >= gs.size   # (every collider requires a cell)
        lost = need[~np.isin(need, pair)]
        assert lost.size == 0, (f"{lost.size} missing (target, collider, cell)", [(t, int(k // cr.CELLS), int(k % cr.CELLS)) for k in lost[:12]])
        # ---- no bloat
        if bloat:
            ok = ref.justified(t, cell, g, bounds["factor"][g].astype(np.float64), float(L.far[t]))
            assert ok.all(), (f"{int((~ok).sum())} unjustified (target, collider, cell)", [(t, int(a), int(b)) for a, b in
                                                                                           zip(g[~ok][:12], cell[~ok][:12])])
    if full:
        assert total == info["tail"] and L.start[T * stride] == info["tail"], (total, info)
    else:
        assert total <= info["tail"]
    return L


def list_lengths(L, T):
    return np.concatenate([np.diff(target_lists(L, t)[0]) for t in range(T)])


# ------------------------------------------------------------------------------------------------
# Builds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "edges-wide", "edges-inside", "edges-far", "seam-255", "seam-256", "seam-257", "seam-513", "resident"])
def test_build_lists(ctx, name):
    """Geometry edges (hand-placed colliders on axes, cube edges and corners, around the `wide` and `all`
    thresholds, tangent to and behind face planes, on and around targets, degenerate shapes, with and without
    colliders near 10^4) and the chunk seams of the row passes (255 .. 513 colliders)."""
    sph, box, obb, targets = cs.BUILD_SCENES[name]()
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    L = check_lists(ctx, (sph, box, obb), targets, name)
    assert L.info["compact"] == 1 and L.ok.all() and L.info["dropped"] == 0


def test_sort_paths(ctx):
    """Lists of every length class of cells_sort_kernel: at most 1, 2..64, 65..256 and more than 256."""
    sph, box, obb, targets = cs.sort_paths()
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    L = check_lists(ctx, (sph, box, obb), targets, "sort-paths")
    ln = list_lengths(L, len(targets))
    classes = [(ln <= 1).sum(), ((ln >= 2) & (ln <= 64)).sum(), ((ln >= 65) & (ln <= 256)).sum(), (ln > 256).sum()]
    assert all(classes), classes


def test_grid_stride_rows(ctx):
    """8 targets x 11 000 spheres: 8 * 6 * 32 * 43 = 66 048 row units, more than the 2^16 workgroups of a
    launch, so the row passes stride. Coverage on a random tenth of the pairs (cells_scenes.COVERAGE_FRACTION),
    everything else on every entry."""
    sph, box, obb, targets = cs.BUILD_SCENES["rows"]()
    assert len(targets) * 6 * cr.G * ((sph.size + 255) // 256) > 1 << 16
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    L = check_lists(ctx, (sph, box, obb), targets, "rows")
    assert L.ok.all() and L.info["tail"] > sph.size * len(targets)


def test_eight_byte_entries(ctx):
    """65 536 spheres: an index no longer fits 16 bits, so the entries are (code, near bits) pairs. Coverage on
    a random eighth of the colliders (the reference's samples of all 65 536 take about 20 s of NumPy; the
    collider count is what selects the entry form), everything else on every entry."""
    sph, box, obb, targets = cs.BUILD_SCENES["wide-entries"]()
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    L = check_lists(ctx, (sph, box, obb), targets, "wide-entries")
    assert L.info["compact"] == 0 and L.near is not None and L.ok.all()


def test_nonfinite_scene(ctx):
    """One collider of infinite extent: no segment bound exists, so no target has lists."""
    sph, box, obb, targets = cs.nonfinite()
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    L = read_lists(ctx)
    assert np.isposinf(L.far).all() and not L.ok.any() and L.info["tail"] == 0 and L.info["dropped"] == 0
    assert (L.start == 0).all() and L.start.size == len(targets) * L.info["kCellStride"] + 1


def test_check_lists_notices(ctx):
    """check_lists on lists edited after the read-back: an entry replaced by another collider (the replaced one
    is then missing from a cell it must be in), a near key raised above the distance to the shape, two entries
    of a list out of order. Each is reported by the assertion meant for it."""
    sph, box, obb, targets = cs.small_resident()
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb, targets))
    recs = (sph, box, obb)
    check_lists(ctx, recs, targets)

    def first_required_entry(L, ref):
        """(arena position, list) of a list's first entry whose collider the reference requires in that cell."""
        s, lid, pos = target_lists(L, 0)
        sh = ref.shapes
        need, _ = ref.required_many(0, np.nonzero(sh.tid != 0)[0])
        for k in need:
            g, cell = int(k // cr.CELLS), int(k % cr.CELLS)
            l = cell * 3 + int(sh.kind[g])
            if s[l + 1] > s[l] and int(L.code[s[l]]) == int(sh.code[g]):
                return int(s[l]), l, g
        raise AssertionError("no list starts with a required collider")

    def replace(L, ref):
        p, l, g = first_required_entry(L, ref)
        sh = ref.shapes
        s = target_lists(L, 0)[0]
        listed = set(int(x) for x in L.code[s[l]:s[l + 1]])
        other = next(int(x) for x in np.nonzero((sh.kind == sh.kind[g]) & (sh.tid != 0))[0] if int(sh.code[x]) not in listed)
        L.code[p], L.key[p] = sh.code[other], 0

    def raise_key(L, ref):
        p, l, g = first_required_entry(L, ref)
        s = target_lists(L, 0)[0]
        L.key[s[l]:s[l + 1]] = 0x4300   # the key of 128.0: beyond every shape of the 40-unit scene

    def disorder(L, ref):
        s, lid, pos = target_lists(L, 0)
        k = L.key[pos].astype(np.int64)
        j = np.nonzero((lid[1:] == lid[:-1]) & (k[1:] > k[:-1]))[0][0]
        a, b = pos[j], pos[j + 1]
        L.code[[a, b]], L.key[[a, b]] = L.code[[b, a]], L.key[[b, a]]

    for mutate, what in ((replace, "missing"), (raise_key, "near bound above"), (disorder, "near keys decrease")):
        with pytest.raises(AssertionError, match=what):
            check_lists(ctx, recs, targets, mutate=mutate)


def test_capacity(monkeypatch):
    """ART_CELLS_CAP between the first target's total and the sum: targets keep their lists in index order while
    the running total fits, the others are dropped (ok 0, empty lists); ART_CELLS_MAX_PAIRS below the pair
    count: no lists at all."""
    sph, box, obb, targets = cs.chunk_seams(257)
    fr = make_frame(sph, box, obb, targets)
    with art.Context(1) as c:
        c.bind(fr)
        L = read_lists(c)
        totals = [int(np.diff(target_lists(L, t)[0]).sum()) for t in range(3)]
    cap = totals[0] + totals[1] // 2
    kept, run = [], 0
    for n in totals:  # (cells_block_scan_kernel's rule)
        kept.append(run + n <= cap)
        run += n if kept[-1] else 0
    assert kept[0] and not all(kept)
    monkeypatch.setenv("ART_CELLS_CAP", str(cap))
    with art.Context(1) as c:
        c.bind(fr)
        L = check_lists(c, (sph, box, obb), targets)
        assert L.info["cap"] == cap and L.ok.tolist() == [int(k) for k in kept] and L.info["dropped"] == kept.count(False)
        assert L.info["tail"] == run
    monkeypatch.delenv("ART_CELLS_CAP")
    monkeypatch.setenv("ART_CELLS_MAX_PAIRS", "1")
    with art.Context(1) as c:
        c.bind(fr)
        L = read_lists(c)
        assert L.info["cap"] == 0 and L.start.size == 0 and L.code.size == 0 and L.far.size == 0
        assert L.ok.size == 3 and not L.ok.any()


def test_read_back_errors():
    with art.Context(1) as c:
        buf = (C.c_uint32 * 8)()
        assert c.lib.art_debug_cells_lists(c.ptr, abi.ART_DEBUG_CELLS_INFO, buf, 8) == abi.ART_E_STATE  # nothing bound
        sph, box, obb, targets = cs.small_resident()
        c.bind(make_frame(sph, box, obb, targets))
        assert c.lib.art_debug_cells_lists(c.ptr, 5, buf, 8) == abi.ART_E_INVALID
        assert c.lib.art_debug_cells_lists(c.ptr, abi.ART_DEBUG_CELLS_OK, None, 4) == abi.ART_E_INVALID
        assert c.lib.art_debug_cells_lists(c.ptr, abi.ART_DEBUG_CELLS_INFO, buf, 8) == 6
        assert list(buf)[4:6] == [cr.G, LISTS + 256] and buf[0] == 1
        assert c.lib.art_debug_cells_lists(c.ptr, abi.ART_DEBUG_CELLS_STARTS, buf, 2) == 4 * (LISTS + 256) + 1  # the size, whatever cap


# ------------------------------------------------------------------------------------------------
# Resident target store: partial builds, adds and removes
# ------------------------------------------------------------------------------------------------
def bind_resident_targets(c, recs, targets, reserve=0):
    store = TargetStore(c)
    store.clear()
    store.add_many(targets)
    store.sync()
    if reserve:
        store.reserve(reserve)
    c.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
    c.bind(resident_targets_frame(make_frame(*recs, targets)))
    return store


def blocks(L, t):
    """Target t's block of starts (pads included), ok and far bits."""
    stride = L.info["kCellStride"]
    return L.start[t * stride:(t + 1) * stride].copy(), int(L.ok[t]), L.far[t:t + 1].view(np.uint32)[0]


def test_partial_build():
    """art_targets_sync with one target of four moved: its lists alone are rebuilt, at the arena's former
    tail; the others' are untouched. A move out of the colliders' box gives a new segment bound."""
    sph, box, obb, targets = cs.small_resident()
    recs = (sph, box, obb)
    with art.Context(1) as c:
        store = bind_resident_targets(c, recs, targets)
        before = check_lists(c, recs, targets)
        now = targets.copy()
        for step, p in enumerate(([4.5, -7.25, 3.0], [90.0, -60.0, 45.0])):
            now[2] = p
            store.set(2, now[2])
            st = store.sync()
            assert st["lists_rebuilt"] == 1 and st["lists_full_rebuild"] == 0, st
            after = check_lists(c, recs, now, full=False)
            for t in (0, 1, 3):
                a, b = blocks(before, t), blocks(after, t)
                assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], f"step {step}: target {t}'s lists changed"
            tail0 = before.info["tail"]
            assert np.array_equal(after.raw[:before.raw.size], before.raw), f"step {step}: the arena below the former tail changed"
            s, _, pos = target_lists(after, 2)
            assert s[0] == tail0 and after.info["tail"] == tail0 + pos.size, (s[0], tail0, after.info)
            if step == 1:
                assert after.far[2] > 2 * before.far[2]  # (the target left the scene box)
            before = after
        c.set_flags(0)


def test_target_add_and_remove():
    """art_targets_reserve: a target added on the bound scene gets its lists at the tail; removing index 0 then
    re-indexes the last target, whose block of starts, ok and far move with it unchanged."""
    sph, box, obb, targets = cs.small_resident(owners=(1, 2))
    recs = (sph, box, obb)
    with art.Context(1) as c:
        store = bind_resident_targets(c, recs, targets, reserve=6)
        check_lists(c, recs, targets)
        new = np.array([-6.5, 8.0, -2.25], np.float32)
        assert store.add(new) == 4
        store.sync()
        rs = store.last_resize()
        assert rs["kept_bound"] == 1 and rs["added"] == 1 and rs["lists_rebuilt"] == 1 and rs["lists_full_rebuild"] == 0, rs
        five = np.concatenate([targets, new[None]])
        grown = check_lists(c, recs, five, full=False)
        store.remove_swapback(0)   # no collider names target 0 or 4: the survivor's block moves
        store.sync()
        rs = store.last_resize()
        assert rs["kept_bound"] == 1 and rs["removed"] == 1 and rs["lists_moved"] == 1 and rs["lists_rebuilt"] == 0, rs
        four = np.concatenate([new[None], targets[1:]])
        after = check_lists(c, recs, four, full=False)
        a, b = blocks(grown, 4), blocks(after, 0)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], "the moved survivor's lists, ok or far changed"
        for t in (1, 2, 3):
            a, b = blocks(grown, t), blocks(after, t)
            assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
        c.set_flags(0)


# ------------------------------------------------------------------------------------------------
# Resident collider store: lists kept under small moves, count changes
# ------------------------------------------------------------------------------------------------
KIND_OF = {SPH: 0, BOX: 1, OBB: 2}


class ResidentColliders:
    def __init__(self, c, recs, targets, reserve=None):
        self.c, self.recs, self.targets = c, [r.copy() for r in recs], targets
        self.store = ColliderStore(c)
        self.store.clear()
        if reserve:
            self.store.reserve(*reserve)
        for k in (SPH, BOX, OBB):
            self.store.add_many(k, self.recs[k])
        self.store.sync()
        c.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
        c.bind(resident_frame(make_frame(*self.recs, targets)))

    def radius(self, k, i):
        """The bounding radius cell_slack takes: |radius|, or |size|_2."""
        r = self.recs[k][i]
        e = r["radius"] if k == SPH else r["size"]
        return float(np.linalg.norm(np.atleast_1d(e).view(np.float16).astype(np.float64)))

    def nudge(self, k, i, frac, rng, inward=True):
        """Move collider i of kind k by frac * cell_slack(r) in a random direction; the new centre is a half
        vector, each coordinate rounded towards its old value (inward: the move is at most that long, and
        shorter by less than 0.03 at these coordinates) or to the nearest. Returns the length moved."""
        r = self.recs[k][i:i + 1].copy()
        c0 = r["center"].view(np.float16).astype(np.float64).reshape(3)
        d = rng.normal(size=3)
        want = c0 + d / np.linalg.norm(d) * frac * cr.cell_slack(self.radius(k, i))
        h = want.astype(np.float16)
        if inward:
            over = np.abs(h.astype(np.float64) - c0) > np.abs(want - c0)
            h[over] = np.nextafter(h[over], c0[over].astype(np.float16))
        moved = float(np.linalg.norm(h.astype(np.float64) - c0))
        assert not inward or moved <= frac * cr.cell_slack(self.radius(k, i))
        r["center"] = h.view(np.uint16).reshape(1, 3)
        self.recs[k][i] = r[0]
        self.store.set(k, i, r[0])
        return moved


def test_lists_kept_under_small_moves():
    """A fifth of the colliders moved by 0.499 cell_slack(r): the sync keeps the lists (byte-identical), and they
    still cover the moved shapes with valid near bounds; one collider moved by 0.6 cell_slack(r): rebuilt."""
    sph, box, obb, targets = cs.small_resident()
    rng = np.random.default_rng(10)
    with art.Context(1) as c:
        res = ResidentColliders(c, (sph, box, obb), targets)
        before = check_lists(c, res.recs, targets)
        bounds0 = c.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS)
        moved = []
        for k in (SPH, BOX, OBB):
            for i in rng.choice(res.recs[k].size, res.recs[k].size // 5, replace=False):
                moved.append(res.nudge(k, int(i), 0.499, rng) / cr.cell_slack(res.radius(k, int(i))))
        assert min(moved) > 0.35, min(moved)   # (of the slack: 0.499 less the rounding to halves)
        st = res.store.sync()
        assert st["cells_rebuilt"] == 0 and st["dirty_records"] == len(moved), st
        kept = check_lists(c, res.recs, targets, bloat=False, far_bounds=bounds0)   # coverage and near bounds at the moved positions
        assert np.array_equal(kept.start, before.start) and np.array_equal(kept.raw, before.raw) and kept.info == before.info
        assert kept.raw.size == before.info["tail"]
        big = int(np.argmax([res.radius(BOX, i) for i in range(res.recs[BOX].size)]))
        assert res.nudge(BOX, big, 0.6, rng, inward=False) > 0.55 * cr.cell_slack(res.radius(BOX, big))
        st = res.store.sync()
        assert st["cells_rebuilt"] == 1, st
        check_lists(c, res.recs, targets)
        c.set_flags(0)


def test_collider_count_changes():
    """art_colliders_reserve: colliders added, removed (swap-back) and re-owned on the bound scene; the lists
    are rebuilt by each sync and hold the new indices and owners."""
    sph, box, obb, targets = cs.small_resident()
    rng = np.random.default_rng(11)
    with art.Context(1) as c:
        res = ResidentColliders(c, (sph, box, obb), targets, reserve=(sph.size + 8, box.size + 8, obb.size + 8))
        check_lists(c, res.recs, targets)

        def synced(what):
            st, rs = res.store.sync(), res.store.last_resize()
            assert st["cells_rebuilt"] == 1, (what, st, rs)
            check_lists(c, res.recs, targets)
            return rs

        new = cs.records(0, [[3.0, -4.0, 5.0]], [1.25], rng, tid=2)
        assert res.store.add(SPH, new[0]) == sph.size
        res.recs[SPH] = np.concatenate([res.recs[SPH], new])
        rs = synced("a sphere added")
        assert rs["kept_bound"] == 1 and rs["added"] == 1, rs
        res.store.remove_swapback(BOX, 0)   # the last box takes index 0
        res.recs[BOX][0] = res.recs[BOX][-1]
        res.recs[BOX] = res.recs[BOX][:-1].copy()
        rs = synced("a box removed")
        assert rs["kept_bound"] == 1 and rs["removed"] == 1, rs
        i = int(np.nonzero(res.recs[OBB]["audio_target_id"] == -1)[0][0])   # an unowned OBB becomes target 1's
        r = res.recs[OBB][i].copy()
        r["audio_target_id"] = 1
        res.recs[OBB][i] = r
        res.store.set(OBB, i, r)
        synced("an OBB changed owner")
        j = int(np.nonzero(res.recs[SPH]["audio_target_id"] == 2)[0][0])    # and an owned sphere is released
        r = res.recs[SPH][j].copy()
        r["audio_target_id"] = -1
        res.recs[SPH][j] = r
        res.store.set(SPH, j, r)
        synced("a sphere released")
        c.set_flags(0)


# ------------------------------------------------------------------------------------------------
# The walk: a scene whose every shell collider is some muffle ray's sole blocker
# ------------------------------------------------------------------------------------------------
def test_sole_blockers_outputs(monkeypatch):
    """Outputs of a scene in which each of 48 shell colliders decides some muffle ray alone
    (test_cells_ref_cpu.py shows that on the oracle): a walk that steps over an entry, stops a list early or
    reads past its end changes the muffle counts. Byte parity with the oracle through the lists (no ray falls
    back), and the same bytes from the brute path (ART_CELLS_MAX_PAIRS=1)."""
    sph, box, obb, targets, origins = cs.sole_blockers()
    scene, params, org = sole_blocker_frame(sph, box, obb, targets, origins)
    want = art.FanOutputs(2, 512, 1, scene.T, params.thread_count)
    oracle.run(scene, params, org, want)

    def run():
        out = art.FanOutputs(2, 512, 1, scene.T, params.thread_count)
        with art.Context(1) as c:
            c.set_flags(abi.ART_CTX_COUNT_EXECUTED)
            c.executed_counts()
            c.run(art.Frame(scene, params, org, out))
            return out, c.executed_counts()

    out, ex = run()
    eq = out.equal(want)
    assert all(eq.values()), eq
    assert (out.muffle != 0).any() and ex["muffle_fallback"] == 0 and ex["cell_entries"] > 0, ex
    monkeypatch.setenv("ART_CELLS_MAX_PAIRS", "1")
    brute, ex = run()
    assert all(brute.equal(out).values()) and ex["muffle_fallback"] > 0 and ex["cell_entries"] == 0, ex

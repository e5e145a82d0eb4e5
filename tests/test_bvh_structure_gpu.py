"""The collider BVH (csrc/art_bvh.hip) against the host restatement of its rules (tests/bvh_ref.py),
bit for bit: the broad-phase bounds of spheres and AABBs, the leaf order of every size class of the
build, and node boxes that are the exact unions of their colliders' bounds, after a build and after
every resident sync's refit. Output parity cannot see these: any leaf order with boxes that contain
their colliders gives the same outputs.

Scenes are bound only (one fan of 8 rays, no frame) unless a test says otherwise; the structures are
read back through art_debug_leaf_order and art_debug_bvh_records. OBB bounds are taken as read back
(test_cull_bounds.py checks their arithmetic)."""
import ctypes as C

import numpy as np
import pytest

import art
import bvh_ref
from art import abi
from art.colliders import ColliderStore, resident_frame
from art.synth import fibonacci_directions
from bvh_ref import check_tree, cull_bounds, kd_order

pytestmark = pytest.mark.gpu

# every switch of the build's implementation and every partial-leaf edge
COUNTS = [1, 4, 5, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385,
          65536, 65537]
EXTRA = [65, 1025, 4097, 16385]
TARGETS = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 2.0]], np.float32)


def make_frame(sph, box, obb, S=1, R=8):
    scene = art.Scene(dirs=fibonacci_directions(R), targets=TARGETS, spheres=sph, aabbs=box, obbs=obb)
    params = art.FrameParams(max_hits_per_ray=2)
    org = np.linspace(-3.0, 3.0, 3 * S, dtype=np.float32).reshape(S, 3)
    return art.Frame(scene, params, org, art.FanOutputs(S, R, params.max_hits_per_ray, scene.T, params.thread_count))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 8)


def read_back(c, ns, na, n):
    """(bounds, leaf order as global indices, nodes) of the scene bound on c."""
    bounds = c.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS)
    nodes = c.debug_bvh_records(abi.ART_DEBUG_BVH_NODES)
    ref = c.debug_leaf_order(n)
    assert bounds.size == n and ref.size == n and nodes.size == (bvh_ref.capacity(n) - 1) // 3
    kind, idx = ref >> 30, (ref & 0x3fffffff).astype(np.int64)
    assert (kind <= 2).all()
    return bounds, idx + np.where(kind == 0, 0, np.where(kind == 1, ns, ns + na)), nodes


def differing(got, want):
    return np.nonzero((bits(got) != bits(want)).any(axis=1))[0]


def check_bound_scene(c, sph, box, obb, order_is=None):
    """The three structural checks on the scene bound on c; returns what was read back. order_is: the
    leaf order a refit must have kept (otherwise the order must be the build's)."""
    ns, na = sph.size, box.size
    n = ns + na + obb.size
    bounds, order, nodes = read_back(c, ns, na, n)
    d = differing(bounds[:ns + na], cull_bounds(sph, box))
    assert d.size == 0, f"{d.size} sphere / AABB bounds differ, first {d[:8]}"
    want = kd_order(bounds["lo"], bounds["hi"]) if order_is is None else order_is
    d = np.nonzero(order != want)[0]
    assert d.size == 0, f"{d.size} of {n} leaf positions differ, first {d[:8]}"
    d = check_tree(bounds, order, nodes)
    assert d.size == 0, f"{d.size} of {nodes.size} nodes are not the union of their colliders, first {d[:8]}"
    return bounds, order, nodes


def scene_of(kind, n):
    if kind == "random":
        return bvh_ref.random_scene(n, 7 * n + 1, with_obb=COUNTS.index(n) % 3 == 2)
    make = {"ties": bvh_ref.ties_scene, "line": bvh_ref.line_scene, "nonfinite": bvh_ref.nonfinite_scene}[kind]
    return make(n, 7 * n + 2)


@pytest.mark.parametrize("kind,n", [("random", n) for n in COUNTS] + [(k, n) for k in ("ties", "line", "nonfinite") for n in EXTRA])
def test_build_matches_the_reference(ctx, kind, n):
    sph, box, obb = scene_of(kind, n)
    ctx.set_flags(0)
    ctx.bind(make_frame(sph, box, obb))
    check_bound_scene(ctx, sph, box, obb)


@pytest.mark.parametrize("n", [65, 1025, 4097])
def test_block_passes_match_the_reference(monkeypatch, n):
    """ART_KD_WAVE=0: the block passes run every level, pinned to the same reference as the wave pass."""
    monkeypatch.setenv("ART_KD_WAVE", "0")
    sph, box, obb = scene_of("random", n)
    with art.Context(1) as c:
        c.bind(make_frame(sph, box, obb))
        check_bound_scene(c, sph, box, obb)


def test_read_back_errors_and_empty_scene():
    none = np.zeros(0, abi.SPHERE)
    with art.Context(1) as c:
        buf = np.zeros(8, np.float32)
        p = buf.ctypes.data_as(C.POINTER(C.c_float))
        assert c.lib.art_debug_bvh_records(c.ptr, abi.ART_DEBUG_BVH_NODES, p, 1) == abi.ART_E_STATE  # nothing bound
        c.bind(make_frame(none, np.zeros(0, abi.AABB), np.zeros(0, abi.OBB)))
        assert c.debug_bvh_records(abi.ART_DEBUG_BVH_NODES).size == 0  # no colliders: no BVH
        assert c.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS).size == 0
        sph, box, obb = scene_of("random", 5)
        c.bind(make_frame(sph, box, obb))
        assert c.lib.art_debug_bvh_records(c.ptr, 2, p, 1) == abi.ART_E_INVALID
        assert c.lib.art_debug_bvh_records(c.ptr, abi.ART_DEBUG_BVH_NODES, None, 1) == abi.ART_E_INVALID
        assert c.lib.art_debug_bvh_records(c.ptr, abi.ART_DEBUG_BVH_NODES, p, 1) == 5  # 4 leaves and the root
        assert np.array_equal(buf.view(np.uint32), bits(c.debug_bvh_records(abi.ART_DEBUG_BVH_NODES))[0])


# ------------------------------------------------------------------------------------------------
# Refit: a resident scene through a sequence of syncs.
# ------------------------------------------------------------------------------------------------
KINDS = (abi.ART_KIND_SPHERE, abi.ART_KIND_AABB, abi.ART_KIND_OBB)
INF16, FAR = 0x7C00, 30000.0


def refit_scene(name):
    if name == "5":
        return bvh_ref.random_scene(5, 31, with_obb=True)
    if name == "4096":
        return bvh_ref.random_scene(4096, 32)
    if name == "4096-obb":
        rng = np.random.default_rng(33)
        return bvh_ref.make_records(rng.uniform(-40.0, 40.0, (4096, 3)), rng.uniform(0.05, 2.0, (4096, 3)), rng, 0, 0)
    return bvh_ref.random_scene(int(name), 34)  # 65536: the fused sync's limit; 65537: the unfused refit


class Resident:
    """A resident scene and the host's copy of its records."""

    def __init__(self, c, recs, S, R):
        self.c, self.recs, self.S, self.R = c, [r.copy() for r in recs], S, R
        self.store = ColliderStore(c)
        for k in KINDS:
            self.store.add_many(k, self.recs[k])
        self.store.sync()
        self.bind()

    def bind(self):
        self.c.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
        self.c.bind(resident_frame(make_frame(*self.recs, S=self.S, R=self.R)))

    @property
    def n(self):
        return sum(r.size for r in self.recs)

    def split(self, ids):
        """Global indices -> (kind, indices in that kind's list), kind by kind."""
        ids = np.sort(np.asarray(ids, np.int64))
        first = 0
        for k in KINDS:
            m = ids[(ids >= first) & (ids < first + self.recs[k].size)] - first
            if m.size:
                yield k, m
            first += self.recs[k].size

    def move(self, ids, rng=None, scale=4.0, centre=None):
        """Jitter the centres of colliders ids (or set them to centre: 3 half-precision bit patterns)."""
        for k, m in self.split(ids):
            r = self.recs[k][m].copy()
            if centre is not None:
                r["center"] = np.asarray(centre, np.uint16)
            else:
                c = r["center"].view(np.float16).astype(np.float32) + rng.uniform(-scale, scale, (m.size, 3)).astype(np.float32)
                r["center"] = c.astype(np.float16).view(np.uint16).reshape(m.size, 3)
            self.recs[k][m] = r
            self.store.set_many(k, m.astype(np.int32), r)

    def centre_of(self, g):
        (k, m), = self.split([g])
        return self.recs[k]["center"][m[0]].copy()


@pytest.mark.parametrize("name", ["5", "4096", "4096-obb", "65536", "65537"])
def test_refit_keeps_exact_unions(name):
    """Every sync of moved colliders leaves the bound scene with the bind's leaf order, the moved records'
    bounds and node boxes that are exact unions again: the fused one-workgroup sync (sync_refit_kernel:
    only the dirty leaves and their ancestors) up to 65536 colliders, the full refit above. Boxes that
    grew for a far collider must shrink when it returns. A count change asks for a new bind, whose order
    is the build's at the new count. At 65537 colliders a small frame on the refit tree must equal an
    upload frame of the same records."""
    # Which refit runs is not reported by the library; the sizes assume art_store.cpp's choice: the
    # fused launch for a bound resident scene of at most kSyncRefitMax = 65536 colliders with a BVH,
    # launch_refit_scene above it. If kSyncRefitMax moves, move the last two sizes with it.
    rng = np.random.default_rng(5)
    big = name == "65537"
    S, R = (4, 64) if big else (1, 8)
    with art.Context(1) as c:
        res = Resident(c, refit_scene(name), S, R)
        n, f16 = res.n, bvh_ref._f16
        bounds0, order0, nodes0 = check_bound_scene(c, *res.recs)  # the bind: a build

        def synced(moved_ids, what):
            st = res.store.sync()
            assert st["dirty_records"] == len(moved_ids) and not st["reallocated"] and not st["full_prep"], (what, st)
            return check_bound_scene(c, *res.recs, order_is=order0)

        one = int(rng.integers(0, n))
        res.move([one], rng)
        synced([one], "one collider moved")
        some = rng.choice(n, max(1, n // 100), replace=False)
        res.move(some, rng)
        bounds, _, nodes = synced(some, "1 % moved")
        # untouched OBB bounds stay as they were
        keep = np.setdiff1d(np.arange(n), np.concatenate([some, [one]]))
        assert np.array_equal(bits(bounds)[keep], bits(bounds0)[keep])

        far = int(rng.integers(0, n))
        home = res.centre_of(far)
        res.move([far], centre=f16([FAR, -FAR, FAR]))
        _, _, grown = synced([far], "one collider far outside")
        assert grown[0]["hi"][0] > FAR - 100 and grown[0]["lo"][1] < -FAR + 100 and nodes[0]["hi"][0] < 1000
        res.move([far], centre=home)
        _, _, shrunk = synced([far], "the far collider back")
        assert np.array_equal(bits(shrunk), bits(nodes)), "the boxes before the excursion"

        res.move([far], centre=[INF16, home[1], home[2]])
        b, _, hollow = synced([far], "one collider non-finite")
        assert b[far]["lo"][2] == -np.inf and hollow[0]["hi"][1] == np.inf
        res.move([far], centre=home)
        _, _, again = synced([far], "the non-finite collider restored")
        assert np.array_equal(bits(again), bits(nodes))

        res.move(np.arange(n), rng)
        bounds, _, _ = synced(np.arange(n), "every collider moved")
        with art.Context(1) as up:  # the bounds a sync writes are those an upload of the same records computes (OBBs too)
            up.bind(make_frame(*res.recs, S=S, R=R))
            assert np.array_equal(bits(up.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS)), bits(bounds))
            if big:  # an output-level check of the unfused refit
                fr = make_frame(*res.recs, S=S, R=R)
                o_res, o_up = fr.out, fr.out.copy()
                c.run(resident_frame(fr))
                up.run(art.Frame(fr.scene, fr.params, fr.origins, o_up))
                eq = o_res.equal(o_up)
                assert all(eq.values()), eq
                assert (o_res.echo != 0).any()
                check_bound_scene(c, *res.recs, order_is=order0)  # the frame used the refit tree as it was

        k = abi.ART_KIND_OBB if name == "4096-obb" else abi.ART_KIND_SPHERE  # a count change: sync, then bind again
        rec = res.recs[k][:1].copy()
        rec["center"] = f16([[3.0, -2.0, 1.0]])
        res.store.add(k, rec[0])
        res.recs[k] = np.concatenate([res.recs[k], rec])
        res.store.sync()
        res.bind()
        check_bound_scene(c, *res.recs)
        c.set_flags(0)

"""Colliders that appear and disappear on a bound scene (include/art_colliders.h, ABI 3.10;
DESIGN.md §3b, "Colliders that appear and disappear").

A resident scene bound after art_colliders_reserve follows an art_colliders_sync that changes a
count: the leaf order is relabelled on the device (or sorted again in place), every node box is
recomputed and the cell lists are rebuilt, with nothing allocated or rebound. Every step is checked
three ways, as in test_targets_resize_gpu.py: the launch on the synced context, without a rebind, is
byte-equal to a fresh context bound with the model's arrays and to the oracle, and the statistics
say kept_bound 1 and reallocated 0. After every step the structure is checked too: the leaf order
read back equals the host restatement of the relabel rule (bvh_relabel_ref.py) applied to the order
read before the step, and the nodes equal bvh_ref.build_nodes over the device's bounds in that order,
bit for bit. Shapes: S = 4 fans, R = 128 rays, T = 4, config 2's generator at 256 colliders (the scene
of test_targets_gpu.py); 256 -> 257 colliders crosses a tree level (64 -> 65 leaves), 4 -> 5 too.
"""
import numpy as np
import pytest

import art
from art import abi
from art.colliders import KINDS, ColliderStore, resident_frame
from art.targets import TargetStore, resident_targets_frame
import bvh_ref
import bvh_relabel_ref as rr
import oracle
from test_colliders_gpu import KIND_FIELDS, ListsModel, scene_with
from test_targets_gpu import R, S, base_scene

pytestmark = pytest.mark.gpu

SPH, BOX, OBB = abi.ART_KIND_SPHERE, abi.ART_KIND_AABB, abi.ART_KIND_OBB
CAP = (136, 136, 8)


@pytest.fixture(autouse=True)
def relabel_between_sorts(monkeypatch):
    """The shipped default sorts the leaf order again at every count change (its own test below); the
    other tests ask for the relabel path, with a re-sort once an eighth of the colliders has churned."""
    monkeypatch.setenv("ART_BVH_RESORT_DEN", "8")


def pools():
    """Replacement and new records: config 2's generator with another seed, config 3's for the OBBs."""
    p2 = art.synth(art.CONFIGS[2], S=S, R=R, C_scale=0.0625, seed=77)[0]
    p3 = art.synth(art.CONFIGS[3], S=S, R=R, C_scale=0.0625, seed=78)[0]
    p3.obbs["audio_target_id"] = -1
    return {SPH: p2.spheres, BOX: p2.aabbs, OBB: p3.obbs}


def subset(scene, ns, na, no=0, obbs=None):
    return art.Scene(dirs=scene.dirs, targets=scene.targets, spheres=scene.spheres[:ns].copy(),
                     aabbs=scene.aabbs[:na].copy(), obbs=(obbs[:no].copy() if no else np.zeros(0, abi.OBB)))


class CRig:
    """A context whose bound resident scene follows the collider store, and the model that checks it."""

    def __init__(self, scene, org, params, cap=CAP, target_cap=0):
        import torch
        self.torch = torch
        self.scene, self.org, self.params, self.cap = scene, org, params, cap
        self.ctx = art.Context(1)
        self.store, self.model = ColliderStore(self.ctx), ListsModel()
        self.dev = torch.device("cuda", 0)
        self.d_org = torch.from_numpy(np.ascontiguousarray(org)).to(self.dev)
        self.targets = [p.copy() for p in scene.targets]
        self.flags = abi.ART_CTX_RESIDENT_COLLIDERS
        self.tstore = None
        if target_cap:
            self.tstore = TargetStore(self.ctx)
            self.tstore.reserve(target_cap)
            self.tstore.add_many(scene.targets)
            self.tstore.sync()
            self.flags |= abi.ART_CTX_RESIDENT_TARGETS
        self.store.reserve(*cap)
        assert [self.store.capacity(k) for k in KINDS] == list(cap)
        for k, name in KIND_FIELDS.items():
            for rec in getattr(scene, name):
                assert self.store.add(k, rec) == self.model.add(k, rec)
        st = self.store.sync()
        assert st["reallocated"] == 1
        assert self.store.last_resize()["kept_bound"] == 0  # nothing bound yet
        self.model.synced()
        self.ctx.set_flags(self.flags)
        self.bind()

    def counts(self):
        return tuple(len(self.model.lists[k]) for k in KINDS)

    def model_scene(self):
        sc = scene_with(self.scene, self.model)
        sc.targets = np.ascontiguousarray(np.array(self.targets, np.float32).reshape(-1, 3))
        return sc

    def outputs(self, T):
        return art.FanOutputs(S, R, self.params.max_hits_per_ray, T, self.params.thread_count)

    def bind(self):
        fr = resident_frame(art.Frame(self.model_scene(), self.params, self.org, self.outputs(len(self.targets))))
        self.ctx.bind(resident_targets_frame(fr) if self.tstore else fr)

    def lay(self, scene):
        return art.fan_layout(art.Frame(scene, self.params, self.org, self.outputs(scene.T)))

    def block(self, scene=None):
        scene = scene or self.model_scene()
        return self.torch.from_numpy(art.pack_block(self.outputs(scene.T), self.lay(scene))).to(self.dev)

    def launch(self, blk=None):
        blk = self.block() if blk is None else blk
        self.ctx.launch_device(self.d_org.data_ptr(), S, blk.data_ptr(), 0, self.torch.cuda.current_stream().cuda_stream)
        return blk

    def check(self, blk, scene=None, what="", plan=True):
        """blk against a fresh context bound with the model's arrays (its plan bits and leaf order are
        returned too), and against the oracle."""
        torch = self.torch
        scene = scene or self.model_scene()
        torch.cuda.synchronize()
        with art.Context(1) as ref:
            ref.bind(art.Frame(scene, self.params, self.org, self.outputs(scene.T)))
            rblk = self.block(scene)
            ref.launch_device(self.d_org.data_ptr(), S, rblk.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ref_plan, ref_order = ref.debug_last_plan(), ref.debug_leaf_order(max(scene.C, 1))
        assert torch.equal(blk, rblk), f"{what}: differs from a fresh bind"
        if plan:
            assert self.ctx.debug_last_plan() == ref_plan, (what, abi.plan_names(self.ctx.debug_last_plan()), abi.plan_names(ref_plan))
        o_ref = self.outputs(scene.T)
        oracle.run_frame(art.Frame(scene, self.params, self.org, o_ref), threads=8)
        got = art.unpack_block(blk.cpu().numpy(), self.lay(scene), S, R, self.params.max_hits_per_ray, scene.T,
                               self.params.thread_count)
        eq = got.equal(o_ref)
        assert all(eq.values()), f"{what}: oracle {eq}"
        self.ref_order = ref_order
        return got

    def apply(self, ops):
        for op in ops:
            if op[0] == "add":
                assert self.store.add(op[1], op[2]) == self.model.add(op[1], op[2])
            elif op[0] == "remove":
                self.store.remove_swapback(op[1], op[2])
                self.model.remove_swapback(op[1], op[2])
            else:
                self.store.set(op[1], op[2], op[3])
                self.model.set(op[1], op[2], op[3])

    def edit(self, ops, kept=True, structure=True):
        """ops: ("add", kind, rec) | ("remove", kind, index) | ("set", kind, index, rec), applied to the
        store and the model, then one sync. Returns art_collider_resize_stats after the checks every kept
        step shares: the statistics, and the structure against the relabel rule."""
        old = self.counts()
        before = self.ctx.debug_leaf_order(max(sum(old), 1)) if structure else None
        self.apply(ops)
        new = self.counts()
        st = self.store.sync()
        rs = self.store.last_resize()
        self.model.synced()
        for k in KINDS:
            assert self.store.count(k) == new[k]
        assert rs["added"] == sum(max(0, b - a) for a, b in zip(old, new)), rs
        assert rs["removed"] == sum(max(0, a - b) for a, b in zip(old, new)), rs
        assert rs["cells_rebuilt"] == st["cells_rebuilt"] and rs["bytes_uploaded"] == st["bytes_uploaded"], (st, rs)
        if not kept:
            assert rs["kept_bound"] == 0, rs
            return rs
        assert st["reallocated"] == 0, st
        if new == old:
            assert rs["kept_bound"] == 0 and st["full_prep"] == 0, rs  # no count change: the move path
            return rs
        assert rs["kept_bound"] == 1 and rs["cells_rebuilt"] == 1 and st["full_prep"] == 1, (rs, st)
        if structure and sum(new):
            after = self.ctx.debug_leaf_order(sum(new))
            bounds = self.ctx.debug_bvh_records(abi.ART_DEBUG_BVH_BOUNDS)
            nodes = self.ctx.debug_bvh_records(abi.ART_DEBUG_BVH_NODES)
            assert after.size == sum(new) and bounds.size == sum(new)
            assert sorted(after.tolist()) == rr.labels_of(new)
            if rs["bvh_rebuilt"]:
                assert rs["relabelled"] == 0
                assert bvh_ref.check_tree(bounds, rr.order_of(after, new), nodes).size == 0
            else:
                assert rs["relabelled"] == rr.check(before, old, new, after, bounds, nodes), rs
            levels = [bvh_ref.capacity(n) if n else 0 for n in (sum(old), sum(new))]
            assert rs["levels_changed"] == (1 if levels[0] != levels[1] else 0), (rs, levels)
        return rs

    def close(self):
        self.ctx.set_flags(0)
        self.ctx.close()


def test_adds():
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        got = rig.check(rig.launch(), what="bound")
        assert (got.echo != 0).any() and (got.muffle != 0).any()
        plan = rig.ctx.debug_last_plan()
        for step, k in enumerate((SPH, BOX, SPH, BOX)):
            rs = rig.edit([("add", k, pool[k][step])])
            assert rs["added"] == 1 and rs["removed"] == 0 and rs["bvh_rebuilt"] == 0 and rs["relabelled"] == 1, (step, rs)
            assert rs["bytes_uploaded"] > 0
            rig.check(rig.launch(), what=f"add {step}")
            assert rig.ctx.debug_last_plan() == plan  # the kind set is unchanged
        rs = rig.edit([("add", OBB, pool[OBB][0])])  # the third kind (its own test looks at the plan bits)
        assert rs["added"] == 1 and rs["relabelled"] == 1, rs
        rig.check(rig.launch(), what="add an OBB")
        st = rig.store.sync()  # nothing changed: nothing moves
        assert st["dirty_records"] == 0 and rig.store.last_resize()["kept_bound"] == 0
        rig.check(rig.launch(), what="empty sync")
    finally:
        rig.close()


def test_removes():
    scene, org, params = base_scene(2, T=4)
    rig = CRig(scene, org, params)
    try:
        rig.check(rig.launch(), what="bound")
        # index 0 of the spheres shifts every AABB's global index; the last index moves nothing
        for what, k, i in (("sphere 0", SPH, 0), ("last sphere", SPH, 126), ("AABB 0", BOX, 0), ("last AABB", BOX, 126),
                           ("a middle sphere", SPH, 60)):
            rs = rig.edit([("remove", k, i)])
            assert rs["removed"] == 1 and rs["added"] == 0 and rs["bvh_rebuilt"] == 0, (what, rs)
            assert rs["relabelled"] <= 1  # the tail position moves into the hole, unless the hole is the tail
            rig.check(rig.launch(), what=what)
        for k, i in ((SPH, -1), (SPH, 125), (BOX, 1 << 20)):  # invalid ids: skipped, nothing to sync
            rig.edit([("remove", k, i)])
        rig.check(rig.launch(), what="invalid ids")
    finally:
        rig.close()


def test_mixed_batches():
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        rig.check(rig.launch(), what="bound")
        # a > h: three adds, one remove, and a survivor set
        rs = rig.edit([("add", SPH, pool[SPH][0]), ("remove", BOX, 5), ("add", SPH, pool[SPH][1]), ("add", SPH, pool[SPH][2]),
                       ("set", BOX, 9, pool[BOX][9])])
        assert (rs["added"], rs["removed"]) == (3, 1) and rs["relabelled"] == 3, rs
        rig.check(rig.launch(), what="a > h")
        # a = h: a sphere leaves, an AABB comes, a collider added in the batch is removed again
        rs = rig.edit([("remove", SPH, 0), ("add", BOX, pool[BOX][0]), ("add", BOX, pool[BOX][1]), ("remove", BOX, 128),
                       ("set", SPH, 3, pool[SPH][3])])
        assert (rs["added"], rs["removed"]) == (1, 1) and rs["relabelled"] == 1, rs
        rig.check(rig.launch(), what="a = h")
        # h > a: four removes over both kinds (index 0 included), one add
        rs = rig.edit([("remove", SPH, 0), ("remove", SPH, 17), ("remove", SPH, 127), ("remove", SPH, 40),
                       ("add", BOX, pool[BOX][2]), ("set", BOX, 0, pool[BOX][3])])
        assert (rs["added"], rs["removed"]) == (1, 4) and 1 <= rs["relabelled"] <= 4, rs
        rig.check(rig.launch(), what="h > a")
        # the same number in and out of one kind: no label changes, the move path takes it
        rs = rig.edit([("remove", SPH, 2), ("add", SPH, pool[SPH][4])])
        assert (rs["added"], rs["removed"], rs["kept_bound"]) == (0, 0, 0)
        rig.check(rig.launch(), what="remove + add of one kind")
    finally:
        rig.close()


def test_level_crossing_256(monkeypatch):
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        rig.check(rig.launch(), what="256")
        rs = rig.edit([("add", BOX, pool[BOX][0])])  # 65 leaves: 4 -> 5 levels
        assert rs["levels_changed"] == 1 and rs["bvh_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="257")
        rs = rig.edit([("remove", SPH, 7)])
        assert rs["levels_changed"] == 1 and rs["bvh_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="256 again")
    finally:
        rig.close()


def test_level_crossing_small_and_empty(monkeypatch):
    monkeypatch.setenv("ART_BVH_RESORT_DEN", "0")  # (an eighth of 4 colliders is 0: it would sort again)
    scene, org, params = base_scene(2, T=4)
    pool = pools()
    rig = CRig(subset(scene, 2, 2), org, params, cap=(8, 8, 0))
    try:
        rig.check(rig.launch(), what="4")
        rs = rig.edit([("add", SPH, pool[SPH][0])])  # 2 leaves: 1 -> 2 levels
        assert rs["levels_changed"] == 1 and rs["bvh_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="5")
        rs = rig.edit([("remove", BOX, 0)])
        assert rs["levels_changed"] == 1 and rs["bvh_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="4 again")
    finally:
        rig.close()
    rig = CRig(subset(scene, 1, 0), org, params, cap=(8, 8, 0))
    try:
        rig.check(rig.launch(), what="1")
        rs = rig.edit([("remove", SPH, 0)])
        assert rs["bvh_rebuilt"] == 1 and rs["kept_bound"] == 1, rs
        got = rig.check(rig.launch(), what="empty")
        assert not (got.echo != 0).any()  # every ray misses
        rs = rig.edit([("add", BOX, pool[BOX][0]), ("add", SPH, scene.spheres[0]), ("add", BOX, pool[BOX][1])])
        assert rs["bvh_rebuilt"] == 1 and rs["added"] == 3, rs
        rig.check(rig.launch(), what="3")
        assert np.array_equal(rig.ctx.debug_leaf_order(3), rig.ref_order)
    finally:
        rig.close()


def test_obb_kind_appears_and_leaves():
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        rig.check(rig.launch(), what="bound")
        plan = rig.ctx.debug_last_plan()
        assert not plan & abi.ART_PLAN_OBB
        rs = rig.edit([("add", OBB, pool[OBB][3])])  # the leaf slots go from 32 B to 64 B
        assert rs["kept_bound"] == 1 and rs["bvh_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="first OBB")  # (check compares the plan bits with the fresh bind's)
        assert rig.ctx.debug_last_plan() & abi.ART_PLAN_OBB
        rs = rig.edit([("add", OBB, pool[OBB][4]), ("remove", OBB, 0)])  # the survivor jumps to index 0
        rig.check(rig.launch(), what="one OBB, swapped")
        rs = rig.edit([("remove", OBB, 0)])
        assert rs["kept_bound"] == 1 and rs["removed"] == 1, rs
        rig.check(rig.launch(), what="last OBB gone")
        assert rig.ctx.debug_last_plan() == plan
    finally:
        rig.close()


def test_an_add_that_matters():
    scene, org, params = base_scene(2, T=4)
    rig = CRig(scene, org, params)
    try:
        before = rig.check(rig.launch(), what="bound")
        mid = 0.5 * (org[0] + scene.targets[1])
        rec = scene.spheres[-1:].copy()
        rec["center"][0] = bvh_ref._f16(mid)
        rec["radius"][0] = bvh_ref._f16(0.25 * np.linalg.norm(scene.targets[1] - org[0]))
        rec["audio_target_id"][0] = -1
        rs = rig.edit([("add", SPH, rec[0])])
        assert rs["kept_bound"] == 1
        after = rig.check(rig.launch(), what="a sphere between fan 0 and target 1")
        assert not np.array_equal(before.muffle[0], after.muffle[0]) and not np.array_equal(before.echo[0], after.echo[0])
    finally:
        rig.close()


def test_churn_resort_every_change(monkeypatch):
    monkeypatch.setenv("ART_BVH_RESORT_DEN", "1")
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        for what, ops in (("add", [("add", SPH, pool[SPH][0])]), ("remove", [("remove", BOX, 3), ("remove", SPH, 0)])):
            rs = rig.edit(ops)
            assert rs["kept_bound"] == 1 and rs["bvh_rebuilt"] == 1 and rs["relabelled"] == 0, rs
            rig.check(rig.launch(), what=f"sorted again: {what}")
            assert np.array_equal(rig.ctx.debug_leaf_order(sum(rig.counts())), rig.ref_order)
    finally:
        rig.close()


def test_churn_never_resort(monkeypatch):
    monkeypatch.setenv("ART_BVH_RESORT_DEN", "0")
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    rng = np.random.default_rng(5)
    try:
        for step in range(64):  # alternating: 257, 256, 257, ... across the level boundary every time
            k = (SPH, BOX)[(step // 2) % 2]
            if step % 2 == 0:
                ops = [("add", k, pool[k][step % 128])]
            else:
                ops = [("remove", k, int(rng.integers(0, len(rig.model.lists[k]))))]
            rs = rig.edit(ops)
            assert rs["kept_bound"] == 1 and rs["bvh_rebuilt"] == 0, (step, rs)
            if step % 16 == 15:
                rig.check(rig.launch(), what=f"step {step}")
        assert not np.array_equal(rig.ctx.debug_leaf_order(256), rig.ref_order)  # (it did drift from the kd order)
    finally:
        rig.close()


def test_default_sorts_again_at_every_count_change(monkeypatch):
    monkeypatch.delenv("ART_BVH_RESORT_DEN")
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        for what, ops in (("add", [("add", BOX, pool[BOX][0])]), ("remove", [("remove", SPH, 5)]),
                          ("both", [("add", OBB, pool[OBB][0]), ("remove", BOX, 0), ("remove", BOX, 1)])):
            rs = rig.edit(ops)
            assert rs["kept_bound"] == 1 and rs["bvh_rebuilt"] == 1 and rs["relabelled"] == 0, (what, rs)
            rig.check(rig.launch(), what=f"default: {what}")
            assert np.array_equal(rig.ctx.debug_leaf_order(sum(rig.counts())), rig.ref_order)
    finally:
        rig.close()


def test_churn_threshold_of_an_eighth():
    """ART_BVH_RESORT_DEN=8: the 33rd churned collider of a 256-collider scene sorts again."""
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    try:
        rs = rig.edit([("remove", SPH, i) for i in range(16)] + [("add", BOX, pool[BOX][i]) for i in range(8)])
        assert rs["bvh_rebuilt"] == 0 and (rs["added"], rs["removed"]) == (8, 16), rs  # churn 24 <= 248 / 8
        rs = rig.edit([("add", SPH, pool[SPH][i]) for i in range(8)])
        assert rs["bvh_rebuilt"] == 0, rs                                                  # churn 32 <= 256 / 8
        rs = rig.edit([("add", SPH, pool[SPH][9])])
        assert rs["bvh_rebuilt"] == 1, rs                                                  # churn 33 > 257 / 8
        rig.check(rig.launch(), what="sorted again")
        assert np.array_equal(rig.ctx.debug_leaf_order(257), rig.ref_order)
        rs = rig.edit([("remove", BOX, 0)])
        assert rs["bvh_rebuilt"] == 0, rs                                                  # the count starts again
    finally:
        rig.close()


def test_over_capacity_unbinds_as_before():
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params, cap=(130, 128, 0)), pools()
    try:
        blk = rig.launch()
        rig.check(blk, what="bound")
        rs = rig.edit([("add", SPH, pool[SPH][i]) for i in range(3)], kept=False)  # 131 spheres > 130
        assert rs["added"] == 3 and rs["relabelled"] == 0 and rs["bvh_rebuilt"] == 0, rs
        with pytest.raises(art.ArtError) as e:
            rig.launch(blk)
        assert e.value.code == abi.ART_E_STATE
        rig.bind()  # more spheres than reserved: the kind's own count is its capacity
        rig.check(rig.launch(), what="rebound")
        rs = rig.edit([("remove", SPH, 4)])
        assert rs["kept_bound"] == 1, rs
        rig.check(rig.launch(), what="130 after the rebind")
        rs = rig.edit([("add", OBB, pool[OBB][0])], kept=False)  # no room for the kind at all
        with pytest.raises(art.ArtError) as e:
            rig.launch(blk)
        assert e.value.code == abi.ART_E_STATE
    finally:
        rig.close()


def test_nothing_reserved_unbinds_as_before():
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params, cap=(0, 0, 0)), pools()
    try:
        blk = rig.launch()
        rs = rig.edit([("add", SPH, pool[SPH][0])], kept=False, structure=False)
        with pytest.raises(art.ArtError) as e:
            rig.launch(blk)
        assert e.value.code == abi.ART_E_STATE
    finally:
        rig.close()


@pytest.mark.parametrize("switch_stream", [False, True])
def test_back_to_back_on_one_stream(switch_stream):
    """6 frames and 6 count-changing syncs with no host wait between them; every frame's block equals a
    frame computed from its own snapshot (test_pipelined_device_frames_and_syncs, with count changes)."""
    import torch
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params), pools()
    other = torch.cuda.Stream()  # (alive until the context has been closed)
    snapshots, blocks = [], []
    steps = [[("add", SPH, pool[SPH][0])], [("remove", SPH, 0), ("remove", BOX, 7)], [("add", OBB, pool[OBB][0])],
             [("add", BOX, pool[BOX][1]), ("add", BOX, pool[BOX][2]), ("set", SPH, 5, pool[SPH][5])],
             [("remove", OBB, 0), ("remove", SPH, 126)], [("add", SPH, pool[SPH][3])]]
    try:
        blks = [rig.block() for _ in steps]
        torch.cuda.synchronize()
        for step, ops in enumerate(steps):
            snapshots.append(rig.model_scene())
            stm = other.cuda_stream if switch_stream and step >= 3 else torch.cuda.current_stream().cuda_stream
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blks[step].data_ptr(), 0, stm)  # (ART_E_STATE if a sync unbound it)
            blocks.append(blks[step])
            rig.apply(ops)
            st = rig.store.sync()
            rig.model.synced()
            assert st["reallocated"] == 0 and st["full_prep"] == 1, (step, st)
        rs = rig.store.last_resize()  # (waits for the last sync: only now)
        assert rs["kept_bound"] == 1, rs
        last = rig.launch()
        torch.cuda.synchronize()
        for step, (snap, blk) in enumerate(zip(snapshots, blocks)):
            rig.check(blk, snap, what=f"frame {step}", plan=False)
        rig.check(last, what="after the run")
    finally:
        rig.close()


def test_both_reserves_together():
    """A target and a collider that it owns appear in one step (both stores reserved)."""
    scene, org, params = base_scene(2, T=4)
    rig, pool = CRig(scene, org, params, target_cap=6), pools()
    try:
        rig.check(rig.launch(), what="bound")
        new_t = base_scene(2, T=8, seed=21)[0].targets[5]
        rec = pool[SPH][:1].copy()
        rec["center"][0] = bvh_ref._f16(new_t)
        rec["audio_target_id"][0] = 4  # the new target's index
        rig.apply([("add", SPH, rec[0])])
        assert rig.tstore.add(new_t) == 4
        rig.targets.append(new_t.copy())
        st = rig.store.sync()
        rs = rig.store.last_resize()
        rig.model.synced()
        assert rs["kept_bound"] == 1 and rs["added"] == 1 and st["reallocated"] == 0, (rs, st)
        rig.tstore.sync()
        ts = rig.tstore.last_resize()
        assert ts["kept_bound"] == 1 and ts["added"] == 1, ts
        got = rig.check(rig.launch(), what="a target and its collider")
        assert got.muffle.shape[1] == 5 * params.thread_count
        # and out again, the target first
        rig.tstore.remove_swapback(4)
        rig.targets.pop()
        rig.tstore.sync()
        assert rig.tstore.last_resize()["kept_bound"] == 1
        rs = rig.edit([("remove", SPH, 128)])
        assert rs["kept_bound"] == 1, rs
        rig.check(rig.launch(), what="both gone")
    finally:
        rig.close()


def test_two_shards_host_api():
    """Two in-process shards on one GPU: every device of the context takes the same path."""
    scene, org, params = base_scene(2, T=4)
    pool = pools()
    ctx = art.Context(devices=[0, 0])
    store, model = ColliderStore(ctx), ListsModel()
    try:
        store.reserve(*CAP)
        for k, name in KIND_FIELDS.items():
            for rec in getattr(scene, name):
                assert store.add(k, rec) == model.add(k, rec)
        store.sync()
        ctx.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
        for step, op in enumerate([None, ("add", BOX, pool[BOX][0]), ("remove", SPH, 0)]):
            if op and op[0] == "add":
                assert store.add(op[1], op[2]) == model.add(op[1], op[2])
            elif op:
                store.remove_swapback(op[1], op[2])
                model.remove_swapback(op[1], op[2])
            st = store.sync()
            rs = store.last_resize()
            if op:  # (the schedule before bound both shards' scenes)
                assert rs["kept_bound"] == 1 and st["reallocated"] == 0 and rs["bvh_rebuilt"] == 0, (step, rs, st)
                assert rs["relabelled"] == 1
            sc = scene_with(scene, model)
            o_res = art.FanOutputs(S, R, params.max_hits_per_ray, sc.T, params.thread_count)
            o_ref = o_res.copy()
            ctx.run(resident_frame(art.Frame(sc, params, org, o_res)))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=8)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, op, eq)  # both shards' fans see the new lists
    finally:
        ctx.set_flags(0)
        ctx.close()

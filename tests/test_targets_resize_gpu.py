"""Targets that appear and disappear on a bound scene (include/art_colliders.h, ABI 3.7;
DESIGN.md §3b-targets).

A scene bound after art_targets_reserve follows an art_targets_sync that changes the target count:
new targets' lists are built on their own, a survivor that a swap-back re-indexed keeps its lists
(its block of list starts moves) unless colliders name its old or its new index, and nothing is
allocated or rebound. Every step's check is the triple of test_targets_gpu.py: the launch on the
synced context, byte-equal to a fresh context bound with the model's targets, byte-equal to the
oracle. Shapes: S = 4 fans, R = 128 rays, 256 colliders, T = 7 (targets 0-3 own colliders, 4-6 none),
capacity 9.
"""
import numpy as np
import pytest

import art
from art import abi
from art.targets import TargetStore, resident_targets_frame
import oracle
from test_targets_cpu import TargetsModel
from test_targets_gpu import MOVES, R, S, Rig, _jitter, base_scene, moved

pytestmark = pytest.mark.gpu

CAP = 9


def pool(ci=2):
    """Positions for new targets: the further ones base_scene spreads over the colliders' box."""
    return base_scene(ci, T=16, seed=21)[0].targets[7:]


class ResizeRig(Rig):
    """Rig whose scene is bound with a reserved target capacity; edit() is a count-changing sync."""

    def __init__(self, *a, cap=CAP, **k):
        self.cap = cap
        super().__init__(*a, **k)

    def bind(self):
        self.store.reserve(self.cap)
        assert self.store.capacity() == self.cap
        super().bind()

    def lay_for(self, T):
        sc = art.Scene(dirs=self.scene.dirs, targets=np.zeros((T, 3), np.float32), spheres=self.scene.spheres,
                       aabbs=self.scene.aabbs, obbs=self.scene.obbs)
        return art.fan_layout(art.Frame(sc, self.params, self.org, self.outputs(T)), self.out_flags)

    def block_for(self, T):
        return self.torch.from_numpy(art.pack_block(self.outputs(T), self.lay_for(T))).to(self.dev)

    _check_T = None  # the target count of the scene being checked (an older frame's, in the stream test)

    def block(self):
        return self.block_for(self._check_T or len(self.model.pos))

    def check(self, blk, scene=None, what=""):
        scene = scene or self.model_scene()
        self.lay, self._check_T = self.lay_for(scene.T), scene.T
        try:
            return super().check(blk, scene, what)
        finally:
            self._check_T = None

    def edit(self, ops):
        """ops: ("add", pos) | ("remove", index) | ("clear",) | ("set", index, pos), applied to the store and the model,
        then one sync. Returns (art_target_sync_stats, art_target_resize_stats). The fan layout follows
        the synced count (the caller's duty, art_colliders.h)."""
        before = len(self.model.pos)
        for op in ops:
            if op[0] == "add":
                assert self.store.add(op[1]) == self.model.add(op[1])
            elif op[0] == "remove":
                self.store.remove_swapback(op[1])
                self.model.remove_swapback(op[1])
            elif op[0] == "clear":
                self.store.clear()
                self.model.clear()
            else:
                self.store.set(op[1], op[2])
                self.model.set(op[1], op[2])
        st = self.store.sync()
        rs = self.store.last_resize()
        self.model.synced()
        T = len(self.model.pos)
        assert self.store.synced_count() == T
        assert st["count_changed"] == (1 if T != before else 0)
        assert st["lists_rebuilt"] == rs["lists_rebuilt"] and st["lists_full_rebuild"] == rs["lists_full_rebuild"], (st, rs)
        if T:
            self.lay = self.lay_for(T)
        return st, rs


def test_adds():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        got = rig.check(rig.launch(), what="bound")
        assert (got.echo != 0).any() and (got.muffle != 0).any()
        plan = rig.ctx.debug_last_plan()
        used = rig.store.cells_arena()["used"]
        for step, p in enumerate(pool()[:2]):
            st, rs = rig.edit([("add", p)])
            assert rs["kept_bound"] == 1 and rs["added"] == 1 and rs["removed"] == 0, (step, rs)
            assert rs["lists_rebuilt"] == 1 and rs["lists_moved"] == 0 and rs["lists_full_rebuild"] == 0, (step, rs)
            assert rig.store.sync_map().tolist() == list(range(7 + step)) + [-1]
            rig.check(rig.launch(), what=f"add {step}")
            assert rig.ctx.debug_last_plan() == plan
            arena = rig.store.cells_arena()
            print("adds step", step, arena, "before", used)
            assert arena["used"] > used and arena["dropped_targets"] == 0, (step, arena, used)
            used = arena["used"]
        st = rig.move([7], moved(rig.model, [7], np.random.default_rng(1)))  # an added target moves like any other
        assert st["lists_rebuilt"] == 1
        rig.check(rig.launch(), what="added target moved")
    finally:
        rig.close()


def test_removes_on_the_move_path():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        rig.check(rig.launch(), what="bound")
        used = rig.store.cells_arena()["used"]
        st, rs = rig.edit([("remove", 5)])  # 6 -> 5: colliders name neither index
        assert rs == {"kept_bound": 1, "added": 0, "removed": 1, "lists_moved": 1, "lists_rebuilt": 0,
                      "lists_full_rebuild": 0, "bytes_uploaded": rs["bytes_uploaded"]}, rs
        assert rs["bytes_uploaded"] > 0 and rig.store.sync_map().tolist() == [0, 1, 2, 3, 4, 6]
        rig.check(rig.launch(), what="6 moved to 5")
        assert rig.store.cells_arena()["used"] == used
        st, rs = rig.edit([("remove", 5)])  # the last one: nothing moves
        assert rs["kept_bound"] == 1 and rs["removed"] == 1 and rs["lists_moved"] == 0 and rs["lists_rebuilt"] == 0, rs
        rig.check(rig.launch(), what="last removed")
        assert rig.store.cells_arena()["used"] == used
    finally:
        rig.close()


def test_removes_on_the_rebuild_path():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        rig.check(rig.launch(), what="bound")
        st, rs = rig.edit([("remove", 1)])  # 6 lands on an index that colliders name
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 0 and rs["lists_rebuilt"] == 1 and rs["lists_full_rebuild"] == 0, rs
        rig.check(rig.launch(), what="6 moved to 1")
        for T, i in ((5, 0), (4, 2), (3, 0)):  # down to T = 3: colliders name index 3, owned by nobody now
            st, rs = rig.edit([("remove", i)])
            assert rs["kept_bound"] == 1 and rs["removed"] == 1 and rs["lists_moved"] == 0 and rs["lists_rebuilt"] == 1, (T, rs)
            assert rig.store.synced_count() == T
            rig.check(rig.launch(), what=f"T = {T}")
    finally:
        rig.close()


def test_mixed_edits_in_one_sync():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        rig.check(rig.launch(), what="bound")
        a, b = pool()[:2]
        p4 = moved(rig.model, [4], np.random.default_rng(3))[0]
        st, rs = rig.edit([("remove", 2), ("add", a), ("add", b), ("remove", 0), ("set", 4, p4)])
        assert rig.store.sync_map().tolist() == [-1, 1, 6, 3, 4, 5, -1]
        # B at 0 and A at 6 are new, 6 landed on the owned index 2, 4 moved in space
        assert rs["kept_bound"] == 1 and rs["added"] == 2 and rs["removed"] == 2, rs
        assert rs["lists_rebuilt"] == 4 and rs["lists_moved"] == 0 and rs["lists_full_rebuild"] == 0, rs
        assert st["count_changed"] == 0
        rig.check(rig.launch(), what="mixed")
        st, rs = rig.edit([("remove", 4), ("add", pool()[2]), ("add", pool()[3])])  # 6 -> 4 moves, two new: T = 8
        assert rig.store.sync_map().tolist() == [0, 1, 2, 3, 6, 5, -1, -1]
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 1 and rs["lists_rebuilt"] == 2, rs
        rig.check(rig.launch(), what="mixed, with a move")
    finally:
        rig.close()


def test_capacity_exceeded():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        blk = rig.launch()
        rig.check(blk, what="bound")
        st, rs = rig.edit([("add", p) for p in pool()[:3]])  # T = 10 > 9
        assert rs["kept_bound"] == 0 and rs["added"] == 3 and rs["lists_rebuilt"] == 0, rs
        with pytest.raises(art.ArtError) as e:
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blk.data_ptr(), 0, rig.torch.cuda.current_stream().cuda_stream)
        assert e.value.code == abi.ART_E_STATE
        rig.bind()  # more targets than reserved: its own count is the scene's capacity
        rig.check(rig.launch(), what="rebound with T = 10")
        st, rs = rig.edit([("remove", 4)])  # 9 -> 4
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 1, rs
        rig.check(rig.launch(), what="T = 9 after the rebind")
        st, rs = rig.edit([("add", pool()[3])])
        assert rs["kept_bound"] == 1 and rs["lists_rebuilt"] == 1, rs
        rig.check(rig.launch(), what="T = 10 again")
        st, rs = rig.edit([("add", pool()[4])])  # T = 11: past the bound scene's room
        assert rs["kept_bound"] == 0
        st, rs = rig.edit([("clear",)])  # (nothing bound: an empty list is just published)
        assert rs["kept_bound"] == 0 and rs["removed"] == 11
    finally:
        rig.close()


def test_sync_to_zero_targets_unbinds():
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        blk = rig.launch()
        st, rs = rig.edit([("clear",)])
        assert rs["kept_bound"] == 0 and rs["removed"] == 7
        with pytest.raises(art.ArtError) as e:
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blk.data_ptr(), 0, rig.torch.cuda.current_stream().cuda_stream)
        assert e.value.code == abi.ART_E_STATE
    finally:
        rig.close()


@pytest.mark.parametrize("name", ["fold_h3", "hit_results", "obb_permeation", "batch_slots_3"])
def test_plans_and_layouts(name):
    out_flags, ci, must = 0, 2, 0
    scene, org, params = base_scene(3 if name == "obb_permeation" else 2, T=7)
    if name == "fold_h3":
        params.max_hits_per_ray = 3
        must = abi.ART_PLAN_FOLD
    elif name == "hit_results":
        out_flags = abi.ART_OUT_HIT_RESULTS
        must = abi.ART_PLAN_SPLIT | abi.ART_PLAN_HM
    elif name == "obb_permeation":
        ci = 3
        assert scene.obbs.size == 256 and params.stages & abi.ART_STAGE_PERMEATE
        must = abi.ART_PLAN_OBB
    else:
        params.thread_count = 3
    rig = ResizeRig(scene, org, params, out_flags=out_flags)
    try:
        got = rig.check(rig.launch(), what="bound")
        assert (got.muffle != 0).any()
        plan = rig.ctx.debug_last_plan()
        assert not must or plan & must, abi.plan_names(plan)
        st, rs = rig.edit([("add", pool(ci)[0])])
        assert rs["kept_bound"] == 1 and rs["lists_rebuilt"] == 1, rs
        rig.check(rig.launch(), what=f"{name}: add")
        assert rig.ctx.debug_last_plan() == plan
        st, rs = rig.edit([("remove", 4)])  # 7 -> 4
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 1 and rs["lists_rebuilt"] == 0, rs
        rig.check(rig.launch(), what=f"{name}: remove")
        assert rig.ctx.debug_last_plan() == plan
    finally:
        rig.close()


def test_with_the_collider_store():
    """The ownership histogram comes from the collider store; collider moves inside the lists' slack
    happen between the target edits; re-numbering an owner before a remove turns a rebuild into a move."""
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params, colliders=True)
    rng = np.random.default_rng(6)
    kinds = ((abi.ART_KIND_SPHERE, "spheres"), (abi.ART_KIND_AABB, "aabbs"))
    cur = {name: getattr(scene, name).copy() for _, name in kinds}
    base = {name: getattr(scene, name).copy() for _, name in kinds}

    def scene_now():
        return art.Scene(dirs=scene.dirs, targets=rig.model.array(), spheres=cur["spheres"], aabbs=cur["aabbs"])

    def move_colliders(scale):
        for k, name in kinds:  # always from the base records: every move stays within `scale` of them
            ids = rng.choice(cur[name].size, 24, replace=False)
            recs = _jitter(base[name][ids], rng, scale)
            rig.cstore.set_many(k, ids.astype(np.int32), recs)
            cur[name][ids] = recs
        return rig.cstore.sync()

    try:
        rig.check(rig.launch(), scene_now(), what="bound")
        assert move_colliders(0.05)["cells_rebuilt"] == 0
        st, rs = rig.edit([("add", pool()[0])])
        assert rs["kept_bound"] == 1 and rs["lists_rebuilt"] == 1, rs
        rig.check(rig.launch(), scene_now(), what="add")
        assert move_colliders(0.05)["cells_rebuilt"] == 0
        st, rs = rig.edit([("remove", 5)])  # 7 -> 5: nobody's colliders
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 1 and rs["lists_rebuilt"] == 0, rs
        rig.check(rig.launch(), scene_now(), what="remove on the move path")
        assert move_colliders(0.05)["cells_rebuilt"] == 0
        st, rs = rig.edit([("remove", 2)])  # 6 -> 2: colliders name 2
        assert rs["lists_moved"] == 0 and rs["lists_rebuilt"] == 1, rs
        rig.check(rig.launch(), scene_now(), what="remove on the rebuild path")
        # the caller re-numbers target 1's colliders to nobody, then removes target 1: 5 -> 1 is a move now
        for k, name in kinds:
            ids = np.flatnonzero(cur[name]["audio_target_id"] == 1).astype(np.int32)
            if not ids.size:
                continue
            recs = cur[name][ids].copy()
            recs["audio_target_id"] = -1
            rig.cstore.set_many(k, ids, recs)
            cur[name][ids] = recs
            base[name][ids] = recs
        cs = rig.cstore.sync()
        assert cs["cells_rebuilt"] == 1  # (an owner changed: the lists of every target)
        rig.check(rig.launch(), scene_now(), what="owner re-numbered")
        st, rs = rig.edit([("remove", 1)])
        assert rs["kept_bound"] == 1 and rs["lists_moved"] == 1 and rs["lists_rebuilt"] == 0, rs
        rig.check(rig.launch(), scene_now(), what="remove after the re-numbering")
    finally:
        rig.close()


def test_scene_without_lists(monkeypatch):
    monkeypatch.setenv("ART_CELLS_MAX_PAIRS", "1")
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        assert rig.store.cells_arena() == {"used": 0, "cap": 0, "dropped_targets": 0}
        st, rs = rig.edit([("add", pool()[0]), ("add", pool()[1])])
        assert rs["kept_bound"] == 1 and rs["added"] == 2 and rs["lists_rebuilt"] == 0 and rs["lists_moved"] == 0, rs
        rig.check(rig.launch(), what="no lists, T = 9")
        st, rs = rig.edit([("remove", 1), ("remove", 4)])
        assert rs["kept_bound"] == 1 and rs["removed"] == 2 and rs["lists_rebuilt"] == 0 and rs["lists_moved"] == 0, rs
        rig.check(rig.launch(), what="no lists, T = 7")
    finally:
        rig.close()


def test_arena_overflow_drops_a_new_target_then_compacts(monkeypatch):
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    used = rig.store.cells_arena()["used"]
    rig.close()
    # room for one average target past the compact lists: of two targets added in one sync the second
    # does not fit unless both have less than half the average's entries
    monkeypatch.setenv("ART_CELLS_CAP", str(used + used // 7))
    rig = ResizeRig(scene, org, params)
    try:
        arena = rig.store.cells_arena()
        assert arena["cap"] == used + used // 7 and arena["used"] == used and arena["dropped_targets"] == 0
        st, rs = rig.edit([("add", pool()[0]), ("add", pool()[1])])
        assert rs["kept_bound"] == 1 and rs["lists_rebuilt"] == 2 and rs["lists_full_rebuild"] == 0, rs
        blk = rig.launch()
        arena = rig.store.cells_arena()
        print("arena after two adds", arena, "compact", used)
        assert arena["dropped_targets"] > 0 and arena["used"] <= arena["cap"], arena
        rig.check(blk, what="dropped")  # the fallback (every collider) is exact
        st, rs = rig.edit([("remove", 8), ("remove", 7)])  # the seven of the bind: their lists fit again
        assert rs["kept_bound"] == 1 and rs["lists_full_rebuild"] == 1 and rs["lists_rebuilt"] == 0, rs
        blk = rig.launch()
        arena = rig.store.cells_arena()
        assert arena["dropped_targets"] == 0 and arena["used"] == used, (arena, used)
        rig.check(blk, what="compacted")
    finally:
        rig.close()


@pytest.mark.parametrize("switch_stream", [False, True])
def test_stream_order(switch_stream):
    """20 x (edit, sync, launch) back to back with no host synchronisation, the count going up and
    down between 5 and 9; every frame has its own block, made before the run; three are kept."""
    import torch
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    rng = np.random.default_rng(7)
    # +1 +1, then four removes, four adds, ... : 7 8 9 8 7 6 5 6 7 8 9 8 ...
    counts, T, up = [], 7, True
    for _ in range(20):
        up = False if T == 9 else True if T == 5 else up
        T += 1 if up else -1
        counts.append(T)
    assert min(counts) == 5 and max(counts) == 9
    keep = {7: None, 13: None, 19: None}
    other = torch.cuda.Stream()  # (alive until the context has been closed)
    new = iter(base_scene(2, T=40, seed=22)[0].targets[7:])
    try:
        blocks = [rig.block_for(T) for T in counts]
        torch.cuda.synchronize()
        for step, T in enumerate(counts):
            before = len(rig.model.pos)
            if T > before:
                ops = [("add", next(new))]
            else:
                ops = [("remove", int(rng.integers(0, before)))]
            if step % 3 == 0:  # and a survivor moves in space in the same sync
                ops.append(("set", 0, moved(rig.model, [0], rng)[0]))
            st, rs = rig.edit(ops)
            assert rs["kept_bound"] == 1 and len(rig.model.pos) == T, (step, rs)
            stm = other.cuda_stream if switch_stream and step >= 10 else torch.cuda.current_stream().cuda_stream
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blocks[step].data_ptr(), 0, stm)
            if step in keep:
                keep[step] = (blocks[step], rig.model_scene())
        torch.cuda.synchronize()
        for step, (blk, snap) in keep.items():
            rig.check(blk, snap, what=f"frame {step}")
    finally:
        rig.close()


def test_tick_after_a_resize():
    """art_dsp_tick_params_device at the new T equals art_dsp_tick_params_host byte for byte."""
    import torch
    from test_tick_cpu import random_case
    from test_tick_gpu import dev, stream
    from art.dsp import SpatializerSettings
    scene, org, params = base_scene(2, T=7)
    rig = ResizeRig(scene, org, params)
    try:
        st = SpatializerSettings()
        art.dsp.bind_settings(rig.ctx, st, 48000)
        rng = np.random.default_rng(5)
        for what, ops in (("add", [("add", pool()[0])]), ("remove", [("remove", 2), ("remove", 5)])):
            _, rs = rig.edit(ops)
            assert rs["kept_bound"] == 1
            T = len(rig.model.pos)
            listeners, _, _ = random_case(rng, S, T)
            d_ls = dev(listeners)
            d_params = dev(np.zeros(S * T, abi.DSP_SOURCE_PARAMS))
            blk = rig.launch()
            art.dsp.tick_params_device(rig.ctx, blk, S, d_ls, d_params, None, 0, stream())
            torch.cuda.synchronize()
            got = d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS).copy()
            fs = art.unpack_block(blk.cpu().numpy(), rig.lay, S, R, params.max_hits_per_ray, T, params.thread_count).settings
            want = art.dsp.tick_params_host(st, listeners, fs, rig.model.array(), None, 48000)
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), what
            rig.check(blk, what=f"tick: frame after {what}")
    finally:
        rig.close()


def test_host_api_on_three_shards():
    scene, org, params = base_scene(2, T=7)
    ctx = art.Context(devices=[0, 0, 0])
    store, model = TargetStore(ctx), TargetsModel()
    try:
        store.reserve(CAP)
        for p in scene.targets:
            assert store.add(p) == model.add(p)
        store.sync()
        ctx.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        for step, op in enumerate([None, ("add", pool()[0]), ("remove", 1), ("remove", 5)]):
            if op and op[0] == "add":
                assert store.add(op[1]) == model.add(op[1])
            elif op:
                store.remove_swapback(op[1])
                model.remove_swapback(op[1])
            st = store.sync()
            assert st["count_changed"] == (1 if op else 0)
            T = len(model.pos)
            sc = art.Scene(dirs=scene.dirs, targets=model.array(), spheres=scene.spheres, aabbs=scene.aabbs)
            o_res = art.FanOutputs(S, R, params.max_hits_per_ray, T, params.thread_count)
            o_ref = o_res.copy()
            ctx.run(resident_targets_frame(art.Frame(sc, params, org, o_res)))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=8)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, op, eq)  # every shard's fans see the new list
    finally:
        ctx.set_flags(0)
        ctx.close()

"""Resident audio-target store (include/art_colliders.h, second half) on the GPU.

A bound device scene follows art_targets_sync: a sync that moves K of T targets uploads K positions
and rebuilds those targets' muffle cell lists on their own at the tail of the entry arena
(DESIGN.md §3b-targets). The check of a step is always the same three comparisons: the result
blocks of art_launch_device on the synced context, byte-equal to a fresh context bound with the
model's positions, byte-equal to the oracle.
"""
import numpy as np
import pytest

import art
from art import abi
from art.colliders import ColliderStore, resident_frame
from art.targets import TargetStore, resident_targets_frame
import oracle
from test_targets_cpu import TargetsModel

pytestmark = pytest.mark.gpu

S, R = 4, 128


def base_scene(ci=2, T=7, seed=1):
    """The reduced config (128 spheres + 128 AABBs, or 256 OBBs) with T targets: the config's own
    four, which own colliders, and further ones spread over the colliders' box."""
    scene, org, params = art.synth(art.CONFIGS[ci], S=S, R=R, C_scale=0.0625)
    assert scene.C == 256
    rng = np.random.default_rng(seed)
    cs = [a["center"].view(np.float16).astype(np.float32).reshape(-1, 3)
          for a in (scene.spheres, scene.aabbs, scene.obbs) if a.size]
    c = np.concatenate(cs)
    extra = rng.uniform(c.min(axis=0), c.max(axis=0), (max(0, T - scene.T), 3)).astype(np.float32)
    targets = np.concatenate([scene.targets, extra])[:T]
    return art.Scene(dirs=scene.dirs, targets=np.ascontiguousarray(targets), spheres=scene.spheres, aabbs=scene.aabbs,
                     obbs=scene.obbs), org, params


class Rig:
    """A context whose bound scene follows the target store, and the model that checks it."""

    def __init__(self, scene, org, params, out_flags=0, colliders=False):
        import torch
        self.torch = torch
        self.scene, self.org, self.params, self.out_flags = scene, org, params, out_flags
        self.hits = bool(out_flags & abi.ART_OUT_HIT_RESULTS)
        self.dsp = params.dsp is not None
        self.ctx = art.Context(1)
        self.store, self.model = TargetStore(self.ctx), TargetsModel()
        self.cstore = ColliderStore(self.ctx) if colliders else None
        self.flags = abi.ART_CTX_RESIDENT_TARGETS | (abi.ART_CTX_RESIDENT_COLLIDERS if colliders else 0)
        self.dev = torch.device("cuda", 0)
        self.d_org = torch.from_numpy(np.ascontiguousarray(org)).to(self.dev)
        for p in scene.targets:
            assert self.store.add(p) == self.model.add(p)
        st = self.store.sync()
        assert st["count_changed"] == 1 and st["lists_rebuilt"] == 0 and st["lists_full_rebuild"] == 0
        self.model.synced()
        if colliders:
            for k, name in ((abi.ART_KIND_SPHERE, "spheres"), (abi.ART_KIND_AABB, "aabbs"), (abi.ART_KIND_OBB, "obbs")):
                for rec in getattr(scene, name):
                    self.cstore.add(k, rec)
            self.cstore.sync()
        self.ctx.set_flags(self.flags)
        self.bind()

    def outputs(self, T=None):
        return art.FanOutputs(S, R, self.params.max_hits_per_ray, T or len(self.model.pos), self.params.thread_count,
                              hits=self.hits, dsp=self.dsp)

    def model_scene(self):
        return art.Scene(dirs=self.scene.dirs, targets=self.model.array(), spheres=self.scene.spheres,
                         aabbs=self.scene.aabbs, obbs=self.scene.obbs)

    def frame(self, scene=None):
        return art.Frame(scene or self.model_scene(), self.params, self.org, self.outputs())

    def bind(self):
        fr = self.frame()
        self.lay = art.fan_layout(fr, self.out_flags)
        fr = resident_targets_frame(fr)
        self.ctx.bind(resident_frame(fr) if self.cstore else fr)

    def block(self):
        return self.torch.from_numpy(art.pack_block(self.outputs(), self.lay)).to(self.dev)

    def launch(self, stream=None):
        blk = self.block()
        st = stream if stream is not None else self.torch.cuda.current_stream().cuda_stream
        self.ctx.launch_device(self.d_org.data_ptr(), S, blk.data_ptr(), self.out_flags, st)
        return blk

    def move(self, ids, positions):
        self.store.set_many(ids, positions)
        assert self.model.set_many(list(ids), positions)
        st = self.store.sync()
        assert st["dirty_targets"] == self.model.expected_dirty() and st["count_changed"] == 0, st
        self.model.synced()
        return st

    def check(self, blk, scene=None, what=""):
        """blk against a fresh context bound with the model's positions, and against the oracle."""
        torch = self.torch
        scene = scene or self.model_scene()
        torch.cuda.synchronize()
        with art.Context(1) as ref:
            ref.bind(art.Frame(scene, self.params, self.org, self.outputs(scene.T)))
            rblk = self.block()
            ref.launch_device(self.d_org.data_ptr(), S, rblk.data_ptr(), self.out_flags,
                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        assert torch.equal(blk, rblk), f"{what}: differs from a fresh bind"
        o_ref = self.outputs(scene.T)
        oracle.run_frame(art.Frame(scene, self.params, self.org, o_ref), threads=8)
        got = art.unpack_block(blk.cpu().numpy(), self.lay, S, R, self.params.max_hits_per_ray, scene.T,
                               self.params.thread_count, hits=self.hits, dsp=self.dsp)
        eq = got.equal(o_ref)
        assert all(eq.values()), f"{what}: oracle {eq}"
        return got

    def close(self):
        self.ctx.set_flags(0)
        self.ctx.close()


# the moved pairs of the move sequence, T = 7: the block-boundary targets 0 and T - 1, an adjacent
# pair in one sync, the same target in consecutive syncs
MOVES = [(0, 6), (2, 3), (3, 5), (3, 4), (6, 1), (0, 1), (5, 6), (4, 0)]


def moved(model, ids, rng):
    """The targets ids moved by 0.5 to 5 units in a random direction."""
    d = rng.standard_normal((len(ids), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (model.array()[list(ids)] + d * rng.uniform(0.5, 5.0, (len(ids), 1))).astype(np.float32)


def test_move_sequence():
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    rng = np.random.default_rng(2)
    try:
        got = rig.check(rig.launch(), what="bound")
        assert (got.echo != 0).any() and (got.muffle != 0).any()
        plan = rig.ctx.debug_last_plan()
        used = rig.store.cells_arena()["used"]
        assert used > 0
        for step, ids in enumerate(MOVES):
            st = rig.move(ids, moved(rig.model, ids, rng))
            assert st["lists_rebuilt"] == 2 and st["lists_full_rebuild"] == 0 and st["bytes_uploaded"] == 32, (step, st)
            rig.check(rig.launch(), what=f"step {step}")
            assert rig.ctx.debug_last_plan() == plan
            arena = rig.store.cells_arena()
            print("move sequence step", step, arena, "before", used)
            assert arena["used"] > used and arena["dropped_targets"] == 0, (step, arena, used)
            used = arena["used"]
        st = rig.store.sync()  # nothing moved: nothing rebuilt
        assert st["dirty_targets"] == 0 and st["lists_rebuilt"] == 0 and st["bytes_uploaded"] == 0
        assert rig.store.cells_arena()["used"] == used
    finally:
        rig.close()


@pytest.mark.parametrize("name", ["fold_h3", "hit_results", "obb_permeation"])
def test_plans(name):
    out_flags = 0
    if name == "fold_h3":
        scene, org, params = base_scene(2, T=7)
        params.max_hits_per_ray = 3
        must = abi.ART_PLAN_FOLD
    elif name == "hit_results":
        scene, org, params = base_scene(2, T=7)
        out_flags = abi.ART_OUT_HIT_RESULTS
        must = abi.ART_PLAN_SPLIT | abi.ART_PLAN_HM
    else:
        scene, org, params = base_scene(3, T=7)
        assert scene.obbs.size == 256 and params.stages & abi.ART_STAGE_PERMEATE
        must = abi.ART_PLAN_OBB
    rig = Rig(scene, org, params, out_flags=out_flags)
    rng = np.random.default_rng(3)
    try:
        got = rig.check(rig.launch(), what="bound")
        assert (got.muffle != 0).any()
        plan = rig.ctx.debug_last_plan()
        assert plan & must, abi.plan_names(plan)
        if name == "fold_h3":
            assert not plan & (abi.ART_PLAN_FUSED | abi.ART_PLAN_PER_BOUNCE), abi.plan_names(plan)
        perms = []
        for step, ids in enumerate(MOVES[:3]):
            st = rig.move(ids, moved(rig.model, ids, rng))
            assert st["lists_rebuilt"] == 2 and st["lists_full_rebuild"] == 0, (step, st)
            got = rig.check(rig.launch(), what=f"{name} step {step}")
            assert rig.ctx.debug_last_plan() == plan
            perms.append(got.perm.copy())
        if name == "obb_permeation":  # the loss rays read the moved positions too
            assert any(not np.array_equal(perms[0], p) for p in perms[1:])
    finally:
        rig.close()


def test_geometry_edges_in_one_sync():
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    try:
        rig.check(rig.launch(), what="bound")
        centre = scene.spheres["center"].view(np.float16).astype(np.float32).reshape(-1, 3)
        free = int(np.flatnonzero(scene.spheres["audio_target_id"] == -1)[0])
        pos = np.stack([centre[free],                                # inside a collider nobody owns: `all` entries
                        rig.model.array()[2] + np.float32(5000.0),   # far outside the scene box: cell_far changes
                        rig.model.array()[1]]).astype(np.float32)    # exactly onto target 1
        st = rig.move([4, 2, 5], pos)
        assert st["lists_rebuilt"] == 3 and st["lists_full_rebuild"] == 0
        rig.check(rig.launch(), what="edges")
        st = rig.move([2], rig.scene.targets[2:3])  # and back into the scene
        assert st["lists_rebuilt"] == 1
        rig.check(rig.launch(), what="back")
    finally:
        rig.close()


def test_arena_overflow_drops_then_compacts(monkeypatch):
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    used = rig.store.cells_arena()["used"]
    rig.close()
    # room for one and a half average targets past the compact lists: of three targets relocated
    # in one sync the second or the third no longer fits
    monkeypatch.setenv("ART_CELLS_CAP", str(used + used * 3 // 14))
    rig = Rig(scene, org, params)
    rng = np.random.default_rng(4)
    try:
        arena = rig.store.cells_arena()
        assert arena["cap"] == used + used * 3 // 14 and arena["used"] == used and arena["dropped_targets"] == 0
        ids = [1, 3, 5]
        jit = lambda: (rig.model.array()[ids] + rng.uniform(-0.3, 0.3, (3, 3))).astype(np.float32)
        st = rig.move(ids, jit())
        assert st["lists_rebuilt"] == 3 and st["lists_full_rebuild"] == 0
        blk = rig.launch()
        arena = rig.store.cells_arena()
        print("arena after three relocations", arena, "compact", used)
        assert arena["dropped_targets"] > 0 and arena["used"] <= arena["cap"], arena
        rig.check(blk, what="dropped")  # the fallback (every collider) is exact
        st = rig.move(ids[:1], jit()[:1])
        assert st["lists_full_rebuild"] == 1 and st["lists_rebuilt"] == 0, st
        blk = rig.launch()
        arena = rig.store.cells_arena()
        assert arena["dropped_targets"] == 0 and arena["used"] <= used * 23 // 20, (arena, used)
        rig.check(blk, what="compacted")
    finally:
        rig.close()


def test_scene_without_lists(monkeypatch):
    monkeypatch.setenv("ART_CELLS_MAX_PAIRS", "1")
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    rng = np.random.default_rng(5)
    try:
        assert rig.store.cells_arena() == {"used": 0, "cap": 0, "dropped_targets": 0}
        for step, ids in enumerate(MOVES[:3]):
            st = rig.move(ids, moved(rig.model, ids, rng))
            assert st["lists_rebuilt"] == 0 and st["lists_full_rebuild"] == 0 and st["dirty_targets"] == 2
            rig.check(rig.launch(), what=f"no lists, step {step}")
    finally:
        rig.close()


def _jitter(recs, rng, scale):
    out = recs.copy()
    c = out["center"].view(np.float16).astype(np.float32)
    c += rng.uniform(-scale, scale, c.shape).astype(np.float32)
    out["center"] = c.astype(np.float16).view(np.uint16).reshape(out["center"].shape)
    return out


def test_with_the_collider_store():
    """Collider moves inside the lists' slack alternate with target moves: a target's lists are
    rebuilt from colliders that have drifted from the records the other targets' lists hold
    (DESIGN.md §5 item 11), and later collider moves are still checked against the older records."""
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params, colliders=True)
    rng = np.random.default_rng(6)
    kinds = ((abi.ART_KIND_SPHERE, "spheres"), (abi.ART_KIND_AABB, "aabbs"))
    cur = {name: getattr(scene, name).copy() for _, name in kinds}

    def scene_now():
        return art.Scene(dirs=scene.dirs, targets=rig.model.array(), spheres=cur["spheres"], aabbs=cur["aabbs"])

    def move_colliders(scale):
        for k, name in kinds:  # always from the original records: every move stays within `scale` of the base
            ids = rng.choice(cur[name].size, 24, replace=False)
            recs = _jitter(getattr(scene, name)[ids], rng, scale)
            rig.cstore.set_many(k, ids.astype(np.int32), recs)
            cur[name][ids] = recs
        return rig.cstore.sync()

    try:
        compact = rig.store.cells_arena()["used"]
        rig.check(rig.launch(), scene_now(), what="bound")
        for rnd, ids in enumerate(MOVES[:4]):
            cs = move_colliders(0.05)
            assert cs["cells_rebuilt"] == 0, (rnd, cs)
            rig.check(rig.launch(), scene_now(), what=f"colliders {rnd}")
            st = rig.move(ids, moved(rig.model, ids, rng))
            assert st["lists_rebuilt"] == 2 and st["lists_full_rebuild"] == 0, (rnd, st)
            rig.check(rig.launch(), scene_now(), what=f"targets {rnd}")
        grown = rig.store.cells_arena()["used"]
        assert grown > compact
        cs = move_colliders(3.0)  # out of the slack: every list is rebuilt, the arena compacted
        assert cs["cells_rebuilt"] == 1
        blk = rig.launch()
        arena = rig.store.cells_arena()
        assert arena["used"] < grown and arena["used"] <= compact * 5 // 4 and arena["dropped_targets"] == 0, (arena, compact)
        rig.check(blk, scene_now(), what="rebuilt")
        st = rig.move(MOVES[4], moved(rig.model, MOVES[4], rng))
        assert st["lists_rebuilt"] == 2 and st["lists_full_rebuild"] == 0
        rig.check(rig.launch(), scene_now(), what="after the rebuild")
    finally:
        rig.close()


@pytest.mark.parametrize("switch_stream", [False, True])
def test_stream_order_and_ring_wrap(switch_stream):
    """20 x (set_many, sync, launch) back to back with no host synchronisation (the syncs wrap the
    ring of pinned update images); three frames are kept and compared after one final sync."""
    import torch
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    rng = np.random.default_rng(7)
    keep = {7: None, 13: None, 19: None}
    other = torch.cuda.Stream()  # (alive until the context has been closed)
    try:
        blocks = [rig.block() for _ in range(20)]  # every frame's own device buffer, made before the run
        torch.cuda.synchronize()
        for step in range(20):
            ids = MOVES[step % len(MOVES)]
            rig.move(ids, moved(rig.model, ids, rng))
            st = other.cuda_stream if switch_stream and step >= 10 else torch.cuda.current_stream().cuda_stream
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blocks[step].data_ptr(), 0, st)
            if step in keep:
                keep[step] = (blocks[step], rig.model_scene())
        torch.cuda.synchronize()
        for step, (blk, snap) in keep.items():
            rig.check(blk, snap, what=f"frame {step}")
    finally:
        rig.close()


def test_host_api_on_three_shards():
    scene, org, params = base_scene(2, T=7)
    ctx = art.Context(devices=[0, 0, 0])
    store, model = TargetStore(ctx), TargetsModel()
    rng = np.random.default_rng(8)
    try:
        for p in scene.targets:
            assert store.add(p) == model.add(p)
        store.sync()
        model.synced()
        ctx.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        for step in range(3):
            sc = art.Scene(dirs=scene.dirs, targets=model.array(), spheres=scene.spheres, aabbs=scene.aabbs)
            o_res = art.FanOutputs(S, R, params.max_hits_per_ray, 7, params.thread_count)
            o_ref = o_res.copy()
            ctx.run(resident_targets_frame(art.Frame(sc, params, org, o_res)))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=8)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, eq)  # every shard's fans see the move
            ids = MOVES[step]
            pos = moved(model, ids, rng)
            store.set_many(ids, pos)
            model.set_many(list(ids), pos)
            st = store.sync()
            assert st["dirty_targets"] == 2
            model.synced()
    finally:
        ctx.set_flags(0)
        ctx.close()


def test_count_change_unbinds():
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    try:
        blk = rig.launch()
        rig.check(blk, what="bound")
        rig.store.remove_swapback(5)  # (targets 4 .. 6 own no colliders: nothing to re-number)
        rig.model.remove_swapback(5)
        st = rig.store.sync()
        rig.model.synced()
        assert st["count_changed"] == 1 and st["lists_rebuilt"] == 0 and rig.store.synced_count() == 6
        with pytest.raises(art.ArtError) as e:  # the scene is unbound: T is part of the frame layout
            rig.ctx.launch_device(rig.d_org.data_ptr(), S, blk.data_ptr(), 0, rig.torch.cuda.current_stream().cuda_stream)
        assert e.value.code == abi.ART_E_STATE
        rig.bind()
        rig.check(rig.launch(), what="rebound with T = 6")
        st = rig.move([5], moved(rig.model, [5], np.random.default_rng(9)))
        assert st["lists_rebuilt"] == 1
        rig.check(rig.launch(), what="moved after the rebind")
    finally:
        rig.close()

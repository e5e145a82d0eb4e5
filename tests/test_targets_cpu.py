"""Resident audio-target store (include/art_colliders.h, second half) on the CPU backend.

A pure-Python model of the reference's target list (AudioTargetManager over
NativeJobBatch<float3>, Audio/AudioTargetManager.cs:49-110: add returns the index, set, swap-back
remove with invalid ids skipped, clear) checks the store's mirror. Frames that read the resident
targets (ART_CTX_RESIDENT_TARGETS) must equal, byte for byte, frames that pass the model's
positions in the desc, and those equal the oracle. These tests need no GPU.
"""
import numpy as np
import pytest

import art
from art import abi
from art.targets import TargetStore, resident_targets_frame
import oracle


class TargetsModel:
    """The list semantics of AudioTargetPositions, plus the indices touched since the last sync."""

    def __init__(self):
        self.pos = []
        self.touched = set()

    def add(self, p):
        self.pos.append(np.array(p, np.float32))
        self.touched.add(len(self.pos) - 1)
        return len(self.pos) - 1

    def set(self, i, p):
        p = np.array(p, np.float32)
        if self.pos[i].tobytes() != p.tobytes():  # the same 12 bytes: nothing moved
            self.pos[i] = p
            self.touched.add(i)

    def set_many(self, ids, ps):
        if any(i < 0 or i >= len(self.pos) for i in ids):
            return False  # one bad id: nothing changes
        for i, p in zip(ids, ps):
            self.set(i, p)
        return True

    def remove_swapback(self, i):
        if i < 0 or i >= len(self.pos):
            return
        if i != len(self.pos) - 1:
            self.pos[i] = self.pos[-1]
            self.touched.add(i)
        self.pos.pop()

    def clear(self):
        self.pos = []

    def array(self):
        return np.array(self.pos, np.float32).reshape(-1, 3)

    def expected_dirty(self):
        return len([i for i in self.touched if i < len(self.pos)])

    def synced(self):
        self.touched = set()


@pytest.fixture
def cpu():
    c = art.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_store_semantics_random_sequences(cpu, seed):
    rng = np.random.default_rng(seed)
    store, model = TargetStore(cpu), TargetsModel()
    last_n = None
    for op in range(400):
        r = rng.random()
        n = len(model.pos)
        p = rng.uniform(-50, 50, 3).astype(np.float32)
        if r < 0.25 or n == 0:
            assert store.add(p) == model.add(p)
        elif r < 0.50:
            i = int(rng.integers(0, n))
            if rng.random() < 0.2:
                p = model.pos[i].copy()  # a set to the same bytes
            store.set(i, p)
            model.set(i, p)
        elif r < 0.65:
            k = int(rng.integers(1, 5))
            ids = rng.integers(0, n, k).tolist()
            if rng.random() < 0.3:
                ids[int(rng.integers(0, k))] = int(rng.choice([-1, n, n + 3]))  # one bad id
            ps = rng.uniform(-50, 50, (k, 3)).astype(np.float32)
            if model.set_many(ids, ps):
                store.set_many(ids, ps)
            else:
                with pytest.raises(art.ArtError) as e:
                    store.set_many(ids, ps)
                assert e.value.code == abi.ART_E_INVALID
        elif r < 0.80:
            i = int(rng.integers(-2, n + 3))  # some invalid
            store.remove_swapback(i)
            model.remove_swapback(i)
        elif r < 0.82:
            store.clear()
            model.clear()
        else:
            st = store.sync()
            assert store.count() == len(model.pos) == store.synced_count()
            assert store.array().tobytes() == model.array().tobytes()
            assert st["dirty_targets"] == model.expected_dirty(), (op, st)
            assert st["count_changed"] == (1 if last_n is None or last_n != len(model.pos) else 0)
            assert st["lists_rebuilt"] == 0 and st["lists_full_rebuild"] == 0 and st["bytes_uploaded"] == 0
            last_n = len(model.pos)
            model.synced()
        assert store.count() == len(model.pos)
    st = store.sync()
    assert store.array().tobytes() == model.array().tobytes()
    assert st["dirty_targets"] == model.expected_dirty()
    st = store.sync()  # nothing changed: an empty sync
    assert st == {"dirty_targets": 0, "count_changed": 0, "lists_rebuilt": 0, "lists_full_rebuild": 0, "bytes_uploaded": 0}


def _scene_T4():
    return art.synth(art.CONFIGS[1], S=2, R=64, C_scale=0.25)  # config 1: 64 AABBs, T = 4


def test_cpu_frames_read_the_synced_targets(cpu):
    scene, org, params = _scene_T4()
    assert scene.aabbs.size == 64 and scene.T == 4
    store, model = TargetStore(cpu), TargetsModel()
    for p in scene.targets:
        assert store.add(p) == model.add(p)
    store.sync()
    model.synced()
    rng = np.random.default_rng(9)
    for step in range(2):
        sc = art.Scene(dirs=scene.dirs, targets=model.array(), aabbs=scene.aabbs)
        o_desc = art.FanOutputs(2, 64, params.max_hits_per_ray, 4, params.thread_count)
        o_res, o_ref = o_desc.copy(), o_desc.copy()
        cpu.set_flags(0)
        cpu.run(art.Frame(sc, params, org, o_desc))
        cpu.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        cpu.run(resident_targets_frame(art.Frame(sc, params, org, o_res)))
        cpu.set_flags(0)
        oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=4)
        assert all(o_res.equal(o_desc).values()), (step, o_res.equal(o_desc))
        assert all(o_desc.equal(o_ref).values()), (step, o_desc.equal(o_ref))
        # move two targets; an unsynced move must not reach the frame above's successor until the sync
        ids = [0, 3]
        ps = model.array()[ids] + rng.uniform(-4, 4, (2, 3)).astype(np.float32)
        store.set_many(ids, ps)
        model.set_many(ids, ps)
        st = store.sync()
        assert st["dirty_targets"] == 2 and st["count_changed"] == 0
        model.synced()


def test_unsynced_moves_do_not_reach_frames(cpu):
    scene, org, params = _scene_T4()
    store = TargetStore(cpu)
    store.add_many(scene.targets)
    store.sync()
    store.set(1, scene.targets[1] + np.float32(7.0))  # NextBatch only
    o_res = art.FanOutputs(2, 64, params.max_hits_per_ray, 4, params.thread_count)
    o_ref = o_res.copy()
    cpu.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
    cpu.run(resident_targets_frame(art.Frame(scene, params, org, o_res)))
    cpu.set_flags(0)
    oracle.run_frame(art.Frame(scene, params, org, o_ref), threads=4)
    assert all(o_res.equal(o_ref).values())


def test_error_paths(cpu):
    scene, org, params = _scene_T4()
    store = TargetStore(cpu)
    out = art.FanOutputs(2, 64, params.max_hits_per_ray, 4, params.thread_count)
    fr = art.Frame(scene, params, org, out)
    cpu.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
    with pytest.raises(art.ArtError) as e:  # no sync yet
        cpu.run(resident_targets_frame(fr))
    assert e.value.code == abi.ART_E_STATE
    store.add_many(scene.targets)
    store.sync()
    with pytest.raises(art.ArtError) as e:  # the desc still carries positions
        cpu.run(fr)
    assert e.value.code == abi.ART_E_INVALID
    h = cpu.schedule(resident_targets_frame(fr))
    with pytest.raises(art.ArtError) as e:  # sync while a frame is in flight
        store.sync()
    assert e.value.code == abi.ART_E_STATE
    h.complete()
    cpu.set_flags(0)
    with pytest.raises(art.ArtError) as e:
        store.set(4, scene.targets[0])
    assert e.value.code == abi.ART_E_INVALID
    with pytest.raises(art.ArtError) as e:
        store.get(-1)
    assert e.value.code == abi.ART_E_INVALID
    store.remove_swapback(9)  # skipped
    assert store.count() == 4
    store.clear()
    st = store.sync()
    assert store.count() == 0 and st["count_changed"] == 1
    cpu.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
    with pytest.raises(art.ArtError) as e:  # a frame without targets (AudioRayTracer.cs:95)
        cpu.run(resident_targets_frame(fr))
    assert e.value.code == abi.ART_E_INVALID
    cpu.set_flags(0)


def test_abi_version_and_struct():
    import ctypes as C
    lib = art.load_library()
    v = lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 4
    assert C.sizeof(abi.art_target_sync_stats) == 4 * 4 + 8
    assert C.sizeof(abi.art_collider_sync_stats) == 4 * 4 + 8  # untouched

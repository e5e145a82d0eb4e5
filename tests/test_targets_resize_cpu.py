"""Targets that appear and disappear (include/art_colliders.h, ABI 3.7), the host half: the reserve
call's error codes, the statistics, and the planner's identity map of a sync against a Python model of
the reference's list (AudioTargetManager.cs:49-96: add appends, remove moves the last into the hole).
These tests need no GPU.
"""
import ctypes as C

import numpy as np
import pytest

import art
from art import abi
from art.targets import TargetStore, resident_targets_frame
import oracle
from test_targets_cpu import TargetsModel


class IdentityModel(TargetsModel):
    """TargetsModel plus who is who: every target gets a serial number when it is added."""

    def __init__(self):
        super().__init__()
        self.ids, self.at_sync, self.serial = [], {}, 0

    def add(self, p):
        self.ids.append(self.serial)
        self.serial += 1
        return super().add(p)

    def remove_swapback(self, i):
        if 0 <= i < len(self.pos):
            self.ids[i] = self.ids[-1]
            self.ids.pop()
        super().remove_swapback(i)

    def clear(self):
        self.ids = []
        super().clear()

    def sync_map(self):
        """For each index the index the same target had at the previous sync, or -1; then this sync
        becomes the previous one."""
        m = [self.at_sync.get(s, -1) for s in self.ids]
        self.at_sync = {s: i for i, s in enumerate(self.ids)}
        return m


def check_move_invariant(m):
    """The survivors' old indices are distinct, and no re-indexed survivor's old index is where
    another re-indexed survivor lands: their per-target blocks can move in parallel, in place."""
    src = [s for s in m if s >= 0]
    assert len(set(src)) == len(src), m
    moved = [(s, i) for i, s in enumerate(m) if s >= 0 and s != i]
    dst = {i for _, i in moved}
    assert not ({s for s, _ in moved} & dst), m


@pytest.fixture
def cpu():
    c = art.Context(0)
    yield c
    c.close()


def test_reserve_error_codes_and_capacity(cpu):
    store = TargetStore(cpu)
    assert store.capacity() == 0
    store.reserve(9)
    assert store.capacity() == 9
    for cap, code in ((-1, abi.ART_E_INVALID), (257, abi.ART_E_UNSUPPORTED)):
        with pytest.raises(art.ArtError) as e:
            store.reserve(cap)
        assert e.value.code == code
        assert store.capacity() == 9
    store.reserve(256)
    assert store.capacity() == 256
    store.reserve(0)
    assert store.capacity() == 0
    assert cpu.lib.art_targets_reserve(None, 4) == abi.ART_E_INVALID
    assert cpu.lib.art_target_capacity(None) == abi.ART_E_INVALID
    # while a frame is in flight
    scene, org, params = art.synth(art.CONFIGS[1], S=2, R=64, C_scale=0.25)
    fr = art.Frame(scene, params, org, art.FanOutputs(2, 64, params.max_hits_per_ray, 4, params.thread_count))
    h = cpu.schedule(fr)  # (fr owns the arrays the frame writes: alive until complete)
    with pytest.raises(art.ArtError) as e:
        store.reserve(5)
    assert e.value.code == abi.ART_E_STATE
    h.complete()
    store.reserve(5)
    assert store.capacity() == 5


def test_last_resize_before_any_sync_and_struct(cpu):
    store = TargetStore(cpu)
    st = store.last_resize()
    assert st == {"kept_bound": 0, "added": 0, "removed": 0, "lists_moved": 0, "lists_rebuilt": 0,
                  "lists_full_rebuild": 0, "bytes_uploaded": 0}
    assert C.sizeof(abi.art_target_resize_stats) == 6 * 4 + 8
    assert C.sizeof(abi.art_target_sync_stats) == 4 * 4 + 8  # kept
    v = cpu.lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 7
    assert store.sync_map().size == 0
    assert cpu.lib.art_debug_target_sync_map(cpu.ptr, None, 1) == abi.ART_E_INVALID
    assert cpu.lib.art_targets_last_resize(cpu.ptr, None) == abi.ART_E_INVALID


def test_header_struct_size(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "art_colliders.h"\n'
                   'int main(void) { printf("%zu\\n", sizeof(art_target_resize_stats)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "size")])
    assert int(subprocess.check_output([str(tmp_path / "size")], text=True)) == C.sizeof(abi.art_target_resize_stats)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planner_fuzz(cpu, seed):
    """100 syncs per seed, each after a random run of add / set / remove-swapback / clear."""
    rng = np.random.default_rng(seed)
    store, model = TargetStore(cpu), IdentityModel()
    store.reserve(64)
    serial = 0
    reindexed = 0
    for sync in range(100):
        for _ in range(int(rng.integers(0, 9))):
            r, n = rng.random(), len(model.pos)
            serial += 1
            p = np.array([serial, rng.uniform(-50, 50), rng.uniform(-50, 50)], np.float32)  # unique: identity is the 12 bytes
            if r < 0.35 or n == 0:
                assert store.add(p) == model.add(p)
            elif r < 0.55:
                i = int(rng.integers(0, n))
                store.set(i, p)
                model.set(i, p)
            elif r < 0.99:
                i = int(rng.integers(-1, n + 1))  # some invalid
                store.remove_swapback(i)
                model.remove_swapback(i)
            else:
                store.clear()
                model.clear()
        before = store.synced_count()
        st = store.sync()
        rs = store.last_resize()
        want = model.sync_map()
        got = store.sync_map().tolist()
        assert got == want, (sync, got, want)
        check_move_invariant(got)
        assert store.array().tobytes() == model.array().tobytes()
        survivors = sum(1 for s in got if s >= 0)
        assert rs["added"] == len(got) - survivors and rs["removed"] == before - survivors, (sync, rs)
        assert rs["kept_bound"] == 0 and rs["lists_moved"] == 0 and rs["lists_rebuilt"] == st["lists_rebuilt"] == 0
        assert st["dirty_targets"] == model.expected_dirty()
        model.synced()
        reindexed += sum(1 for i, s in enumerate(got) if s >= 0 and s != i)
    assert reindexed >= 10  # the sequences do exercise re-indexed survivors (a check of this generator)


def test_vacated_and_refilled_slot_is_new(cpu):
    store = TargetStore(cpu)
    pos = np.arange(15, dtype=np.float32).reshape(5, 3)
    store.add_many(pos)
    store.sync()
    assert store.sync_map().tolist() == [-1] * 5
    store.sync()
    assert store.sync_map().tolist() == [0, 1, 2, 3, 4]
    store.remove_swapback(4)           # [0 1 2 3]
    store.add(np.float32([9, 9, 9]))   # index 4 again: a new target, same index
    store.remove_swapback(1)           # the new one lands on 1
    store.sync()
    assert store.sync_map().tolist() == [0, -1, 2, 3]
    rs = store.last_resize()
    assert rs["added"] == 1 and rs["removed"] == 2


def test_cpu_frames_after_resizes(cpu):
    scene, org, params = art.synth(art.CONFIGS[1], S=2, R=64, C_scale=0.25)  # 64 AABBs, T = 4
    store, model = TargetStore(cpu), TargetsModel()
    store.reserve(6)
    for p in scene.targets:
        assert store.add(p) == model.add(p)
    store.sync()
    rng = np.random.default_rng(11)
    lo, hi = scene.targets.min(axis=0) - 3, scene.targets.max(axis=0) + 3
    cpu.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
    try:
        for step, op in enumerate(["add", "add", "remove 1", "remove 0", "remove 2", "add"]):
            if op == "add":
                p = rng.uniform(lo, hi).astype(np.float32)
                assert store.add(p) == model.add(p)
            else:
                i = int(op.split()[1])
                store.remove_swapback(i)
                model.remove_swapback(i)
            st = store.sync()
            assert st["count_changed"] == 1
            T = len(model.pos)
            sc = art.Scene(dirs=scene.dirs, targets=model.array(), aabbs=scene.aabbs)
            o_res = art.FanOutputs(2, 64, params.max_hits_per_ray, T, params.thread_count)
            o_ref = o_res.copy()
            cpu.run(resident_targets_frame(art.Frame(sc, params, org, o_res)))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=4)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, op, eq)
    finally:
        cpu.set_flags(0)

"""Resident audio-target store (include/art_colliders.h, second half).

Mirrors the reference's target list: AudioTargetManager (Audio/AudioTargetManager.cs:49-110) over
NativeJobBatch<float3> AudioTargetPositions. `add` / `set` / `remove_swapback` edit the NextBatch
mirror; `sync` is UpdateJobBatch and publishes the mirror. On a bound device scene a sync that only
moves targets uploads the moved positions and rebuilds those targets' muffle cell lists alone.
Frames then take the positions and the target count from the store (`resident_targets_frame`,
ART_CTX_RESIDENT_TARGETS). `follow_map` / `follow_mark` give the syncs' maps composed since the last
mark, for arrays kept per target or per source (art.dsp.sources_follow_device); with
ART_CTX_TARGET_OWNERS_FOLLOW a `remove_swapback` also re-numbers the swapped target's colliders.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from . import abi
from .frame import Context, Frame


class TargetStore:
    """The resident target positions of one Context."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def _check(self, rc: int):
        if rc < 0:
            self.ctx._raise(rc)
        return rc

    def add(self, pos) -> int:
        """AddAudioTargetToSystem (:49-57); returns the new target's index."""
        p = np.ascontiguousarray(pos, np.float32).reshape(3)
        out = C.c_int32()
        self._check(self.ctx.lib.art_target_add(self.ctx.ptr, p.ctypes.data, C.byref(out)))
        return out.value

    def add_many(self, positions) -> list[int]:
        return [self.add(p) for p in np.asarray(positions, np.float32).reshape(-1, 3)]

    def set(self, idx: int, pos):
        """UpdateToAudioSystem (AudioTarget/AudioTargetRT.cs:45-48)."""
        p = np.ascontiguousarray(pos, np.float32).reshape(3)
        self._check(self.ctx.lib.art_target_set(self.ctx.ptr, idx, p.ctypes.data))

    def set_many(self, ids, positions):
        """Batched set: positions[j] -> ids[j] (one call, all ids checked first)."""
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
        assert i.size == p.shape[0]
        self._check(self.ctx.lib.art_target_set_many(self.ctx.ptr, i.ctypes.data, p.ctypes.data, i.size))

    def remove_swapback(self, idx: int):
        """RemoveAudioTargetFromSystem (:59-96); out-of-range ids are skipped."""
        self._check(self.ctx.lib.art_target_remove_swapback(self.ctx.ptr, idx))

    def get(self, idx: int) -> np.ndarray:
        p = np.zeros(3, np.float32)
        self._check(self.ctx.lib.art_target_get(self.ctx.ptr, idx, p.ctypes.data))
        return p

    def count(self) -> int:
        return self._check(self.ctx.lib.art_target_count(self.ctx.ptr))

    def synced_count(self) -> int:
        """T of the last sync: what resident-target frames (and their fan layout) use."""
        return self._check(self.ctx.lib.art_target_synced_count(self.ctx.ptr))

    def array(self) -> np.ndarray:
        """The whole NextBatch mirror, float32 [count, 3]."""
        return np.array([self.get(i) for i in range(self.count())], np.float32).reshape(-1, 3)

    def clear(self):
        self._check(self.ctx.lib.art_targets_clear(self.ctx.ptr))

    def sync(self) -> dict:
        """UpdateJobBatch (:105-110); returns what the sync moved (art_target_sync_stats)."""
        self._check(self.ctx.lib.art_targets_sync(self.ctx.ptr))
        st = abi.art_target_sync_stats()
        self._check(self.ctx.lib.art_targets_last_sync(self.ctx.ptr, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in abi.art_target_sync_stats._fields_}

    def reserve(self, capacity: int):
        """Room for up to `capacity` targets in scenes bound from now on (art_targets_reserve): a sync
        whose count stays in [1, capacity] keeps such a scene bound. 0: a count change unbinds."""
        self._check(self.ctx.lib.art_targets_reserve(self.ctx.ptr, capacity))

    def capacity(self) -> int:
        return self._check(self.ctx.lib.art_target_capacity(self.ctx.ptr))

    def last_resize(self) -> dict:
        """What the last sync did to the list and to a bound scene's lists (art_target_resize_stats)."""
        st = abi.art_target_resize_stats()
        self._check(self.ctx.lib.art_targets_last_resize(self.ctx.ptr, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in abi.art_target_resize_stats._fields_}

    def sync_map(self) -> np.ndarray:
        """For each synced index, the synced index the same target held before the last sync (-1: new)."""
        n = self.synced_count()
        src = np.full(max(n, 1), -2, np.int32)
        assert self._check(self.ctx.lib.art_debug_target_sync_map(self.ctx.ptr, src.ctypes.data, n)) == n
        return src[:n]

    def follow_map(self) -> tuple[np.ndarray, int]:
        """art_target_follow_map: (src, base_count). src[i] is the index the target now at synced index
        i held in the base list (the synced list at the last follow_mark), -1 if it was not in it."""
        n = self.synced_count()
        src = np.full(max(n, 1), -2, np.int32)
        base = C.c_int32()
        assert self._check(self.ctx.lib.art_target_follow_map(self.ctx.ptr, src.ctypes.data, n, C.byref(base))) == n
        return src[:n], base.value

    def follow_mark(self):
        """art_target_follow_mark: the synced list becomes the base list of the follow map."""
        self._check(self.ctx.lib.art_target_follow_mark(self.ctx.ptr))

    def last_remove_owners(self) -> list[int]:
        """Collider records re-numbered by the most recent remove_swapback (ART_CTX_TARGET_OWNERS_FOLLOW),
        per kind: spheres, AABBs, OBBs."""
        out = np.zeros(3, np.int32)
        self._check(self.ctx.lib.art_target_last_remove_owners(self.ctx.ptr, out.ctypes.data))
        return out.tolist()

    def cells_arena(self) -> dict:
        """art_debug_cells_arena of the bound scene (diagnostics, synchronizes)."""
        used, cap, dropped = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self.ctx.lib.art_debug_cells_arena(self.ctx.ptr, C.byref(used), C.byref(cap), C.byref(dropped)))
        return {"used": int(used.value), "cap": int(cap.value), "dropped_targets": int(dropped.value)}


def resident_targets_frame(frame: Frame) -> Frame:
    """A shallow copy of `frame` whose desc carries no targets (for ART_CTX_RESIDENT_TARGETS). Its
    outputs keep the frame's T, which must be the store's synced count."""
    f = copy.copy(frame)
    d = abi.art_frame_desc()
    C.pointer(d)[0] = frame.desc
    d.audio_target_positions = None
    d.audio_target_count = 0
    f.desc = d
    return f

"""Colliders that appear and disappear (include/art_colliders.h, ABI 3.10), the host half: the relabel
rule's invariants on its host restatement (bvh_relabel_ref.py), the reserve call's error codes and
defaults, the statistics on the CPU backend, and CPU-backend frames after adds and removes against
the oracle. These tests need no GPU.
"""
import ctypes as C

import numpy as np
import pytest

import art
from art import abi
from art.colliders import ColliderStore, resident_frame
import bvh_relabel_ref as rr
import oracle

KINDS = ((abi.ART_KIND_SPHERE, "spheres"), (abi.ART_KIND_AABB, "aabbs"), (abi.ART_KIND_OBB, "obbs"))
ZERO_STATS = {"kept_bound": 0, "added": 0, "removed": 0, "relabelled": 0, "bvh_rebuilt": 0, "levels_changed": 0,
              "cells_rebuilt": 0, "bytes_uploaded": 0}


@pytest.fixture
def cpu():
    c = art.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------- the relabel rule
def check_rule(ref, old, new):
    """The invariants of one application of the rule; returns (ref', a, h)."""
    out, written = rr.relabel(ref, old, new)
    n, n2 = sum(old), sum(new)
    assert out.size == n2
    assert sorted(out.tolist()) == rr.labels_of(new)  # a left-packed permutation of all labels
    gone = {rr.label(k, i) for k in range(3) for i in range(new[k], old[k])}
    new_labels = {rr.label(k, i) for k in range(3) for i in range(old[k], new[k])}
    a, h = len(new_labels), len(gone)
    holes = [p for p in range(n) if int(ref[p]) in gone]
    # untouched positions keep their reference: everything below min(n, n') that was not a hole
    for p in range(min(n, n2)):
        if p not in holes:
            assert out[p] == ref[p], (p, old, new)
    # the first min(a, h) holes hold A in ascending order (those that lie below n')
    A = sorted(new_labels)
    for j in range(min(a, h)):
        if holes[j] < n2:
            assert out[holes[j]] == A[j]
    if a > h:
        assert n2 == n + a - h and out[n:].tolist() == A[h:]
    changed = int(sum(1 for p in range(min(n, n2)) if out[p] != ref[p])) + max(0, n2 - n)
    assert written == changed  # every write changes its position (a hole never keeps its vanished label)
    assert changed <= a + max(0, h - a)
    # bvh_pos is the inverse under the new counts
    g = rr.global_index(out, new)
    assert sorted(g.tolist()) == list(range(n2))
    return out, a, h


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_rule_on_random_orders_and_count_pairs(seed):
    rng = np.random.default_rng(seed)
    seen = set()
    for it in range(150):
        old = [int(x) for x in rng.integers(0, 3 if it % 4 == 0 else 24, 3)]
        if sum(old) == 0:
            old[int(rng.integers(0, 3))] = 1
        new = [max(0, o + int(rng.integers(-6, 7))) for o in old]
        if sum(new) == 0:
            new[int(rng.integers(0, 3))] = 1
        ref = rng.permutation(np.array(rr.labels_of(old), np.uint32))
        _, a, h = check_rule(ref, old, new)
        seen.add("a>h" if a > h else "a=h" if a == h else "h>a")
        if a and h:
            seen.add("both")
    assert seen == {"a>h", "a=h", "h>a", "both"}


def test_rule_branches_by_hand():
    S, A, O = (lambda i: rr.label(0, i)), (lambda i: rr.label(1, i)), (lambda i: rr.label(2, i))
    ref = np.array([A(0), S(1), O(0), S(0), A(1)], np.uint32)
    # a = h: sphere 1 vanishes, OBB 1 appears in its place
    out, w = rr.relabel(ref, (2, 2, 1), (1, 2, 2))
    assert out.tolist() == [A(0), O(1), O(0), S(0), A(1)] and w == 1
    # a > h: the hole takes the first appearing label (lowest kind rank), the rest is appended
    out, w = rr.relabel(ref, (2, 2, 1), (1, 3, 2))
    assert out.tolist() == [A(0), A(2), O(0), S(0), A(1), O(1)] and w == 2
    # h > a: holes at 1 (sphere 1) and 2 (OBB 0); n' = 3; the hole at 1 takes M[0] = position 3, and the
    # hole at 2 takes M[1] = position 4
    out, w = rr.relabel(ref, (2, 2, 1), (1, 2, 0))
    assert out.tolist() == [A(0), S(0), A(1)] and w == 2
    # h > a with a filled hole in the tail: holes at 1 and 4 (AABB 1), a = 1 (OBB 1); n' = 4: hole 1 takes
    # OBB 1, hole 4 is past n' and nothing moves
    out, w = rr.relabel(ref, (2, 2, 1), (1, 1, 2))
    assert out.tolist() == [A(0), O(1), O(0), S(0)] and w == 1
    # three holes, a = 0: S(1) at 1, A(0) at 0, A(1) at 4; n' = 2: B = [0, 1] takes M = [2, 3]
    out, w = rr.relabel(ref, (2, 2, 1), (1, 0, 1))
    assert out.tolist() == [O(0), S(0)] and w == 2
    # from and to one element
    out, w = rr.relabel(np.array([S(0)], np.uint32), (1, 0, 0), (1, 1, 1))
    assert out.tolist() == [S(0), A(0), O(0)] and w == 2
    out, w = rr.relabel(np.array([A(0), O(0), S(0)], np.uint32), (1, 1, 1), (0, 0, 1))
    assert out.tolist() == [O(0)] and w == 1
    out, w = rr.relabel(np.array([A(0)], np.uint32), (0, 1, 0), (1, 0, 0))  # the only element is replaced
    assert out.tolist() == [S(0)] and w == 1
    with pytest.raises(AssertionError):
        rr.relabel(np.array([S(0), S(0)], np.uint32), (2, 0, 0), (1, 0, 0))  # not a permutation


def test_rule_composes_over_a_long_run():
    """200 steps from one order: every intermediate is a permutation, so the rule applies again."""
    rng = np.random.default_rng(9)
    cur = [5, 4, 3]
    ref = rng.permutation(np.array(rr.labels_of(cur), np.uint32))
    for _ in range(200):
        new = [min(12, max(0, c + int(rng.integers(-2, 3)))) for c in cur]
        if sum(new) == 0:
            new[0] = 1
        ref, _, _ = check_rule(ref, cur, new)
        cur = new


# ------------------------------------------------------------------------------- the reserve API
def test_reserve_error_codes_and_defaults(cpu):
    store = ColliderStore(cpu)
    assert [store.capacity(k) for k, _ in KINDS] == [0, 0, 0]  # the default: a count change unbinds
    store.reserve(10, 20, 30)
    assert [store.capacity(k) for k, _ in KINDS] == [10, 20, 30]
    for caps, code in (((-1, 0, 0), abi.ART_E_INVALID), ((0, -5, 0), abi.ART_E_INVALID), ((0, 0, -1), abi.ART_E_INVALID),
                       ((1 << 24, 1, 0), abi.ART_E_UNSUPPORTED), ((1 << 23, 1 << 23, 1), abi.ART_E_UNSUPPORTED)):
        with pytest.raises(art.ArtError) as e:
            store.reserve(*caps)
        assert e.value.code == code
        assert [store.capacity(k) for k, _ in KINDS] == [10, 20, 30]
    store.reserve(1 << 24, 0, 0)  # the limit itself, in total
    assert store.capacity(abi.ART_KIND_SPHERE) == 1 << 24
    store.reserve(0, 0, 0)
    assert [store.capacity(k) for k, _ in KINDS] == [0, 0, 0]
    assert cpu.lib.art_colliders_reserve(None, 1, 1, 1) == abi.ART_E_INVALID
    assert cpu.lib.art_collider_capacity(None, 0) == abi.ART_E_INVALID
    for kind in (-1, 3):
        with pytest.raises(art.ArtError) as e:
            store.capacity(kind)
        assert e.value.code == abi.ART_E_INVALID
    # while a frame is in flight
    scene, org, params = art.synth(art.CONFIGS[1], S=2, R=64, C_scale=0.25)
    fr = art.Frame(scene, params, org, art.FanOutputs(2, 64, params.max_hits_per_ray, 4, params.thread_count))
    h = cpu.schedule(fr)
    with pytest.raises(art.ArtError) as e:
        store.reserve(5, 5, 5)
    assert e.value.code == abi.ART_E_STATE
    h.complete()
    store.reserve(5, 6, 7)
    assert [store.capacity(k) for k, _ in KINDS] == [5, 6, 7]


def test_last_resize_before_any_sync_struct_and_version(cpu):
    store = ColliderStore(cpu)
    assert store.last_resize() == ZERO_STATS
    assert C.sizeof(abi.art_collider_resize_stats) == 7 * 4 + 4 + 8  # seven ints, padding, one u64
    assert C.sizeof(abi.art_collider_sync_stats) == 4 * 4 + 8  # untouched
    v = cpu.lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 10
    assert cpu.lib.art_colliders_last_resize(cpu.ptr, None) == abi.ART_E_INVALID
    assert cpu.lib.art_colliders_last_resize(None, C.byref(abi.art_collider_resize_stats())) == abi.ART_E_INVALID


def test_header_struct_size(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "art_colliders.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(art_collider_resize_stats), '
                   'offsetof(art_collider_resize_stats, bytes_uploaded)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "size")])
    size, off = (int(x) for x in subprocess.check_output([str(tmp_path / "size")], text=True).split())
    assert size == C.sizeof(abi.art_collider_resize_stats)
    assert off == abi.art_collider_resize_stats.bytes_uploaded.offset


def test_last_resize_counts_on_the_cpu_backend(cpu):
    """The CPU backend keeps no device scene: kept_bound 0 and the labels that appeared and vanished."""
    scene, _, _ = art.synth(art.CONFIGS[2], S=2, R=64, C_scale=0.0625)  # 128 spheres + 128 AABBs
    store = ColliderStore(cpu)
    store.reserve(200, 200, 8)
    counts = [0, 0, 0]
    for k, name in KINDS[:2]:
        store.add_many(k, getattr(scene, name)[:100])
        counts[k] = 100
    store.sync()
    assert store.last_resize() == dict(ZERO_STATS, added=200)
    rng = np.random.default_rng(4)
    for step in range(40):
        before = list(counts)
        for _ in range(int(rng.integers(0, 7))):
            k = int(rng.integers(0, 2))
            if rng.random() < 0.5:
                store.add(k, getattr(scene, KINDS[k][1])[int(rng.integers(0, 128))])
                counts[k] += 1
            else:
                i = int(rng.integers(-1, counts[k] + 1))  # some invalid: skipped
                store.remove_swapback(k, i)
                counts[k] -= 1 if 0 <= i < counts[k] else 0
        st = store.sync()
        rs = store.last_resize()
        assert [store.count(k) for k, _ in KINDS] == counts
        want = dict(ZERO_STATS, added=sum(max(0, c - b) for c, b in zip(counts, before)),
                    removed=sum(max(0, b - c) for c, b in zip(counts, before)), bytes_uploaded=st["bytes_uploaded"])
        assert rs == want, (step, rs, want)
        assert st["full_prep"] == (1 if counts != before else 0) and st["reallocated"] == 0
    store.clear()
    store.sync()
    assert store.last_resize() == dict(ZERO_STATS, removed=sum(counts))


def test_cpu_frames_after_adds_and_removes(cpu):
    scene, org, params = art.synth(art.CONFIGS[2], S=2, R=64, C_scale=0.0625)  # 128 spheres + 128 AABBs, T = 4
    store = ColliderStore(cpu)
    store.reserve(80, 80, 0)
    cur = {"spheres": scene.spheres[:64].copy(), "aabbs": scene.aabbs[:64].copy()}
    for k, name in KINDS[:2]:
        store.add_many(k, cur[name])
    store.sync()
    cpu.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
    try:
        steps = [[("add", 0, 64)], [("remove", 0, 0)], [("add", 1, 70), ("add", 1, 71), ("remove", 1, 3)],
                 [("remove", 0, 63), ("remove", 1, 65), ("remove", 1, 99)], [("add", 0, 90), ("remove", 0, 64)]]
        for step, ops in enumerate(steps):
            for op, k, i in ops:
                name = KINDS[k][1]
                if op == "add":
                    rec = getattr(scene, name)[i]
                    assert store.add(k, rec) == cur[name].size
                    cur[name] = np.append(cur[name], rec)
                else:
                    store.remove_swapback(k, i)
                    if 0 <= i < cur[name].size:
                        cur[name][i] = cur[name][-1]
                        cur[name] = cur[name][:-1].copy()
            store.sync()
            rs = store.last_resize()
            assert rs["kept_bound"] == 0 and rs["relabelled"] == 0 and rs["bvh_rebuilt"] == 0, rs
            sc = art.Scene(dirs=scene.dirs, targets=scene.targets, spheres=cur["spheres"], aabbs=cur["aabbs"])
            o_res = art.FanOutputs(2, 64, params.max_hits_per_ray, scene.T, params.thread_count)
            o_ref = o_res.copy()
            cpu.run(resident_frame(art.Frame(sc, params, org, o_res)))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=4)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, ops, eq)
    finally:
        cpu.set_flags(0)

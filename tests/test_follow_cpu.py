"""Target churn, the host half (ABI 3.13): per-source filter states and volumes follow the targets
(art_dsp_sources_follow_host against a numpy model of its contract), the store's composed follow map
against a Python identity model, and collider owners that follow a swapped target
(ART_CTX_TARGET_OWNERS_FOLLOW) against the reference's rule (AudioTargetManager.cs:86 ->
AudioCollider.UpdateAudioTargetId, AudioCollider.cs:46-50). These tests need no GPU.
"""
import ctypes as C

import numpy as np
import pytest

import art
from art import abi, dsp
from art.colliders import ColliderStore, resident_frame
from art.targets import TargetStore, resident_targets_frame
import oracle
from test_targets_resize_cpu import IdentityModel

KINDS = ((abi.ART_KIND_SPHERE, "spheres"), (abi.ART_KIND_AABB, "aabbs"), (abi.ART_KIND_OBB, "obbs"))


@pytest.fixture
def cpu():
    c = art.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------- the follow contract
def random_states(rng, n):
    """n states of random bits (NaN payloads, infinities and denormals among them), some -0.0."""
    raw = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    raw[rng.random((n, 8)) < 0.1] = 0x80000000  # -0.0
    raw[rng.random((n, 8)) < 0.1] = 0x7fc12345  # a quiet NaN with a payload
    raw[rng.random((n, 8)) < 0.05] = 0xff800001  # a signalling NaN
    return raw.view(abi.DSP_STATE).reshape(n)


def follow_model(target_src, T_old, fan_src, F_new, F_old, state_old, volume_old, new_volume):
    """The contract of art_dsp.h, literally, on raw bits."""
    T_new = len(target_src)
    so = state_old.view(np.uint32).reshape(-1, 8)
    sn = np.zeros((F_new * T_new, 8), np.uint32)
    vn = np.zeros(F_new * T_new, np.uint32)
    nv = np.float32(new_volume).view(np.uint32)
    for f in range(F_new):
        fo = f if fan_src is None else int(fan_src[f])
        for t in range(T_new):
            s, to = f * T_new + t, int(target_src[t])
            if 0 <= fo < F_old and 0 <= to < T_old:
                sn[s] = so[fo * T_old + to]
                vn[s] = volume_old.view(np.uint32)[fo * T_old + to] if volume_old is not None else nv
            else:
                vn[s] = nv
    return sn, vn


def swapback_map(T_old, removes):
    m = list(range(T_old))
    for i in removes:
        m[i] = m[-1]
        m.pop()
    return m


# (name, target_src, T_old)
TARGET_MAPS = [
    ("identity", list(range(4)), 4),
    ("add 4->5", [0, 1, 2, 3, -1], 4),
    ("remove in the middle 5->4", swapback_map(5, [1]), 5),
    ("T_old = 0", [-1, -1, -1], 0),
    ("33->32", swapback_map(33, [7]), 33),
    ("256->255 removing 0", swapback_map(256, [0]), 256),
]


@pytest.mark.parametrize("name,target_src,T_old", TARGET_MAPS, ids=[m[0] for m in TARGET_MAPS])
@pytest.mark.parametrize("fans", ["identity", "mapped"])
def test_host_twin_against_the_contract(name, target_src, T_old, fans):
    rng = np.random.default_rng(len(target_src) * 1000 + T_old)
    F_old = 5
    if fans == "identity":
        F_new, fan_src = 5, None
    else:  # permutes, drops (1 and 3), adds (-1) and holds out-of-range values on both sides
        fan_src = np.array([4, -1, 0, 5, 2, -7, 1 << 30, 2], np.int32)
        F_new = fan_src.size
    state_old = random_states(rng, F_old * T_old)
    volume_old = rng.integers(0, 1 << 32, F_old * T_old, dtype=np.uint64).astype(np.uint32).view(np.float32)
    keep_s, keep_v = state_old.copy(), volume_old.copy()
    for vo, want_volume in ((volume_old, True), (None, True), (volume_old, False)):
        sn, vn = dsp.sources_follow_host(target_src, T_old, F_new, F_old, state_old, vo, fan_src, new_volume=0.75,
                                         want_volume=want_volume)
        ms, mv = follow_model(target_src, T_old, fan_src, F_new, F_old, state_old, vo, 0.75)
        assert sn.tobytes() == ms.tobytes()
        if want_volume:
            assert vn.tobytes() == mv.tobytes()
        else:
            assert vn is None
    assert state_old.tobytes() == keep_s.tobytes() and volume_old.tobytes() == keep_v.tobytes()


def test_host_twin_moves_something():
    """The cases above are not vacuous: a removed target's successor carries its own state along."""
    rng = np.random.default_rng(1)
    state_old = random_states(rng, 2 * 5)
    sn, vn = dsp.sources_follow_host(swapback_map(5, [1]), 5, 2, 2, state_old)
    so = state_old.view(np.uint32).reshape(2, 5, 8)
    got = sn.view(np.uint32).reshape(2, 4, 8)
    assert (got[:, 1] == so[:, 4]).all() and (got[:, 0] == so[:, 0]).all() and (got[:, 3] == so[:, 3]).all()
    assert (vn == 1.0).all()


def test_host_twin_rejects_a_bad_map_and_writes_nothing():
    lib = art.load_library()
    state_old = random_states(np.random.default_rng(2), 3 * 4)
    for bad in ([0, 1, 4], [0, -2, 1], [3, 2, 1 << 20]):
        ts = np.array(bad, np.int32)
        sn = np.full(3 * 3 * 8, 0xabababab, np.uint32)
        vn = np.full(3 * 3, 0xabababab, np.uint32)
        rc = lib.art_dsp_sources_follow_host(ts.ctypes.data, 3, 4, None, 3, 3, state_old.ctypes.data, None, sn.ctypes.data,
                                             vn.ctypes.data, 1.0)
        assert rc == abi.ART_E_INVALID
        assert (sn == 0xabababab).all() and (vn == 0xabababab).all()


# ------------------------------------------------------------------------------- the composed follow map
class FollowModel(IdentityModel):
    """IdentityModel plus the base list of the follow map: serial -> index at the last mark."""

    def __init__(self):
        super().__init__()
        self.base, self.synced_ids = {}, []

    def sync(self):
        self.synced_ids = list(self.ids)

    def follow_map(self):
        return [self.base.get(s, -1) for s in self.synced_ids], len(self.base)

    def mark(self):
        self.base = {s: i for i, s in enumerate(self.synced_ids)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_follow_map_fuzz(cpu, seed):
    """100 marks per seed, one to three syncs between two marks, a random edit run before every sync."""
    rng = np.random.default_rng(seed)
    store, model = TargetStore(cpu), FollowModel()
    src, base = store.follow_map()
    assert src.size == 0 and base == 0
    serial = 0
    composed = reindexed = 0
    for mark in range(100):
        syncs = int(rng.integers(1, 4))
        for k in range(syncs):
            for _ in range(int(rng.integers(0, 7))):
                r, n = rng.random(), len(model.pos)
                serial += 1
                p = np.array([serial, rng.uniform(-50, 50), rng.uniform(-50, 50)], np.float32)
                if r < 0.35 or n == 0:
                    assert store.add(p) == model.add(p)
                elif r < 0.5:
                    i = int(rng.integers(0, n))
                    store.set(i, p)
                    model.set(i, p)
                elif r < 0.985:
                    i = int(rng.integers(-1, n + 1))  # some invalid
                    store.remove_swapback(i)
                    model.remove_swapback(i)
                else:
                    store.clear()
                    model.clear()
            store.sync()
            model.sync()
            want, want_base = model.follow_map()
            got, got_base = store.follow_map()
            assert got.tolist() == want and got_base == want_base, (mark, k, got.tolist(), want)
            survivors = [s for s in want if s >= 0]
            assert len(set(survivors)) == len(survivors) and all(s < want_base for s in survivors)
            if mark == 0:
                assert want == [-1] * len(want) and want_base == 0  # before the first mark everything is new
            if k > 0:
                composed += 1
                reindexed += sum(1 for i, s in enumerate(want) if s >= 0 and s != i)
            # a short buffer takes min(cap, count) entries
            if len(want) >= 2:
                short = np.full(len(want), -2, np.int32)
                assert cpu.lib.art_target_follow_map(cpu.ptr, short.ctypes.data, 1, None) == len(want)
                assert short[0] == want[0] and (short[1:] == -2).all()
        store.follow_mark()
        model.mark()
        got, got_base = store.follow_map()
        assert got.tolist() == list(range(store.synced_count())) and got_base == store.synced_count()
    assert composed >= 50 and reindexed >= 10  # the runs do compose maps with re-indexed survivors


def test_follow_map_composes_two_syncs(cpu):
    store = TargetStore(cpu)
    store.add_many(np.arange(15, dtype=np.float32).reshape(5, 3))
    store.sync()
    store.follow_mark()
    store.remove_swapback(1)            # [0 4 2 3]
    store.add(np.float32([9, 9, 9]))    # [0 4 2 3 n]
    store.sync()
    assert store.follow_map()[0].tolist() == [0, 4, 2, 3, -1]
    store.remove_swapback(0)            # [n 4 2 3]
    store.sync()
    assert store.sync_map().tolist() == [4, 1, 2, 3]          # the last sync alone
    assert store.follow_map()[0].tolist() == [-1, 4, 2, 3]    # both
    assert store.follow_map()[1] == 5
    store.follow_mark()
    assert store.follow_map()[0].tolist() == [0, 1, 2, 3] and store.follow_map()[1] == 4


# ------------------------------------------------------------------------------- collider owners
def owned_scene():
    """Config 2's scene at 1/16 (128 spheres, 128 AABBs, T = 4) with a fifth target and every third
    collider owned by one of the five targets, 16 OBBs made from AABBs among them."""
    scene, org, params = art.synth(art.CONFIGS[2], S=2, R=64, C_scale=0.0625)
    spheres, aabbs = scene.spheres[:48].copy(), scene.aabbs[:48].copy()
    obbs = np.zeros(16, abi.OBB)
    for n in ("center", "size", "material"):
        obbs[n] = scene.aabbs[48:64][n]
    for arr, shift in ((spheres, 0), (aabbs, 1), (obbs, 2)):
        tid = np.full(arr.size, -1, np.int16)
        idx = np.arange(arr.size)
        own = idx % 3 == 0
        tid[own] = ((idx[own] // 3 + shift) % 5).astype(np.int16)
        arr["audio_target_id"] = tid
    targets = np.concatenate([scene.targets, scene.targets[:1] + np.float32([1.5, 0.5, -2.0])]).astype(np.float32)
    # every owned sphere is a shell around its target: it muffles the target unless the owner skip sees it
    for i in np.flatnonzero(spheres["audio_target_id"] >= 0):
        spheres["center"][i] = targets[spheres["audio_target_id"][i]].astype(np.float16).view(np.uint16)
        spheres["radius"][i] = np.float16(1.5 + 0.125 * (i % 4)).view(np.uint16)
    return scene, org, params, {"spheres": spheres, "aabbs": aabbs, "obbs": obbs}, targets


def model_remove(cols, targets, i, follow=True):
    """The reference's rule on numpy arrays: the last target moves to i and its colliders name i."""
    n = len(targets)
    if not 0 <= i < n:
        return cols, targets, [0, 0, 0]
    counts = [0, 0, 0]
    last = n - 1
    if i != last:
        targets = targets.copy()
        targets[i] = targets[last]
        if follow:
            cols = {k: v.copy() for k, v in cols.items()}
            for kk, (_, name) in enumerate(KINDS):
                hit = cols[name]["audio_target_id"] == last
                cols[name]["audio_target_id"][hit] = i
                counts[kk] = int(hit.sum())
    return cols, targets[:last], counts


def fill(cstore, tstore, cols, targets):
    for k, name in KINDS:
        cstore.add_many(k, cols[name])
    tstore.add_many(targets)


def mirror(cstore):
    return {name: cstore.array(k) for k, name in KINDS}


def test_owners_follow_the_swapped_target(cpu):
    _, _, _, cols, targets = owned_scene()
    cstore, tstore = ColliderStore(cpu), TargetStore(cpu)
    fill(cstore, tstore, cols, targets)
    assert tstore.last_remove_owners() == [0, 0, 0]
    cpu.set_flags(abi.ART_CTX_TARGET_OWNERS_FOLLOW)
    try:
        for i in (1, 9, -1, 3, 0, 0, 0, 0):  # in the middle, out of range (twice), the last, down to none
            before = mirror(cstore)
            cols, targets, counts = model_remove(cols, targets, i)
            tstore.remove_swapback(i)
            assert tstore.last_remove_owners() == counts, i
            after = mirror(cstore)
            for _, name in KINDS:
                assert after[name].tobytes() == cols[name].tobytes(), (i, name)
            if i in (9, -1, 3):
                assert counts == [0, 0, 0] and all(after[n].tobytes() == before[n].tobytes() for _, n in KINDS)
            assert tstore.array().tobytes() == targets.tobytes()
        assert tstore.count() == 0
    finally:
        cpu.set_flags(0)


def test_owners_stay_without_the_flag(cpu):
    _, _, _, cols, targets = owned_scene()
    cstore, tstore = ColliderStore(cpu), TargetStore(cpu)
    fill(cstore, tstore, cols, targets)
    cstore.sync()
    tstore.remove_swapback(1)
    assert tstore.last_remove_owners() == [0, 0, 0]
    after = mirror(cstore)
    assert all(after[n].tobytes() == cols[n].tobytes() for _, n in KINDS)
    assert cstore.sync()["dirty_records"] == 0
    # with the flag the re-numbered records are dirty, as after art_collider_set
    cpu.set_flags(abi.ART_CTX_TARGET_OWNERS_FOLLOW)
    try:
        cols2, _, counts = model_remove(cols, targets[:4], 0)
        tstore.remove_swapback(0)
        assert tstore.last_remove_owners() == counts and sum(counts) > 0
        assert cstore.sync()["dirty_records"] == sum(counts)
    finally:
        cpu.set_flags(0)


@pytest.mark.parametrize("order", ["targets first", "colliders first"])
def test_cpu_frames_after_removes_with_owners(cpu, order):
    scene, org, params, cols, targets = owned_scene()
    cstore, tstore = ColliderStore(cpu), TargetStore(cpu)
    fill(cstore, tstore, cols, targets)
    cstore.sync()
    tstore.sync()
    flags = abi.ART_CTX_RESIDENT_COLLIDERS | abi.ART_CTX_RESIDENT_TARGETS
    cpu.set_flags(flags | abi.ART_CTX_TARGET_OWNERS_FOLLOW)
    try:
        differs = 0
        for step, i in enumerate((1, 0, 0)):
            stale = cols
            cols, targets, counts = model_remove(cols, targets, i)
            assert sum(counts) > 0
            tstore.remove_swapback(i)
            for sync in ((tstore.sync, cstore.sync) if order == "targets first" else (cstore.sync, tstore.sync)):
                sync()
            T = len(targets)
            sc = art.Scene(dirs=scene.dirs, targets=targets, spheres=cols["spheres"], aabbs=cols["aabbs"], obbs=cols["obbs"])
            o_res = art.FanOutputs(2, 64, params.max_hits_per_ray, T, params.thread_count)
            o_ref, o_stale = o_res.copy(), o_res.copy()
            cpu.run(resident_targets_frame(resident_frame(art.Frame(sc, params, org, o_res))))
            oracle.run_frame(art.Frame(sc, params, org, o_ref), threads=4)
            eq = o_res.equal(o_ref)
            assert all(eq.values()), (step, i, eq)
            # what a caller who forgot to re-number would get: wrong owner skips
            sc2 = art.Scene(dirs=scene.dirs, targets=targets, spheres=stale["spheres"], aabbs=stale["aabbs"],
                            obbs=stale["obbs"])
            oracle.run_frame(art.Frame(sc2, params, org, o_stale), threads=4)
            differs += 0 if all(o_stale.equal(o_ref).values()) else 1
        assert differs > 0  # the owners matter in this scene
    finally:
        cpu.set_flags(0)


# ------------------------------------------------------------------------------- ABI
def test_abi_version_and_null_arguments(cpu):
    lib = cpu.lib
    v = lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 13
    assert abi.ART_CTX_TARGET_OWNERS_FOLLOW == 0x1000
    buf = np.zeros(4, np.int32)
    base = C.c_int32(-5)
    assert lib.art_target_follow_map(None, buf.ctypes.data, 4, C.byref(base)) == abi.ART_E_INVALID
    assert lib.art_target_follow_map(cpu.ptr, None, 1, C.byref(base)) == abi.ART_E_INVALID
    assert lib.art_target_follow_map(cpu.ptr, buf.ctypes.data, -1, C.byref(base)) == abi.ART_E_INVALID
    assert lib.art_target_follow_map(cpu.ptr, None, 0, C.byref(base)) == 0 and base.value == 0
    assert lib.art_target_follow_map(cpu.ptr, None, 0, None) == 0
    assert lib.art_target_follow_mark(None) == abi.ART_E_INVALID
    assert lib.art_target_follow_mark(cpu.ptr) == abi.ART_OK
    assert lib.art_target_last_remove_owners(None, buf.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_target_last_remove_owners(cpu.ptr, None) == abi.ART_E_INVALID
    st = np.zeros(4, abi.DSP_STATE)
    ts = np.array([0, 1], np.int32)
    follow = lib.art_dsp_sources_follow_host
    assert follow(None, 2, 2, None, 2, 2, st.ctypes.data, None, st.ctypes.data, None, 1.0) == abi.ART_E_INVALID
    assert follow(ts.ctypes.data, 2, 2, None, 2, 2, None, None, st.ctypes.data, None, 1.0) == abi.ART_E_INVALID
    assert follow(ts.ctypes.data, 2, 2, None, 2, 2, st.ctypes.data, None, None, None, 1.0) == abi.ART_E_INVALID
    assert follow(ts.ctypes.data, -1, 2, None, 2, 2, st.ctypes.data, None, st.ctypes.data, None, 1.0) == abi.ART_E_INVALID
    assert follow(None, 0, 2, None, 2, 2, None, None, None, None, 1.0) == abi.ART_OK  # nothing to write
    # the device call: no context, and the CPU backend
    dev = lib.art_dsp_sources_follow_device
    assert dev(None, ts.ctypes.data, 2, 2, None, 2, 2, None, None, None, None, 1.0, None) == abi.ART_E_INVALID
    assert dev(cpu.ptr, ts.ctypes.data, 2, 2, None, 2, 2, None, None, None, None, 1.0, None) == abi.ART_E_UNSUPPORTED

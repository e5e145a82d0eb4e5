"""Target churn on the GPU (ABI 3.13): dsp_sources_follow_kernel against its host twin
(art_dsp_sources_follow_host, which tests/test_follow_cpu.py pins against the contract), the whole
step remove / add -> syncs -> follow -> mark -> frame -> tick_mix against states the test keeps per
target identity, and collider owners that follow a swapped target on a bound scene, in both sync
orders. Every comparison is byte equality.
"""
import numpy as np
import pytest

import art
from art import abi, dsp
from art.targets import TargetStore, resident_targets_frame
import oracle
from test_dsp import random_settings
from test_follow_cpu import random_states, swapback_map
from test_mix_gpu import CANARY, split_canary, with_canary
from test_tick_cpu import random_case
from test_tick_gpu import R, dev, stream, tiny_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
KINDS = (abi.ART_KIND_SPHERE, abi.ART_KIND_AABB, abi.ART_KIND_OBB)

# (F_old, F_new, T_old, target_src, fan_src)
SHAPES = [
    (1, 1, 1, [0], None),
    (7, 7, 4, [0, 1, 2, 3, -1], None),
    (13, 13, 5, swapback_map(5, [1]), None),
    (2, 2, 33, swapback_map(33, [7]), None),
    (3, 3, 256, swapback_map(256, [0]), None),
    (9, 6, 3, [0, 2, 1], [8, -1, 3, 9, 1 << 30, -5]),  # a fan map with -1 and out-of-range entries, both sides
    (70000, 70000, 1, [0], None),                      # more fans than a grid's y extent
    (5, 5, 0, [-1, -1, -1], None),                     # all new
]
IDS = ["%d->%d fans, T %d->%d" % (s[0], s[1], s[2], len(s[3])) for s in SHAPES]


def shifted(a, lead, fill=0xC3):
    """A device buffer holding `lead` bytes, then a copy of `a`, then CANARY bytes; returns (tensor, pointer to a)."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.from_numpy(np.concatenate([np.full(lead, fill, np.uint8), raw, np.full(CANARY, fill, np.uint8)])).to(
        torch.device("cuda", 0))
    return t, t.data_ptr() + lead


def unshift(t, lead, fill=0xC3):
    h = t.cpu().numpy()
    assert (h[:lead] == fill).all() and (h[h.size - CANARY:] == fill).all(), "bytes around the buffer were written"
    return h[lead:h.size - CANARY]


def run_case(ctx, F_old, F_new, T_old, target_src, fan_src, lead, volumes):
    import torch
    T_new = len(target_src)
    rng = np.random.default_rng(1000 * F_new + 10 * T_new + lead)
    state_old = random_states(rng, F_old * T_old)
    volume_old = rng.integers(0, 1 << 32, F_old * T_old, dtype=np.uint64).astype(np.uint32).view(f32)
    vo = volume_old if volumes in ("both",) else None
    want_s, want_v = dsp.sources_follow_host(target_src, T_old, F_new, F_old, state_old, vo, fan_src, new_volume=0.625,
                                             want_volume=volumes != "none")
    d_so, p_so = shifted(state_old, lead)
    d_vo, p_vo = shifted(volume_old, lead)
    d_sn, p_sn = shifted(np.full(F_new * T_new * 32, 0x5A, np.uint8), lead)
    d_vn, p_vn = shifted(np.full(F_new * T_new * 4, 0x5A, np.uint8), lead)
    d_fs = p_fs = None
    if fan_src is not None:
        d_fs, p_fs = shifted(np.array(fan_src, np.int32), lead)
    dsp.sources_follow_device(ctx, target_src, T_new, T_old, F_new, F_old, p_so, p_sn, p_vo if vo is not None else None,
                              p_vn if volumes != "none" else None, p_fs, 0.625, stream())
    torch.cuda.synchronize()
    assert unshift(d_so, lead).tobytes() == state_old.tobytes(), "d_state_old was written"
    assert unshift(d_vo, lead).tobytes() == volume_old.tobytes(), "d_volume_old was written"
    got_s, got_v = unshift(d_sn, lead), unshift(d_vn, lead)
    bad = np.flatnonzero((got_s.reshape(-1, 32) != want_s.view(np.uint8).reshape(-1, 32)).any(axis=1))
    assert bad.size == 0, f"states of sources {bad[:8]} differ"
    if volumes == "none":
        assert (got_v == 0x5A).all(), "volumes were written without d_volume_new"
    else:
        assert got_v.tobytes() == want_v.tobytes()
    if d_fs is not None:
        assert unshift(d_fs, lead).tobytes() == np.array(fan_src, np.int32).tobytes()
    return want_s


@pytest.mark.parametrize("F_old,F_new,T_old,target_src,fan_src", SHAPES, ids=IDS)
def test_follow_device_equals_host(ctx, F_old, F_new, T_old, target_src, fan_src):
    """States and volumes against the host twin; the old arrays are only read; nothing is written
    around the new arrays."""
    want = run_case(ctx, F_old, F_new, T_old, target_src, fan_src, 0, "both")
    if T_old:  # not vacuous: some source did take an old state
        assert want.view(np.uint32).any()


@pytest.mark.parametrize("volumes", ["both", "new only", "none"])
def test_follow_device_unaligned_and_volume_forms(ctx, volumes):
    """Every device pointer 4 bytes past a 16-byte boundary (the 4-byte access path), with both volume
    arrays, with d_volume_old NULL (every source gets new_volume) and with d_volume_new NULL."""
    run_case(ctx, 13, 13, 5, swapback_map(5, [1]), None, 4, volumes)
    run_case(ctx, 9, 6, 3, [0, 2, 1], [8, -1, 3, 9, 1 << 30, -5], 4, volumes)


def test_follow_errors_gpu():
    import torch
    with art.Context(1) as c:
        lib = c.lib
        d = torch.full((8192,), 0x11, dtype=torch.uint8, device="cuda:0")
        p = d.data_ptr()
        ts = np.array([0, 1, -1], np.int32)
        tp = ts.ctypes.data
        call = lambda src=tp, Tn=3, To=2, fs=None, Fn=2, Fo=2, so=p, vo=None, sn=p + 4096, vn=None: (  # noqa: E731
            lib.art_dsp_sources_follow_device(c.ptr, src, Tn, To, fs, Fn, Fo, so, vo, sn, vn, 1.0, None))
        assert call() == abi.ART_OK
        # overlapping old and new ranges: the same array, a partial overlap, a volume inside a state array
        assert call(sn=p) == abi.ART_E_INVALID
        assert "overlap" in lib.art_last_error(c.ptr).decode()
        assert call(sn=p + 2 * 2 * 32 - 4) == abi.ART_E_INVALID
        assert call(so=p + 4096 + 2 * 3 * 32 - 32) == abi.ART_E_INVALID
        assert call(vn=p + 64) == abi.ART_E_INVALID
        assert call(vo=p + 4096 + 16, vn=p + 2048) == abi.ART_E_INVALID
        assert call(vo=p + 1024, vn=p + 2048) == abi.ART_OK  # adjacent ranges are fine
        assert call(so=p, sn=p + 2 * 2 * 32) == abi.ART_OK
        # required pointers, alignment, the map's range, the counts
        assert call(sn=None) == abi.ART_E_INVALID and call(so=None) == abi.ART_E_INVALID
        assert call(so=None, To=0, src=np.array([-1, -1, -1], np.int32).ctypes.data) == abi.ART_OK  # no old source
        assert call(sn=p + 4096 + 2) == abi.ART_E_INVALID and call(fs=p + 1) == abi.ART_E_INVALID
        for bad in ([0, 2, 1], [0, -2, 1]):
            assert call(src=np.array(bad, np.int32).ctypes.data) == abi.ART_E_INVALID
        assert call(Tn=-1) == abi.ART_E_INVALID and call(Fo=-1) == abi.ART_E_INVALID
        big = np.zeros(257, np.int32)
        assert call(src=big.ctypes.data, Tn=257, To=1) == abi.ART_E_UNSUPPORTED
        assert call(To=257) == abi.ART_E_UNSUPPORTED
        assert call(src=big.ctypes.data, Tn=256, To=1, Fn=1 << 23) == abi.ART_E_UNSUPPORTED  # 2^31 sources
        # nothing to do: no launch, nothing written (the pointers are not even looked at)
        before = d.cpu().numpy().copy()
        assert call(Fn=0, sn=None, so=None) == abi.ART_OK
        assert call(Tn=0, sn=None, so=None) == abi.ART_OK
        # store-map mode: the caller's counts must be the store's
        store = TargetStore(c)
        store.add_many(np.arange(9, dtype=f32).reshape(3, 3))
        store.sync()
        assert store.follow_map()[1] == 0
        assert call(src=None, Tn=3, To=0, so=None) == abi.ART_OK  # three new targets
        assert call(src=None, Tn=4, To=0, so=None) == abi.ART_E_INVALID
        assert "store" in lib.art_last_error(c.ptr).decode()
        assert call(src=None, Tn=3, To=1) == abi.ART_E_INVALID
        store.follow_mark()
        assert call(src=None, Tn=3, To=0, so=None) == abi.ART_E_INVALID  # the base list has three targets now
        assert call(src=None, Tn=3, To=3) == abi.ART_OK
        assert call(src=None, Tn=3, To=3, Fn=0) == abi.ART_OK
        torch.cuda.synchronize()
        after = d.cpu().numpy()
        # the calls since `before` wrote d_state_new only
        assert after[:2048].tobytes() == before[:2048].tobytes()


def test_follow_nothing_to_do_writes_nothing(ctx):
    import torch
    d = torch.full((1024,), 0x77, dtype=torch.uint8, device="cuda:0")
    p = d.data_ptr()
    ts = np.array([0, 1], np.int32)
    lib = ctx.lib
    assert lib.art_dsp_sources_follow_device(ctx.ptr, ts.ctypes.data, 2, 2, None, 0, 2, p, None, p + 512, p + 768, 1.0,
                                             stream()) == abi.ART_OK
    assert lib.art_dsp_sources_follow_device(ctx.ptr, ts.ctypes.data, 0, 2, None, 2, 2, p, None, p + 512, p + 768, 1.0,
                                             stream()) == abi.ART_OK
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 0x77).all()


# ------------------------------------------------------------------------------- end to end
def test_churn_end_to_end():
    """Resident targets with a reserved capacity on the tiny scene, 3 fans, T = 5: a frame and two
    tick_mix calls build states up; target 1 leaves (4 -> 1 by swap-back) and one joins; a first sync,
    a second one after another remove that moves one more target (the follow map is a composition);
    follow in store-map mode, mark, the layout again, a frame and a tick_mix. The expected mix and
    states come from the host twins over states the test keeps per target identity; the mix that the
    un-followed states would have given differs."""
    import torch
    S, T, frames = 3, 5, 48
    rng = np.random.default_rng(31)
    scene, org, params = tiny_scene(T, S)
    st = random_settings(rng)
    listeners, _, _ = random_case(rng, S, T)
    listeners["position"] = org + rng.uniform(-0.5, 0.5, (S, 3)).astype(f32)
    new_volume = f32(0.5)

    with art.Context(1) as c:
        store = TargetStore(c)
        store.reserve(6)
        ident = list(range(T))  # the identity of the target at every index
        store.add_many(scene.targets)
        store.sync()
        store.follow_mark()
        c.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        positions = {i: scene.targets[i].copy() for i in ident}
        serial = T

        def frame_of(tgts):
            sc = art.Scene(dirs=scene.dirs, targets=np.ascontiguousarray(tgts), spheres=scene.spheres, aabbs=scene.aabbs)
            fr = art.Frame(sc, params, org, art.FanOutputs(S, R, 1, len(tgts), 1))
            fr.scene = sc
            return fr

        fr = frame_of(scene.targets)
        c.bind(resident_targets_frame(fr))
        lay = art.fan_layout(fr)
        dsp.bind_settings(c, st, 48000)
        d_org, d_ls = torch.from_numpy(np.ascontiguousarray(org)).to("cuda:0"), dev(listeners)

        # per (fan, identity): state and volume, as the host twins leave them
        states = {(f, i): np.zeros(1, abi.DSP_STATE) for f in range(S) for i in ident}
        volumes = {(f, i): f32(rng.uniform(0.25, 2.0)) for f in range(S) for i in ident}
        dry_of = {}

        def host_tick(d_block, lay, ident, state_arr=None):
            """Expected (mix, states) of one tick_mix over the device block's settings; state_arr
            overrides the states kept per identity (which are then left alone)."""
            Tn = len(ident)
            tgts = np.array([positions[i] for i in ident], f32)
            fs = art.unpack_block(d_block.cpu().numpy(), lay, S, R, 1, Tn, 1).settings
            vol = np.array([volumes[(f, i)] for f in range(S) for i in ident], f32)
            prm = dsp.tick_params_host(st, listeners, fs, tgts, vol, 48000)
            arr = state_arr.copy() if state_arr is not None else np.concatenate([states[(f, i)] for f in range(S) for i in ident])
            mix = dsp.mix_host(prm, arr, np.stack([dry_of[i] for i in ident]), S, Tn)
            if state_arr is None:
                for k, key in enumerate((f, i) for f in range(S) for i in ident):
                    states[key] = arr[k:k + 1].copy()
            return mix, arr

        def device_tick(d_block, lay, ident, d_state, d_vol):
            Tn = len(ident)
            d_dry = dev(np.stack([dry_of[i] for i in ident]))
            d_params = dev(np.zeros(S * Tn, abi.DSP_SOURCE_PARAMS))
            d_mix = dev(np.zeros((S, frames * 2), f32))
            c.launch_device(d_org.data_ptr(), S, d_block.data_ptr(), 0, stream())
            dsp.tick_mix_device(c, d_block, S, d_ls, d_dry, d_state, frames, d_params, d_mix, d_vol, 0, stream())
            torch.cuda.synchronize()
            return d_mix.cpu().numpy().view(f32).reshape(S, -1)

        # 1. a frame, then two ticks: the states build up
        d_state = dev(np.zeros(S * T, abi.DSP_STATE))
        d_vol = dev(np.array([volumes[(f, i)] for f in range(S) for i in ident], f32))
        d_block = dev(art.pack_block(art.FanOutputs(S, R, 1, T, 1), lay))
        for tick in range(2):
            for i in ident:
                dry_of[i] = (rng.standard_normal(frames * 2) * 0.5).astype(f32)
            got = device_tick(d_block, lay, ident, d_state, d_vol)
            want, want_state = host_tick(d_block, lay, ident)
            assert got.tobytes() == want.tobytes(), f"tick {tick} before the churn"
            assert d_state.cpu().numpy().tobytes() == want_state.tobytes()
        state_before = d_state.cpu().numpy().view(abi.DSP_STATE).copy()

        # 2. target 1 leaves (4 -> 1), one joins; 3. sync, another remove that moves one target, sync
        def remove(i):
            store.remove_swapback(i)
            ident[i] = ident[-1]
            ident.pop()

        remove(1)
        p_new = (scene.targets[0] + f32([0.75, -0.5, 1.25])).astype(f32)
        assert store.add(p_new) == len(ident)
        ident.append(serial)
        positions[serial] = p_new
        serial += 1
        assert store.sync()["count_changed"] == 0 and store.last_resize()["kept_bound"] == 1
        assert store.follow_map()[0].tolist() == [0, 4, 2, 3, -1]
        remove(0)  # the new target moves to index 0
        store.sync()
        rs = store.last_resize()
        assert rs["kept_bound"] == 1 and rs["removed"] == 1, rs
        src, base = store.follow_map()
        assert store.sync_map().tolist() == [4, 1, 2, 3] and src.tolist() == [-1, 4, 2, 3] and base == 5
        assert src.tolist() == [i if i < T else -1 for i in ident]
        Tn = len(ident)
        d_state_new = with_canary(np.full(S * Tn * 32, 0x5A, np.uint8))
        d_vol_new = with_canary(np.full(S * Tn * 4, 0x5A, np.uint8))
        dsp.sources_follow_device(c, None, Tn, T, S, S, d_state, d_state_new, d_vol, d_vol_new, None, float(new_volume),
                                  stream())
        store.follow_mark()
        assert store.follow_map()[0].tolist() == list(range(Tn)) and store.follow_map()[1] == Tn
        for f in range(S):
            states[(f, ident[0])] = np.zeros(1, abi.DSP_STATE)
            volumes[(f, ident[0])] = new_volume
        torch.cuda.synchronize()
        got_state = split_canary(d_state_new)
        assert got_state.tobytes() == np.concatenate([states[(f, i)] for f in range(S) for i in ident]).tobytes()
        assert split_canary(d_vol_new).tobytes() == np.array([volumes[(f, i)] for f in range(S) for i in ident], f32).tobytes()
        assert d_state.cpu().numpy().tobytes() == state_before.tobytes()

        # 4. the layout for the new count; 5. a frame, then a tick
        fr = frame_of(np.array([positions[i] for i in ident], f32))
        lay = art.fan_layout(fr)
        d_block = dev(art.pack_block(art.FanOutputs(S, R, 1, Tn, 1), lay))
        for i in ident:
            dry_of[i] = (rng.standard_normal(frames * 2) * 0.5).astype(f32)
        d_state_t, d_vol_t = d_state_new[:-CANARY].clone(), d_vol_new[:-CANARY].clone()  # (16-byte aligned copies)
        got = device_tick(d_block, lay, ident, d_state_t, d_vol_t)
        unfollowed, _ = host_tick(d_block, lay, ident, state_arr=state_before[:S * Tn])
        want, want_state = host_tick(d_block, lay, ident)
        assert got.tobytes() == want.tobytes(), "the mix after the churn"
        assert d_state_t.cpu().numpy().tobytes() == want_state.tobytes(), "the states after the churn"
        assert unfollowed.tobytes() != want.tobytes()  # playing the targets through other targets' filter memory is audible
        # the frame itself is the oracle's for the model's targets (its settings are what the tick read)
        o_ref, _ = oracle.run(fr.scene, params, org, art.FanOutputs(S, R, 1, Tn, 1))
        fs = art.unpack_block(d_block.cpu().numpy(), lay, S, R, 1, Tn, 1).settings
        assert fs.tobytes() == o_ref.settings.tobytes()
        c.set_flags(0)


# ------------------------------------------------------------------------------- owners on the device
@pytest.mark.parametrize("order", ["targets first", "colliders first"])
def test_owners_follow_on_a_bound_scene(order):
    """Resident colliders and targets with both reserves and ART_CTX_TARGET_OWNERS_FOLLOW; the last
    target owns colliders of every kind. Removing an earlier target dirties both stores: after both
    syncs, in either order, the frame is that of a fresh bind of the model's scene and the oracle's."""
    from test_colliders_resize_gpu import CRig, pools
    from test_targets_gpu import base_scene
    scene, org, params = base_scene(2, T=4)
    scene.aabbs = scene.aabbs.copy()
    scene.aabbs["audio_target_id"][::9] = 3
    scene.aabbs["audio_target_id"][4::9] = 2
    scene.obbs = pools()[abi.ART_KIND_OBB][:4].copy()
    scene.obbs["audio_target_id"] = [3, -1, 2, 3]
    assert (scene.spheres["audio_target_id"] == 3).any() and (scene.spheres["audio_target_id"] == 2).any()
    rig = CRig(scene, org, params, target_cap=6)
    try:
        rig.ctx.set_flags(rig.flags | abi.ART_CTX_TARGET_OWNERS_FOLLOW)
        rig.check(rig.launch(), what="bound")
        for step, i in enumerate((1, 0)):
            last = len(rig.targets) - 1
            counts = [0, 0, 0]
            for kk, k in enumerate(KINDS):  # the reference's rule on the model
                for rec in rig.model.lists[k]:
                    if rec["audio_target_id"] == last:
                        rec["audio_target_id"] = i
                        counts[kk] += 1
            rig.targets[i] = rig.targets[last]
            rig.targets.pop()
            rig.tstore.remove_swapback(i)
            assert rig.tstore.last_remove_owners() == counts and min(counts) > 0, counts
            if order == "targets first":
                rig.tstore.sync()
                st = rig.store.sync()
            else:
                st = rig.store.sync()
                rig.tstore.sync()
            assert st["dirty_records"] == sum(counts) and st["full_prep"] == 0 and st["cells_rebuilt"] == 1, st
            assert rig.tstore.last_resize()["kept_bound"] == 1
            rig.check(rig.launch(), what=f"step {step}: remove {i}, {order}")
    finally:
        rig.close()


@pytest.mark.parametrize("order", ["targets first", "colliders first"])
def test_owner_counts_follow_either_order(order):
    """Counting frames of a scene with permeation (art_count_device): the permeation loss counts sum, over
    the targets, the colliders each target does not own. After a remove that re-numbers owners and both
    syncs, in either order, they are the oracle's for the model's scene."""
    from test_colliders_resize_gpu import CRig
    from test_targets_gpu import R as RR, S as RS
    scene, org, params = art.synth(art.CONFIGS[1], S=RS, R=RR)  # 256 AABBs owned by the 4 targets, permeation
    assert scene.T == 4 and scene.aabbs.size == 256 and (scene.aabbs["audio_target_id"] == 3).any()
    rig = CRig(scene, org, params, cap=(8, 264, 8), target_cap=6)
    try:
        rig.ctx.set_flags(rig.flags | abi.ART_CTX_TARGET_OWNERS_FOLLOW)
        moved = 0
        for rec in rig.model.lists[abi.ART_KIND_AABB]:
            if rec["audio_target_id"] == 3:
                rec["audio_target_id"] = 1
                moved += 1
        rig.targets[1] = rig.targets[3]
        rig.targets.pop()
        rig.tstore.remove_swapback(1)
        assert rig.tstore.last_remove_owners() == [0, moved, 0]
        for sync in ((rig.tstore.sync, rig.store.sync) if order == "targets first" else (rig.store.sync, rig.tstore.sync)):
            sync()
        assert rig.tstore.last_resize()["kept_bound"] == 1
        sc = rig.model_scene()
        rig.check(rig.launch(), sc, what=f"remove 1, {order}")
        counts = rig.ctx.count_device(rig.d_org.data_ptr(), RS, rig.block(sc).data_ptr(), 0, stream())
        want = oracle.run(sc, params, org, rig.outputs(sc.T), threads=8)[1]
        assert want["perm_loss_aabb"] > 0
        assert counts == want, (counts, want)
    finally:
        rig.close()

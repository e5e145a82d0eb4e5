"""The audio tick on the GPU (include/art_dsp.h: art_dsp_settings_bind, art_dsp_tick_params_device,
art_dsp_tick_device).

dsp_tick_params_kernel turns the settings section of a frame's result blocks into the spatializer's
per-buffer scalars. Its check is always byte equality with the host twin (art_dsp_tick_params_host,
which tests/test_tick_cpu.py pins against the definition), on blocks the test synthesises and on
blocks a frame wrote; the chained entry point is checked against the oracle's per-sample chain.
"""
import numpy as np
import pytest

import art
from art import abi
from art.dsp import AudioSource, SpatializerSettings
import oracle
from test_dsp import random_settings
from test_tick_cpu import definition_params, random_case

pytestmark = pytest.mark.gpu

f32 = np.float32
R = 64
FLOAT_FIELDS = ("muffle_alpha", "dry_boost", "gain_left", "gain_right", "filter_alpha", "volume")


def tiny_scene(T, S=1, seed=1):
    """The smallest config (one hit per ray, a few dozen colliders) with T targets: the config's own
    four, which own colliders, and further ones spread over the colliders' box."""
    scene, org, params = art.synth(art.CONFIGS[2], S=S, R=R, C_scale=0.01)
    assert params.max_hits_per_ray == 1 and scene.C <= 48
    rng = np.random.default_rng(seed)
    c = np.concatenate([a["center"].view(np.float16).astype(f32).reshape(-1, 3) for a in (scene.spheres, scene.aabbs)])
    extra = rng.uniform(c.min(axis=0), c.max(axis=0), (max(0, T - scene.T), 3)).astype(f32)
    targets = np.ascontiguousarray(np.concatenate([scene.targets, extra])[:T])
    return art.Scene(dirs=scene.dirs, targets=targets, spheres=scene.spheres, aabbs=scene.aabbs), org, params


def bind(ctx, T, S=1, out_flags=0):
    """Bind the tiny scene with T targets; returns (scene, origins, params, layout for out_flags)."""
    scene, org, params = tiny_scene(T, S)
    fr = art.Frame(scene, params, org, art.FanOutputs(S, R, 1, T, 1))
    ctx.bind(fr)
    if out_flags:  # another stride: a kernel using the plain layout would read garbage
        assert art.fan_layout(fr, out_flags)["stride"] > art.fan_layout(fr, 0)["stride"]
    return scene, org, params, art.fan_layout(fr, out_flags)


def synth_block(fs, lay):
    """Result blocks holding the settings fs (abi.SETTINGS [S, T]) at the layout's offsets, 0xA5 elsewhere."""
    S, T = fs.shape
    b = np.full((S, lay["stride"]), 0xA5, np.uint8)
    b[:, lay["settings_off"]:lay["settings_off"] + T * 24] = np.ascontiguousarray(fs).view(np.uint8).reshape(S, T * 24)
    return b.reshape(-1)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_params(ctx, block, S, T, listeners, volume, out_flags=0):
    """art_dsp_tick_params_device over a host block; returns (params, the block read back)."""
    import torch
    d_block, d_ls = dev(block), dev(listeners)
    d_vol = dev(volume) if volume is not None else None
    d_params = torch.full((S * T * 32,), 0x5A, dtype=torch.uint8, device=d_block.device)
    art.dsp.tick_params_device(ctx, d_block, S, d_ls, d_params, d_vol, out_flags, stream())
    torch.cuda.synchronize()
    return d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS), d_block.cpu().numpy()


@pytest.mark.parametrize("S,T,out_flags", [(1, 1, 0), (3, 5, 0), (3, 5, abi.ART_OUT_HIT_RESULTS), (13, 5, 0)])
def test_params_device_equals_host(ctx, S, T, out_flags):
    rng = np.random.default_rng(100 * S + T + out_flags)
    scene, _, _, lay = bind(ctx, T, out_flags=out_flags)
    st = random_settings(rng)
    art.dsp.bind_settings(ctx, st, 48000)
    listeners, fs, _ = random_case(rng, S, T)
    block = synth_block(fs, lay)
    for volume in (None, rng.uniform(0, 2, S * T).astype(f32)):
        want = art.dsp.tick_params_host(st, listeners, fs, scene.targets, volume, 48000)
        got, after = device_params(ctx, block, S, T, listeners, volume, out_flags)
        assert got.tobytes() == want.tobytes(), (volume is None, got, want)
        assert after.tobytes() == block.tobytes()  # the block is only read


def test_params_device_nan_source(ctx):
    """A listener on the perceived position: world = 0, normalize gives NaN. Device and host agree on
    which fields are NaN (the default NaNs differ in sign); every other source is byte-equal."""
    S, T = 3, 5
    rng = np.random.default_rng(77)
    scene, _, _, lay = bind(ctx, T)
    st = random_settings(rng)
    art.dsp.bind_settings(ctx, st, 44100)
    listeners, fs, _ = random_case(rng, S, T)
    fs["perceived_position"][1, 2] = listeners["position"][1]
    want = art.dsp.tick_params_host(st, listeners, fs, scene.targets, None, 44100)
    got, _ = device_params(ctx, synth_block(fs, lay), S, T, listeners, None)
    bad = 1 * T + 2
    nan_w = [bool(np.isnan(want[bad][k])) for k in FLOAT_FIELDS]
    assert any(nan_w) and nan_w == [bool(np.isnan(got[bad][k])) for k in FLOAT_FIELDS]
    for k in FLOAT_FIELDS:
        if not np.isnan(want[bad][k]):
            assert got[bad][k].tobytes() == want[bad][k].tobytes(), k
    assert got[bad]["flags"] == want[bad]["flags"]
    keep = np.arange(S * T) != bad
    assert got[keep].tobytes() == want[keep].tobytes()


def sweep_case(rng, S, T):
    """Listeners, settings and perceived positions of the sweep: special local directions under exact
    rotations in the first fans, random ones after them; listeners around the targets, so that the
    distances lie on both sides of every max_*_distance."""
    listeners = np.zeros(S, abi.LISTENER)
    listeners["position"] = rng.uniform(-1, 1, (S, 3)) * rng.uniform(0, 20, (S, 1))
    q = rng.standard_normal((S, 4))
    listeners["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    exact = [(0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0)]  # identity, 180 degrees about y, x, z
    special = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),  # the axes, directly behind
                        (1, 0.0, 1), (1, -0.0, 1), (-1, 0.0, -1), (0, 0.0, -3), (0, -0.0, -3), (2, 0.0, 0),
                        (1e-30, 0, -1), (-1e-30, 0, -1), (1, 1, 1), (-1, -1, -1)], f32)
    fs = np.zeros((S, T), abi.SETTINGS)
    fs["muffle_strength"] = np.where(rng.random((S, T)) < 0.3, 0.0, rng.random((S, T)))
    fs["reverb_strength"] = rng.random((S, T))
    fs["reverb_volume"] = rng.random((S, T))
    d = rng.standard_normal((S, T, 3))
    d[rng.random((S, T)) < 0.05, 1] = 0.0  # on the horizon: the low-pass branch's boundary
    fs["perceived_position"] = (listeners["position"][:, None, :] + d * rng.uniform(0.01, 40, (S, T, 1))).astype(f32)
    for f, rot in enumerate(exact):
        listeners["rotation"][f] = rot
        listeners["position"][f] = 0.0
        for t in range(T):
            fs["perceived_position"][f, t] = special[t % len(special)] * f32(1 + t // len(special))
    # fan len(exact): the listener at the origin, unrotated; targets 0..5 lie at exactly the three
    # max_*_distance settings and just beyond (sweep_targets)
    listeners["rotation"][len(exact)] = exact[0]
    listeners["position"][len(exact)] = 0.0
    return listeners, fs


def sweep_targets(rng, T, st):
    r = rng.uniform(0.2, 30, T)
    d = rng.standard_normal((T, 3))
    targets = (d / np.linalg.norm(d, axis=1, keepdims=True) * r[:, None]).astype(f32)
    for k, m in enumerate((st.max_pan_distance, st.max_rear_attenuation_distance, st.max_elevation_effect_distance)):
        targets[2 * k] = 0.0
        targets[2 * k, k] = m
        targets[2 * k + 1] = 0.0
        targets[2 * k + 1, k] = np.nextafter(f32(m), f32(100))
    return targets


def test_params_device_sweep():
    """2^18 sources: the device's double atan2 / sin / cos against the host libm's, through the whole
    parameter computation, byte for byte. No differences are expected: the two libraries would have
    to straddle a float rounding boundary within a few double ulps (about 1e-8 per evaluation)."""
    S, T = 4096, 64
    rng = np.random.default_rng(2026)
    st = SpatializerSettings(max_pan_distance=5.0, max_rear_attenuation_distance=15.0, max_elevation_effect_distance=12.0,
                             muffle_curve=rng.random(37).astype(f32), reverb_volume_curve=rng.random(50).astype(f32))
    scene, org, params = tiny_scene(T)
    scene.targets = sweep_targets(rng, T, st)
    with art.Context(1) as c:
        fr = art.Frame(scene, params, org, art.FanOutputs(1, R, 1, T, 1))
        c.bind(fr)
        lay = art.fan_layout(fr)
        art.dsp.bind_settings(c, st, 48000)
        listeners, fs = sweep_case(rng, S, T)
        dist = np.linalg.norm(scene.targets[None] - listeners["position"][:, None, :], axis=2)
        for m in (5.0, 15.0, 12.0):
            assert (dist < m).sum() > 1000 and (dist > m).sum() > 1000
        volume = rng.uniform(0, 2, S * T).astype(f32)
        want = art.dsp.tick_params_host(st, listeners, fs, scene.targets, volume, 48000)
        got, _ = device_params(c, synth_block(fs, lay), S, T, listeners, volume)
    w, g = want.view(np.uint32).reshape(-1, 8), got.view(np.uint32).reshape(-1, 8)
    diff = np.flatnonzero((w != g).any(axis=1))
    for s in diff[:16]:
        print("source", s, "listener", listeners[s // T], "settings", fs[s // T, s % T], "host", want[s], "device", got[s])
    print("sweep:", S * T, "sources,", diff.size, "differ; low pass", int((want["flags"] & 2 != 0).sum()),
          "muffled", int((want["flags"] & 1).sum()))
    assert (want["flags"] & 2 != 0).sum() > 1000 and (want["flags"] & 2 == 0).sum() > 1000
    assert diff.size == 0


@pytest.mark.parametrize("with_volume", [False, True])
@pytest.mark.parametrize("frames", [1, 37, 256])
def test_tick_end_to_end(ctx, frames, with_volume):
    """art_launch_device, then art_dsp_tick_device on the same stream with nothing between them,
    against the oracle's frame, the definition's local_dir / distance and the oracle's per-sample
    chain; a second tick continues from the carried state."""
    import torch
    S, T = 3, 4
    rng = np.random.default_rng(1000 + frames + with_volume)
    scene, org, params, lay = bind(ctx, T, S)
    st = random_settings(rng)
    art.dsp.bind_settings(ctx, st, 48000)
    listeners, _, _ = random_case(rng, S, T)
    listeners["position"] = org + rng.uniform(-0.5, 0.5, (S, 3)).astype(f32)
    volume = rng.uniform(0, 2, S * T).astype(f32) if with_volume else None
    n = S * T
    data = [(rng.standard_normal((n, frames * 2)) * 0.5).astype(f32) for _ in range(2)]
    state = np.zeros(n, abi.DSP_STATE)
    state.view(f32)[:] = rng.standard_normal(n * 8).astype(f32) * 0.1

    d_org = torch.from_numpy(np.ascontiguousarray(org)).to("cuda:0")
    d_block = dev(art.pack_block(art.FanOutputs(S, R, 1, T, 1), lay))
    d_ls, d_vol = dev(listeners), (dev(volume) if with_volume else None)
    d_state, d_params = dev(state), dev(np.zeros(n, abi.DSP_SOURCE_PARAMS))
    d_data = [dev(x) for x in data]
    torch.cuda.synchronize()
    ctx.launch_device(d_org.data_ptr(), S, d_block.data_ptr(), 0, stream())
    art.dsp.tick_device(ctx, d_block, S, d_ls, d_data[0], d_state, frames, d_params, d_vol, 0, stream())
    torch.cuda.synchronize()
    got = [d_data[0].cpu().numpy().view(f32).reshape(n, -1)]
    got_state = [d_state.cpu().numpy().view(abi.DSP_STATE).copy()]
    got_params = d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS).copy()
    art.dsp.tick_device(ctx, d_block, S, d_ls, d_data[1], d_state, frames, d_params, d_vol, 0, stream())
    torch.cuda.synchronize()
    got.append(d_data[1].cpu().numpy().view(f32).reshape(n, -1))
    got_state.append(d_state.cpu().numpy().view(abi.DSP_STATE).copy())

    o_ref, _ = oracle.run(scene, params, org, art.FanOutputs(S, R, 1, T, 1))
    want_params = definition_params(st, 48000, listeners, o_ref.settings, scene.targets, volume)
    assert got_params.tobytes() == want_params.tobytes()
    from test_tick_cpu import local_dir_and_distance
    srcs = []
    for s in range(n):
        f, t = divmod(s, T)
        rec = o_ref.settings[f, t]
        ld, dist = local_dir_and_distance(listeners[f]["position"], listeners[f]["rotation"], rec["perceived_position"],
                                          scene.targets[t])
        srcs.append(AudioSource(data=data[0][s].copy(), muffle_strength=rec["muffle_strength"], reverb_volume=rec["reverb_volume"],
                                local_dir=tuple(ld), listener_distance=dist,
                                volume_multiplier=volume[s] if with_volume else 1.0, state=state[s:s + 1].copy()))
    for tick in range(2):
        for s, src in enumerate(srcs):
            src.data = data[tick][s].copy()
        oracle.dsp_process(st, srcs, 48000)
        assert got[tick].tobytes() == np.stack([s.data for s in srcs]).tobytes(), f"tick {tick} data"
        assert got_state[tick].tobytes() == np.concatenate([s.state for s in srcs]).tobytes(), f"tick {tick} state"


def test_tick_follows_moved_target():
    """Resident targets: set, sync, launch, tick with no host synchronisation; the tick's distance is
    the moved position's. Then a tick on another stream, a sync right after it and a frame: the sync
    ordered itself after the tick (the frame equals a fresh bind)."""
    import torch
    from test_targets_gpu import S as RS, Rig, base_scene
    scene, org, params = base_scene(2, T=7)
    rig = Rig(scene, org, params)
    T, moved = 7, 3
    other = torch.cuda.Stream()  # (alive until the context has been closed)
    try:
        st = SpatializerSettings()  # every distance-based term on
        art.dsp.bind_settings(rig.ctx, st, 48000)
        rng = np.random.default_rng(5)
        listeners, _, _ = random_case(rng, RS, T)
        old = rig.model.array().copy()
        listeners["position"] = old[moved] + np.array([[0.3, 0.2, 0.1]], f32) * np.arange(1, RS + 1, dtype=f32)[:, None]
        new = (old[moved] + np.array([2.0, -1.5, 1.0], f32)).astype(f32)
        d_ls = dev(listeners)
        d_params = dev(np.zeros(RS * T, abi.DSP_SOURCE_PARAMS))
        blk0 = rig.block()
        torch.cuda.synchronize()
        rig.move([moved], new.reshape(1, 3))
        rig.ctx.launch_device(rig.d_org.data_ptr(), RS, blk0.data_ptr(), 0, stream())
        art.dsp.tick_params_device(rig.ctx, blk0, RS, d_ls, d_params, None, 0, stream())
        torch.cuda.synchronize()
        got = d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS).copy()
        fs = art.unpack_block(blk0.cpu().numpy(), rig.lay, RS, rig.scene.R, params.max_hits_per_ray, T, params.thread_count).settings
        now = rig.model.array()
        assert np.array_equal(now[moved], new)
        want_new = art.dsp.tick_params_host(st, listeners, fs, now, None, 48000)
        want_old = art.dsp.tick_params_host(st, listeners, fs, old, None, 48000)
        assert got.tobytes() == want_new.tobytes()
        differs = (want_new.view(np.uint32).reshape(RS, T, 8) != want_old.view(np.uint32).reshape(RS, T, 8)).any(axis=2)
        assert differs[:, moved].all() and not np.delete(differs, moved, axis=1).any()
        # a tick on another stream, then a sync and a frame on this one
        other.wait_stream(torch.cuda.current_stream())
        art.dsp.tick_params_device(rig.ctx, blk0, RS, d_ls, d_params, None, 0, other.cuda_stream)
        rig.move([1, moved], (now[[1, moved]] + f32(1.25)).astype(f32))
        rig.check(rig.launch(), what="frame after a tick on another stream and a sync")
    finally:
        rig.close()


def test_tick_errors_gpu():
    import torch
    st = SpatializerSettings()
    with art.Context(1) as c:
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        args = (c.ptr, d.data_ptr(), 0, 1, d.data_ptr(), None, d.data_ptr(), None)
        assert c.lib.art_dsp_tick_params_device(*args) == abi.ART_E_STATE  # no scene bound
        scene, org, params = tiny_scene(4)
        fr = art.Frame(scene, params, org, art.FanOutputs(1, R, 1, 4, 1))
        c.bind(fr)
        assert c.lib.art_dsp_tick_params_device(*args) == abi.ART_E_STATE  # no settings bound
        assert "settings" in c.lib.art_last_error(c.ptr).decode()
        bad = SpatializerSettings(muffle_curve=np.ones(1, f32)).to_c()
        import ctypes as C
        assert c.lib.art_dsp_settings_bind(c.ptr, C.byref(bad), 48000) == abi.ART_E_INVALID
        assert c.lib.art_dsp_settings_bind(c.ptr, C.byref(st.to_c()), 0) == abi.ART_E_INVALID
        art.dsp.bind_settings(c, st, 48000)
        assert c.lib.art_dsp_tick_params_device(c.ptr, None, 0, 0, None, None, None, None) == abi.ART_OK  # fan_count == 0
        assert c.lib.art_dsp_tick_device(c.ptr, None, 0, 0, None, None, None, None, 16, None, None) == abi.ART_OK
        assert c.lib.art_dsp_tick_params_device(c.ptr, None, 0, 1, d.data_ptr(), None, d.data_ptr(), None) == abi.ART_E_INVALID
        assert c.lib.art_dsp_tick_params_device(c.ptr, d.data_ptr(), 0, 1, None, None, d.data_ptr(), None) == abi.ART_E_INVALID
        assert c.lib.art_dsp_tick_params_device(c.ptr, d.data_ptr(), 0, 1, d.data_ptr(), None, None, None) == abi.ART_E_INVALID
        assert c.lib.art_dsp_tick_device(c.ptr, d.data_ptr(), 0, 1, d.data_ptr(), None, None, None, 16, d.data_ptr(),
                                         None) == abi.ART_E_INVALID
        params.stages = abi.ART_STAGE_RAYTRACE  # no reduce stage: the blocks have no settings
        c.bind(art.Frame(scene, params, org, art.FanOutputs(1, R, 1, 4, 1)))
        assert c.lib.art_dsp_tick_params_device(*args) == abi.ART_E_INVALID
        assert "ART_STAGE_REDUCE" in c.lib.art_last_error(c.ptr).decode()
        torch.cuda.synchronize()

"""The listener mix on the GPU (include/art_dsp.h: art_dsp_mix_device, art_dsp_tick_mix_device).

dsp_mix_kernel packs G = 32 / T whole fans into a wave (T <= 32) or runs one fan in rounds of 32
targets (T > 32). Its check is byte equality with the host twin (art_dsp_mix_host, which
tests/test_mix_cpu.py pins against the oracle's chain and an ordered float32 sum), with the unmixed
device path (art_dsp_process_device) plus the ordered sum, and end to end behind a frame with the
oracle.
"""
import numpy as np
import pytest

import art
from art import abi
from art.dsp import AudioSource, SpatializerSettings
import oracle
from test_dsp import random_settings
from test_mix_cpu import mix_sources, ordered_sum, source_arrays
from test_tick_cpu import definition_params, local_dir_and_distance, random_case
from test_tick_gpu import R, bind, dev, stream, tiny_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
CANARY = 64

# (F, T, frames): T = 1 (the sum starts from y[f,0]); T = 3, 5 (G = 10 and 6, idle source slots, a partial
# last wave, a tile edge); T = 4, 32 (G = 8; G = 1 with a full wave); T = 33 (a second round with one
# source); T = 70 (three rounds)
SHAPES = [(1, 1, 1), (7, 3, 64), (13, 5, 65), (9, 4, 37), (2, 32, 256), (2, 33, 130), (3, 70, 70)]


def with_canary(a):
    """A device copy of `a` followed by CANARY bytes of 0xC3."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([raw, np.full(CANARY, 0xC3, np.uint8)])).to(torch.device("cuda", 0))


def split_canary(d):
    h = d.cpu().numpy()
    assert (h[-CANARY:] == 0xC3).all(), "bytes after the buffer were written"
    return h[:-CANARY]


@pytest.mark.parametrize("single_class", [False, True])
@pytest.mark.parametrize("F,T,frames", SHAPES)
def test_mix_device_equals_host(ctx, F, T, frames, single_class):
    """Mix and state against the host twin over two calls (the state is carried), with mixed filter
    classes in a wave (the per-lane select loop) and with one class (the class loops); d_dry is only
    read; nothing is written past d_mix or d_state."""
    import torch
    rng = np.random.default_rng(100000 * F + 1000 * T + 2 * frames + single_class)
    st = random_settings(rng)
    srcs = mix_sources(rng, F, T, frames, single_class)
    params, states = source_arrays(st, srcs)
    classes = set(int(x) for x in params["flags"] & 3)
    assert classes == {3} if single_class else (len(classes) >= 3 or F * T < 16), classes
    d_params, d_state = dev(params), with_canary(states)
    d_mix = with_canary(np.full((F, frames * 2), np.nan, f32))
    for call in range(2):
        dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
        want = art.dsp.mix_host(params, states, dry, F, T)  # advances `states`
        d_dry = dev(dry)
        art.dsp.mix_device(ctx, d_dry, d_params, d_state, F, T, frames, d_mix, stream())
        torch.cuda.synchronize()
        assert d_dry.cpu().numpy().tobytes() == dry.tobytes(), f"call {call}: d_dry was written"
        got = split_canary(d_mix).view(f32).reshape(F, -1)
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert bad.size == 0, f"call {call}: the mix of fans {bad[:8]} differs"
        got_state = split_canary(d_state).view(abi.DSP_STATE)
        assert got_state.tobytes() == states.tobytes(), f"call {call} state"


def test_mix_device_equals_unmixed_path(ctx):
    """The new kernel against the oracle-checked one: art_dsp_process_device over the dry input
    replicated per fan, then the ordered sum of its wet buffers."""
    import torch
    F, T, frames = 5, 6, 100
    rng = np.random.default_rng(61)
    st = random_settings(rng)
    params, states = source_arrays(st, mix_sources(rng, F, T, frames))
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
    d_params, d_state_a, d_state_b = dev(params), dev(states), dev(states)
    d_data = dev(np.tile(dry, (F, 1)))
    d_mix = dev(np.zeros((F, frames * 2), f32))
    rc = ctx.lib.art_dsp_process_device(ctx.ptr, d_data.data_ptr(), d_params.data_ptr(), d_state_a.data_ptr(), F * T, frames,
                                        stream())
    assert rc == 0
    art.dsp.mix_device(ctx, dev(dry), d_params, d_state_b, F, T, frames, d_mix, stream())
    torch.cuda.synchronize()
    want = ordered_sum(d_data.cpu().numpy().view(f32).reshape(F * T, -1), F, T)
    assert d_mix.cpu().numpy().tobytes() == want.tobytes()
    assert d_state_b.cpu().numpy().tobytes() == d_state_a.cpu().numpy().tobytes()


@pytest.mark.parametrize("F,T,frames", [(3, 5, 70), (1, 34, 9)])
def test_mix_device_non_stereo_source(ctx, F, T, frames):
    """Sources whose params carry flag bit 2 (the first of a fan, one in the middle, the last one)
    contribute their dry frames unchanged and keep their state, as in the host twin."""
    import torch
    rng = np.random.default_rng(500 + T)
    st = random_settings(rng)
    srcs = mix_sources(rng, F, T, frames)
    mono = [0, T // 2, F * T - 1]
    for s in mono:
        srcs[s].channels = 1
    params, states = source_arrays(st, srcs)
    assert (params["flags"][mono] == 4).all()
    kept = states.copy()
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
    d_state, d_mix = dev(states), dev(np.zeros((F, frames * 2), f32))
    art.dsp.mix_device(ctx, dev(dry), dev(params), d_state, F, T, frames, d_mix, stream())
    torch.cuda.synchronize()
    want = art.dsp.mix_host(params, states, dry, F, T)
    assert d_mix.cpu().numpy().tobytes() == want.tobytes()
    got_state = d_state.cpu().numpy().view(abi.DSP_STATE)
    assert got_state.tobytes() == states.tobytes() and got_state[mono].tobytes() == kept[mono].tobytes()


def test_mix_device_nan_source(ctx):
    """One source with NaN gains (a listener on the perceived position): that fan's mix is NaN where
    the host twin's is; every other fan of the packed wave is byte-equal, so nothing leaks across fans."""
    import torch
    F, T, frames = 3, 5, 40
    rng = np.random.default_rng(77)
    st = random_settings(rng)
    listeners, fs, targets = random_case(rng, F, T)
    fs["perceived_position"][1, 2] = listeners["position"][1]
    params = art.dsp.tick_params_host(st, listeners, fs, targets, None, 44100)
    bad = 1 * T + 2
    assert np.isnan(params[bad]["gain_left"]) and not np.isnan(np.delete(params["gain_left"], bad)).any()
    states = np.zeros(F * T, abi.DSP_STATE)
    states.view(f32)[:] = rng.standard_normal(F * T * 8).astype(f32) * 0.1
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
    d_state, d_mix = dev(states), dev(np.zeros((F, frames * 2), f32))
    art.dsp.mix_device(ctx, dev(dry), dev(params), d_state, F, T, frames, d_mix, stream())
    torch.cuda.synchronize()
    want = art.dsp.mix_host(params, states, dry, F, T)
    got = d_mix.cpu().numpy().view(f32).reshape(F, -1)
    got_state = d_state.cpu().numpy().view(f32).reshape(F * T, 8)
    assert np.isnan(want[1]).any()
    assert np.array_equal(np.isnan(got[1]), np.isnan(want[1]))
    ok = ~np.isnan(want[1])
    assert got[1][ok].tobytes() == want[1][ok].tobytes()
    assert got[[0, 2]].tobytes() == want[[0, 2]].tobytes()
    ws = states.view(f32).reshape(F * T, 8)
    assert np.array_equal(np.isnan(got_state[bad]), np.isnan(ws[bad]))
    keep = np.arange(F * T) != bad
    assert got_state[keep].tobytes() == ws[keep].tobytes()


@pytest.mark.parametrize("with_volume", [False, True])
@pytest.mark.parametrize("frames", [37, 256])
def test_tick_mix_end_to_end(ctx, frames, with_volume):
    """art_launch_device, then art_dsp_tick_mix_device on the same stream with nothing between them,
    against the oracle's frame, the definition's parameters, the oracle's per-sample chain and the
    ordered sum; a second tick continues from the carried state."""
    import torch
    S, T = 3, 4
    rng = np.random.default_rng(2000 + frames + with_volume)
    scene, org, params, lay = bind(ctx, T, S)
    st = random_settings(rng)
    art.dsp.bind_settings(ctx, st, 48000)
    listeners, _, _ = random_case(rng, S, T)
    listeners["position"] = org + rng.uniform(-0.5, 0.5, (S, 3)).astype(f32)
    volume = rng.uniform(0, 2, S * T).astype(f32) if with_volume else None
    n = S * T
    dry = [(rng.standard_normal((T, frames * 2)) * 0.5).astype(f32) for _ in range(2)]
    state = np.zeros(n, abi.DSP_STATE)
    state.view(f32)[:] = rng.standard_normal(n * 8).astype(f32) * 0.1

    d_org = torch.from_numpy(np.ascontiguousarray(org)).to("cuda:0")
    d_block = dev(art.pack_block(art.FanOutputs(S, R, 1, T, 1), lay))
    d_ls, d_vol = dev(listeners), (dev(volume) if with_volume else None)
    d_state, d_params = dev(state), dev(np.zeros(n, abi.DSP_SOURCE_PARAMS))
    d_dry = [dev(x) for x in dry]
    d_mix = dev(np.zeros((S, frames * 2), f32))
    torch.cuda.synchronize()
    ctx.launch_device(d_org.data_ptr(), S, d_block.data_ptr(), 0, stream())
    art.dsp.tick_mix_device(ctx, d_block, S, d_ls, d_dry[0], d_state, frames, d_params, d_mix, d_vol, 0, stream())
    torch.cuda.synchronize()
    got = [d_mix.cpu().numpy().view(f32).reshape(S, -1).copy()]
    got_state = [d_state.cpu().numpy().view(abi.DSP_STATE).copy()]
    got_params = d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS).copy()
    art.dsp.tick_mix_device(ctx, d_block, S, d_ls, d_dry[1], d_state, frames, d_params, d_mix, d_vol, 0, stream())
    torch.cuda.synchronize()
    got.append(d_mix.cpu().numpy().view(f32).reshape(S, -1).copy())
    got_state.append(d_state.cpu().numpy().view(abi.DSP_STATE).copy())

    o_ref, _ = oracle.run(scene, params, org, art.FanOutputs(S, R, 1, T, 1))
    want_params = definition_params(st, 48000, listeners, o_ref.settings, scene.targets, volume)
    assert got_params.tobytes() == want_params.tobytes()
    srcs = []
    for s in range(n):
        f, t = divmod(s, T)
        rec = o_ref.settings[f, t]
        ld, dist = local_dir_and_distance(listeners[f]["position"], listeners[f]["rotation"], rec["perceived_position"],
                                          scene.targets[t])
        srcs.append(AudioSource(data=dry[0][t].copy(), muffle_strength=rec["muffle_strength"], reverb_volume=rec["reverb_volume"],
                                local_dir=tuple(ld), listener_distance=dist,
                                volume_multiplier=volume[s] if with_volume else 1.0, state=state[s:s + 1].copy()))
    for tick in range(2):
        for s, src in enumerate(srcs):
            src.data = dry[tick][s % T].copy()
        oracle.dsp_process(st, srcs, 48000)
        want = ordered_sum(np.stack([s.data for s in srcs]), S, T)
        assert got[tick].tobytes() == want.tobytes(), f"tick {tick} mix"
        assert got_state[tick].tobytes() == np.concatenate([s.state for s in srcs]).tobytes(), f"tick {tick} state"
        assert d_dry[tick].cpu().numpy().tobytes() == dry[tick].tobytes()


def test_mix_errors_gpu():
    import ctypes as C
    import torch
    st = SpatializerSettings()
    with art.Context(1) as c:
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
        p, lib = d.data_ptr(), c.lib
        assert p % 8 == 0
        # art_dsp_mix_device: no scene needed (dry, params, state and mix of 2 x 2 x 8 in d's four quarters)
        assert lib.art_dsp_mix_device(c.ptr, p, p + 1024, p + 2048, 2, 2, 8, p + 3072, None) == abi.ART_OK
        assert lib.art_dsp_mix_device(c.ptr, p + 4, p, p, 2, 2, 8, p, None) == abi.ART_E_INVALID  # unaligned d_dry
        assert "aligned" in lib.art_last_error(c.ptr).decode()
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, 2, 2, 8, p + 4, None) == abi.ART_E_INVALID  # unaligned d_mix
        for k in range(4):  # each buffer NULL
            a = [p, p, p, p]
            a[k] = None
            assert lib.art_dsp_mix_device(c.ptr, a[0], a[1], a[2], 2, 2, 8, a[3], None) == abi.ART_E_INVALID
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, -1, 2, 8, p, None) == abi.ART_E_INVALID
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, 2, 2, -8, p, None) == abi.ART_E_INVALID
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, 2, 0, 8, p, None) == abi.ART_E_INVALID  # work to do, no target
        assert lib.art_dsp_mix_device(c.ptr, None, None, None, 0, 2, 8, None, None) == abi.ART_OK
        assert lib.art_dsp_mix_device(c.ptr, None, None, None, 2, 2, 0, None, None) == abi.ART_OK
        # byte offsets are 32-bit: refused, never wrapped (no buffer is touched)
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, 1, 1 << 20, 1 << 8, p, None) == abi.ART_E_UNSUPPORTED
        assert lib.art_dsp_mix_device(c.ptr, p, p, p, 1 << 20, 1, 1 << 8, p, None) == abi.ART_E_UNSUPPORTED
        # art_dsp_tick_mix_device: the state cases of the tick
        tick = lambda dry=p, state=p, mix=p, block=p, ls=p, par=p, fans=1: lib.art_dsp_tick_mix_device(  # noqa: E731
            c.ptr, block, 0, fans, ls, None, dry, state, 16, par, mix, None)
        assert tick() == abi.ART_E_STATE  # no scene bound
        scene, org, params = tiny_scene(4)
        fr = art.Frame(scene, params, org, art.FanOutputs(1, R, 1, 4, 1))
        c.bind(fr)
        assert tick() == abi.ART_E_STATE  # no settings bound
        assert "settings" in lib.art_last_error(c.ptr).decode()
        art.dsp.bind_settings(c, st, 48000)
        assert tick(fans=0, block=None, ls=None, par=None, dry=None, state=None, mix=None) == abi.ART_OK
        for kw in ("block", "ls", "par", "dry", "state", "mix"):
            assert tick(**{kw: None}) == abi.ART_E_INVALID, kw
        assert tick(dry=p + 4) == abi.ART_E_INVALID and tick(mix=p + 4) == abi.ART_E_INVALID
        assert "aligned" in lib.art_last_error(c.ptr).decode()
        assert lib.art_dsp_tick_mix_device(c.ptr, p, 0, 1, p, None, p, p, -1, p, p, None) == abi.ART_E_INVALID
        assert lib.art_dsp_tick_mix_device(c.ptr, p, 0, 1, p, None, p, p, 1 << 28, p, p, None) == abi.ART_E_UNSUPPORTED
        params.stages = abi.ART_STAGE_RAYTRACE  # no reduce stage: the blocks have no settings
        c.bind(art.Frame(scene, params, org, art.FanOutputs(1, R, 1, 4, 1)))
        assert tick() == abi.ART_E_INVALID
        assert "ART_STAGE_REDUCE" in lib.art_last_error(c.ptr).decode()
        torch.cuda.synchronize()

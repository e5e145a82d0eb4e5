"""The listener mix on the host (include/art_dsp.h: art_dsp_mix_host, ABI 3.6): one dry buffer per
audio target in, one mix per fan out.

The contract: source s = f*T + t runs the per-sample chain over dry[t] from state[s], and
mix[f] = ((y[f,0] + y[f,1]) + ...) + y[f,T-1], one fp32 add per target in ascending t, starting
from y[f,0] itself. The reference here is the oracle's per-sample chain (oracle.dsp_process) per
source and an explicit loop of float32 adds; every comparison is byte equality.
"""
import numpy as np
import pytest

import art
from art import abi
import oracle
from test_dsp import random_settings, random_sources

f32 = np.float32
SHAPES = [(1, 1, 1), (3, 5, 37), (2, 33, 65)]


def mix_sources(rng, F, T, frames, single_class=False):
    """F*T stereo AudioSources (source s = f*T + t) with random per-buffer inputs and states: muffle on
    and off and both filter branches, or (single_class) all muffled with the low pass."""
    srcs = random_sources(rng, F * T, frames_choices=(frames,))
    for s in srcs:
        s.channels = 2
        if single_class:
            s.muffle_strength = float(rng.uniform(0.1, 1.0))
            s.local_dir = (s.local_dir[0], -abs(s.local_dir[1]), s.local_dir[2])
    return srcs


def source_arrays(st, srcs, sample_rate=48000):
    """(DSP_SOURCE_PARAMS [n], DSP_STATE [n]) of the sources, as the device-resident calls take them."""
    params = np.concatenate([art.dsp.source_params(st, s, sample_rate) for s in srcs])
    states = np.concatenate([s.state for s in srcs])
    return params, states


def ordered_sum(wet, F, T):
    """wet float32 [F*T, frames*2] -> [F, frames*2]: one float32 add per target, in target order,
    starting from the first target's buffer itself (np.sum would add pairwise)."""
    wet = wet.reshape(F, T, -1)
    mix = np.empty((F, wet.shape[2]), f32)
    for f in range(F):
        acc = wet[f, 0].copy()
        for t in range(1, T):
            acc = np.add(acc, wet[f, t], dtype=f32)
        mix[f] = acc
    return mix


def oracle_mix(st, srcs, dry, F, T, sample_rate=48000):
    """The oracle's chain per source on a copy of dry[t] (the sources' states advance), then the
    ordered sum; returns (mix [F, frames*2], states [F*T])."""
    for s, src in enumerate(srcs):
        src.data = dry[s % T].copy()
    oracle.dsp_process(st, srcs, sample_rate)
    return ordered_sum(np.stack([s.data for s in srcs]), F, T), np.concatenate([s.state for s in srcs])


@pytest.mark.parametrize("F,T,frames", SHAPES)
def test_mix_host_matches_oracle(F, T, frames):
    rng = np.random.default_rng(10000 * F + 100 * T + frames)
    st = random_settings(rng)
    srcs = mix_sources(rng, F, T, frames)
    params, states = source_arrays(st, srcs)
    if F * T > 4:  # muffle off and on, high and low pass
        assert {0, 1} <= set(params["flags"] & 1) and {0, 2} <= set(params["flags"] & 2)
    for call in range(2):  # the second call continues from the carried state
        dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
        before = dry.copy()
        got = art.dsp.mix_host(params, states, dry, F, T)
        want, want_states = oracle_mix(st, srcs, dry, F, T)
        assert dry.tobytes() == before.tobytes()
        assert got.tobytes() == want.tobytes(), f"call {call}"
        assert states.tobytes() == want_states.tobytes(), f"call {call} state"


def test_mix_host_single_target_keeps_negative_zero():
    """T = 1: the mix is the source's wet buffer itself. A silent buffer under a negative volume gives
    -0.0f samples; a sum started from 0 would turn them into +0.0f."""
    rng = np.random.default_rng(3)
    st = random_settings(rng)
    frames = 9
    srcs = mix_sources(rng, 2, 1, frames)
    for s in srcs:
        s.volume_multiplier = -1.0
        s.state[:] = np.zeros(1, abi.DSP_STATE)
    params, states = source_arrays(st, srcs)
    dry = np.zeros((1, frames * 2), f32)
    got = art.dsp.mix_host(params, states, dry, 2, 1)
    want, want_states = oracle_mix(st, srcs, dry, 2, 1)
    assert (want.view(np.uint32) == 0x80000000).all()
    assert got.tobytes() == want.tobytes() and states.tobytes() == want_states.tobytes()


def test_mix_host_non_stereo_source_passes_dry_through():
    """A source whose params carry flag bit 2 contributes its dry frames unchanged and keeps its
    state (AudioSpatializer.cs:72 leaves such a buffer as is)."""
    rng = np.random.default_rng(4)
    st = random_settings(rng)
    F, T, frames = 2, 3, 21
    srcs = mix_sources(rng, F, T, frames)
    for s in (0, 4):  # the first target of fan 0 (the sum starts from it), the middle one of fan 1
        srcs[s].channels = 1
    params, states = source_arrays(st, srcs)
    assert params["flags"][0] == 4 and params["flags"][4] == 4 and (np.delete(params["flags"], [0, 4]) & 4 == 0).all()
    kept = states.copy()
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
    got = art.dsp.mix_host(params, states, dry, F, T)
    want, want_states = oracle_mix(st, srcs, dry, F, T)
    assert got.tobytes() == want.tobytes()
    assert states.tobytes() == want_states.tobytes()
    assert states[[0, 4]].tobytes() == kept[[0, 4]].tobytes() and states[1].tobytes() != kept[1].tobytes()
    # all of a fan's sources non-stereo at T = 1: the mix is the dry buffer
    one = np.zeros(1, abi.DSP_SOURCE_PARAMS)
    one["flags"] = 4
    assert art.dsp.mix_host(one, np.zeros(1, abi.DSP_STATE), dry[:1], 1, 1).tobytes() == dry[:1].tobytes()


def test_mix_errors():
    lib = art.load_library()
    p, s = np.zeros(4, abi.DSP_SOURCE_PARAMS), np.zeros(4, abi.DSP_STATE)
    dry, mix = np.zeros((2, 16), f32), np.full((2, 16), 7, f32)
    a = (p.ctypes.data, s.ctypes.data, dry.ctypes.data)
    assert lib.art_dsp_mix_host(*a, 2, 2, 8, mix.ctypes.data) == abi.ART_OK
    assert lib.art_dsp_mix_host(*a, -1, 2, 8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(*a, 2, -1, 8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(*a, 2, 2, -8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(*a, 2, 0, 8, mix.ctypes.data) == abi.ART_E_INVALID  # work to do, no target
    assert lib.art_dsp_mix_host(None, s.ctypes.data, dry.ctypes.data, 2, 2, 8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(p.ctypes.data, None, dry.ctypes.data, 2, 2, 8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(p.ctypes.data, s.ctypes.data, None, 2, 2, 8, mix.ctypes.data) == abi.ART_E_INVALID
    assert lib.art_dsp_mix_host(*a, 2, 2, 8, None) == abi.ART_E_INVALID
    mix[:] = 7
    assert lib.art_dsp_mix_host(None, None, None, 0, 2, 8, None) == abi.ART_OK  # nothing to do
    assert lib.art_dsp_mix_host(*a, 2, 2, 0, mix.ctypes.data) == abi.ART_OK and (mix == 7).all()
    # the device calls: no context, and the CPU backend (device_mask 0) refuses them
    assert lib.art_dsp_mix_device(None, None, None, None, 1, 1, 1, None, None) == abi.ART_E_INVALID
    assert lib.art_dsp_tick_mix_device(None, None, 0, 1, None, None, None, None, 1, None, None, None) == abi.ART_E_INVALID
    with art.Context(0) as cpu:
        assert cpu.lib.art_dsp_mix_device(cpu.ptr, None, None, None, 0, 1, 16, None, None) == abi.ART_E_UNSUPPORTED
        assert "CPU backend" in cpu.lib.art_last_error(cpu.ptr).decode()
        assert cpu.lib.art_dsp_tick_mix_device(cpu.ptr, None, 0, 0, None, None, None, None, 16, None, None,
                                               None) == abi.ART_E_UNSUPPORTED
        with pytest.raises(art.ArtError) as e:
            art.dsp.mix_device(cpu, 0, 0, 0, 1, 1, 1, 0)
        assert e.value.code == abi.ART_E_UNSUPPORTED
    v = lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 6

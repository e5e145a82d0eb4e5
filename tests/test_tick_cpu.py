"""The audio tick's host side (include/art_dsp.h: art_listener, art_dsp_tick_params_host) and the
refusals of its context calls on the CPU backend.

The tick is AudioSpatializer.UpdateSpatializer / OnLateUpdate (AudioSpatializer.cs:55-67) in front
of the per-buffer scalars: local_dir = normalize(mul(inverse(listener.rotation), perceived -
listener.position)), distance = distance(target position, listener.position). Its definition here
is the oracle's quaternion functions, a numpy float32 normalize and art_dsp_source_params_get (which
test_dsp.py pins against the reference's formulas).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import art
from art import abi
from art.dsp import AudioSource, Listener, SpatializerSettings
import oracle
from test_dsp import random_settings

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dot3(v):
    return f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))


def local_dir_and_distance(listener_pos, listener_rot, perceived, target):
    """The definition: (local_dir float32[3], distance float32) of one source."""
    lib = oracle.load()
    lp = np.asarray(listener_pos, f32)
    world = (np.asarray(perceived, f32) - lp).astype(f32)
    q, qi, out = (C.c_float * 4)(*[float(x) for x in listener_rot]), (C.c_float * 4)(), (C.c_float * 3)()
    lib.or_quat_inverse(q, qi)
    lib.or_quat_mul_vec(qi, (C.c_float * 3)(*[float(x) for x in world]), out)
    v = np.array(list(out), f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        local = (f32(f32(1) / np.sqrt(_dot3(v), dtype=f32)) * v).astype(f32)
        d = (lp - np.asarray(target, f32)).astype(f32)
        dist = np.sqrt(_dot3(d), dtype=f32)
    return local, dist


def definition_params(st, sample_rate, listeners, fan_settings, targets, volume=None):
    """DSP_SOURCE_PARAMS [S * T] from the definition above and art_dsp_source_params_get."""
    S, T = fan_settings.shape
    out = np.zeros(S * T, abi.DSP_SOURCE_PARAMS)
    for f in range(S):
        for t in range(T):
            rec = fan_settings[f, t]
            ld, dist = local_dir_and_distance(listeners[f]["position"], listeners[f]["rotation"], rec["perceived_position"],
                                              targets[t])
            src = AudioSource(data=np.zeros(2, f32), muffle_strength=rec["muffle_strength"], reverb_volume=rec["reverb_volume"],
                              local_dir=tuple(ld), listener_distance=dist,
                              volume_multiplier=1.0 if volume is None else volume[f * T + t])
            out[f * T + t] = art.dsp.source_params(st, src, sample_rate)[0]
    return out


def random_case(rng, S, T):
    """Listeners with unit rotations, settings records and target positions within +-30, no
    perceived or target position on its listener."""
    listeners = np.zeros(S, abi.LISTENER)
    listeners["position"] = rng.uniform(-30, 30, (S, 3))
    q = rng.standard_normal((S, 4))
    listeners["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    fs = np.zeros((S, T), abi.SETTINGS)
    fs["muffle_strength"] = np.where(rng.random((S, T)) < 0.3, 0.0, rng.random((S, T)))
    fs["reverb_strength"] = rng.random((S, T))
    fs["reverb_volume"] = rng.random((S, T))
    fs["perceived_position"] = rng.uniform(-30, 30, (S, T, 3))
    targets = rng.uniform(-30, 30, (T, 3)).astype(f32)
    assert (np.abs(fs["perceived_position"] - listeners["position"][:, None, :]).max(axis=2) > 0).all()
    assert (np.abs(targets[None] - listeners["position"][:, None, :]).max(axis=2) > 0).all()
    return listeners, fs, targets


def test_listener_struct_size(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "art_dsp.h"\nint main(void) { printf("%zu\\n", sizeof(art_listener)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)], text=True)) == 28
    assert C.sizeof(abi.art_listener) == 28 and abi.LISTENER.itemsize == 28


def _one(st, listener, perceived, target, muffle=0.4, reverb=0.3):
    fs = np.zeros((1, 1), abi.SETTINGS)
    fs[0, 0] = (muffle, 0.5, reverb, perceived)
    return art.dsp.tick_params_host(st, [listener], fs, np.array([target], f32))[0]


def _direct(st, local_dir, dist, muffle=0.4, reverb=0.3):
    src = AudioSource(data=np.zeros(2, f32), muffle_strength=muffle, reverb_volume=reverb, local_dir=local_dir,
                      listener_distance=dist)
    return art.dsp.source_params(st, src)[0]


def test_tick_params_host_kats():
    st = SpatializerSettings()
    # listener at the origin, identity rotation, perceived (0, 0, 2): straight ahead
    target = (3.0, 4.0, 12.0)  # |target| = 13, exact
    p = _one(st, Listener(), (0.0, 0.0, 2.0), target)
    assert p.tobytes() == _direct(st, (0.0, 0.0, 1.0), 13.0).tobytes()
    # 180 degrees about y (exact in fp32): (1, 2, 3) is seen in the direction of (-1, 2, -3)
    v = np.array([-1.0, 2.0, -3.0], f32)
    n = (f32(f32(1) / np.sqrt(_dot3(v), dtype=f32)) * v).astype(f32)
    p = _one(st, Listener(rotation=(0.0, 1.0, 0.0, 0.0)), (1.0, 2.0, 3.0), (1.0, 2.0, 3.0))
    assert p.tobytes() == _direct(st, tuple(n), np.sqrt(f32(14), dtype=f32)).tobytes()
    assert not p["flags"] & 2  # above the listener: high pass
    # perceived y exactly the listener's y: the low-pass branch (ld[1] <= 0)
    p = _one(st, Listener(position=(1.0, 5.0, -2.0)), (4.0, 5.0, 2.0), (4.0, 5.0, 2.0))
    assert p["flags"] & 2
    assert p.tobytes() == _direct(st, (0.6, 0.0, 0.8), 5.0).tobytes()


def test_tick_params_host_matches_definition():
    rng = np.random.default_rng(21)
    cases = 0
    for S, T in ((1, 1), (7, 4), (9, 5), (25, 9), (1, 2)):  # 1 + 28 + 45 + 225 + 2 = 301 sources
        st = random_settings(rng)
        listeners, fs, targets = random_case(rng, S, T)
        for volume in (None, rng.uniform(0, 2, S * T).astype(f32)):
            got = art.dsp.tick_params_host(st, listeners, fs, targets, volume, 48000)
            want = definition_params(st, 48000, listeners, fs, targets, volume)
            assert got.tobytes() == want.tobytes(), (S, T, volume is None)
        cases += S * T
    assert cases >= 300


def test_tick_params_host_errors():
    lib = art.load_library()
    good = SpatializerSettings()
    listeners, fs, targets = random_case(np.random.default_rng(3), 2, 3)
    fans = (abi.art_fan * 2)()
    for i in range(2):
        fans[i].settings = fs[i].ctypes.data
    out = np.zeros(6, abi.DSP_SOURCE_PARAMS)

    def call(st, sr=48000, ls=listeners.ctypes.data, fa=fans, tp=targets.ctypes.data, o=out.ctypes.data, S=2):
        return lib.art_dsp_tick_params_host(C.byref(st), sr, ls, fa, S, tp, 3, None, o)

    assert call(good.to_c()) == abi.ART_OK
    for bad in (SpatializerSettings(muffle_curve=np.ones(1, f32)), SpatializerSettings(reverb_volume_curve=np.ones(1, f32))):
        assert call(bad.to_c()) == abi.ART_E_INVALID
    nul = good.to_c()
    nul.muffle_curve.baked = None
    assert call(nul) == abi.ART_E_INVALID
    assert call(good.to_c(), sr=0) == abi.ART_E_INVALID
    assert call(good.to_c(), sr=-48000) == abi.ART_E_INVALID
    assert call(good.to_c(), ls=None) == abi.ART_E_INVALID
    assert call(good.to_c(), fa=None) == abi.ART_E_INVALID
    assert call(good.to_c(), tp=None) == abi.ART_E_INVALID
    assert call(good.to_c(), o=None) == abi.ART_E_INVALID
    assert call(good.to_c(), ls=None, fa=None, tp=None, o=None, S=0) == abi.ART_OK


def test_tick_device_refused_on_cpu_backend():
    st = SpatializerSettings().to_c()
    with art.Context(0) as cpu:
        assert cpu.lib.art_dsp_settings_bind(cpu.ptr, C.byref(st), 48000) == abi.ART_E_UNSUPPORTED
        assert cpu.lib.art_dsp_tick_params_device(cpu.ptr, None, 0, 0, None, None, None, None) == abi.ART_E_UNSUPPORTED
        assert cpu.lib.art_dsp_tick_device(cpu.ptr, None, 0, 0, None, None, None, None, 0, None, None) == abi.ART_E_UNSUPPORTED

"""Spatializer settings per target, the host half (ABI 3.15): art_dsp_tick_params_classes_host against
art_dsp_tick_params_host stitched per class (which tests/test_tick_cpu.py pins against the definition),
its refusals, and the class map's state calls (art_dsp_target_classes_set / _get / _follow) on a
CPU-backend context, alone and over the resident target store's follow map. Every comparison is byte
equality with only a NaN's sign and payload free (dsp_chain_ref.assert_same_bits). These tests need
no GPU.
"""
import ctypes as C

import numpy as np
import pytest

import art
from art import abi, dsp
from art.dsp import SpatializerSettings
from art.targets import TargetStore
from dsp_chain_ref import assert_same_bits
from test_tick_cpu import random_case

f32 = np.float32
CURVE_SAMPLES = (2, 50, 7)
FLAGS = ((True, False), (False, True), (True, True), (False, False))


@pytest.fixture
def cpu():
    c = art.Context(0)
    yield c
    c.close()


def class_settings(rng, k):
    """Class k of a table: every field dsp_source_scalars reads is drawn anew, the distance flags and
    the curves' sample counts (2, 50, 7) and lengths cycle with k."""
    lo = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
    return SpatializerSettings(
        pan_strength=lo(0.05, 1), rear_attenuation_strength=lo(0.05, 1),
        distance_based_panning=FLAGS[k % 4][0], max_pan_distance=lo(1, 10),
        distance_based_rear_attenuation=FLAGS[k % 4][1], max_rear_attenuation_distance=lo(1, 30),
        max_elevation_effect_distance=lo(1, 20),
        low_pass_cutoff=(lo(2000, 6000), lo(12000, 22000)), low_pass_volume=lo(0.5, 1.0),
        high_pass_cutoff=(lo(10, 60), lo(100, 400)), high_pass_volume=lo(1.0, 1.5),
        muffle_curve=rng.random(CURVE_SAMPLES[k % 3]).astype(f32), muffle_curve_length=(0.7, 1.0, 1.6)[k % 3],
        muffle_cutoff=(lo(50, 200), lo(4000, 12000)),
        reverb_volume_curve=rng.random(CURVE_SAMPLES[(k + 1) % 3]).astype(f32),
        reverb_volume_curve_length=(1.3, 0.6, 1.0)[k % 3],
        reverb_dry_boost=(lo(0.5, 1.5), lo(2, 4)))


def make_classes(rng, K):
    return [class_settings(rng, k) for k in range(K)]


def stitched(classes, cls, listeners, fs, targets, volume, sample_rate=48000):
    """The contract: one art_dsp_tick_params_host run per class, each target takes its class's row."""
    S, T = fs.shape
    rows = [dsp.tick_params_host(st, listeners, fs, targets, volume, sample_rate).reshape(S, T) for st in classes]
    out = np.zeros((S, T), abi.DSP_SOURCE_PARAMS)
    for t in range(T):
        out[:, t] = rows[int(cls[t])][:, t]
    return out.reshape(-1)


def same_params(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.dtype == abi.DSP_SOURCE_PARAMS and g.size == w.size, what
    assert_same_bits(g.view(f32).reshape(-1, 8)[:, :6], w.view(f32).reshape(-1, 8)[:, :6], what)
    assert g["flags"].tobytes() == w["flags"].tobytes() and g["reserved"].tobytes() == w["reserved"].tobytes(), what


# ------------------------------------------------------------------------------- the host twin
def test_twin_is_the_existing_code_stitched():
    S, T, K = 3, 5, 3
    cls = np.array([2, 0, 1, 1, 0], np.uint8)
    rng = np.random.default_rng(315)
    classes = make_classes(rng, K)
    assert sorted(c.muffle_curve.size for c in classes) == [2, 7, 50]
    listeners, fs, targets = random_case(rng, S, T)
    for volume in (None, rng.uniform(0, 2, S * T).astype(f32)):
        want = stitched(classes, cls, listeners, fs, targets, volume)
        got = dsp.tick_params_classes_host(classes, listeners, fs, targets, cls, volume)
        same_params(got, want, f"volume {volume is not None}")
        # not vacuous: another class gives every source other parameters
        for k in range(K):
            one = dsp.tick_params_host(classes[k], listeners, fs, targets, volume).reshape(S, T)
            differs = (one.view(np.uint32).reshape(S, T, 8) != want.view(np.uint32).reshape(S, T, 8)).any(axis=2)
            assert differs[:, cls != k].all() and not differs[:, cls == k].any()


def test_trivial_cases_equal_the_single_settings_call():
    S, T = 4, 6
    rng = np.random.default_rng(316)
    classes = make_classes(rng, 3)
    listeners, fs, targets = random_case(rng, S, T)
    volume = rng.uniform(0, 2, S * T).astype(f32)
    want = dsp.tick_params_host(classes[0], listeners, fs, targets, volume)
    same_params(dsp.tick_params_classes_host(classes[:1], listeners, fs, targets, None, volume), want, "K = 1")
    same_params(dsp.tick_params_classes_host(classes[:1], listeners, fs, targets, np.zeros(T, np.uint8), volume), want,
                "K = 1, a map of zeros")
    same_params(dsp.tick_params_classes_host(classes, listeners, fs, targets, None, volume), want, "K = 3, NULL map")


def test_twin_errors_leave_out_untouched():
    lib = art.load_library()
    S, T = 2, 3
    rng = np.random.default_rng(317)
    classes = make_classes(rng, 3)
    listeners, fs, targets = random_case(rng, S, T)
    fans = (abi.art_fan * S)()
    for i in range(S):
        fans[i].settings = fs[i].ctypes.data
    out = np.full(S * T * 8, 0xabababab, np.uint32)
    cls = np.array([0, 2, 1], np.uint8)
    many = dsp.settings_table([classes[0]] * 257)

    def call(table, K, m=cls, sr=48000, o=out.ctypes.data):
        return lib.art_dsp_tick_params_classes_host(table, K, sr, listeners.ctypes.data, fans, S, targets.ctypes.data, T,
                                                    None if m is None else m.ctypes.data, None, o)

    good = dsp.settings_table(classes)
    assert call(good, 0) == abi.ART_E_INVALID
    assert call(many, 257) == abi.ART_E_INVALID
    assert call(good, -1) == abi.ART_E_INVALID
    for k in range(3):  # one class with an unbaked curve, used by the map or not
        for name in ("muffle_curve", "reverb_volume_curve"):
            bad = dsp.settings_table(classes)
            getattr(bad[k], name).baked = None
            assert call(bad, 3) == abi.ART_E_INVALID
            assert call(bad, 3, m=np.full(T, (k + 1) % 3, np.uint8)) == abi.ART_E_INVALID
            short = dsp.settings_table(classes)
            getattr(short[k], name).sample_count = 1
            assert call(short, 3) == abi.ART_E_INVALID
    assert call(good, 3, m=np.array([0, 3, 1], np.uint8)) == abi.ART_E_INVALID  # an entry equal to K
    assert call(good, 2) == abi.ART_E_INVALID                                    # the same, K = 2
    assert call(good, 3, m=np.array([0, 1, 255], np.uint8)) == abi.ART_E_INVALID
    assert call(good, 3, sr=0) == abi.ART_E_INVALID
    assert call(None, 3) == abi.ART_E_INVALID
    assert call(good, 3, o=None) == abi.ART_E_INVALID
    assert (out == 0xabababab).all()
    assert call(many, 256, m=None) == abi.ART_OK and call(good, 3) == abi.ART_OK
    assert not (out == 0xabababab).any()


# ------------------------------------------------------------------------------- the class map
def follow_model(old, target_src, new_class):
    """art_dsp_target_classes_follow: an empty map is all zeros."""
    return [new_class if s < 0 else (old[s] if len(old) else 0) for s in target_src]


def test_map_set_get_round_trip(cpu):
    assert dsp.get_target_classes(cpu).size == 0  # the initial state: every target is class 0
    m = np.array([2, 0, 1, 1, 0], np.uint8)
    dsp.set_target_classes(cpu, m)
    assert dsp.get_target_classes(cpu).tolist() == m.tolist()
    short = np.full(5, 9, np.uint8)
    assert cpu.lib.art_dsp_target_classes_get(cpu.ptr, short.ctypes.data, 2) == 5  # min(cap, count) entries, the count
    assert short.tolist() == [2, 0, 9, 9, 9]
    assert cpu.lib.art_dsp_target_classes_get(cpu.ptr, None, 0) == 5
    full = np.arange(256, dtype=np.uint8)
    dsp.set_target_classes(cpu, full)
    assert dsp.get_target_classes(cpu).tolist() == full.tolist()
    big = np.zeros(257, np.uint8)
    assert cpu.lib.art_dsp_target_classes_set(cpu.ptr, big.ctypes.data, 257) == abi.ART_E_INVALID
    assert cpu.lib.art_dsp_target_classes_set(cpu.ptr, big.ctypes.data, -1) == abi.ART_E_INVALID
    assert cpu.lib.art_dsp_target_classes_set(cpu.ptr, None, 3) == abi.ART_E_INVALID
    assert cpu.lib.art_dsp_target_classes_get(cpu.ptr, None, 4) == abi.ART_E_INVALID
    assert cpu.lib.art_dsp_target_classes_get(cpu.ptr, big.ctypes.data, -1) == abi.ART_E_INVALID
    assert dsp.get_target_classes(cpu).tolist() == full.tolist()  # a refused set changes nothing
    dsp.set_target_classes(cpu, [])
    assert dsp.get_target_classes(cpu).size == 0
    lib = cpu.lib
    assert lib.art_dsp_target_classes_set(None, m.ctypes.data, 5) == abi.ART_E_INVALID
    assert lib.art_dsp_target_classes_get(None, short.ctypes.data, 5) == abi.ART_E_INVALID
    assert lib.art_dsp_target_classes_follow(None, None, 0, 0, 0) == abi.ART_E_INVALID


def test_map_follow_with_an_explicit_target_src(cpu):
    old = [2, 0, 1, 1, 0]
    dsp.set_target_classes(cpu, old)
    src = [4, -1, 0, 3, 2, 1, -1]  # a permutation of the old targets with two new ones
    dsp.follow_target_classes(cpu, src, len(src), 5, new_class=7)
    want = follow_model(old, src, 7)
    assert want == [0, 7, 2, 1, 1, 0, 7]
    assert dsp.get_target_classes(cpu).tolist() == want
    # refused, the map left as it is: a wrong old length, entries outside [-1, T_old), counts
    for ts, Tn, To in (([0, 1], 2, 5), ([0, 7], 2, 7), ([0, -2], 2, 7), ([0], 1, 8)):
        with pytest.raises(art.ArtError) as e:
            dsp.follow_target_classes(cpu, ts, Tn, To)
        assert e.value.code == abi.ART_E_INVALID
        assert dsp.get_target_classes(cpu).tolist() == want
    one = np.zeros(1, np.int32)
    assert cpu.lib.art_dsp_target_classes_follow(cpu.ptr, one.ctypes.data, -1, 7, 0) == abi.ART_E_INVALID
    assert cpu.lib.art_dsp_target_classes_follow(cpu.ptr, np.zeros(257, np.int32).ctypes.data, 257, 7, 0) == abi.ART_E_UNSUPPORTED
    assert dsp.get_target_classes(cpu).tolist() == want
    # an empty map is all zeros, of any old length
    dsp.set_target_classes(cpu, [])
    dsp.follow_target_classes(cpu, [1, -1, 0], 3, 2, new_class=4)
    assert dsp.get_target_classes(cpu).tolist() == follow_model([], [1, -1, 0], 4) == [0, 4, 0]
    dsp.follow_target_classes(cpu, [], 0, 3)
    assert dsp.get_target_classes(cpu).size == 0


def test_map_follows_the_resident_target_store(cpu):
    store = TargetStore(cpu)
    store.add_many(np.arange(15, dtype=f32).reshape(5, 3))
    store.sync()
    store.follow_mark()
    old = [2, 0, 1, 1, 0]
    dsp.set_target_classes(cpu, old)
    store.remove_swapback(1)           # [0 4 2 3]
    store.add(f32([9, 9, 9]))          # [0 4 2 3 n]
    store.sync()
    store.remove_swapback(0)           # [n 4 2 3]
    store.sync()
    src, base = store.follow_map()
    assert src.tolist() == [-1, 4, 2, 3] and base == 5
    for Tn, To in ((5, 5), (4, 4), (3, 5)):  # the caller's counts must be the store's
        with pytest.raises(art.ArtError) as e:
            dsp.follow_target_classes(cpu, None, Tn, To, 1)
        assert e.value.code == abi.ART_E_INVALID and "store" in str(e.value)
    assert dsp.get_target_classes(cpu).tolist() == old
    dsp.follow_target_classes(cpu, None, 4, 5, new_class=1)
    want = follow_model(old, src.tolist(), 1)
    assert want == [1, 0, 1, 1]
    assert dsp.get_target_classes(cpu).tolist() == want
    store.follow_mark()
    # a second round: the map's length is the new base count
    store.add(f32([1, 2, 3]))
    store.remove_swapback(2)           # [n 4 m 3]
    store.sync()
    src, base = store.follow_map()
    assert src.tolist() == [0, 1, -1, 3] and base == 4
    dsp.follow_target_classes(cpu, None, 4, 4, new_class=2)
    assert dsp.get_target_classes(cpu).tolist() == follow_model(want, src.tolist(), 2) == [1, 0, 2, 1]
    # a map whose length is not the base count is refused
    dsp.set_target_classes(cpu, [0, 1, 2])
    with pytest.raises(art.ArtError) as e:
        dsp.follow_target_classes(cpu, None, 4, 4, 0)
    assert e.value.code == abi.ART_E_INVALID
    assert dsp.get_target_classes(cpu).tolist() == [0, 1, 2]


def test_version_and_cpu_backend_refusals(cpu):
    v = cpu.lib.art_version()
    assert v >> 16 == 3 and (v & 0xffff) >= 15
    table = dsp.settings_table(make_classes(np.random.default_rng(1), 2))
    assert cpu.lib.art_dsp_settings_bind_classes(cpu.ptr, table, 2, 48000) == abi.ART_E_UNSUPPORTED
    assert "CPU backend" in cpu.lib.art_last_error(cpu.ptr).decode()
    assert cpu.lib.art_dsp_settings_bind_classes(None, table, 2, 48000) == abi.ART_E_INVALID
    with pytest.raises(art.ArtError) as e:
        dsp.bind_settings_classes(cpu, make_classes(np.random.default_rng(1), 2))
    assert e.value.code == abi.ART_E_UNSUPPORTED

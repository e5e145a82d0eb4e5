"""Spatializer settings per target on the GPU (ABI 3.15: art_dsp_settings_bind_classes, the class map,
the tick entry points under classes).

dsp_tick_params_classes_kernel evaluates source f * T + t with the settings class its target names.
Its check is always equality with the host twin (art_dsp_tick_params_classes_host, which
tests/test_tick_classes_cpu.py pins against art_dsp_tick_params_host stitched per class): byte
equality with only a NaN's sign and payload free. Blocks are synthesised as in tests/test_tick_gpu.py.
Every test has a context of its own: the class map is host state of the context.
"""
import dataclasses

import numpy as np
import pytest

import art
from art import abi, dsp
from art.targets import TargetStore, resident_targets_frame
from dsp_chain_ref import assert_same_bits
from test_follow_cpu import random_states
from test_tick_classes_cpu import follow_model, make_classes, same_params
from test_tick_cpu import random_case
from test_tick_gpu import R, bind, dev, device_params, stream, sweep_case, synth_block, tiny_scene

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture
def c():
    with art.Context(1) as own:
        yield own


def classes_with_a_pan_pair(rng, K):
    """K classes that differ in every field, except classes 0 and 1, which differ in pan_strength only:
    a kernel that reads the other record of the pair fails on exactly that target's gains."""
    classes = make_classes(rng, K)
    if K > 1:
        classes[1] = dataclasses.replace(classes[0], pan_strength=classes[0].pan_strength * 0.5 + 0.01)
    return classes


def covering_map(rng, T, K):
    """uint8 [T]: a random map that names every class it can (a permutation when T == K)."""
    m = np.concatenate([rng.permutation(K)[:T], rng.integers(0, K, max(0, T - K))]).astype(np.uint8)
    return m[rng.permutation(T)]


# (S, T, K, out_flags)
SHAPES = [(1, 1, 1, 0), (3, 5, 3, 0), (13, 5, 2, abi.ART_OUT_HIT_RESULTS), (130, 3, 3, 0), (2, 70, 70, 0)]


@pytest.mark.parametrize("S,T,K,out_flags", SHAPES, ids=["%dx%d K=%d" % s[:3] for s in SHAPES])
def test_device_equals_twin(c, S, T, K, out_flags):
    rng = np.random.default_rng(10000 * S + 100 * T + K)
    scene, _, _, lay = bind(c, T, out_flags=out_flags)
    classes = classes_with_a_pan_pair(rng, K)
    cls = np.array([2, 0, 1, 1, 0], np.uint8) if (T, K) == (5, 3) else covering_map(rng, T, K)
    assert set(cls.tolist()) == set(range(min(T, K)))
    dsp.bind_settings_classes(c, classes, 48000)
    dsp.set_target_classes(c, cls)
    listeners, fs, _ = random_case(rng, S, T)
    block = synth_block(fs, lay)
    for volume in (None, rng.uniform(0, 2, S * T).astype(f32)):
        want = dsp.tick_params_classes_host(classes, listeners, fs, scene.targets, cls, volume, 48000)
        got, after = device_params(c, block, S, T, listeners, volume, out_flags)
        same_params(got, want, f"S {S} T {T} K {K} volume {volume is not None}")
        assert after.tobytes() == block.tobytes()  # the block is only read
    if K > 1:  # the pair's targets tell the two records apart, in the gains alone
        t0, t1 = int(np.flatnonzero(cls == 0)[0]), int(np.flatnonzero(cls == 1)[0])
        swapped = cls.copy()
        swapped[t0], swapped[t1] = 1, 0
        other = dsp.tick_params_classes_host(classes, listeners, fs, scene.targets, swapped, volume, 48000)
        w, o = want.reshape(S, T), other.reshape(S, T)
        for t in (t0, t1):
            assert (w["gain_left"][:, t] != o["gain_left"][:, t]).any()
            for k in ("muffle_alpha", "dry_boost", "filter_alpha", "volume", "flags"):
                assert w[k][:, t].tobytes() == o[k][:, t].tobytes()
        keep = np.delete(np.arange(T), [t0, t1])
        assert w[:, keep].tobytes() == o[:, keep].tobytes()


SPECIAL = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),  # the axes, directly behind
                    (1, 0.0, 1), (1, -0.0, 1), (-1, 0.0, -1), (0, 0.0, -3), (0, -0.0, -3), (2, 0.0, 0),
                    (1e-30, 0, -1), (-1e-30, 0, -1), (1, 1, 1), (-1, -1, -1)], f32)
EXACT = [(0, 0, 0, 1), (0, 1, 0, 0), (1, 0, 0, 0), (0, 0, 1, 0)]  # identity, 180 degrees about y, x, z


def test_sweep(c):
    """2^14 sources of 8 random classes: the placements of test_params_device_sweep's generator, every
    special direction (the axes, directly behind, y = +-0) under the exact rotations for every target,
    and targets at their own class's max distances seen from the listener at the origin."""
    S, T, K = 4096, 4, 8
    rng = np.random.default_rng(2027)
    classes = make_classes(rng, K)
    cls = covering_map(rng, T, K)
    scene, org, params = tiny_scene(T)
    r = rng.uniform(0.2, 30, T)
    d = rng.standard_normal((T, 3))
    targets = (d / np.linalg.norm(d, axis=1, keepdims=True) * r[:, None]).astype(f32)
    own = [classes[int(k)] for k in cls]
    targets[0] = (own[0].max_pan_distance, 0, 0)
    targets[1] = (0, np.nextafter(f32(own[1].max_rear_attenuation_distance), f32(100)), 0)
    targets[2] = (0, 0, own[2].max_elevation_effect_distance)
    scene.targets = np.ascontiguousarray(targets)
    fr = art.Frame(scene, params, org, art.FanOutputs(1, R, 1, T, 1))
    c.bind(fr)
    lay = art.fan_layout(fr)
    dsp.bind_settings_classes(c, classes, 48000)
    dsp.set_target_classes(c, cls)
    listeners, fs = sweep_case(rng, S, T)  # fans 0..3: four special directions; fan 4: at the origin, unrotated
    seen = set()
    for j in range(64):  # fans 5..68: every special direction at every target (and so class), under every exact rotation
        f = 5 + j
        listeners["rotation"][f] = EXACT[j % 4]
        listeners["position"][f] = 0.0
        for t in range(T):
            k = (j // 4 + 4 * t) % 16
            fs["perceived_position"][f, t] = SPECIAL[k]
            seen.add((t, k, j % 4))
    assert len(seen) == T * 16 * 4
    volume = rng.uniform(0, 2, S * T).astype(f32)
    want = dsp.tick_params_classes_host(classes, listeners, fs, scene.targets, cls, volume, 48000)
    got, _ = device_params(c, synth_block(fs, lay), S, T, listeners, volume)
    w, g = want.view(np.uint32).reshape(-1, 8), got.view(np.uint32).reshape(-1, 8)
    diff = np.flatnonzero((w != g).any(axis=1))
    for s in diff[:16]:
        print("source", s, "class", cls[s % T], "listener", listeners[s // T], "settings", fs[s // T, s % T], "host", want[s],
              "device", got[s])
    print("classes sweep:", S * T, "sources,", diff.size, "differ; low pass", int((want["flags"] & 2 != 0).sum()), "muffled",
          int((want["flags"] & 1).sum()))
    assert (want["flags"] & 2 != 0).sum() > 1000 and (want["flags"] & 2 == 0).sum() > 1000
    same_params(got, want, "sweep")


def test_nothing_changed_for_existing_callers(c):
    """One class and no map is the single bind; a map of zeros goes through the table and gives the
    same bytes."""
    S, T = 13, 5
    rng = np.random.default_rng(41)
    scene, _, _, lay = bind(c, T)
    st = make_classes(rng, 1)[0]
    listeners, fs, _ = random_case(rng, S, T)
    block = synth_block(fs, lay)
    volume = rng.uniform(0, 2, S * T).astype(f32)
    want = dsp.tick_params_host(st, listeners, fs, scene.targets, volume, 48000)
    dsp.bind_settings(c, st, 48000)
    single, _ = device_params(c, block, S, T, listeners, volume)
    same_params(single, want, "art_dsp_settings_bind")
    dsp.bind_settings_classes(c, [st], 48000)
    assert dsp.get_target_classes(c).size == 0
    one, _ = device_params(c, block, S, T, listeners, volume)
    assert one.tobytes() == single.tobytes()
    dsp.set_target_classes(c, np.zeros(T, np.uint8))
    zeros, _ = device_params(c, block, S, T, listeners, volume)
    assert zeros.tobytes() == single.tobytes()
    dsp.bind_settings(c, st, 48000)  # a bind does not touch the map
    assert dsp.get_target_classes(c).tolist() == [0] * T
    again, _ = device_params(c, block, S, T, listeners, volume)
    assert again.tobytes() == single.tobytes()


def test_tick_mix_end_to_end(c):
    """art_dsp_tick_mix_device under three classes, two ticks (the state is carried): parameters,
    states and mixes are the classes host twin's followed by art_dsp_mix_host's."""
    import torch
    S, T, K, frames = 3, 5, 3, 65
    rng = np.random.default_rng(43)
    scene, _, _, lay = bind(c, T)
    classes = classes_with_a_pan_pair(rng, K)
    cls = np.array([2, 0, 1, 1, 0], np.uint8)
    dsp.bind_settings_classes(c, classes, 48000)
    dsp.set_target_classes(c, cls)
    listeners, fs, _ = random_case(rng, S, T)
    volume = rng.uniform(0.25, 2, S * T).astype(f32)
    state = np.zeros(S * T, abi.DSP_STATE)
    state.view(f32)[:] = rng.standard_normal(S * T * 8).astype(f32) * 0.1
    want_params = dsp.tick_params_classes_host(classes, listeners, fs, scene.targets, cls, volume, 48000)
    unclassed = dsp.tick_params_host(classes[0], listeners, fs, scene.targets, volume, 48000)
    d_block, d_ls, d_vol = dev(synth_block(fs, lay)), dev(listeners), dev(volume)
    d_state, d_params = dev(state), dev(np.zeros(S * T, abi.DSP_SOURCE_PARAMS))
    d_mix = dev(np.zeros((S, frames * 2), f32))
    want_state = state.copy()
    for tick in range(2):
        dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(f32)
        d_dry = dev(dry)
        dsp.tick_mix_device(c, d_block, S, d_ls, d_dry, d_state, frames, d_params, d_mix, d_vol, 0, stream())
        torch.cuda.synchronize()
        want_mix = dsp.mix_host(want_params, want_state, dry, S, T)
        same_params(d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS), want_params, f"tick {tick} params")
        assert_same_bits(d_mix.cpu().numpy().view(f32).reshape(S, -1), want_mix, f"tick {tick} mix")
        assert_same_bits(d_state.cpu().numpy().view(abi.DSP_STATE), want_state, f"tick {tick} state")
        if tick == 0:  # the classes are audible: class 0 for every target gives another mix
            assert dsp.mix_host(unclassed, state.copy(), dry, S, T).tobytes() != want_mix.tobytes()


def test_churn(c):
    """A resident target store with room for 8, T = 5, K = 3: a swap-back remove and an add, each
    followed by sync -> (the tick refuses: the map's length is not T) -> art_dsp_target_classes_follow
    -> art_dsp_sources_follow_device -> art_target_follow_mark -> the tick equals the twin with the
    Python model's class list."""
    import torch
    S, T, K = 3, 5, 3
    rng = np.random.default_rng(47)
    scene, org, params = tiny_scene(T)
    classes = classes_with_a_pan_pair(rng, K)
    model = [0, 1, 2, 1, 2]
    positions = [p.copy() for p in scene.targets]
    store = TargetStore(c)
    store.reserve(8)
    store.add_many(scene.targets)
    store.sync()
    store.follow_mark()
    c.set_flags(abi.ART_CTX_RESIDENT_TARGETS)

    def frame_of(tgts):
        sc = art.Scene(dirs=scene.dirs, targets=np.ascontiguousarray(tgts, f32), spheres=scene.spheres, aabbs=scene.aabbs)
        return art.Frame(sc, params, org, art.FanOutputs(1, R, 1, len(tgts), 1))

    c.bind(resident_targets_frame(frame_of(positions)))
    dsp.bind_settings_classes(c, classes, 48000)
    dsp.set_target_classes(c, model)
    state = {"d": dev(random_states(rng, S * T)), "T": T}

    def tick(expect_refusal=False):
        Tn = len(positions)
        lay = art.fan_layout(frame_of(positions))
        listeners, fs, _ = random_case(rng, S, Tn)
        block = synth_block(fs, lay)
        if expect_refusal:
            with pytest.raises(art.ArtError) as e:
                device_params(c, block, S, Tn, listeners, None)
            assert e.value.code == abi.ART_E_STATE and "class map" in str(e.value)
            return
        want = dsp.tick_params_classes_host(classes, listeners, fs, np.array(positions, f32), model, None, 48000)
        got, _ = device_params(c, block, S, Tn, listeners, None)
        same_params(got, want, f"T {Tn}, classes {model}")

    def follow(new_class):
        """The recipe after a sync that changed the targets; the model moves by the store's map."""
        nonlocal model
        Tn, To = len(positions), state["T"]
        src, base = store.follow_map()
        assert base == To == len(model)
        tick(expect_refusal=Tn != To)
        dsp.follow_target_classes(c, None, Tn, To, new_class)
        d_new = dev(np.full(S * Tn * 32, 0x5A, np.uint8))
        dsp.sources_follow_device(c, None, Tn, To, S, S, state["d"], d_new, stream=stream())
        store.follow_mark()
        torch.cuda.synchronize()
        old = state["d"].cpu().numpy().view(abi.DSP_STATE)
        want_state, _ = dsp.sources_follow_host(src, To, S, S, old, want_volume=False)
        assert d_new.cpu().numpy().tobytes() == want_state.tobytes()
        state["d"], state["T"] = d_new, Tn
        model = follow_model(model, src.tolist(), new_class)
        assert dsp.get_target_classes(c).tolist() == model

    tick()
    store.remove_swapback(1)  # 4 -> 1
    positions[1] = positions[-1]
    positions.pop()
    store.sync()
    assert store.last_resize()["kept_bound"] == 1 and store.follow_map()[0].tolist() == [0, 4, 2, 3]
    follow(0)
    assert model == [0, 2, 2, 1]
    tick()
    p_new = (scene.targets[0] + f32([0.75, -0.5, 1.25])).astype(f32)
    assert store.add(p_new) == 4
    positions.append(p_new)
    store.sync()
    assert store.last_resize()["kept_bound"] == 1 and store.follow_map()[0].tolist() == [0, 1, 2, 3, -1]
    follow(2)
    assert model == [0, 2, 2, 1, 2]
    tick()
    c.set_flags(0)


def test_errors_gpu(c):
    import torch
    S, T = 2, 4
    rng = np.random.default_rng(53)
    scene, _, _, lay = bind(c, T)
    classes = make_classes(rng, 2)
    listeners, fs, _ = random_case(rng, S, T)
    d_block, d_ls = dev(synth_block(fs, lay)), dev(listeners)
    d_params = torch.full((S * T * 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_buf = torch.zeros(S * T * 64 * 8, dtype=torch.uint8, device="cuda:0")  # data / dry / mix of 8 frames
    d_state = torch.zeros(S * T * 32, dtype=torch.uint8, device="cuda:0")
    dsp.bind_settings_classes(c, classes, 48000)
    lib, sp = c.lib, stream()
    args = (c.ptr, d_block.data_ptr(), 0, S, d_ls.data_ptr(), None)

    def all_ticks():
        return (lib.art_dsp_tick_params_device(*args, d_params.data_ptr(), sp),
                lib.art_dsp_tick_device(*args, d_buf.data_ptr(), d_state.data_ptr(), 8, d_params.data_ptr(), sp),
                lib.art_dsp_tick_mix_device(*args, d_buf.data_ptr(), d_state.data_ptr(), 8, d_params.data_ptr(),
                                            d_buf.data_ptr() + S * T * 64 * 4, sp))

    dsp.set_target_classes(c, [0, 1, 2, 0])  # an entry equal to the bound K
    assert all_ticks() == (abi.ART_E_STATE,) * 3
    assert "class" in lib.art_last_error(c.ptr).decode()
    dsp.set_target_classes(c, [0, 1, 0])  # a length that is not T
    assert all_ticks() == (abi.ART_E_STATE,) * 3
    dsp.set_target_classes(c, [0, 1, 1, 0, 0])
    assert all_ticks() == (abi.ART_E_STATE,) * 3
    torch.cuda.synchronize()
    assert (d_params.cpu().numpy() == 0x5A).all() and not d_state.cpu().numpy().any()  # nothing was enqueued
    dsp.set_target_classes(c, [0, 1, 1, 0])
    dsp.bind_settings(c, classes[0], 48000)  # one class bound: entry 1 names none
    assert all_ticks() == (abi.ART_E_STATE,) * 3
    dsp.bind_settings_classes(c, classes, 48000)
    assert lib.art_dsp_tick_params_device(*args, d_params.data_ptr(), sp) == abi.ART_OK
    torch.cuda.synchronize()
    want = dsp.tick_params_classes_host(classes, listeners, fs, scene.targets, [0, 1, 1, 0], None, 48000)
    same_params(d_params.cpu().numpy().view(abi.DSP_SOURCE_PARAMS), want, "after the refusals")
    # the bind's own refusals
    many = dsp.settings_table([classes[0]] * 257)
    assert lib.art_dsp_settings_bind_classes(c.ptr, many, 257, 48000) == abi.ART_E_INVALID
    assert lib.art_dsp_settings_bind_classes(c.ptr, many, 0, 48000) == abi.ART_E_INVALID
    assert lib.art_dsp_settings_bind_classes(c.ptr, many, 2, 0) == abi.ART_E_INVALID
    assert lib.art_dsp_settings_bind_classes(c.ptr, None, 2, 48000) == abi.ART_E_INVALID
    bad = dsp.settings_table(classes)
    bad[1].reverb_volume_curve.baked = None
    assert lib.art_dsp_settings_bind_classes(c.ptr, bad, 2, 48000) == abi.ART_E_INVALID
    assert lib.art_dsp_settings_bind_classes(c.ptr, many, 256, 48000) == abi.ART_OK
    with art.Context(0) as cpu:
        assert cpu.lib.art_dsp_settings_bind_classes(cpu.ptr, many, 2, 48000) == abi.ART_E_UNSUPPORTED
    torch.cuda.synchronize()

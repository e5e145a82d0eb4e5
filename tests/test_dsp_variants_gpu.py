"""The three per-sample kernels of csrc/art_dsp.hip on every variant and value class, against the NumPy float32
reference of the chain (tests/dsp_chain_ref.py, which tests/test_dsp_chain_ref_cpu.py pins to the oracle), bit for bit.

  dsp_tiled_kernel (art_dsp_process_device)   the class loops run_tile<0..3> alone and two in one wave, the per-lane
                                              select loop run_tile<4>, full (64-frame, unrolled) and partial tiles,
                                              sources that are not stereo, a wave of only such sources
  dsp_mix_kernel   (art_dsp_mix_device)       the same class matrix with packed fans, idle slots and a second round
  dsp_kernel       (the lane kernel)          its scalar path in process through a 4-byte aligned d_data, its float4
                                              path in a child process started with ART_DSP_KERNEL=lane

Every case runs two calls (the state is carried), asserts the kernel that ran (art_debug_last_dsp_kernel), and keeps a
canary behind every buffer a kernel writes: 1024 B behind d_data (dsp_tiled_kernel issues out-of-range buffer stores
up to 16 * 31 + 8 B past its end and relies on the range check to drop them), 64 B behind states and mixes.
The value classes (subnormal tails, non-finite samples and states, overflow inside the chain, signed zeros, parameters
at their edges) are those of dsp_chain_ref.make_inputs.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import art
from art import abi
from art.dsp import SpatializerSettings
import dsp_chain_ref as ref
import dsp_lane_child as child

pytestmark = pytest.mark.gpu

f32 = np.float32
VALUE_KINDS = [k for k in ref.KINDS if k != "gaussian"]
FRAMES = [1, 64, 65, 130]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_chain_device(ctx, params, states, samples_of_call, frames, kernel, before=0, what=""):
    """art_dsp_process_device over two (or more) calls against ref.chain: data, state, canaries, the kernel that ran."""
    import torch
    n = params.size
    d_params = ref.Guarded(params, 0)
    d_state = ref.Guarded(states, 64)
    for call, samples in enumerate(samples_of_call):
        want, want_states = ref.chain(params, states, samples)
        d_data = ref.Guarded(samples, 1024, before)
        assert d_data.ptr % 8 == (4 if before else 0)
        art.dsp.process_device(ctx, d_data.ptr, d_params.ptr, d_state.ptr, n, frames, stream())
        assert art.dsp.debug_last_dsp_kernel(ctx) == kernel
        torch.cuda.synchronize()
        tag = f"{what} call {call}"
        got = d_data.read(tag + " d_data").view(f32).reshape(n, -1)
        got_states = d_state.read(tag + " d_state").view(abi.DSP_STATE)
        ref.assert_same_bits(got, want, tag + " data")
        ref.assert_same_bits(got_states, want_states, tag + " state")
        mono = np.flatnonzero(params["flags"] & 4)
        if mono.size:  # not stereo: data and state bytes as they were
            assert got[mono].tobytes() == samples[mono].tobytes(), tag
            assert got_states[mono].tobytes() == states[mono].tobytes(), tag
        states = want_states


def inputs_of_calls(kind, seed, params0, frames, calls=2, **kw):
    """(params, initial states, [samples per call]): the class's crafted parameters and states from the first draw."""
    draws = [ref.make_inputs(kind, seed + c, params0, frames, **kw) for c in range(calls)]
    return draws[0][2], draws[0][1], [d[0] for d in draws]


# ---------------------------------------------------------------------------- dsp_tiled_kernel
# one wave of 32 sources unless noted; name -> the filter class of each source in order (4: not stereo)
LAYOUTS = {
    **{f"a{c}": [c] * 32 for c in range(4)},                      # one class loop
    "b03": [0, 3] * 16, "b12": [1, 2] * 16,                       # two class loops in one wave
    "c": [0, 1, 2, 3] * 8,                                        # the per-lane select loop
    # wave 0 with sources that are not stereo at slots 0, 15 and 31; wave 1 holds only such sources (fmax == 0)
    "d": [4 if s in (0, 15, 31) else s % 4 for s in range(32)] + [4] * 32,
}


def layout_params(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    return ref.class_params(rng, LAYOUTS[name])


@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_tiled_kernel_layouts(ctx, layout, frames):
    params0 = layout_params(layout)
    params, states, samples = inputs_of_calls("gaussian", 500 + frames, params0, frames)
    run_chain_device(ctx, params, states, samples, frames, abi.ART_DSP_KERNEL_TILED, what=f"{layout} x {frames}")


@pytest.mark.parametrize("layout", ["a0", "a1", "a2", "a3", "c"])
@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_tiled_kernel_value_classes(ctx, kind, layout):
    frames = 130
    params, states, samples = inputs_of_calls(kind, 800, layout_params(layout), frames)
    run_chain_device(ctx, params, states, samples, frames, abi.ART_DSP_KERNEL_TILED, what=f"{kind} {layout}")


# ---------------------------------------------------------------------------- dsp_mix_kernel
MIX_CLASSES = {**{f"single{c}": (c,) for c in range(4)}, "pair03": (0, 3), "pair12": (1, 2), "generic": (0, 1, 2, 3)}


def mix_params(name, F, T):
    rng = np.random.default_rng(1000 * F + T + sum(map(ord, name)))
    cs = MIX_CLASSES[name]
    return ref.class_params(rng, [cs[s % len(cs)] for s in range(F * T)])


def run_mix_device(ctx, kind, params0, F, T, frames, what):
    import torch
    nf_fan = 1
    params, states, dries = inputs_of_calls(kind, 40 * T + frames, params0, frames, rows=T,
                                            nf_sources=np.arange(nf_fan * T, (nf_fan + 1) * T), nf_samples=False)
    d_params = ref.Guarded(params, 0)
    d_state = ref.Guarded(states, 64)
    d_mix = ref.Guarded(np.full((F, frames * 2), np.nan, f32), 64)
    for call, dry in enumerate(dries):
        want, want_states = ref.mix(params, states, dry, F, T)
        d_dry = ref.Guarded(dry, 64)
        art.dsp.mix_device(ctx, d_dry.ptr, d_params.ptr, d_state.ptr, F, T, frames, d_mix.ptr, stream())
        assert art.dsp.debug_last_dsp_kernel(ctx) == abi.ART_DSP_KERNEL_MIX
        torch.cuda.synchronize()
        tag = f"{what} call {call}"
        assert d_dry.read(tag + " d_dry").tobytes() == dry.tobytes(), f"{tag}: d_dry was written"
        got = d_mix.read(tag + " d_mix").view(f32).reshape(F, -1)
        got_states = d_state.read(tag + " d_state").view(abi.DSP_STATE)
        ref.assert_same_bits(got, want, tag + " mix")
        ref.assert_same_bits(got_states, want_states, tag + " state")
        if kind == "nonfinite":  # only fan nf_fan holds non-finite values: nothing leaks into the wave's other fans
            others = np.arange(F) != nf_fan
            assert not np.isfinite(want[nf_fan]).all() and np.isfinite(want[others]).all()
            assert got[others].tobytes() == want[others].tobytes(), tag
        states = want_states


@pytest.mark.parametrize("F,T,frames", [(7, 3, 64), (13, 5, 65), (2, 33, 65)])
@pytest.mark.parametrize("classes", list(MIX_CLASSES))
def test_mix_kernel_class_matrix(ctx, classes, F, T, frames):
    """(7, 3, 64): packed fans, exactly one full tile; (13, 5, 65): idle slots, a partial last wave, a tile edge;
    (2, 33, 65): a second round."""
    run_mix_device(ctx, "gaussian", mix_params(classes, F, T), F, T, frames, f"{classes} {F}x{T}x{frames}")


@pytest.mark.parametrize("F,T,frames", [(7, 3, 65), (2, 33, 65)])
@pytest.mark.parametrize("classes", ["single0", "single1", "single2", "single3", "generic"])
@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_mix_kernel_value_classes(ctx, kind, classes, F, T, frames):
    run_mix_device(ctx, kind, mix_params(classes, F, T), F, T, frames, f"{kind} {classes} {F}x{T}x{frames}")


# ---------------------------------------------------------------------------- dsp_kernel (the lane kernel)
@pytest.mark.parametrize("frames", [1, 2, 37])
@pytest.mark.parametrize("kind", ["gaussian", "tail", "nonfinite"])
def test_lane_kernel_unaligned_data(ctx, kind, frames):
    """d_data 4 bytes into an allocation: legal by art_dsp.h, not 8-byte aligned, so launch_dsp takes dsp_kernel, and
    no source is 16-byte aligned, so every source runs its scalar loop. 300 sources: two blocks, the second partial;
    mixed classes and a few sources that are not stereo (the early return)."""
    count = 300
    rng = np.random.default_rng(300 + frames)
    classes = rng.integers(0, 4, count)
    classes[[0, 17, 255, 256, 299]] = 4
    params0 = ref.class_params(rng, classes.tolist())
    params, states, samples = inputs_of_calls(kind, 60 + frames, params0, frames)
    run_chain_device(ctx, params, states, samples, frames, abi.ART_DSP_KERNEL_LANE, before=4, what=f"lane {kind} x {frames}")


def test_lane_kernel_vector_path(tmp_path):
    """dsp_kernel's float4 path, in one child process with ART_DSP_KERNEL=lane (tests/dsp_lane_child.py has the cases
    and asserts that the lane kernel ran); its outputs against the reference here."""
    out = tmp_path / "lane.npz"
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dsp_lane_child.py"), str(out)],
                       env={**os.environ, "ART_DSP_KERNEL": "lane"}, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.load(out)
    for kind in child.KINDS:
        for count, frames in child.DEVICE_SHAPES:
            params, states, samples = child.device_case(kind, count, frames)
            for call in range(child.CALLS):
                want, states = ref.chain(params, states, samples[call])
                key = f"{kind}_{count}x{frames}_call{call}"
                ref.assert_same_bits(got[key + "_data"], want, key + " data")
                ref.assert_same_bits(got[key + "_state"].view(abi.DSP_STATE), states, key + " state")
        srcs = child.ragged_sources(kind)
        st = SpatializerSettings()
        params = [art.dsp.source_params(st, s, 48000) for s in srcs]
        assert {s.data.size // s.channels for s in srcs if s.channels == 2} == set(child.RAGGED_FRAMES)
        for call in range(child.CALLS):
            if call:
                child.ragged_next_data(kind, srcs, call)
            for i, s in enumerate(srcs):
                want, want_state = s.data, s.state
                if s.channels == 2 and s.data.size:
                    want, want_state = ref.chain(params[i], s.state, s.data[None, :])
                key = f"{kind}_ragged_call{call}"
                ref.assert_same_bits(got[f"{key}_data{i}"], want.reshape(1, -1), f"{key} source {i} data")
                ref.assert_same_bits(got[f"{key}_state"].view(abi.DSP_STATE)[i:i + 1], want_state, f"{key} source {i} state")
                s.state = np.ascontiguousarray(want_state).copy()

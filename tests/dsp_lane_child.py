"""TEST INFRASTRUCTURE: the child process of tests/test_dsp_variants_gpu.py::test_lane_kernel_vector_path.

ART_DSP_KERNEL is read once per process, so dsp_kernel's float4 path (16-byte aligned sources) is reached only in a
process started with ART_DSP_KERNEL=lane. This script runs the cases below in such a process, asserts after every
call that the lane kernel ran, and writes the outputs to the .npz file named on its command line; the parent
compares them with the NumPy reference (tests/dsp_chain_ref.py). pytest does not collect this file.

    python dsp_lane_child.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(os.path.dirname(HERE), "audio-raytracer_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from art import abi  # noqa: E402
import dsp_chain_ref as ref  # noqa: E402

f32 = np.float32
KINDS = ("gaussian", "tail")
# (count, frames): an odd frame count puts the sources at 16-byte and 8-byte alignment in turn (the float4 loop with
# its one-frame tail, and the scalar loop); 64 x 64 is float4 only
DEVICE_SHAPES = [(33, 37), (64, 64)]
RAGGED_FRAMES = (0, 1, 2, 3, 7, 64, 255)
CALLS = 2


def device_case(kind, count, frames):
    """(params, initial states, [samples of each call]) of one art_dsp_process_device case: mixed filter classes."""
    seed = 9000 + 100 * count + frames + KINDS.index(kind)
    rng = np.random.default_rng(seed)
    params = ref.class_params(rng, rng.integers(0, 4, count).tolist())
    calls = [ref.make_inputs(kind, seed + 1 + c, params, frames) for c in range(CALLS)]
    return params, calls[0][1], [c[0] for c in calls]


def ragged_sources(kind):
    """art_dsp_process sources of ragged length, every seventh one mono."""
    rng = np.random.default_rng(4242 + KINDS.index(kind))
    classes = [4 if i % 7 == 3 else int(rng.integers(0, 4)) for i in range(45)]
    srcs = ref.class_sources(rng, classes, 0)
    for i, s in enumerate(srcs):
        frames = RAGGED_FRAMES[(i // 7 + i) % 7]  # every length on a stereo source
        n = frames * s.channels
        s.state = np.zeros(1, abi.DSP_STATE)
        if kind == "tail":
            s.state.view(f32)[:] = ref.log_uniform(rng, 1e-41, 1e-30, 8)
            s.data = ref.log_uniform(rng, 1e-44, 1e-36, n) if i % 2 else np.zeros(n, f32)
        else:
            s.state.view(f32)[:] = rng.standard_normal(8).astype(f32) * f32(0.1)
            s.data = (rng.standard_normal(n) * 0.5).astype(f32)
    return srcs


def ragged_next_data(kind, srcs, call):
    """The buffers of call `call` > 0 (the states are carried)."""
    rng = np.random.default_rng(777 + call + KINDS.index(kind))
    for i, s in enumerate(srcs):
        if kind == "tail":
            s.data = ref.log_uniform(rng, 1e-44, 1e-36, s.data.size) if i % 2 else np.zeros(s.data.size, f32)
        else:
            s.data = (rng.standard_normal(s.data.size) * 0.5).astype(f32)


def main(out_path):
    import torch

    import art
    from art.dsp import SpatializerSettings
    assert os.environ.get("ART_DSP_KERNEL") == "lane"
    out = {}
    with art.Context(1) as ctx:
        stream = torch.cuda.current_stream().cuda_stream
        for kind in KINDS:
            for count, frames in DEVICE_SHAPES:
                params, states, samples = device_case(kind, count, frames)
                d_params = ref.Guarded(params, 0)
                d_state = ref.Guarded(states, 64)
                for call in range(CALLS):
                    d_data = ref.Guarded(samples[call], 1024)
                    assert d_data.ptr % 16 == 0
                    art.dsp.process_device(ctx, d_data.ptr, d_params.ptr, d_state.ptr, count, frames, stream)
                    assert art.dsp.debug_last_dsp_kernel(ctx) == abi.ART_DSP_KERNEL_LANE
                    torch.cuda.synchronize()
                    key = f"{kind}_{count}x{frames}_call{call}"
                    out[key + "_data"] = d_data.read(key + " data").view(f32).reshape(count, -1)
                    out[key + "_state"] = d_state.read(key + " state")
            srcs = ragged_sources(kind)
            for call in range(CALLS):
                if call:
                    ragged_next_data(kind, srcs, call)
                art.dsp.process(ctx, SpatializerSettings(), srcs, 48000)
                assert art.dsp.debug_last_dsp_kernel(ctx) == abi.ART_DSP_KERNEL_LANE
                for i, s in enumerate(srcs):
                    out[f"{kind}_ragged_call{call}_data{i}"] = s.data.copy()
                out[f"{kind}_ragged_call{call}_state"] = np.concatenate([s.state for s in srcs]).view(np.uint8)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1])

#!/usr/bin/env python3
"""The server's audio tick, timed the way dynamic_run.py times its steps:
every source of a config's frame (fans x targets) spatialized from the frame's own result blocks,
`frames` samples per buffer at 48 kHz. GPU box only.
    python3 tools/tick_run.py [config] [steps] [--frames N]
Per tick, on torch's stream:
  (a) device tick   art_launch_device + art_dsp_tick_device (no host synchronisation)
  (b) host params   art_launch_device, D2H copy of the settings sections (pinned), art_dsp_tick_params_host,
                    H2D copy of the parameters (pinned), art_dsp_process_device: the path (a) replaces
and the parameter step alone (art_dsp_tick_params_device back to back: an upper bound of
dsp_tick_params_kernel's own time; a rocprofv3 --kernel-trace of this tool gives the kernel's)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "audio-raytracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import art  # noqa: E402
from art import abi  # noqa: E402
from art.dsp import SpatializerSettings  # noqa: E402

SAMPLE_RATE = 48000


def timed(one, steps, what, cfg):
    for i in range(10):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(f"config {cfg.index}: {what} {ms:.4f} ms over {steps} steps", flush=True)
    return ms


def main():
    argv = sys.argv[1:]
    frames = 1024
    if "--frames" in argv:
        at = argv.index("--frames")
        frames = int(argv[at + 1])
        del argv[at:at + 2]
    cfg = art.CONFIGS[int(argv[0]) if len(argv) > 0 else 2]
    steps = int(argv[1]) if len(argv) > 1 else 500
    scene, org, params = art.synth(cfg)
    S, T = org.shape[0], scene.T
    n = S * T
    rng = np.random.default_rng(11)
    ctx = art.Context(1)
    frame = art.Frame(scene, params, org, art.FanOutputs(S, cfg.R, cfg.H, T, 1, dsp=params.dsp is not None))
    lay = art.fan_layout(frame)
    ctx.bind(frame)
    st = SpatializerSettings()
    art.dsp.bind_settings(ctx, st, SAMPLE_RATE)
    st_c = st.to_c()
    listeners = np.zeros(S, abi.LISTENER)  # each fan's listener at the fan's origin, any orientation
    listeners["position"] = org
    q = rng.standard_normal((S, 4))
    listeners["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)

    dev = torch.device("cuda", 0)
    d_org = torch.from_numpy(np.ascontiguousarray(org)).to(dev)
    d_blk = torch.zeros(S * lay["stride"], dtype=torch.uint8, device=dev)
    d_ls = torch.from_numpy(listeners.view(np.uint8).copy()).to(dev)
    d_data = torch.from_numpy((rng.standard_normal((n, frames * 2)) * 0.5).astype(np.float32)).to(dev)
    d_state = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_par = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"config {cfg.index}: {S} fans x {T} targets = {n} sources, {frames} frames per buffer at {SAMPLE_RATE} Hz "
          f"({frames / SAMPLE_RATE * 1e3:.2f} ms of audio per tick)", flush=True)

    def tick_a(i):
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        art.dsp.tick_device(ctx, d_blk, S, d_ls, d_data, d_state, frames, d_par, None, 0, sp)

    # (b): pinned staging, the fans' settings pointers and the host call prepared once
    h_set = torch.empty((S, T * 24), dtype=torch.uint8).pin_memory()
    h_par = torch.empty(n * 32, dtype=torch.uint8).pin_memory()
    sec = d_blk.view(S, lay["stride"])[:, lay["settings_off"]:lay["settings_off"] + T * 24]
    fans = (abi.art_fan * S)()
    for f in range(S):
        fans[f].settings = h_set.data_ptr() + f * T * 24
    lib = ctx.lib

    def tick_b(i):
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        h_set.copy_(sec, non_blocking=True)
        torch.cuda.current_stream().synchronize()  # the host needs the settings
        rc = lib.art_dsp_tick_params_host(C.byref(st_c), SAMPLE_RATE, listeners.ctypes.data, fans, S, scene.targets.ctypes.data,
                                          T, None, h_par.data_ptr())
        assert rc == 0, rc
        d_par.copy_(h_par, non_blocking=True)
        rc = lib.art_dsp_process_device(ctx.ptr, d_data.data_ptr(), d_par.data_ptr(), d_state.data_ptr(), n, frames, sp)
        assert rc == 0, rc

    def params_only(i):
        art.dsp.tick_params_device(ctx, d_blk, S, d_ls, d_par, None, 0, sp)

    def frame_only(i):
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)

    # both paths give the same parameters (the tool's own check before it times anything)
    tick_b(0)
    torch.cuda.synchronize()
    host_par = d_par.cpu().numpy().copy()
    params_only(0)
    torch.cuda.synchronize()
    same = bool((d_par.cpu().numpy() == host_par).all())
    print(f"config {cfg.index}: device parameters equal the host twin's: {same}", flush=True)

    t_f = timed(frame_only, steps, "art_launch_device alone", cfg)
    t_a = timed(tick_a, steps, "(a) art_launch_device + art_dsp_tick_device", cfg)
    t_b = timed(tick_b, steps, "(b) art_launch_device + D2H settings + host params + H2D + art_dsp_process_device", cfg)
    t_p = timed(params_only, steps, "art_dsp_tick_params_device alone, back to back", cfg)
    print(f"config {cfg.index}: tick_a_ms {t_a:.4f} tick_b_ms {t_b:.4f} frame_ms {t_f:.4f} params_step_ms {t_p:.4f} "
          f"a_over_b {t_a / t_b:.3f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

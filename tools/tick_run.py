#!/usr/bin/env python3
"""The server's audio tick, timed the way dynamic_run.py times its steps:
every source of a config's frame (fans x targets) spatialized from the frame's own result blocks,
`frames` samples per buffer at 48 kHz. GPU box only.
    python3 tools/tick_run.py [config] [steps] [--frames N]
    python3 tools/tick_run.py --mix-batch FANS [steps] [--frames N] [--targets T]
    python3 tools/tick_run.py --classes K[,K...] [steps] [--shapes FANSxT[,FANSxT...]]
Per tick, on torch's stream:
  (a) device tick   art_launch_device + art_dsp_tick_device (no host synchronisation)
  (b) host params   art_launch_device, D2H copy of the settings sections (pinned), art_dsp_tick_params_host,
                    H2D copy of the parameters (pinned), art_dsp_process_device: the path (a) replaces
  (c) listener mix  art_launch_device + art_dsp_tick_mix_device: one dry buffer per target in, one mix
                    per fan out. Before timing, (c)'s mix is compared with an ordered sum over (a)'s wet
                    buffers. (a+) is the path (c) replaces: (a) with a torch broadcast of the dry input
                    in front and a torch sum of the wet buffers behind it
and the parameter step alone (art_dsp_tick_params_device back to back: an upper bound of
dsp_tick_params_kernel's own time; a rocprofv3 --kernel-trace of this tool gives the kernel's).
--mix-batch times art_dsp_mix_device alone (device events) on FANS fans of random sources beside
art_dsp_process_device on the same FANS * T sources, and prints the algorithmic HBM bytes of both
(a rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE pass of this mode gives the measured ones).
--classes times art_dsp_tick_params_device alone (device events) under a single bind (K = 1) and under K
settings classes (art_dsp_settings_bind_classes), on synthetic blocks of the given shapes (default: 256 fans
x 4 targets and 4096 x 64): profiles/tick_classes.txt."""
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


def take(argv, flag, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    v = int(argv[at + 1])
    del argv[at:at + 2]
    return v


def ordered_sum(wet, S, T):
    """float32 [S*T, n] -> [S, n]: one add per target in ascending order, from the first buffer itself."""
    wet = wet.reshape(S, T, -1)
    acc = wet[:, 0].copy()
    for t in range(1, T):
        acc = np.add(acc, wet[:, t], dtype=np.float32)
    return acc


def mix_batch(F, T, frames, steps):
    """art_dsp_mix_device on F fans x T targets beside art_dsp_process_device on the same F*T sources."""
    from art.dsp import AudioSource
    rng = np.random.default_rng(12)
    n = F * T
    st = SpatializerSettings()
    base = []
    for k in range(64):  # 64 parameter records of every filter class, repeated over the batch
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)
        src = AudioSource(data=np.zeros(2, np.float32), muffle_strength=float(rng.choice([0.0, rng.random()])),
                          reverb_volume=float(rng.random()), local_dir=tuple(float(v) for v in d),
                          listener_distance=float(rng.uniform(0, 30)), volume_multiplier=float(rng.uniform(0.5, 1.0)))
        base.append(art.dsp.source_params(st, src, SAMPLE_RATE))
    params = np.concatenate(base)[rng.integers(0, 64, n)]
    dev = torch.device("cuda", 0)
    ctx = art.Context(1)
    d_par = torch.from_numpy(params.view(np.uint8).copy()).to(dev)
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(np.float32)
    d_dry = torch.from_numpy(dry).to(dev)
    d_mix = torch.zeros((F, frames * 2), dtype=torch.float32, device=dev)
    d_state = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    sp = torch.cuda.current_stream().cuda_stream
    print(f"mix batch: {F} fans x {T} targets = {n} sources, {frames} frames", flush=True)
    alg_mix = 8 * T * frames + 8 * F * frames + 96 * F * T
    alg_unmixed = 16 * n * frames + 96 * n
    print(f"mix batch: algorithmic HBM bytes: art_dsp_mix_device {alg_mix} (8 T frames + 8 F frames + 96 F T), "
          f"art_dsp_process_device {alg_unmixed} (16 n frames + 96 n)", flush=True)

    def ev_time(one, what):
        for _ in range(3):
            one()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        print(f"mix batch: {what}: min {ts[0]:.1f} us, median {ts[len(ts) // 2]:.1f} us over {steps} calls "
              f"(device events around one call)", flush=True)

    ev_time(lambda: art.dsp.mix_device(ctx, d_dry, d_par, d_state, F, T, frames, d_mix, sp), "art_dsp_mix_device")
    if n * frames * 8 < 0x7fffffff:
        d_data = d_dry.repeat(F, 1)
        lib = ctx.lib

        def unmixed():
            rc = lib.art_dsp_process_device(ctx.ptr, d_data.data_ptr(), d_par.data_ptr(), d_state.data_ptr(), n, frames, sp)
            assert rc == 0, rc
        ev_time(unmixed, "art_dsp_process_device, same sources")
    ctx.close()


def take_str(argv, flag, default):
    if flag not in argv:
        return default
    at = argv.index(flag)
    v = argv[at + 1]
    del argv[at:at + 2]
    return v


def classes_run(Ks, shapes, steps):
    """The parameter step alone under a single bind (K = 1: art_dsp_settings_bind, no class map) and under
    K settings classes (art_dsp_settings_bind_classes, target t in class t % K), on a synthetic block of
    random settings records over the tiny scene with T targets. Before timing, the device parameters are
    compared with the host twin's. Device events: around every single call, and around `steps` calls
    back to back (per call). Every (shape, K) is timed in two rounds, K alternating within a round."""
    rng = np.random.default_rng(15)
    dev = torch.device("cuda", 0)
    sp = torch.cuda.current_stream().cuda_stream

    def one_class():
        u = lambda a, b: float(rng.uniform(a, b))  # noqa: E731
        return SpatializerSettings(
            pan_strength=u(0.1, 1), rear_attenuation_strength=u(0.1, 1), distance_based_panning=bool(rng.random() < 0.5),
            max_pan_distance=u(1, 10), distance_based_rear_attenuation=bool(rng.random() < 0.5),
            max_rear_attenuation_distance=u(1, 30), max_elevation_effect_distance=u(1, 20),
            muffle_curve=rng.random(int(rng.integers(2, 60))).astype(np.float32),
            reverb_volume_curve=rng.random(int(rng.integers(2, 60))).astype(np.float32))

    classes = [SpatializerSettings()] + [one_class() for _ in range(max(Ks) - 1)]
    for F, T in shapes:
        scene, org, params = art.synth(art.CONFIGS[2], S=1, R=64, C_scale=0.01)
        extra = rng.uniform(-20, 20, (max(0, T - scene.T), 3)).astype(np.float32)
        scene = art.Scene(dirs=scene.dirs, targets=np.ascontiguousarray(np.concatenate([scene.targets, extra])[:T]),
                          spheres=scene.spheres, aabbs=scene.aabbs)
        ctx = art.Context(1)
        frame = art.Frame(scene, params, org, art.FanOutputs(1, 64, params.max_hits_per_ray, T, 1))
        ctx.bind(frame)
        lay = art.fan_layout(frame)
        listeners = np.zeros(F, abi.LISTENER)
        listeners["position"] = rng.uniform(-30, 30, (F, 3))
        q = rng.standard_normal((F, 4))
        listeners["rotation"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        fs = np.zeros((F, T), abi.SETTINGS)
        fs["muffle_strength"] = np.where(rng.random((F, T)) < 0.3, 0.0, rng.random((F, T)))
        fs["reverb_strength"] = rng.random((F, T))
        fs["reverb_volume"] = rng.random((F, T))
        fs["perceived_position"] = rng.uniform(-30, 30, (F, T, 3))
        block = np.zeros((F, lay["stride"]), np.uint8)
        block[:, lay["settings_off"]:lay["settings_off"] + T * 24] = fs.view(np.uint8).reshape(F, T * 24)
        d_blk = torch.from_numpy(block.reshape(-1)).to(dev)
        d_ls = torch.from_numpy(listeners.view(np.uint8).copy()).to(dev)
        d_par = torch.zeros(F * T * 32, dtype=torch.uint8, device=dev)
        print(f"classes: {F} fans x {T} targets = {F * T} sources", flush=True)

        def call():
            art.dsp.tick_params_device(ctx, d_blk, F, d_ls, d_par, None, 0, sp)

        def setup(K):
            if K == 1:
                art.dsp.bind_settings(ctx, classes[0], SAMPLE_RATE)
                return art.dsp.tick_params_host(classes[0], listeners, fs, scene.targets, None, SAMPLE_RATE)
            cls = (np.arange(T) % K).astype(np.uint8)
            art.dsp.bind_settings_classes(ctx, classes[:K], SAMPLE_RATE)
            art.dsp.set_target_classes(ctx, cls)
            return art.dsp.tick_params_classes_host(classes[:K], listeners, fs, scene.targets, cls, None, SAMPLE_RATE)

        for rnd in range(2):
            for K in Ks:
                want = setup(K)
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                same = d_par.cpu().numpy().tobytes() == want.tobytes()
                ts = []
                for _ in range(steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                ts.sort()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    call()
                e1.record()
                e1.synchronize()
                what = "single bind" if K == 1 else f"K = {K} classes"
                print(f"classes: {F} x {T}, round {rnd}, {what}: params_step_us min {ts[0]:.2f} median {ts[len(ts) // 2]:.2f} "
                      f"(events around one call), {e0.elapsed_time(e1) * 1e3 / steps:.2f} per call over {steps} calls back to "
                      f"back; equals the host twin: {same}", flush=True)
                if K > 1:
                    art.dsp.set_target_classes(ctx, [])
        ctx.close()


def main():
    argv = sys.argv[1:]
    frames = take(argv, "--frames", 1024)
    classes = take_str(argv, "--classes", "")
    shapes = take_str(argv, "--shapes", "256x4,4096x64")
    targets = take(argv, "--targets", 4)
    batch = take(argv, "--mix-batch", 0)
    if classes:
        return classes_run([int(k) for k in classes.split(",")], [tuple(int(v) for v in s.split("x")) for s in shapes.split(",")],
                           int(argv[0]) if argv else 200)
    if batch:
        return mix_batch(batch, targets, frames, int(argv[0]) if argv else 20)
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

    # (c): one dry buffer per target, one mix per fan; (a+): the same through (a)'s interface
    dry = (rng.standard_normal((T, frames * 2)) * 0.5).astype(np.float32)
    d_dry = torch.from_numpy(dry).to(dev)
    d_mix = torch.zeros((S, frames * 2), dtype=torch.float32, device=dev)
    d_mix_t = torch.zeros((S, frames * 2), dtype=torch.float32, device=dev)
    d_state_c = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_par_c = torch.zeros(n * 32, dtype=torch.uint8, device=dev)

    def tick_c(i):
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        art.dsp.tick_mix_device(ctx, d_blk, S, d_ls, d_dry, d_state_c, frames, d_par_c, d_mix, None, 0, sp)

    def tick_a_plus(i):
        d_data.view(S, T, frames * 2).copy_(d_dry.unsqueeze(0).expand(S, T, frames * 2))
        tick_a(i)
        torch.sum(d_data.view(S, T, frames * 2), dim=1, out=d_mix_t)

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

    # (c)'s mix equals the ordered sum over (a)'s wet buffers, from equal (zero) states
    keep = d_data.clone()
    d_data.view(S, T, frames * 2).copy_(d_dry.unsqueeze(0).expand(S, T, frames * 2))
    d_state.zero_()
    d_state_c.zero_()
    tick_a(0)
    tick_c(0)
    torch.cuda.synchronize()
    want = ordered_sum(d_data.cpu().numpy(), S, T)
    same_mix = d_mix.cpu().numpy().tobytes() == want.tobytes() and bool((d_state.cpu() == d_state_c.cpu()).all())
    print(f"config {cfg.index}: (c)'s mix and state equal the ordered sum over (a)'s wet buffers: {same_mix}", flush=True)
    d_data.copy_(keep)

    t_f = timed(frame_only, steps, "art_launch_device alone", cfg)
    t_a = timed(tick_a, steps, "(a) art_launch_device + art_dsp_tick_device", cfg)
    t_b = timed(tick_b, steps, "(b) art_launch_device + D2H settings + host params + H2D + art_dsp_process_device", cfg)
    t_c = timed(tick_c, steps, "(c) art_launch_device + art_dsp_tick_mix_device", cfg)
    t_ap = timed(tick_a_plus, steps, "(a+) torch broadcast of the dry input + (a) + torch sum of the wet buffers", cfg)
    t_p = timed(params_only, steps, "art_dsp_tick_params_device alone, back to back", cfg)
    print(f"config {cfg.index}: tick_a_ms {t_a:.4f} tick_b_ms {t_b:.4f} tick_c_ms {t_c:.4f} tick_a_plus_ms {t_ap:.4f} "
          f"frame_ms {t_f:.4f} params_step_ms {t_p:.4f} a_over_b {t_a / t_b:.3f} c_over_a {t_c / t_a:.3f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

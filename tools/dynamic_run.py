#!/usr/bin/env python3
"""bench.py's dynamic step alone (1 % of the colliders moved per step: art_collider_set_many +
art_colliders_sync + art_launch_device on torch's stream), for its kernel / copy timeline under
rocprofv3 --kernel-trace --memory-copy-trace, and its ms per step. GPU box only.
    python3 tools/dynamic_run.py [config] [steps]
The moving-target step, timed the same way:
    python3 tools/dynamic_run.py [config] [steps] --targets K            K of the T targets moved per step:
                                 art_target_set_many + art_targets_sync + art_launch_device
    python3 tools/dynamic_run.py [config] [steps] --targets K --rebind   the same step without the target
                                 store: art_scene_bind with the new positions + art_launch_device
Targets that spawn and despawn (a scene bound with a reserved capacity follows the count):
    python3 tools/dynamic_run.py [config] [steps] --spawn [--extra E] [--remove I] [--rebind]
                                 steps alternately add one target and remove-swapback target I (default 0: the
                                 spawned one lands on an index that colliders name, its lists are rebuilt); with
                                 --extra 1 --remove T the config's T + 1 targets and target T owns nothing: its
                                 successor's lists move. --rebind: art_scene_bind with each step's list instead."""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "audio-raytracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import art  # noqa: E402
from art import abi  # noqa: E402
from art.colliders import ColliderStore, resident_frame  # noqa: E402
from bench import jitter_records  # noqa: E402


def timed(one, steps, what, cfg):
    for i in range(10):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    print(f"config {cfg.index}: {what} {(time.perf_counter() - t0) / steps * 1e3:.4f} ms over {steps} steps", flush=True)


def target_steps(cfg, steps, K, rebind):
    """K of the T targets moved by up to 2 units per step, eight pre-made variants (a target's
    position differs between the variants that move it, so every step's K sets are real moves)."""
    scene, org, params = art.synth(cfg)
    S, T = org.shape[0], scene.T
    K = min(K, T)
    rng = np.random.default_rng(7)
    variants = []
    for v in range(8):
        ids = np.sort((v * K + np.arange(K)) % T).astype(np.int32)  # every target in turn: each step moves K
        variants.append((ids, (scene.targets[ids] + rng.uniform(-2, 2, (K, 3))).astype(np.float32)))
    ctx = art.Context(1)
    out = art.FanOutputs(S, cfg.R, cfg.H, T, 1, dsp=params.dsp is not None)
    frame = art.Frame(scene, params, org, out)
    lay = art.fan_layout(frame)
    d_org = torch.from_numpy(np.ascontiguousarray(org)).cuda()
    d_blk = torch.zeros(S * lay["stride"], dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    if rebind:
        frames, pos = [], scene.targets.copy()
        for ids, p in variants:  # each variant's whole scene, as a caller without the store binds it
            pos = pos.copy()
            pos[ids] = p
            sc = art.Scene(dirs=scene.dirs, targets=pos, spheres=scene.spheres, aabbs=scene.aabbs, obbs=scene.obbs)
            frames.append(art.Frame(sc, params, org, out))

        def one(i):
            ctx.bind(frames[i % len(frames)])
            ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        timed(one, steps, f"{K} of {T} targets moved, art_scene_bind + launch", cfg)
    else:
        from art.targets import TargetStore, resident_targets_frame
        store = TargetStore(ctx)
        store.add_many(scene.targets)
        store.sync()
        ctx.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        ctx.bind(resident_targets_frame(frame))
        stats = {}

        def one(i):
            ids, p = variants[i % len(variants)]
            store.set_many(ids, p)
            st = store.sync()
            stats[(st["lists_rebuilt"], st["lists_full_rebuild"])] = stats.get((st["lists_rebuilt"], st["lists_full_rebuild"]), 0) + 1
            ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        timed(one, steps, f"{K} of {T} targets moved, art_target_set_many + art_targets_sync + launch", cfg)
        print(f"  syncs by (lists_rebuilt, lists_full_rebuild): {stats}; arena {store.cells_arena()}", flush=True)
    ctx.close()


def spawn_steps(cfg, steps, rebind, extra, remove):
    """Steps alternately add one target and remove-swapback target `remove` (the config's T + extra
    targets and one more); `extra` targets that own no colliders are added first and stay. With the
    store the scene is bound once with a reserved capacity; --rebind binds each step's list."""
    scene, org, params = art.synth(cfg)
    S = org.shape[0]
    rng = np.random.default_rng(7)
    lo, hi = scene.targets.min(axis=0) - 2, scene.targets.max(axis=0) + 2
    pos = [p for p in scene.targets] + [rng.uniform(lo, hi).astype(np.float32) for _ in range(extra)]
    T0 = len(pos)
    spawn = [rng.uniform(lo, hi).astype(np.float32) for _ in range(8)]
    ctx = art.Context(1)
    outs = {T: art.FanOutputs(S, cfg.R, cfg.H, T, 1, dsp=params.dsp is not None) for T in (T0, T0 + 1)}

    def frame_of(p):
        sc = art.Scene(dirs=scene.dirs, targets=np.array(p, np.float32), spheres=scene.spheres, aabbs=scene.aabbs, obbs=scene.obbs)
        return art.Frame(sc, params, org, outs[len(p)])
    stride = max(art.fan_layout(frame_of(pos + [spawn[0]][:k]))["stride"] for k in (0, 1))
    d_org = torch.from_numpy(np.ascontiguousarray(org)).cuda()
    d_blk = torch.zeros(S * stride, dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    what = f"T {T0} <-> {T0 + 1}, add / remove-swapback {remove}"
    if rebind:
        frames = {}

        def one(i):
            if i % 2 == 0:
                pos.append(spawn[(i // 2) % len(spawn)])
            else:
                pos[remove] = pos[-1]
                pos.pop()
            key = b"".join(p.tobytes() for p in pos)
            if key not in frames:  # (the lists repeat with the eight spawn positions: made once)
                frames[key] = frame_of(pos)
            ctx.bind(frames[key])
            ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        for i in range(32):  # every list of the cycle, before the timed steps
            one(i)
        timed(one, steps, f"{what}, art_scene_bind + launch", cfg)
    else:
        from art.targets import TargetStore, resident_targets_frame
        store = TargetStore(ctx)
        store.add_many(pos)
        store.sync()
        store.reserve(T0 + 1)
        ctx.set_flags(abi.ART_CTX_RESIDENT_TARGETS)
        ctx.bind(resident_targets_frame(frame_of(pos)))
        stats = {}

        def one(i):
            if i % 2 == 0:
                store.add(spawn[(i // 2) % len(spawn)])
            else:
                store.remove_swapback(remove)
            store.sync()
            rs = store.last_resize()
            key = (rs["kept_bound"], rs["lists_moved"], rs["lists_rebuilt"], rs["lists_full_rebuild"])
            stats[key] = stats.get(key, 0) + 1
            ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)
        timed(one, steps, f"{what}, art_target_add / remove + art_targets_sync + launch", cfg)
        print(f"  syncs by (kept_bound, lists_moved, lists_rebuilt, lists_full_rebuild): {stats}; arena {store.cells_arena()}",
              flush=True)
    ctx.close()


def main():
    argv = sys.argv[1:]
    opts = {"--extra": 0, "--remove": 0}
    for name in opts:
        if name in argv:
            at = argv.index(name)
            opts[name] = int(argv[at + 1])
            del argv[at:at + 2]
    K = None
    if "--targets" in argv:
        at = argv.index("--targets")
        K = int(argv[at + 1])
        del argv[at:at + 2]
    args = [a for a in argv if not a.startswith("--")]
    cfg = art.CONFIGS[int(args[0]) if len(args) > 0 else 2]
    steps = int(args[1]) if len(args) > 1 else 500
    if "--spawn" in argv:
        return spawn_steps(cfg, steps, "--rebind" in argv, opts["--extra"], opts["--remove"])
    if K is not None:
        return target_steps(cfg, steps, K, "--rebind" in argv)
    scene, org, params = art.synth(cfg)
    S = org.shape[0]
    ctx = art.Context(1)
    store = ColliderStore(ctx)
    fields = {abi.ART_KIND_SPHERE: scene.spheres, abi.ART_KIND_AABB: scene.aabbs, abi.ART_KIND_OBB: scene.obbs}
    for k, arr in fields.items():
        for i in range(arr.size):
            store.add(k, arr[i])
    store.sync()
    ctx.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
    out = art.FanOutputs(S, cfg.R, cfg.H, cfg.T, 1, dsp=params.dsp is not None)
    rframe = resident_frame(art.Frame(scene, params, org, out))
    lay = art.fan_layout(rframe)
    ctx.bind(rframe)
    d_org = torch.from_numpy(np.ascontiguousarray(org)).cuda()
    d_blk = torch.zeros(S * lay["stride"], dtype=torch.uint8, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(7)
    variants = []
    for _ in range(8):
        moves = {}
        for k, arr in fields.items():
            if arr.size:
                ids = rng.choice(arr.size, max(1, arr.size // 100), replace=False).astype(np.int32)
                moves[k] = (ids, jitter_records(rng, arr[ids], 0.05))
        variants.append(moves)

    def one(i):
        for k, (ids, recs) in variants[i % len(variants)].items():
            store.set_many(k, ids, recs)
        store.sync()
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), 0, sp)

    for i in range(10):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(i)
    torch.cuda.synchronize()
    print(f"config {cfg.index}: dynamic step {(time.perf_counter() - t0) / steps * 1e3:.4f} ms over {steps} steps", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

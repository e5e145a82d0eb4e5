#!/usr/bin/env python3
"""Colliders that appear and disappear on a bound scene, measured. GPU box only.

    python3 tools/collider_churn_run.py [--out DIR]

runs the two measurements below, each GPU step as a child process of its own under its own time
limit, stops at the first child that fails, and writes DIR/collider_resize_step.txt and
DIR/collider_churn.txt (default: profiles/).

The resize step against the rebind it replaces (config 2 at full size: 2048 spheres + 2048 AABBs,
capacity 4096 + 64 shared between the kinds): one step removes one collider of one kind and adds one
of the other (so a count changes every step), syncs and launches. With a reserved capacity the bound
scene follows (art_colliders_reserve); without, the sync unbinds and the step is sync,
art_scene_bind, launch, as before ABI 3.10. Both run in one process, in alternating blocks; every
step ends in a device synchronise and the p50 of the step times is reported.
    python3 tools/collider_churn_run.py --child step [--blocks B] [--steps N]

The churn denominator (ART_BVH_RESORT_DEN=0: never sort again): after adds and removes that sum to a
fraction of the colliders, the total held constant, the static frame's ms per step on the relabelled
tree against a fresh bind of the same final scene, each measured `--repeats` times.
    python3 tools/collider_churn_run.py --child churn --fraction F [--steps N] [--repeats K]
The driver picks the largest fraction whose median stays within twice the spread seen between the
repeated fresh-bind measurements of the session.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "audio-raytracer_amd"))

FRACTIONS = ("1/64", "1/32", "1/16", "1/8", "1/4", "1/2")
SLACK = 32  # room per kind past the config's count


def setup(reserve):
    import numpy as np
    import torch
    import art
    from art import abi
    from art.colliders import ColliderStore, resident_frame
    cfg = art.CONFIGS[2]
    scene, org, params = art.synth(cfg)
    pool = art.synth(cfg, seed=cfg.seed + 1000)[0]
    ctx = art.Context(1)
    store = ColliderStore(ctx)
    if reserve:
        store.reserve(scene.spheres.size + SLACK, scene.aabbs.size + SLACK, 0)
    for k, arr in ((abi.ART_KIND_SPHERE, scene.spheres), (abi.ART_KIND_AABB, scene.aabbs)):
        store.add_many(k, arr)
    store.sync()
    ctx.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
    out = art.FanOutputs(org.shape[0], cfg.R, cfg.H, scene.T, 1)
    frame = art.Frame(scene, params, org, out)
    rframe = resident_frame(frame)
    ctx.bind(rframe)
    lay = art.fan_layout(frame)
    d_org = torch.from_numpy(np.ascontiguousarray(org)).cuda()
    d_blk = torch.zeros(org.shape[0] * lay["stride"], dtype=torch.uint8, device="cuda")
    return dict(ctx=ctx, store=store, rframe=rframe, frame=frame, pool=pool, scene=scene, org=org, params=params,
                d_org=d_org, d_blk=d_blk, S=org.shape[0], out=out, lay=lay)


def swap_one(r, i, rng):
    """Step i's edit: one collider of one kind out (a random index), one of the other kind in."""
    from art import abi
    out_k, in_k = (abi.ART_KIND_SPHERE, abi.ART_KIND_AABB) if i % 2 == 0 else (abi.ART_KIND_AABB, abi.ART_KIND_SPHERE)
    r["store"].remove_swapback(out_k, int(rng.integers(0, r["store"].count(out_k))))
    src = r["pool"].spheres if in_k == abi.ART_KIND_SPHERE else r["pool"].aabbs
    r["store"].add(in_k, src[i % src.size])


def child_step(blocks, steps):
    import numpy as np
    import torch
    kept, rebind = setup(True), setup(False)
    sp = torch.cuda.current_stream().cuda_stream
    rngs = {id(kept): np.random.default_rng(3), id(rebind): np.random.default_rng(3)}
    serial = {id(kept): 0, id(rebind): 0}
    resorted = {id(kept): 0, id(rebind): 0}

    def one(r, bind):
        i = serial[id(r)]
        serial[id(r)] += 1
        t0 = time.perf_counter()
        swap_one(r, i, rngs[id(r)])
        r["store"].sync()
        if bind:
            r["ctx"].bind(r["rframe"])
        r["ctx"].launch_device(r["d_org"].data_ptr(), r["S"], r["d_blk"].data_ptr(), 0, sp)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        resorted[id(r)] += r["store"].last_resize()["bvh_rebuilt"]  # (outside the timed window)
        return ms

    for _ in range(10):  # warm-up: both paths, both directions of the edit
        one(kept, False)
        one(rebind, True)
    assert kept["store"].last_resize()["kept_bound"] == 1 and rebind["store"].last_resize()["kept_bound"] == 0
    t = {"kept": [], "rebind": []}
    for _ in range(blocks):
        t["kept"] += [one(kept, False) for _ in range(steps)]
        t["rebind"] += [one(rebind, True) for _ in range(steps)]
    rs = kept["store"].last_resize()
    assert rs["kept_bound"] == 1, rs
    assert torch.equal(kept["d_blk"], rebind["d_blk"]), "the two paths' last frames differ"
    for name, v in t.items():
        q = np.percentile(v, [10, 50, 90])
        print(f"  {name:7s} step: p50 {q[1]:.4f} ms (p10 {q[0]:.4f}, p90 {q[2]:.4f}) over {len(v)} steps", flush=True)
    print(f"  ratio rebind / kept (p50): {np.median(t['rebind']) / np.median(t['kept']):.2f}; kept steps that sorted again: "
          f"{resorted[id(kept)]}; last kept step: {rs}", flush=True)
    kept["ctx"].close()
    rebind["ctx"].close()


def static_ms(ctx, r, steps, repeats, blk):
    import torch
    sp = torch.cuda.current_stream().cuda_stream
    for _ in range(20):
        ctx.launch_device(r["d_org"].data_ptr(), r["S"], blk.data_ptr(), 0, sp)
    torch.cuda.synchronize()
    res = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.launch_device(r["d_org"].data_ptr(), r["S"], blk.data_ptr(), 0, sp)
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) / steps * 1e3)
    return res


def child_churn(fraction, steps, repeats):
    import numpy as np
    import torch
    import art
    from art import abi
    assert os.environ.get("ART_BVH_RESORT_DEN") == "0"
    num, den = (int(x) for x in fraction.split("/"))
    r = setup(True)
    store, rng = r["store"], np.random.default_rng(11)
    C = r["scene"].C
    want = C * num // den  # adds + removes
    churned, batch, rebuilt = 0, 0, 0
    while churned < want:
        k = min(SLACK, (want - churned + 1) // 2)
        out_k, in_k = (abi.ART_KIND_SPHERE, abi.ART_KIND_AABB) if batch % 2 == 0 else (abi.ART_KIND_AABB, abi.ART_KIND_SPHERE)
        src = r["pool"].spheres if in_k == abi.ART_KIND_SPHERE else r["pool"].aabbs
        for j in range(k):
            store.remove_swapback(out_k, int(rng.integers(0, store.count(out_k))))
            store.add(in_k, src[(churned + j) % src.size])
        store.sync()
        rs = store.last_resize()
        assert rs["kept_bound"] == 1, rs
        rebuilt += rs["bvh_rebuilt"]
        churned += 2 * k
        batch += 1
    assert rebuilt == 0
    counts = [store.count(k) for k in (abi.ART_KIND_SPHERE, abi.ART_KIND_AABB)]
    assert sum(counts) == C
    final = art.Scene(dirs=r["scene"].dirs, targets=r["scene"].targets, spheres=store.array(abi.ART_KIND_SPHERE),
                      aabbs=store.array(abi.ART_KIND_AABB))
    fresh = art.Context(1)
    fresh.bind(art.Frame(final, r["params"], r["org"], r["out"]))
    fblk = torch.zeros_like(r["d_blk"])
    a, b = [], []
    for _ in range(repeats):  # alternating, one measurement each
        a += static_ms(r["ctx"], r, steps, 1, r["d_blk"])
        b += static_ms(fresh, r, steps, 1, fblk)
    assert torch.equal(r["d_blk"], fblk), "the relabelled tree's frame differs from the fresh bind's"
    print(f"CHURN {fraction} churned {churned} of {C} counts {counts} relabelled_ms {' '.join(f'{x:.5f}' for x in a)} "
          f"fresh_ms {' '.join(f'{x:.5f}' for x in b)}", flush=True)
    fresh.close()
    r["ctx"].close()


def run_child(args, limit, env=None):
    """One GPU step as a process of its own under its own time limit; its output, or None if it failed."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", *args]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    sys.stdout.write(p.stdout)
    if p.returncode != 0:
        sys.stdout.write(f"child {' '.join(args)} failed with status {p.returncode}; stopping\n{p.stderr[-2000:]}\n")
        return None
    return p.stdout


def driver(out_dir, steps, repeats):
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    text = run_child(["step"], 300)
    if text is None:
        return 1
    with open(os.path.join(out_dir, "collider_resize_step.txt"), "w") as f:
        f.write("tools/collider_churn_run.py --child step: config 2 (256 fans x 512 rays, 2048 spheres + 2048 AABBs), one collider\n"
                "out and one of the other kind in per step, then sync and launch; each step ends in a device synchronise.\n"
                "kept: bound with capacity 4096 + 64 (the scene follows); rebind: nothing reserved (sync, art_scene_bind, launch).\n" + text)
    rows = []
    for fr in FRACTIONS:
        text = run_child(["churn", "--fraction", fr, "--steps", str(steps), "--repeats", str(repeats)], 300,
                         {"ART_BVH_RESORT_DEN": "0"})
        if text is None:
            return 1
        line = [l for l in text.splitlines() if l.startswith("CHURN")][0].split()
        a = [float(x) for x in line[line.index("relabelled_ms") + 1:line.index("fresh_ms")]]
        b = [float(x) for x in line[line.index("fresh_ms") + 1:]]
        rows.append((fr, int(line[3]), a, b))
    spread = max(max(b) - min(b) for _, _, _, b in rows)
    chosen = None
    with open(os.path.join(out_dir, "collider_churn.txt"), "w") as f:
        f.write("tools/collider_churn_run.py --child churn: config 2's static frame (ms per step) after adds + removes summing to a\n"
                f"fraction of its 4096 colliders without a re-sort (ART_BVH_RESORT_DEN=0), against a fresh bind of the same final scene;\n"
                f"{repeats} x {steps} launches each, alternating. spread: the largest max - min of a fraction's fresh-bind repeats.\n\n")
        f.write("fraction churned  relabelled median [min, max]      fresh median [min, max]           delta     within 2 x spread\n")
        for fr, ch, a, b in rows:
            delta = float(np.median(a) - np.median(b))
            ok = delta <= 2 * spread
            if ok:
                chosen = fr
            f.write(f"{fr:8s} {ch:7d}  {np.median(a):.5f} [{min(a):.5f}, {max(a):.5f}]  {np.median(b):.5f} [{min(b):.5f}, {max(b):.5f}]  "
                    f"{delta:+.5f}  {'yes' if ok else 'no'}\n")
        f.write(f"\nspread {spread:.5f} ms; the largest fraction within twice the spread: {chosen}\n")
    sys.stdout.write(open(os.path.join(out_dir, "collider_churn.txt")).read())
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["step", "churn"])
    ap.add_argument("--fraction", default="1/8")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.child == "step":
        child_step(a.blocks, min(a.steps, 50))
    elif a.child == "churn":
        child_churn(a.fraction, a.steps, a.repeats)
    else:
        sys.exit(driver(a.out, a.steps, a.repeats))

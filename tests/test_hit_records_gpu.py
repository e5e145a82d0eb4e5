"""One-hit frames of the fused plan: hit records handed from the bounce-0 cast to the echo and muffle waves.

The cast's epilogue (fold_path<true>, csrc/art_trace_nearest.hpp) stores for every ray slot of a 64-ray
group its hit record (echo distance and half, offset hit point, accumulator base) or a no-record
marker, and the hit's provisional echo half or a miss's 0 in the fan block; the echo waves of
echo_muffle_kernel start from the records and store only a blocked echo's 0, the muffle waves read
the hit records alone.

Every case runs the fused plan (asserted) on outputs pre-filled with 0xA5 and compares every output
with the oracle byte for byte; each asserts on the oracle's output alone that it holds what its name
says. The shapes are the smallest at which the handoff can go wrong: ray counts that leave a fan's
last 64-ray group full, nearly empty or absent, group counts on both XCD mappings of the launch
(multiples of 8 and not), target counts on both muffle placements, frames after frames on one
context, fan chunks, and every cast instantiation the plan launches (logging, plain, OBB, TAB,
counting). The blocked-echo cases run at both settings of ART_REPLAY_DEAL: the shipped one in this
process, the other one in a child process on a library built with tools/build_variant.sh (a module
fixture; the only case here that compiles or starts a process, because the other setting exists only
as a compile-time variant).
"""
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of test_blocked_echoes_other_dealing
    sys.path.insert(0, os.path.join(ROOT, "audio-raytracer_amd"))

import numpy as np
import pytest

import art
from art import abi
import oracle
from test_broadphase_gpu import _targets_scene
from test_echo_replay_gpu import (all_miss_scene, dirs_of, grazing_scene, hit_mask, inside_scene, params_one_hit)
from test_plan_matrix_gpu import check_equal, stale_outputs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hit_records_exec_counts.json")
_REF = {}


def oracle_ref(key, scene, org, params=None):
    """The oracle's outputs (hit results included) for a case, computed once and left unchanged."""
    if key not in _REF:
        ref = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, True, False)
        oracle.run(scene, params or params_one_hit(), org, ref, threads=8)
        _REF[key] = ref
    return _REF[key]


def run_fused(ctx, scene, org, params=None, flags=0):
    """The frame without hit outputs on stale outputs: (outputs, plan, (replayed, traversed))."""
    out = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, False, False)
    ctx.set_flags(flags)
    try:
        ctx.run(art.Frame(scene, params or params_one_hit(), org, out))
        plan, decided = ctx.debug_last_plan(), ctx.debug_echo_decided()
    finally:
        ctx.set_flags(0)
    assert plan & abi.ART_PLAN_FUSED, abi.plan_names(plan)
    return out, plan, decided


def echo_bits(o):
    return np.asarray(o.echo).view(np.uint16)


def synth_scene(ci, S, R, colliders, seed=None):
    scene, org, _ = art.synth(art.CONFIGS[ci], S=S, R=R, C_scale=colliders / 4096, seed=seed)
    return scene, org


# ---- partial and padded groups: 1, 3, 8 | 2, 6, 16 groups; R = 65 leaves one ray in a fan's last group
@pytest.mark.parametrize("S", [1, 3, 8])
@pytest.mark.parametrize("R", [5, 64, 65, 100])
def test_partial_groups(ctx, R, S):
    scene, org = synth_scene(2, S, R, 64, seed=4100 + R)
    assert scene.C <= 64 and scene.obbs.size == 0
    ref = oracle_ref(("groups", R, S), scene, org)
    hit = hit_mask(ref)
    assert hit.any() and not hit.all() and (echo_bits(ref) != 0).any() and (ref.muffle != 0).any()
    out, plan, (rep, trav) = run_fused(ctx, scene, org)
    assert not plan & (abi.ART_PLAN_OBB | abi.ART_PLAN_TAB | abi.ART_PLAN_EX), abi.plan_names(plan)
    assert np.array_equal(echo_bits(out), echo_bits(ref))
    check_equal(out, ref, f"R={R} S={S}")
    assert rep + trav == int(hit.sum())  # every record is decided once, no padded slot is


def zero_distance_scene():
    """test_echo_replay_gpu's inside scene (fan 0 inside an AABB, fan 1 inside a sphere) with the
    infinite-direction ray added, and two more fans whose origins lie on the room's face x = -3 and on
    the ball's surface: their inward rays hit at distance 0."""
    sc, org, _ = inside_scene()
    bits = np.concatenate([sc.dirs.reshape(-1, 3), dirs_of([[np.inf, 0, 0]])[0]])
    scene = art.Scene(dirs=bits, targets=sc.targets, spheres=sc.spheres, aabbs=sc.aabbs)
    return scene, np.concatenate([org, np.array([[-3, 0.25, -0.5], [8, 0, 0]], np.float32)])


def test_zero_distance_winners(ctx):
    scene, org = zero_distance_scene()
    ref = oracle_ref("zero", scene, org)
    hit = hit_mask(ref).reshape(4, -1)
    hp = np.asarray(ref.hit_points).view(np.float16).astype(np.float32).reshape(4, scene.R, 3)
    at_origin = (hp == org[:, None, :]).all(2) & hit
    assert at_origin[2].any() and at_origin[3].any(), "no hit at distance 0 on the box face / the sphere surface"
    ids = np.asarray(ref.hit_ids).reshape(4, -1)
    assert (ids[2][at_origin[2]] >> 30 == 1).all() and (ids[3][at_origin[3]] >> 30 == 3).all()  # a box, a sphere
    assert hit[:, -1].all() and np.isnan(hp[:, -1, 0]).all()  # the infinite ray: a hit at 0 * inf
    assert hit[0].all() and hit[1].all() and (echo_bits(ref)[:2] != 0).any()  # the fans inside a collider
    out, _, (rep, trav) = run_fused(ctx, scene, org)
    assert np.array_equal(echo_bits(out), echo_bits(ref))
    check_equal(out, ref, "zero-distance winners")
    assert rep + trav == int(hit.sum()) and trav >= 4  # (the infinite rays keep the traversal)


HIT_ORIGINS = np.array([[60, 50, 40], [65, 50, 40]], np.float32)  # beyond the all-miss scene's colliders


def test_all_miss_frame(ctx):
    scene, org, _ = all_miss_scene()
    ref = oracle_ref("all-miss", scene, org)
    assert not hit_mask(ref).any() and not echo_bits(ref).any() and not ref.muffle.any()
    out, _, decided = run_fused(ctx, scene, org)
    assert not echo_bits(out).any() and not out.muffle.any()
    check_equal(out, ref, "all-miss")
    assert decided == (0, 0)


def test_frame_after_frame(ctx):
    """Hits, then an all-miss frame of the same scene from other origins, then the hits again, on one
    context: no record and no echo half of a frame survives into the next."""
    scene, miss_org, _ = all_miss_scene()
    hit_ref, miss_ref = oracle_ref("faf-hit", scene, HIT_ORIGINS), oracle_ref("all-miss", scene, miss_org)
    n = int(hit_mask(hit_ref).sum())
    assert n > 0 and (echo_bits(hit_ref) != 0).any() and hit_ref.muffle.any()
    assert not hit_mask(miss_ref).any()
    for k, (org, ref) in enumerate([(HIT_ORIGINS, hit_ref), (miss_org, miss_ref), (HIT_ORIGINS, hit_ref)]):
        out, _, (rep, trav) = run_fused(ctx, scene, org)
        check_equal(out, ref, f"frame {k + 1}")
        assert rep + trav == (n if k != 1 else 0)


@pytest.mark.parametrize("T", [1, 3, 4, 5])
def test_targets_and_muffle_cutoff(ctx, T):
    """T targets (the muffle waves' two placements: 8 % T == 0 or not); max_muffle_hit_distance 25 cuts
    off some (ray, target) pairs and keeps others."""
    scene, org, _ = _targets_scene(2, 3, 100, 64 / 4096, T, seed=200 + T)
    assert scene.T == T and scene.obbs.size == 0
    uncut = oracle_ref(("targets", T), scene, org)
    p = params_one_hit()
    p.max_muffle_hit_distance = 25.0
    cut = oracle_ref(("targets-cut", T), scene, org, p)
    mu, mc = uncut.muffle.astype(np.int64), cut.muffle.astype(np.int64)
    assert (mc <= mu).all() and mc.sum() < mu.sum() and mc.sum() > 0, (mu, mc)
    for params, ref, what in ((None, uncut, "uncut"), (p, cut, "cut")):
        out, _, _ = run_fused(ctx, scene, org, params)
        check_equal(out, ref, f"T={T} {what}")


def test_fan_chunks(ctx, monkeypatch):
    scene, org = synth_scene(2, 8, 100, 256, seed=4300)
    ref = oracle_ref("chunks", scene, org)
    assert hit_mask(ref).any() and (echo_bits(ref) != 0).any() and ref.muffle.any()
    whole, plan, decided = run_fused(ctx, scene, org)
    assert not plan & abi.ART_PLAN_CHUNKED
    check_equal(whole, ref, "unchunked")
    monkeypatch.setenv("ART_FAST_CHUNK_FANS", "3")
    out, plan, chunked = run_fused(ctx, scene, org)
    assert plan & abi.ART_PLAN_CHUNKED
    check_equal(out, whole, "chunked against unchunked")
    check_equal(out, ref, "chunked")
    assert chunked == decided and sum(decided) == int(hit_mask(ref).sum())


# ---- every cast instantiation of the fused plan: logging (OBB-free), plain OBB, TAB, and the counting ones
COUNT_SCENES = {"noobb": (2, 8, 64, 4400), "obb": (3, 8, 64, 4401), "obb-tab": (3, 8, 256, 4402)}
COUNT_FIELDS = ("sphere", "aabb", "obb", "cull_box", "cell_entries")
# The kernels whose executed tests are a function of the frame alone: the cast and the echo waves.
# The muffle waves' exact tests and scanned entries also depend on the order of equal-key entries in
# the direction-cell lists, which the list build's atomics set anew for every context: three
# processes of the commit before the records counted 1420 / 1425 / 1414 AABB tests on the OBB-free
# scene and 11818 / 11869 / 11960 list entries on the TAB scene (every nearest and echo count equal),
# so no build can match a recorded muffle count; the muffle waves' inputs are checked through the
# muffle outputs, byte for byte.
COUNT_KERNELS = ("nearest", "echo")


def count_scene(name):
    ci, S, R, seed = COUNT_SCENES[name]
    scene, org = synth_scene(ci, S, R, 256, seed=seed)
    assert 250 <= scene.C <= 260 and (scene.obbs.size > 0) == (ci == 3)
    return scene, org


def executed_counts(ctx, scene, org):
    """The frame with ART_CTX_COUNT_EXECUTED: (outputs, plan, the rays cast and COUNT_KERNELS' executed tests)."""
    ctx.set_flags(abi.ART_CTX_COUNT_EXECUTED)
    ctx.executed_counts()  # reset
    out, plan, decided = run_fused(ctx, scene, org, flags=abi.ART_CTX_COUNT_EXECUTED)
    ctx.set_flags(abi.ART_CTX_COUNT_EXECUTED)
    try:
        ex = ctx.executed_counts()
    finally:
        ctx.set_flags(0)
    assert decided == (0, 0)
    assert ex["by_kernel"]["muffle"]["cell_entries"] > 0
    counts = {"bounce_rays": ex["bounce_rays"][:2],
              "by_kernel": {k: {f: ex["by_kernel"][k][f] for f in COUNT_FIELDS} for k in COUNT_KERNELS}}
    return out, plan, counts


@pytest.mark.parametrize("name", list(COUNT_SCENES))
def test_cast_instantiations(ctx, name):
    scene, org = count_scene(name)
    ref = oracle_ref(("count", name), scene, org)
    hit = hit_mask(ref)
    assert hit.any() and not hit.all() and (echo_bits(ref) != 0).any() and ref.muffle.any()
    want = (abi.ART_PLAN_OBB if name != "noobb" else 0) | (abi.ART_PLAN_TAB if name == "obb-tab" else 0)
    out, plan, decided = run_fused(ctx, scene, org)
    assert plan & (abi.ART_PLAN_OBB | abi.ART_PLAN_TAB | abi.ART_PLAN_EX) == want, abi.plan_names(plan)
    check_equal(out, ref, name)
    assert (sum(decided) == int(hit.sum())) if name == "noobb" else decided == (0, 0)
    out, plan, counts = executed_counts(ctx, scene, org)
    assert plan & (abi.ART_PLAN_OBB | abi.ART_PLAN_TAB | abi.ART_PLAN_EX) == want | abi.ART_PLAN_EX, abi.plan_names(plan)
    check_equal(out, ref, f"{name} counting")
    with open(GOLDEN) as f:
        golden = json.load(f)[name]  # taken on the commit before the records (golden/make_hit_records_counts.py)
    assert counts == golden, f"{name}: the cast's or the echo waves' executed tests differ from the rebuild-per-consumer build's"


# ---- blocked echoes: 0 over the cast's provisional half; a returned echo keeps its value
@pytest.mark.parametrize("seed", [156, 191])
def test_blocked_echoes(ctx, seed):
    scene, org, _ = grazing_scene(seed)
    ref = oracle_ref(("grazing", seed), scene, org)
    hit, echo = hit_mask(ref), echo_bits(ref).reshape(-1)
    blocked = hit & (echo == 0)
    assert blocked.any() and (echo[hit] != 0).any()
    out, _, (rep, trav) = run_fused(ctx, scene, org)
    got = echo_bits(out).reshape(-1)
    assert not got[blocked].any(), "a blocked echo kept the cast's provisional half"
    assert np.array_equal(got[hit & ~blocked], echo[hit & ~blocked]) and not got[~hit].any()
    check_equal(out, ref, f"grazing {seed}")
    assert (rep, trav) == (int(hit.sum()), 0)


# ---- ... and at the other setting of ART_REPLAY_DEAL, which stays in the source as the switch's other value
OUTPUT_FIELDS = ("echo", "muffle", "perm", "settings")


@pytest.fixture(scope="module")
def other_dealing_lib():
    """libart.so built with the value of ART_REPLAY_DEAL the source does not ship (tools/build_variant.sh),
    rebuilt only when a source is newer than it."""
    csrc = os.path.join(ROOT, "audio-raytracer_amd", "csrc")
    with open(os.path.join(csrc, "art_trace.hip")) as f:
        shipped = int(re.search(r"^#define ART_REPLAY_DEAL (\d)", f.read(), re.M).group(1))
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    if shutil.which("hipcc", path=env["PATH"]) is None:
        pytest.skip("no hipcc: the other setting of ART_REPLAY_DEAL cannot be built")
    other = 1 - shipped
    lib = os.path.join(ROOT, "variants", f"libart_replay_deal{other}.so")
    srcs = [os.path.join(csrc, n) for n in os.listdir(csrc)] + [os.path.join(ROOT, "tools", "build_variant.sh")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in srcs):
        p = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), f"replay_deal{other}",
                            f"-DART_REPLAY_DEAL={other}"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-4000:]
    return lib, other


def child_main(out_path):
    """Both grazing scenes through the fused plan on the library ART_LIB names: every output and the
    (replayed, traversed) counts, saved for the parent process to check."""
    saved = {}
    with art.Context(1) as ctx:
        for seed in (156, 191):
            scene, org, _ = grazing_scene(seed)
            out, _, decided = run_fused(ctx, scene, org)
            for f in OUTPUT_FIELDS:
                saved[f"{seed}_{f}"] = getattr(out, f)
            saved[f"{seed}_decided"] = np.array(decided, np.int64)
    np.savez(out_path, **saved)


def test_blocked_echoes_other_dealing(other_dealing_lib, tmp_path):
    lib, other = other_dealing_lib
    refs = {}
    for seed in (156, 191):  # (the oracle's share first: nothing starts before the cases hold what they are named for)
        scene, org, _ = grazing_scene(seed)
        ref = oracle_ref(("grazing", seed), scene, org)
        hit, echo = hit_mask(ref), echo_bits(ref).reshape(-1)
        assert (hit & (echo == 0)).any() and (echo[hit] != 0).any()
        refs[seed] = (scene, org, ref, hit, echo)
    path = str(tmp_path / "out.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=dict(os.environ, ART_LIB=lib),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    saved = np.load(path)
    for seed, (scene, org, ref, hit, echo) in refs.items():
        out = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, False, False)
        for f in OUTPUT_FIELDS:
            getattr(out, f)[...] = saved[f"{seed}_{f}"]
        got, blocked = echo_bits(out).reshape(-1), hit & (echo == 0)
        assert not got[blocked].any(), f"ART_REPLAY_DEAL={other}: a blocked echo kept the cast's provisional half"
        assert np.array_equal(got[hit & ~blocked], echo[hit & ~blocked]) and not got[~hit].any()
        check_equal(out, ref, f"grazing {seed}, ART_REPLAY_DEAL={other}")
        assert tuple(saved[f"{seed}_decided"]) == (int(hit.sum()), 0)


if __name__ == "__main__":
    child_main(sys.argv[1])

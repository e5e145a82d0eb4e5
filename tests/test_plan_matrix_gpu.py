"""Every launch plan of the throughput raytrace stage, by name, at the smallest shapes that reach it.

launch_raytrace_fast (csrc/art_trace.hip) picks one of five plans from the frame's shape (FUSED,
HM, SPLIT, FOLD, PER_BOUNCE) and three switches on top (TAB at bounce 0, the OBB or OBB-free
instantiations, the ART_CTX_COUNT_EXECUTED counting instantiations); art_enqueue.cpp adds CHUNKED
when the frame runs as several fan chunks. `expected_plan` restates that dispatch in Python; each
case below
  * runs the frame through the host API (ctx.run) and through art_scene_bind + art_launch_device,
    every output slot pre-filled with 0xA5 (the oracle starts from the same bytes),
  * asserts that art_debug_last_plan reports exactly the plan the restated dispatch expects, and that
    this plan has the bits the case is named for,
  * compares every requested output with the oracle (oracle/art_oracle.c) bit for bit.
No case passes vacuously: the oracle's own output must have a returned echo and a clear muffle ray,
for H > 1 a ray with two hits (six in the H = 32 box), checked before anything runs on the GPU. The
empty scene is the one deliberate exception.
"""
from dataclasses import dataclass
from functools import partial

import numpy as np
import pytest

import art
from art import abi
import oracle
from test_broadphase_gpu import _targets_scene, aabbs, fib_dirs, obbs, spheres
from test_parity_gpu import _diff_report

pytestmark = pytest.mark.gpu

FUSED, HM, SPLIT, FOLD, PER_BOUNCE = (abi.ART_PLAN_FUSED, abi.ART_PLAN_HM, abi.ART_PLAN_SPLIT, abi.ART_PLAN_FOLD,
                                      abi.ART_PLAN_PER_BOUNCE)
TAB, OBB, EX, CHUNKED = abi.ART_PLAN_TAB, abi.ART_PLAN_OBB, abi.ART_PLAN_EX, abi.ART_PLAN_CHUNKED
BASE_PLANS = FUSED | HM | SPLIT | FOLD | PER_BOUNCE

K_TAB_NODES = 1365  # kTabNodes (art_trace_nearest.hpp): BVH nodes the bounce-0 node table holds
K_BVH_LEAF = 4      # kBvhLeaf (art_internal.hpp): colliders per BVH leaf


def bvh_leaf0(n: int) -> int:
    """bvh_layout (art_bvh.hip): nodes above the leaf level of the complete 4-ary tree over n colliders."""
    nleaf = (n + K_BVH_LEAF - 1) // K_BVH_LEAF
    w = 1
    while w < nleaf:
        w *= 4
    return (w - 1) // 3


def expected_plan(scene, params, S, hits, cus, ex=False, chunk=None) -> int:
    """The dispatch of launch_raytrace_fast, restated (plans)."""
    if not params.stages & abi.ART_STAGE_RAYTRACE or S == 0:
        return 0
    R, H, TC = scene.R, params.max_hits_per_ray, params.thread_count
    fans = min(S, chunk) if chunk else S
    groups = fans * ((R + 63) // 64)
    if H == 1:
        if TC == 1 and not hits:
            plan = FUSED
        elif TC == 1 and groups <= cus * 8:
            plan = HM
        else:
            plan = SPLIT
    else:
        plan = FOLD if TC == 1 and not hits else PER_BOUNCE
    has_obb = scene.obbs.size > 0
    tab = has_obb and ((R + 63) // 64) % 4 == 0 and scene.C > 0 and bvh_leaf0(scene.C) * 4 + 1 <= K_TAB_NODES
    return (plan | (TAB if tab else 0) | (OBB if has_obb else 0) | (EX if ex else 0) |
            (CHUNKED if chunk and S > chunk else 0))


@dataclass
class Case:
    scene: art.Scene
    params: art.FrameParams
    org: np.ndarray
    hits: bool = False
    must: int = 0        # plan bits the case exists for
    must_not: int = 0
    min_hits: int = 0    # some ray of the oracle's run has at least this many hits
    empty: bool = False  # the deliberate empty scene: nothing returns


def synth_case(ci, S, R, scale, H, TC=1, hits=False, **kw):
    """A reduced BASELINE config: 2 is OBB-free (spheres + AABBs, raytrace + reduce), 3 is OBBs only
    (+ permeation), 5 is mixed with OBBs (+ permeation and DSP parameters)."""
    scene, org, params = art.synth(art.CONFIGS[ci], S=S, R=R, C_scale=scale)
    params.max_hits_per_ray, params.thread_count = H, TC
    return Case(scene, params, org, hits=hits, min_hits=2 if H > 1 else 0, **kw)


def targets_case(T, H, **kw):
    """T targets spread over a mixed scene, colliders of every kind owned by random targets."""
    sc, org, params = _targets_scene(5, 4, 128, 0.1, T, seed=100 + T)
    params.max_hits_per_ray = H
    return Case(sc, params, org, min_hits=2 if H > 1 else 0, **kw)


def box_case(S, R, H, **kw):
    """A closed box of six walls around the origins with spheres, boxes and OBBs inside: every ray
    keeps bouncing until its life or its hit budget runs out."""
    rng = np.random.default_rng(7)
    walls = aabbs(np.array([[21.0, 0, 0], [-21.0, 0, 0], [0, 21.0, 0], [0, -21.0, 0], [0, 0, 21.0], [0, 0, -21.0]]),
                  np.array([[1.0, 22, 22], [1.0, 22, 22], [22, 1.0, 22], [22, 1.0, 22], [22, 22, 1.0], [22, 22, 1.0]]), rng)
    c = rng.uniform(-16, 16, (60, 3)).astype(np.float32)
    c = c[np.linalg.norm(c, axis=1) > 6][:48]
    n = len(c) // 3
    # (the Fibonacci sphere of one ray divides by R - 1: a fixed direction instead)
    dirs = fib_dirs(R) if R > 1 else np.array([[0.6, 0.64, 0.48]], np.float32).astype(np.float16).view(np.uint16)
    scene = art.Scene(dirs=dirs, targets=np.array([[3, 2, -4], [-9, 5, 6], [8, -7, 1], [-2, -3, 9]], np.float32),
                      spheres=spheres(c[:n], rng.uniform(0.5, 2, n), rng, tid=rng.integers(-1, 4, n)),
                      aabbs=np.concatenate([walls, aabbs(c[n:2 * n], rng.uniform(0.5, 2, (n, 3)), rng,
                                                         tid=rng.integers(-1, 4, n))]),
                      obbs=obbs(c[2 * n:3 * n], rng.uniform(0.5, 2, (n, 3)), rng))
    org = rng.uniform(-3, 3, (S, 3)).astype(np.float32)
    org[0] = 0
    params = art.FrameParams(max_hits_per_ray=H, max_ray_life=1e4, max_muffle_hit_distance=1e5,
                             stages=abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_PERMEATE | abi.ART_STAGE_REDUCE)
    return Case(scene, params, org, **kw)


def empty_case(H, **kw):
    c = synth_case(1, 2, 64, None, H, **kw)
    c.scene.aabbs = c.scene.aabbs[:0]
    c.empty, c.min_hits = True, 0
    return c


def deep_case(H, **kw):
    """122,880 colliders: a 9-level BVH (test_deep_bvh_large_scene's scene; two fans of 64 rays and
    no permeation job keep the brute-force oracle short)."""
    c = synth_case(5, 2, 64, 30, H, **kw)
    c.params.stages, c.params.dsp = abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_REDUCE, None
    assert c.scene.C > 4 * 4 ** 7
    return c


CASES = {}  # name -> builder of the Case (built on first use: `reference`)


def case(name, builder, *args, **kw):
    CASES[name] = partial(builder, *args, **kw)


# ---- the five plans at S = 4, R = 128, on an OBB-free scene (config 2 style) and one with OBBs
# (config 5 style)
for tag, ci, ob in (("noobb", 2, 0), ("obb", 5, OBB)):
    nob = OBB & ~ob
    case(f"fused-{tag}", synth_case, ci, 4, 128, 0.1, 1, must=FUSED | ob, must_not=nob | TAB)
    case(f"hm-{tag}", synth_case, ci, 4, 128, 0.1, 1, hits=True, must=HM | ob, must_not=nob)
    case(f"fold-{tag}", synth_case, ci, 4, 128, 0.1, 3, must=FOLD | ob, must_not=nob | TAB)
    case(f"per_bounce-hits-{tag}", synth_case, ci, 4, 128, 0.1, 3, hits=True, must=PER_BOUNCE | ob, must_not=nob)
    case(f"per_bounce-tc2-{tag}", synth_case, ci, 4, 128, 0.1, 3, TC=2, must=PER_BOUNCE | ob, must_not=nob)
    # split two ways: three batch slots, and hit outputs past cus * 8 ray groups (33 fans x 64
    # groups; ~64 colliders keep the oracle cheap)
    case(f"split-tc3-{tag}", synth_case, ci, 4, 128, 0.1, 1, TC=3, must=SPLIT | ob, must_not=nob)
    case(f"split-tc3-hits-{tag}", synth_case, ci, 4, 128, 0.1, 1, TC=3, hits=True, must=SPLIT | ob, must_not=nob)
    case(f"split-groups-{tag}", synth_case, ci, 33, 4096, 64 / 4096, 1, hits=True, must=SPLIT | ob, must_not=nob)
# ---- TAB: OBB scene, S = 2; R = 256 is four full 64-ray groups, 200 and 193 four groups with a
# ragged last one (8 rays, 1 ray), 128 two groups (no TAB); with and without hit outputs, H = 1, 3
for R in (256, 200, 193, 128):
    for H in (1, 3):
        for hits in (False, True):
            case(f"tab-R{R}-H{H}-{'hits' if hits else 'nohits'}", synth_case, 5, 2, R, 0.1, H, hits=hits,
                 must=OBB | (TAB if R != 128 else 0), must_not=TAB if R == 128 else 0)
# the table's limit: 4096 colliders are a 6-level BVH (leaf0 = 341, 4 * 341 + 1 = 1365 nodes: TAB),
# one more collider is a 7-level BVH (leaf0 = 1365: no TAB)
case("tab-4096-colliders", synth_case, 3, 2, 256, 1.0, 1, must=FUSED | TAB | OBB)
case("tab-4097-colliders", synth_case, 3, 2, 256, 4097 / 4096, 1, must=FUSED | OBB, must_not=TAB)
case("tab-4096-colliders-fold", synth_case, 5, 2, 256, 1.0, 2, must=FOLD | TAB | OBB)
# ---- ray and fan edges on FUSED and FOLD: one fan of 1, 63, 64, 65 rays
for R in (1, 63, 64, 65):
    case(f"edge-fused-R{R}", box_case, 1, R, 1, must=FUSED | OBB, must_not=TAB)
    case(f"edge-fold-R{R}", box_case, 1, R, 3, must=FOLD | OBB, must_not=TAB, min_hits=2)
# ---- bounce depth on FOLD (32 is the limit kLiveCounters and the frame check allow), target count
for H in (2, 5):
    case(f"fold-H{H}", synth_case, 5, 4, 128, 0.1, H, must=FOLD | OBB)
case("fold-H32-box", box_case, 2, 64, 32, must=FOLD | OBB, min_hits=6)
for T in (1, 9, 64, 256):
    case(f"fused-T{T}", targets_case, T, 1, must=FUSED | OBB)
    case(f"fold-T{T}", targets_case, T, 3, must=FOLD | OBB)
# ---- no colliders at all, and a 9-level BVH
case("fused-empty", empty_case, 1, must=FUSED, must_not=OBB | TAB)
case("fold-empty", empty_case, 5, must=FOLD, must_not=OBB | TAB)
case("fused-deep-bvh", deep_case, 1, must=FUSED | OBB, must_not=TAB)
# ---- seven fans (test_forced_chunks runs them as chunks of 3, 3 and 1)
case("seven-fans-H1", synth_case, 5, 7, 128, 0.1, 1, must=FUSED | OBB, must_not=CHUNKED)
case("seven-fans-H3", synth_case, 5, 7, 128, 0.1, 3, must=FOLD | OBB, must_not=CHUNKED)

_BUILT = {}


def stale_outputs(S, R, H, T, TC, hits, dsp):
    """FanOutputs with every byte 0xA5: no slot starts from a stale zero."""
    o = art.FanOutputs(S, R, H, T, TC, hits=hits, dsp=dsp)
    for v in o.__dict__.values():
        if isinstance(v, np.ndarray):
            v.view(np.uint8)[...] = 0xA5
    return o


def reference(name):
    """The case and the oracle's outputs for it (hit results included), computed once per case and
    left unchanged; asserts on the oracle's output alone that the case is not vacuous."""
    if name in _BUILT:
        return _BUILT[name]
    case = CASES[name]()
    sc, p = case.scene, case.params
    S = case.org.shape[0]
    ref = stale_outputs(S, sc.R, p.max_hits_per_ray, sc.T, p.thread_count, True, p.dsp is not None)
    oracle.run(sc, p, case.org, ref, threads=16)
    if case.empty:
        assert not ref.echo.any() and not ref.muffle.any()
    else:
        assert (ref.echo != 0).any(), f"{name}: the oracle returns no echo"
        assert (ref.muffle != 0).any(), f"{name}: the oracle sees no target"
        assert int(ref.hit_counts.max()) >= case.min_hits, f"{name}: at most {int(ref.hit_counts.max())} hits per ray"
    _BUILT[name] = (case, ref)
    return case, ref


def check_equal(got, ref, what):
    eq = got.equal(ref)
    assert all(eq.values()), f"{what}: {eq}\n{_diff_report(got, ref)}"


def run_host(ctx, case, flags=0):
    sc, p = case.scene, case.params
    out = stale_outputs(case.org.shape[0], sc.R, p.max_hits_per_ray, sc.T, p.thread_count, case.hits, p.dsp is not None)
    ctx.set_flags(flags)
    try:
        ctx.run(art.Frame(sc, p, case.org, out))
    finally:
        ctx.set_flags(0)
    return out, ctx.debug_last_plan()


def run_device(ctx, case, flags=0):
    """art_scene_bind + art_launch_device on a torch-allocated block of 0xA5 bytes."""
    import torch
    sc, p = case.scene, case.params
    S, R, H, T, TC, dsp = case.org.shape[0], sc.R, p.max_hits_per_ray, sc.T, p.thread_count, p.dsp is not None
    oflags = abi.ART_OUT_HIT_RESULTS if case.hits else 0
    fr = art.Frame(sc, p, case.org, art.FanOutputs(S, R, H, T, TC, hits=case.hits, dsp=dsp))
    lay = art.fan_layout(fr, oflags)
    ctx.set_flags(flags)
    try:
        ctx.bind(fr)
        d_org = torch.from_numpy(np.ascontiguousarray(case.org)).cuda()
        d_blk = torch.full((S * lay["stride"],), 0xA5, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream()
        ctx.launch_device(d_org.data_ptr(), S, d_blk.data_ptr(), oflags, st.cuda_stream)
        plan = ctx.debug_last_plan()  # a host-side decision: read before the frame has finished
        st.synchronize()
    finally:
        ctx.set_flags(0)
    return art.unpack_block(d_blk.cpu().numpy(), lay, S, R, H, T, TC, hits=case.hits, dsp=dsp), plan


@pytest.fixture(scope="module")
def cus():
    torch = pytest.importorskip("torch")
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_plan(name, case, plan, want):
    assert plan == want, f"{name}: ran {abi.plan_names(plan)}, the dispatch mirror expects {abi.plan_names(want)}"
    assert bin(plan & BASE_PLANS).count("1") == 1, abi.plan_names(plan)
    assert plan & case.must == case.must and not plan & case.must_not, \
        f"{name}: ran {abi.plan_names(plan)}; needs {abi.plan_names(case.must)}, without {abi.plan_names(case.must_not)}"


@pytest.mark.parametrize("name", list(CASES))
def test_plan_matrix(ctx, cus, name):
    case, ref = reference(name)
    S = case.org.shape[0]
    want = expected_plan(case.scene, case.params, S, case.hits, cus)
    out, plan = run_host(ctx, case)
    check_plan(name, case, plan, want)
    check_equal(out, ref, f"{name} host API ({abi.plan_names(plan)})")
    got, plan = run_device(ctx, case)
    check_plan(name, case, plan, want)
    check_equal(got, ref, f"{name} device path ({abi.plan_names(plan)})")


def test_tab_limit_is_the_bvh_level():
    """The collider counts of the TAB limit cases come from the BVH layout, not from a guess."""
    assert bvh_leaf0(4096) * 4 + 1 == K_TAB_NODES and bvh_leaf0(4097) * 4 + 1 > K_TAB_NODES
    assert reference("tab-4096-colliders")[0].scene.C == 4096 and reference("tab-4097-colliders")[0].scene.C == 4097
    assert reference("tab-4096-colliders-fold")[0].scene.C == 4096


EX_CASES = [("fused-noobb", FUSED), ("fused-obb", FUSED | OBB), ("fold-noobb", FOLD), ("fold-obb", FOLD | OBB),
            ("tab-R200-H1-nohits", FUSED | TAB | OBB), ("tab-R193-H3-nohits", FOLD | TAB | OBB),
            ("tab-R256-H3-hits", PER_BOUNCE | TAB | OBB)]


@pytest.mark.parametrize("name,bits", EX_CASES, ids=[n for n, _ in EX_CASES])
def test_counting_instantiations(ctx, cus, name, bits):
    """ART_CTX_COUNT_EXECUTED (bench.py --full's roofline) runs the EX instantiations of the same
    plans: the outputs stay equal to the oracle's, bounce_rays obeys test_exec_counts_gpu.py's bounds
    (#(hits > k) <= bounce_rays[k] <= #(hits >= k), hit counts from the oracle) and the per-kernel
    split sums to the totals."""
    case, ref = reference(name)
    S, H = case.org.shape[0], case.params.max_hits_per_ray
    want = expected_plan(case.scene, case.params, S, case.hits, cus, ex=True)
    assert want == bits | EX
    hc = ref.hit_counts.astype(np.int64).ravel()
    for runner in (run_host, run_device):
        ctx.set_flags(abi.ART_CTX_COUNT_EXECUTED)
        ctx.executed_counts()  # reset
        got, plan = runner(ctx, case, flags=abi.ART_CTX_COUNT_EXECUTED)
        ex = ctx.executed_counts()
        assert plan == want, (abi.plan_names(plan), abi.plan_names(want))
        check_equal(got, ref, f"{name} {runner.__name__} ({abi.plan_names(plan)})")
        assert ex["launches"] == 1
        br = ex["bounce_rays"]
        assert br[0] == S * case.scene.R
        for k in range(H):
            assert int((hc > k).sum()) <= br[k] <= int((hc >= k).sum()), (k, br[:H])
        assert all(v == 0 for v in br[H:])
        assert ex["sphere"] + ex["aabb"] + ex["obb"] > 0 and ex["cull_box"] > 0
        for f in ("sphere", "aabb", "obb", "cull_box", "cell_entries"):
            assert sum(ex["by_kernel"][k][f] for k in abi.EXEC_KERNELS) == ex[f], f


@pytest.mark.parametrize("H,bits", [(1, FUSED), (3, FOLD)], ids=["fused", "fold"])
def test_forced_chunks(ctx, cus, monkeypatch, H, bits):
    """ART_FAST_CHUNK_FANS=3 runs 7 fans as chunks of 3, 3 and 1: CHUNKED is reported, and the bytes
    equal the unchunked run's and the oracle's (per-chunk accumulator offsets, pair counter reset)."""
    name = f"seven-fans-H{H}"
    case, ref = reference(name)
    whole, plan = run_host(ctx, case)
    assert plan == expected_plan(case.scene, case.params, 7, False, cus) == bits | OBB
    check_equal(whole, ref, f"{name} unchunked")
    monkeypatch.setenv("ART_FAST_CHUNK_FANS", "3")
    want = expected_plan(case.scene, case.params, 7, False, cus, chunk=3)
    assert want == bits | OBB | CHUNKED
    for runner in (run_host, run_device):
        got, plan = runner(ctx, case)
        assert plan == want, (abi.plan_names(plan), abi.plan_names(want))
        check_equal(got, whole, f"{name} {runner.__name__} chunked against unchunked")
        check_equal(got, ref, f"{name} {runner.__name__} chunked")

"""GPU parity of the traversals with the per-ray cap of the BVH node margins (the
capped node margin).

Every traversal but the counting ones widens a BVH node by min(fma(factor, om, fscale), cap), cap =
`node_margin_cap` (art_frame_math.hpp; tests/test_node_margin_cpu.py checks the bound itself). That is
exact only if every hit the reference's float sphere test reports outside the true sphere still enters the
narrower boxes, so the cases put spheres where the float test reports such hits and compare every output
with the oracle byte for byte.

The scene (`graze_scene`): fan f starts at (0, 0, z_f) and shoots 32 "axis" rays (0.25, dy_k, 0) whose
heights at distance x grow geometrically with k; on its row sits one sphere of radius r_f whose top
touches the x axis at distance x_f, so ray k clears the true sphere by delta_k = x_f dy_k / 0.25: offsets
from below 1/16 slack(r_f, x_f) up, past 2 slack on the rows up to 300. The radii are 0.25, 0.5, 1.0 and
2.5 at |oc| = 150 and 300, and 0.25 again at 600 and 1025. Each sphere shares its leaf with three small
boxes inside it alone (checked against the host reference of the build), so the leaf's box is the sphere's
and inner nodes test it. The rays that report no hit on the sphere end on a wall at x = 1044; 32 more rays
spread around +x. The scene's extent is chosen by two conditions, both asserted from
art_debug_node_margin_cap on every case (`check_reference`):

  * the cap binds on the far row's leaf: S_root = 1084 gives D = 1100 for its rays, below the 1290 at
    which the r-aware form at r_min = 0.25 meets the square-root form, so cap = 3.75 against the leaf's
    uncapped 4e-3 (scale + om) = 4.2 (the logging cast: 5.2 against 5.6). The nearer rows' leaves have a
    smaller scale and keep their own margin, below the ray's cap;
  * the negative control bites on that row: the float test reports hits up to 0.20 outside the sphere at
    |oc| = 1025 (the distance scanned with the float32 restatement: for these near-axis rays the test
    reports hits out to about 1.2e-4 |oc| below |oc| = 1024, just at the cap's floor 1.01e-4 D, and twice
    as far above it), against the floor's 0.11.

What the cases cannot show, because the float test's error on these rays stays some 15 times below the
proven bound: a sphere term up to about 15 times too small. The control (the floor alone, the sphere term
0) is what separates them from a cap that is too narrow. In the logging cast the reach term, which keeps
its full factor, alone exceeds every offset (1.4 units here), so no build with a narrower cap could change
the logging case's outputs; the case checks parity and that its cap binds.

Plans: the fused logging cast (the sphere hits up to 300 lie inside the replay's reach and are replayed),
fused with one OBB (plain cast, echo traversal), TAB (R = 256 with the OBB), FOLD (H = 3), hit outputs on
with H = 3 (per-bounce). Work sharing: fans of 16 rays, 13 that miss the root box and 3 axis rays, one wave
each (the thieves traverse the home ray's subtrees with the home ray's cap; all rays of a bounce-0 wave
share one origin, so thief and home caps are equal here). Resident store: a sphere shrunk below the bound
r_min, and a collider moved far out and back (S_root grows and shrinks without a rebind): parity after
set + sync, and the values the next frame reads through the debug entries. Negative control: the OBB-free
cases on a library built with -DART_NODE_CAP_SLACK_SCALE=0 (the cap's sphere term 0, its floor alone) in a
child process; at least one must differ from the oracle.
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the child process of test_negative_control
    sys.path.insert(0, os.path.join(ROOT, "audio-raytracer_amd"))

import numpy as np
import pytest

import art
from art import abi
from art.colliders import ColliderStore, resident_frame
import bvh_ref
import oracle
from test_broadphase_gpu import aabbs, f16bits, obbs, spheres
from test_plan_matrix_gpu import check_equal, stale_outputs
from test_sphere_slack_cpu import ray_sphere32
from test_sphere_slack_gpu import slack

pytestmark = pytest.mark.gpu

R = 64
N_AXIS = 32
WALL_X = 1044.0
ROWS = [(0.25, 150.0), (0.5, 150.0), (1.0, 150.0), (2.5, 150.0), (0.25, 300.0), (2.5, 300.0), (0.25, 600.0), (0.25, 1025.0)]
ROW_Z = [6.0 * f - 21.0 for f in range(8)]
TARGETS = np.array([[3, 2, -4], [-9, 5, 6], [8, -7, 1], [-2, -3, 9]], np.float32)
K_BOX, K_SPHERE = 1e-4, 4e-3   # kCullBox, kCullSphere
OUTPUT_FIELDS = ("echo", "muffle")
_BUILT = {}


def half32(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def axis_dy():
    """The axis rays' y components as the kernels read them: 5e-4 * 2^(-k/3) in half precision."""
    return half32(5e-4 * 2.0 ** (-np.arange(N_AXIS) / 3.0))


def graze_dirs(n_rays, seed):
    rng = np.random.default_rng(seed)
    ax = np.stack([np.full(N_AXIS, 0.25), axis_dy(), np.zeros(N_AXIS)], 1)
    sp = np.concatenate([np.ones((n_rays - N_AXIS, 1)), rng.uniform(-0.005, 0.005, (n_rays - N_AXIS, 2))], axis=1)
    sp /= np.linalg.norm(sp, axis=1, keepdims=True)
    return f16bits(np.concatenate([ax, sp])).reshape(-1, 3)


def graze_scene(obb=False, n_rays=R, dirs=None):
    """(scene, origins). Sites of four colliders (one leaf each): the eight row spheres and the wall, each
    with three small boxes inside it; optionally an OBB beside the rows."""
    rng = np.random.default_rng(4242)
    sc, sr, bc, bh = [], [], [], []
    for (r, x), z in zip(ROWS, ROW_Z):
        sc.append([x, -r, z]), sr.append(r)
        bc += [[x, -r, z]] * 3
        bh += [[r / 8, r / 8, r / 8]] * 3
    bc.append([WALL_X + 1.0, 0, 0]), bh.append([1.0, 8.0, 30.0])
    bc += [[WALL_X + 1.0, 0, 0]] * 3
    bh += [[0.25, 0.25, 0.25]] * 3
    kw = {}
    if obb:
        kw["obbs"] = obbs(np.array([[100.0, 12.0, 0.0]]), np.array([[1.0, 1.5, 0.5]]), rng)
        bc += [[100.0, 12.0, 0.0]] * 3
        bh += [[0.125, 0.125, 0.125]] * 3
    scene = art.Scene(dirs=graze_dirs(n_rays, 4243) if dirs is None else dirs, targets=TARGETS,
                      spheres=spheres(np.array(sc, np.float32), np.array(sr, np.float32), rng),
                      aabbs=aabbs(np.array(bc, np.float32), np.array(bh, np.float32), rng), **kw)
    # (origins off the lattice of the half-precision centres, so that the float test's operands round)
    org = np.stack([np.full(8, 0.0123), np.zeros(8), np.array(ROW_Z) + 0.0071], 1).astype(np.float32)
    assert scene.C <= 110
    return scene, org


def params(H=1):
    return art.FrameParams(max_hits_per_ray=H, max_ray_life=1e4, max_muffle_hit_distance=1e5,
                           stages=abi.ART_STAGE_RAYTRACE | abi.ART_STAGE_REDUCE)


def s_root_of(scene):
    """Sum over the axes of max(|lo|, |hi|) of the union of the sphere and AABB bounds (OBB-free scenes)."""
    cull = bvh_ref.cull_bounds(scene.spheres, scene.aabbs)
    return float(np.maximum(np.abs(cull["lo"].min(0)), np.abs(cull["hi"].max(0))).sum())


def cap_of(r_min, s_root, om, has_obb=False, reach=0.0):
    import ctypes as C
    out = C.c_float()
    rc = art.load_library().art_debug_node_margin_cap(None, C.c_float(r_min), C.c_float(s_root), C.c_float(om), int(has_obb),
                                                      C.c_float(reach), C.byref(out), None)
    assert rc == 0
    return float(out.value)


CASES = {
    "fused-log": dict(H=1, hits=False, want=abi.ART_PLAN_FUSED, wont=abi.ART_PLAN_OBB | abi.ART_PLAN_EX),
    "fused-obb": dict(obb=True, H=1, hits=False, want=abi.ART_PLAN_FUSED | abi.ART_PLAN_OBB, wont=abi.ART_PLAN_TAB | abi.ART_PLAN_EX),
    "tab": dict(obb=True, n_rays=256, H=1, hits=False, want=abi.ART_PLAN_TAB | abi.ART_PLAN_OBB, wont=abi.ART_PLAN_EX),
    "fold": dict(H=3, hits=False, want=abi.ART_PLAN_FOLD, wont=abi.ART_PLAN_OBB | abi.ART_PLAN_EX),
    "per-bounce": dict(H=3, hits=True, want=abi.ART_PLAN_PER_BOUNCE, wont=abi.ART_PLAN_OBB | abi.ART_PLAN_EX),
}
CONTROL_CASES = ["fold", "per-bounce"]   # OBB-free plain casts: an OBB's floor (1e-3 D) and the logging cast's reach term exceed every offset


def reference(name):
    """(scene, origins, oracle outputs with hit results) of a case, built once and left unchanged."""
    if name not in _BUILT:
        c = CASES[name]
        scene, org = graze_scene(obb=c.get("obb", False), n_rays=c.get("n_rays", R))
        ref = stale_outputs(org.shape[0], scene.R, c["H"], scene.T, 1, True, False)
        oracle.run(scene, params(c["H"]), org, ref, threads=8)
        _BUILT[name] = (scene, org, ref)
    return _BUILT[name]


def first_hit_x(ref, S, n_rays, H):
    hp = np.asarray(ref.hit_points).view(np.float16).astype(np.float32).reshape(S, n_rays, H, -1)
    return hp[:, :, 0, 0], np.asarray(ref.hit_counts).reshape(S, n_rays) > 0


def restated_axis_hits(scene, org):
    """The float32 restatement of the reference's sphere test for every (fan, axis ray) on the fan's row
    sphere: (reported hit, the ray's clearance delta of the true sphere in float64)."""
    d = scene.dirs.view(np.float16).astype(np.float32).reshape(-1, 3)[:N_AXIS]
    hit = np.zeros((8, N_AXIS), bool)
    delta = np.zeros((8, N_AXIS))
    for f, ((r, x), z) in enumerate(zip(ROWS, ROW_Z)):
        o = [np.full(N_AXIS, org[f, i], np.float32) for i in range(3)]
        c = [np.full(N_AXIS, v, np.float32) for v in (x, -r, z)]
        h, dist = ray_sphere32(o, [d[:, i] for i in range(3)], c, np.full(N_AXIS, r, np.float32))
        hit[f] = h & np.isfinite(dist) & (dist >= 0)
        dd = d.astype(np.float64)
        oc = np.array([x, -r, z]) - org[f].astype(np.float64)
        perp = np.linalg.norm(np.cross(dd, oc[None, :]), axis=1) / np.linalg.norm(dd, axis=1)
        delta[f] = perp - r
    return hit, delta


def check_reference(name, scene, org, ref):
    """What the case is named for, on the oracle's output and the float32 restatement alone."""
    c = CASES[name]
    S, n_rays, H = org.shape[0], scene.R, c["H"]
    x0, has_hit = first_hit_x(ref, S, n_rays, H)
    assert has_hit[:, :N_AXIS].all()             # an axis ray ends on its row's sphere or on the wall
    rest_hit, delta = restated_axis_hits(scene, org)
    assert (delta > 0).all()                     # in exact arithmetic every axis ray clears its sphere
    on_sphere = x0[:, :N_AXIS] < WALL_X - 10.0
    assert np.array_equal(on_sphere, rest_hit), "the restatement and the oracle disagree on the grazing hits"
    for f, (r, x) in enumerate(ROWS):            # both verdicts on every row, offsets on both sides of the slack
        s = slack(r, x)
        assert on_sphere[f].any() and (~on_sphere[f]).any(), (f, r, x)
        assert delta[f].min() < s / 16, (f, delta[f].min(), s)
        # (the helper's value grows with |oc|^2: past 300 the offsets stop short of twice its value, and both
        # verdicts above show that they straddle what the float test does report)
        assert x > 300.0 or delta[f].max() > 2 * s, (f, delta[f].max(), s)
        # every reported hit lies within the lemma's bound at the sphere's own radius (half the helper's value)
        assert (delta[f][on_sphere[f]] < slack(r, 1.001 * (x + r)) / 2).all(), (f, delta[f][on_sphere[f]].max())
    # The cap binds on the far row's leaf (its box is the sphere's: scale = |c|_1 + r), for the operand of the
    # case's bounce-0 cast: |O|_1, or the logging cast's b + T with its cap(b) + kCullSphere T.
    far = len(ROWS) - 1
    (r, x), z = ROWS[far], ROW_Z[far]
    r_min, s_root, has_obb = 0.25, s_root_of(scene), bool(c.get("obb"))
    scale, om = x + r + abs(z) + r, float(np.abs(org[far]).sum())
    if name == "fused-log":
        cull = bvh_ref.cull_bounds(scene.spheres, scene.aabbs)
        X = 0.3 * float((cull["hi"].max(0) - cull["lo"].min(0)).sum())          # kLogCapFrac * the root's L1 diagonal
        T = min(0.4 * X, 2e-4 * (r_min + X) ** 2 / r_min + 2.8e-2 * X)            # log_margin_om's reach term
        b = 1.05 * om + 4.0 * 0.25                                                # (|d|_1 of an axis ray: 0.25 and a tiny dy)
        cap, m_old = cap_of(r_min, s_root, b, False, T), K_SPHERE * (scale + b + T)
        root_form = K_SPHERE * (s_root + b) + K_SPHERE * T
        assert T < 0.4 * X and (delta[on_sphere] < K_SPHERE * T).all()            # (why no control can bite here)
    else:
        cap, m_old = cap_of(r_min, s_root, om, has_obb), K_SPHERE * (scale + om)
        root_form = K_SPHERE * (s_root + om)
    print(f"{name}: far row cap {cap:.3f} against the uncapped {m_old:.3f}; S_root {s_root:.1f}")
    assert cap < 0.95 * m_old, (cap, m_old)          # the cap narrows this leaf's box
    assert cap < 0.999 * root_form, (cap, root_form)  # and it is the r-aware form, not the square-root form at D
    if not has_obb and name != "fused-log":
        # some reported hit clears its sphere by more than the cap's floor (what the control build is left with)
        floor = 1.01 * K_BOX * (s_root + np.abs(org).sum(1)[:, None])
        assert (on_sphere & (delta > 1.3 * floor)).any(), "no reported hit lies clearly outside the cap's floor"
    if H == 1:
        echo = np.asarray(ref.echo).view(np.uint16).reshape(S, n_rays)
        assert (echo[:, :N_AXIS] != 0).any()


def run_case(ctx, name):
    c = CASES[name]
    scene, org, _ = reference(name)
    out = stale_outputs(org.shape[0], scene.R, c["H"], scene.T, 1, c["hits"], False)
    ctx.set_flags(0)
    ctx.run(art.Frame(scene, params(c["H"]), org, out))
    plan = ctx.debug_last_plan()
    assert plan & c["want"] == c["want"] and not plan & c["wont"], abi.plan_names(plan)
    return out, ctx.debug_echo_decided()


def test_sites_are_leaves():
    """Each row sphere's leaf holds the sphere and its three inner boxes alone (host reference of the build)."""
    scene, _ = graze_scene()
    cull = bvh_ref.cull_bounds(scene.spheres, scene.aabbs)
    order = np.asarray(bvh_ref.kd_order(cull["lo"], cull["hi"]))
    ns = scene.spheres.size
    for s in range(8):
        at = int(np.nonzero(order == s)[0][0])
        leaf = order[at - at % 4: at - at % 4 + 4]
        assert sorted(leaf) == sorted([s, ns + 3 * s, ns + 3 * s + 1, ns + 3 * s + 2]), (s, leaf)
        assert (cull["lo"][leaf] >= cull["lo"][s]).all() and (cull["hi"][leaf] <= cull["hi"][s]).all()


@pytest.mark.parametrize("name", list(CASES))
def test_grazing_spheres(ctx, name):
    scene, org, ref = reference(name)
    check_reference(name, scene, org, ref)
    out, (rep, trav) = run_case(ctx, name)
    check_equal(out, ref, name)
    if name == "fused-log":   # the sphere hits of the rows up to 300 lie inside the replay's reach
        x0, _ = first_hit_x(ref, 8, scene.R, 1)
        assert rep >= int((x0[:6, :N_AXIS] < 400.0).sum()) > 0, (rep, trav)


def share_scene():
    """Fans of 16 rays: whatever the direction-coherent order, the fan's one wave holds them all. 13 rays
    point down -x, where nothing lies (they finish after the root's children), 3 are axis rays that
    report grazing hits or pass just outside them: the 13 idle quads take over parts of the 3 traversals."""
    full, org = graze_scene()
    d = full.dirs.reshape(-1, 3)
    rng = np.random.default_rng(99)
    back = np.concatenate([-np.ones((13, 1)), rng.uniform(-0.3, 0.3, (13, 2))], axis=1)
    back /= np.linalg.norm(back, axis=1, keepdims=True)
    dirs = np.concatenate([d[[12, 16, 20]], f16bits(back).reshape(-1, 3)])
    scene, org = graze_scene(dirs=dirs)
    return scene, org


@pytest.mark.parametrize("H", [1, 3])
def test_work_sharing(ctx, H):
    if ("share", H) not in _BUILT:
        scene, org = share_scene()
        ref = stale_outputs(org.shape[0], scene.R, H, scene.T, 1, True, False)
        oracle.run(scene, params(H), org, ref, threads=8)
        _BUILT[("share", H)] = (scene, org, ref)
    scene, org, ref = _BUILT[("share", H)]
    assert scene.R == 16
    x0, has_hit = first_hit_x(ref, 8, 16, H)
    assert has_hit[:, :3].all() and not has_hit[:, 3:].any()
    assert (x0[:, :3] < WALL_X - 10.0).any() and (x0[:, :3] > WALL_X - 10.0).any()   # grazing hits and passes
    out = stale_outputs(8, 16, H, scene.T, 1, False, False)
    ctx.set_flags(0)
    ctx.run(art.Frame(scene, params(H), org, out))
    plan = ctx.debug_last_plan()
    assert plan & (abi.ART_PLAN_FUSED if H == 1 else abi.ART_PLAN_FOLD) and not plan & abi.ART_PLAN_EX, abi.plan_names(plan)
    check_equal(out, ref, f"work sharing H={H}")


def _resident(c, scene, org):
    store = ColliderStore(c)
    for k, arr in ((abi.ART_KIND_SPHERE, scene.spheres), (abi.ART_KIND_AABB, scene.aabbs)):
        for i in range(arr.size):
            store.add(k, arr[i])
    store.sync()
    fr = art.Frame(scene, params(), org, art.FanOutputs(org.shape[0], scene.R, 1, scene.T, 1))
    lay = art.fan_layout(fr)
    c.set_flags(abi.ART_CTX_RESIDENT_COLLIDERS)
    c.bind(resident_frame(fr))
    return store, lay


def _device_frame(c, scene, org, lay):
    import torch
    S = org.shape[0]
    d_org = torch.from_numpy(np.ascontiguousarray(org)).cuda()
    blk = torch.full((S * lay["stride"],), 0xA5, dtype=torch.uint8, device="cuda")
    c.launch_device(d_org.data_ptr(), S, blk.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert c.debug_last_plan() & abi.ART_PLAN_FUSED
    return art.frame.unpack_block(blk.cpu().numpy(), lay, S, scene.R, 1, scene.T, 1)


def _oracle(scene, org):
    ref = stale_outputs(org.shape[0], scene.R, 1, scene.T, 1, False, False)
    oracle.run(scene, params(), org, ref, threads=8)
    return ref


def test_resident_store_shrinks_a_sphere():
    """The row sphere of radius 0.25 at 300 replaced by one of radius 2^-4 with the same top point, through
    set + sync on a bound resident scene: the next frame's caps use the lowered r_min."""
    scene, org, _ = reference("fused-log")
    with art.Context(1) as c:
        store, lay = _resident(c, scene, org)
        assert c.debug_scene_r_min() == 0.25
        edited = scene.spheres.copy()
        r = 2.0 ** -4
        edited["center"][4][1] = f16bits(-r)
        edited["radius"][4] = f16bits(r)
        store.set(abi.ART_KIND_SPHERE, 4, edited[4])
        store.sync()
        assert c.debug_scene_r_min() == r
        got = _device_frame(c, scene, org, lay)
    sc2 = art.Scene(dirs=scene.dirs, targets=scene.targets, spheres=edited, aabbs=scene.aabbs)
    ref = _oracle(sc2, org)
    assert (np.asarray(ref.echo).view(np.uint16) != 0).any()
    check_equal(got, ref, "after the shrinking sync")


def test_resident_store_root_box_grows_and_shrinks():
    """The wall's first inner box moved to x = -8000 and back by set + sync, no rebind: S_root, which the
    caps read from the BVH root on the device, follows both ways, and both frames equal the oracle."""
    scene, org, ref0 = reference("fold")   # (the OBB-free scene without the anchor; here with H = 1)
    far = scene.aabbs.copy()
    wall_box = 8 * 3 + 1                   # the first small box inside the wall
    far["center"][wall_box][0] = f16bits(-8000.0)
    with art.Context(1) as c:
        store, lay = _resident(c, scene, org)
        s0 = c.debug_scene_s_root()
        assert abs(s0 - s_root_of(scene)) <= 1e-3 * s0
        store.set(abi.ART_KIND_AABB, wall_box, far[wall_box])
        store.sync()
        s1 = c.debug_scene_s_root()
        assert s1 > s0 + 2500.0
        got_far = _device_frame(c, scene, org, lay)
        store.set(abi.ART_KIND_AABB, wall_box, scene.aabbs[wall_box])
        store.sync()
        assert c.debug_scene_s_root() == s0
        got_back = _device_frame(c, scene, org, lay)
    check_equal(got_far, _oracle(art.Scene(dirs=scene.dirs, targets=scene.targets, spheres=scene.spheres, aabbs=far), org),
                "with the box far out")
    check_equal(got_back, _oracle(scene, org), "with the box back")


# ---------------------------------------------------------------- negative control
@pytest.fixture(scope="module")
def nodecap0_lib():
    """variants/libart_nodecap0.so, built with -DART_NODE_CAP_SLACK_SCALE=0 (tools/build_variant.sh) unless
    one newer than the sources is there."""
    csrc = os.path.join(ROOT, "audio-raytracer_amd", "csrc")
    env = dict(os.environ, PATH=os.environ.get("PATH", "") + os.pathsep + "/opt/rocm/bin")
    if shutil.which("hipcc", path=env["PATH"]) is None:
        pytest.skip("no hipcc: the variant without the cap's sphere term cannot be built")
    lib = os.path.join(ROOT, "variants", "libart_nodecap0.so")
    srcs = [os.path.join(csrc, n) for n in os.listdir(csrc)] + [os.path.join(ROOT, "tools", "build_variant.sh")]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in srcs):
        p = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), "nodecap0", "-DART_NODE_CAP_SLACK_SCALE=0"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-4000:]
    return lib


def child_main(out_path):
    """The OBB-free cases on the library ART_LIB names: the outputs, saved for the parent process to compare."""
    saved = {}
    with art.Context(1) as ctx:
        for name in CONTROL_CASES:
            out, _ = run_case(ctx, name)
            for f in OUTPUT_FIELDS:
                saved[f"{name}_{f}"] = getattr(out, f)
    np.savez(out_path, **saved)


def test_negative_control(nodecap0_lib, tmp_path):
    refs = {name: reference(name) for name in CONTROL_CASES}
    path = str(tmp_path / "out.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=dict(os.environ, ART_LIB=nodecap0_lib),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    saved = np.load(path)
    differ = []
    for name, (_, _, ref) in refs.items():
        same = all(np.array_equal(np.asarray(getattr(ref, f)).view(np.uint8), np.asarray(saved[f"{name}_{f}"]).view(np.uint8))
                   for f in OUTPUT_FIELDS)
        if not same:
            differ.append(name)
    print("cases that differ from the oracle with the cap's sphere term at 0:", differ)
    assert differ, "no case probes the bound: with ART_NODE_CAP_SLACK_SCALE=0 every one still equals the oracle"


if __name__ == "__main__":
    child_main(sys.argv[1])

"""The host restatement of the BVH build (tests/bvh_ref.py) checked on its own, without a GPU: the
leaf order is a permutation whose segments are kd cells at every level, the top split takes the axis a
float64 evaluation of the surface-area costs takes, and check_tree accepts the reference's own nodes
and reports single perturbed nodes (so the GPU comparisons of test_bvh_structure_gpu.py can fail)."""
import numpy as np
import pytest

import bvh_ref
from bvh_ref import REC, build_nodes, capacity, check_tree, cull_bounds, f32_key, kd_order

SIZES = [1, 4, 5, 17, 65, 513, 4097, 16385]


def scene_bounds(n, kind="random"):
    make = {"random": bvh_ref.random_scene, "ties": bvh_ref.ties_scene, "line": bvh_ref.line_scene,
            "nonfinite": bvh_ref.nonfinite_scene}[kind]
    sph, box, _ = make(n, 100 + n)
    return cull_bounds(sph, box)


_orders = {}


def order_of(n, kind="random"):
    if (n, kind) not in _orders:
        cull = scene_bounds(n, kind)
        _orders[(n, kind)] = (cull, kd_order(cull["lo"], cull["hi"]))
    return _orders[(n, kind)]


def split_segments(n):
    """(first, half, count) of every segment the build splits, level by level."""
    for lg in range(capacity(n).bit_length() - 1, 2, -1):
        seg, half = 1 << lg, 1 << (lg - 1)
        for a0 in range(0, n, seg):
            cnt = min(seg, n - a0)
            if cnt > half:
                yield a0, half, cnt


@pytest.mark.parametrize("kind", ["random", "ties", "line", "nonfinite"])
@pytest.mark.parametrize("n", SIZES)
def test_order_is_a_permutation_of_kd_cells(n, kind):
    """Every collider once, and for every split segment an axis on which no centre of the left half
    lies beyond a centre of the right half (read off the order alone)."""
    cull, order = order_of(n, kind)
    assert np.array_equal(np.sort(order), np.arange(n))
    keys = f32_key(bvh_ref.centres(cull["lo"], cull["hi"]))[order].astype(np.int64)
    for a0, half, cnt in split_segments(n):
        left, right = keys[a0:a0 + half], keys[a0 + half:a0 + cnt]
        assert (left.max(axis=0) <= right.min(axis=0)).any(), (a0, half, cnt)


def test_bounds_of_non_finite_records():
    sph, box, _ = bvh_ref.nonfinite_scene(513, 7)
    cull = cull_bounds(sph, box)
    def f32(bits):
        return bits.view(np.float16).astype(np.float32).reshape(bits.shape[0], -1)

    values = np.concatenate([np.concatenate([f32(sph["center"]), f32(sph["radius"]), f32(sph["radius"]), f32(sph["radius"])], axis=1),
                             np.concatenate([f32(box["center"]), f32(box["size"])], axis=1)])
    bad = ~np.isfinite(values).all(axis=1)
    assert bad.sum() == 5
    assert (cull["lo"][bad] == -np.inf).all() and (cull["hi"][bad] == np.inf).all() and (cull["fscale"][bad] == 0).all()
    assert np.isfinite(cull["lo"][~bad]).all() and np.isfinite(cull["hi"][~bad]).all() and (cull["fscale"][~bad] > 0).all()
    assert (cull[:sph.size]["factor"] == np.float32(4e-3)).all() and (cull[sph.size:]["factor"] == np.float32(1e-4)).all()
    # Their centres are FLT_MAX on every axis, so they sort last on whichever axis a segment splits:
    # the top split (512 + 1 positions) puts one of them alone in the right half, and every later
    # split of the first 512 positions sends the other four to the end of its last segment.
    order = kd_order(cull["lo"], cull["hi"])
    inf_ids = np.nonzero(bad)[0]
    assert order[512] in inf_ids
    assert sorted(order[508:513].tolist()) == inf_ids.tolist()


def test_equal_keys_keep_id_order_and_negative_zero_sorts_first():
    same = np.zeros((37, 3), np.float32)
    assert np.array_equal(kd_order(same, same + 1), np.arange(37))
    # centres -0.0 and +0.0 (equal as floats, distinct keys) on x, everything else equal
    lo = np.zeros((8, 3), np.float32)
    lo[::2, 0] = -0.0
    order = kd_order(lo, lo.copy())
    assert sorted(order[:4]) == [0, 2, 4, 6] and sorted(order[4:]) == [1, 3, 5, 7]


@pytest.mark.parametrize("n", [5, 17, 33, 48, 64])
def test_top_split_takes_the_cheapest_axis(n):
    """The first split of a small scene against a float64 evaluation of the three surface-area costs,
    on scenes whose costs differ by more than 1e-3 relative (so rounding cannot decide)."""
    half = capacity(n) // 2
    while half >= n:
        half //= 2
    checked = 0
    for seed in range(12):
        sph, box, _ = bvh_ref.random_scene(n, 1000 * n + seed)
        cull = cull_bounds(sph, box)
        lo, hi = cull["lo"].astype(np.float64), cull["hi"].astype(np.float64)
        keys = f32_key(bvh_ref.centres(cull["lo"], cull["hi"]))
        costs, lefts = [], []
        for x in range(3):
            ids = sorted(range(n), key=lambda i: (int(keys[i, x]), i))
            cost = 0.0
            for part in (ids[:half], ids[half:]):
                e = np.maximum(hi[part].max(axis=0) - lo[part].min(axis=0), 0.0)
                cost += (e[0] * e[1] + e[1] * e[2] + e[2] * e[0]) * len(part)
            costs.append(cost)
            lefts.append(set(ids[:half]))
        by_cost = sorted(costs)
        if by_cost[1] - by_cost[0] <= 1e-3 * by_cost[1]:
            continue
        checked += 1
        order = kd_order(cull["lo"], cull["hi"])
        assert set(order[:half].tolist()) == lefts[int(np.argmin(costs))], (seed, costs)
    assert checked >= 6


@pytest.mark.parametrize("n", [1, 4, 5, 17, 65, 257, 1025])
def test_check_tree_accepts_its_own_nodes(n):
    cull, order = order_of(n) if n in SIZES else (scene_bounds(n), None)
    if order is None:
        order = kd_order(cull["lo"], cull["hi"])
    nodes = build_nodes(cull, order)
    assert nodes.dtype == REC and nodes.size == (capacity(n) - 1) // 3
    assert check_tree(cull, order, nodes).size == 0
    # the root holds every collider
    assert (nodes[0]["lo"] == cull["lo"].min(axis=0)).all() and (nodes[0]["hi"] == cull["hi"].max(axis=0)).all()
    assert nodes[0]["fscale"] == cull["fscale"].max() and nodes[0]["factor"] == cull["factor"].max()


def test_check_tree_reports_exactly_the_perturbed_node():
    cull, order = order_of(65)  # 17 leaves of 64: 85 nodes, the leaves from 21 on, the last 47 empty
    good = build_nodes(cull, order)
    assert good.size == 85 and np.isinf(good[84]["lo"]).all() and good[84]["hi"][0] == np.inf

    bad = good.copy()  # an ancestor too large by one ulp
    bad["hi"][1, 0] = np.nextafter(bad["hi"][1, 0], np.float32(np.inf))
    assert check_tree(cull, order, bad).tolist() == [1]

    bad = good.copy()  # an ancestor's margin scale too small
    bad["fscale"][2] *= np.float32(0.5)
    assert good["fscale"][2] > 0 and check_tree(cull, order, bad).tolist() == [2]

    bad = good.copy()  # an empty leaf left as the empty union (+inf, -inf) instead of the stored form
    bad["hi"][84] = -np.inf
    assert check_tree(cull, order, bad).tolist() == [84]

    swapped = order.copy()  # and a wrong order shows in the leaves that changed (and their ancestors)
    swapped[[0, 64]] = swapped[[64, 0]]
    assert 21 in check_tree(cull, swapped, good) and 21 + 16 in check_tree(cull, swapped, good)

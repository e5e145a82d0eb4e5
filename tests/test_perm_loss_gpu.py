"""permeate_bvh_kernel (csrc/art_permeate.hip) on every path of its control flow, each path shown to be
taken before the outputs are compared: the chunk shapes of the loss rays (P = 4, 3, 2, 1 quads per ray,
tail chunks), rays that fit their quads' kept lists, rays that fit only list by list, lists of exactly 48
and 49 terms, the whole-wave overflow sum (alone, several per chunk, in tail chunks, in batch slots above
0), terms that are never kept (zero and owned colliders), the first-hit search over a batch, first hits at
distance 0, axis-aligned loss rays and trees of one to five colliders.

Every case (tests/perm_loss_ref.py, shared with test_perm_loss_ref_cpu.py) first binds its scene, reads
the device's leaf order back and requires it to be bvh_ref.kd_order of the device's bounds; the host
model then counts, on that order, the kept terms of every loss ray's quads and the case's declared
classes are asserted, so a failure names the case and the class it lost. Then the frame runs through
test_parity_gpu.gpu_vs_oracle from stale contents (the throughput plan, the reference-order kernel, the
counting kernel, the shipped plan without hit outputs), byte for byte against the oracle, and
PermeationPowerRemains also against the model's own values (kat_scenes.perm_value)."""
import numpy as np
import pytest

import art
import perm_loss_ref as M
from art import abi
from bvh_ref import kd_order
from test_bvh_structure_gpu import read_back
from test_parity_gpu import gpu_vs_oracle

pytestmark = pytest.mark.gpu

CASES = M.cases()
STALE = 29


@pytest.mark.parametrize("name", sorted(CASES))
def test_permeation_case(ctx, name):
    case = CASES[name]()
    sc, p = case.scene, case.params
    S, ns, na = len(case.org), sc.spheres.size, sc.aabbs.size
    hits = bool(p.stages & abi.ART_STAGE_RAYTRACE)
    ctx.set_flags(0)
    ctx.bind(art.Frame(sc, p, case.org, art.FanOutputs(S, sc.R, p.max_hits_per_ray, sc.T, p.thread_count)))
    bounds, order, _ = read_back(ctx, ns, na, sc.C)  # (OBB bounds as the device computed them)
    want = kd_order(bounds["lo"], bounds["hi"])
    d = np.nonzero(order != want)[0]
    assert d.size == 0, f"{name}: {d.size} of {sc.C} leaf positions differ from kd_order, first {d[:8]}"
    info, line = M.check_classes(case, order)
    print(line)
    out, _ = gpu_vs_oracle(ctx, sc, p, case.org, hits=hits, stale=STALE)
    stale = art.FanOutputs(S, sc.R, p.max_hits_per_ray, sc.T, p.thread_count, hits=hits).fill_random(STALE).perm
    model = M.expected_perm(case, info, stale)
    bad = np.argwhere(out.perm.view(np.uint32) != model.view(np.uint32))
    assert bad.size == 0, f"{name}: perm differs from the model at (fan, slot * T + t) {bad[:8].tolist()}"

"""The host model of the permeation loss pass (tests/perm_loss_ref.py) on its own, without a GPU: the chunk
plan against a hand-written table, the quad parts, and for every case of the matrix that
test_perm_loss_gpu.py runs (a) the classes it declares are reached under bvh_ref.kd_order, which is what
keeps the GPU cases from passing without taking the paths they are built for, and (b) three independent
restatements agree bit for bit on PermeationPowerRemains: the model's values (kat_scenes.perm_value, and
the sum of the kept terms the classes are counted from), the oracle and the CPU backend."""
import numpy as np
import pytest

import art
import oracle
import perm_loss_ref as M

# quads per ray by the rays left, 1..16 (art_permeate.hip: min(4, 16 / left)); one chunk takes 16 / P rays
QUADS = [4, 4, 4, 4, 3, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1]
TAILS = {17: (16, 4, 1), 21: (16, 3, 5), 22: (16, 2, 6), 33: (32, 4, 1), 37: (32, 3, 5)}
CASES = M.cases()


def table(T):
    """The chunks of T rays written out by hand: full chunks of 16 single-quad rays, then the rest in one."""
    full, left = (T - 1) // 16, T - 16 * ((T - 1) // 16)
    return [(16 * i, 1, 16) for i in range(full)] + [(16 * full, QUADS[left - 1], left)]


def test_plan_matches_the_table():
    assert [QUADS[n - 1] for n in (1, 4, 5, 6, 8, 9, 16)] == [4, 4, 3, 2, 2, 1, 1]
    for T in range(1, 41):
        got = M.plan(T, 21)
        assert got == table(T), (T, got)
        assert sum(c[2] for c in got) == T and all(c[2] <= 16 // c[1] for c in got)
        assert M.plan(T, 0) == [(16 * i, 1, min(16, T - 16 * i)) for i in range((T + 15) // 16)]  # a leaf root: P = 1
        assert all(M.chunk_of(T, 21, t) == next(c for c in got if c[0] <= t < c[0] + c[2]) for t in range(T))
    for T, tail in TAILS.items():
        assert M.plan(T, 21)[-1] == tail and M.plan(T, 1)[-1] == tail
    assert M.plan(16, 21) == [(0, 1, 16)] and M.plan(32, 21) == [(0, 1, 16), (16, 1, 16)]


def test_parts_and_slots():
    assert [M.leaf0_of(n) for n in (1, 4, 5, 16, 17, 64, 65, 256, 257)] == [0, 0, 1, 1, 5, 5, 21, 21, 85]
    assert [M.part_of(p, 3) for p in range(3)] == [0, 0, 0]
    assert [M.part_of(p, 5) for p in range(5)] == [0, 0, 0, 0, 1]
    assert [M.part_of(p, 200) for p in (0, 63, 64, 127, 128, 191, 192, 199)] == [0, 0, 1, 1, 2, 2, 3, 3]
    # quad parts of the root children 0..3 at P = 4, 3, 2, 1
    assert [[(c % 4) % P for c in range(4)] for P in (4, 3, 2, 1)] == [[0, 1, 2, 3], [0, 1, 2, 0], [0, 1, 0, 1], [0, 0, 0, 0]]
    assert M.slot_batches(64, 1, 6) == {0: (0, 64)}
    assert M.slot_batches(64, 3, 6) == {0: (44, 64)} and M.slot_batches(9, 3, 6) == {0: (6, 9)}
    assert M.slot_batches(9, 5, 6) == {0: (4, 6), 1: (6, 8), 4: (8, 9)}
    assert M.slot_batches(3, 3, 3) == {0: (0, 1), 1: (1, 2), 2: (2, 3)}
    assert M.classes_of([48, 0]) == {"fit", "edge48"} and M.classes_of([48, 1]) == {"fit", "fit_wide", "edge48"}
    assert M.classes_of([49, 48]) == {"overflow", "edge49"} and M.classes_of([50]) == {"overflow"}
    assert M.classes_of([12, 12, 12, 13]) == {"fit", "fit_wide"}


@pytest.fixture(scope="module")
def cpu():
    c = art.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_classes_and_three_restatements_agree(cpu, name):
    case = CASES[name]()
    sc, p = case.scene, case.params
    order = M.host_order(sc)
    assert sorted(order) == list(range(sc.C))
    info, line = M.check_classes(case, order)
    print(line)
    S = len(case.org)
    o_cpu = art.FanOutputs(S, sc.R, p.max_hits_per_ray, sc.T, p.thread_count, hits=True).fill_random(17)
    o_ref = o_cpu.copy()
    want = M.expected_perm(case, info, o_cpu.perm)
    for (f, slot), e in info.items():  # the terms the classes are counted from sum to the same values
        if e is not None:
            got = np.array([r["value"] for r in e["rays"]], np.float32)
            assert np.array_equal(got.view(np.uint32), want[f, slot * sc.T:(slot + 1) * sc.T].view(np.uint32)), (name, f, slot)
    oracle.run_frame(art.Frame(sc, p, case.org, o_ref), threads=4)
    cpu.run(art.Frame(sc, p, case.org, o_cpu))
    assert np.array_equal(o_ref.perm.view(np.uint32), want.view(np.uint32)), f"{name}: oracle differs from the model"
    assert np.array_equal(o_cpu.perm.view(np.uint32), want.view(np.uint32)), f"{name}: CPU backend differs from the model"
    eq = o_cpu.equal(o_ref)
    assert all(eq.values()), eq

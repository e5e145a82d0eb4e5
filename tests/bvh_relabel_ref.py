"""A plain NumPy restatement of the BVH relabel rule (csrc/art_bvh.hip, bvh_relabel_kernel; DESIGN.md
§3b, "Colliders that appear and disappear"), for the structural tests.

Sequential host code written from the rule, sharing nothing with the kernel. A label is
`kind rank << 30 | in-type index` (bvh_ref's encoding; ranks: sphere 0, AABB 1, OBB 2), a leaf order
is the array of labels by leaf position. Between two syncs labels change only at the kinds' tails:
labels [n'_k, n_k) vanish and labels [n_k, n'_k) appear.

  A = the appearing labels, ascending (kind rank, index); a = |A|
  H = the old leaf positions of the vanishing labels, ascending; h = |H|
  ref[H[j]] = A[j] for j < min(a, h)
  a > h: ref[n + (j - h)] = A[j] for j in [h, a); n' = n + a - h
  h > a: n' = n - (h - a); B = the unfilled holes below n', ascending; M = the positions in [n', n) that
         still hold a label (holes filled in the first step included), ascending; ref[B[j]] = ref[M[j]]
  every other position keeps its reference; bvh_pos[global'(ref[k])] = k for k < n'
"""
import numpy as np

import bvh_ref

KIND_SHIFT = 30
INDEX_MASK = (1 << KIND_SHIFT) - 1


def label(kind: int, index: int) -> int:
    return (kind << KIND_SHIFT) | index


def labels_of(counts) -> list:
    """Every label of a scene with these per-kind counts, ascending (kind rank, index)."""
    return [label(k, i) for k in range(3) for i in range(int(counts[k]))]


def global_index(ref, counts) -> np.ndarray:
    """The global index (spheres, AABBs, OBBs) of each label under these counts."""
    ref = np.asarray(ref, np.uint32).astype(np.int64)
    kind, idx = ref >> KIND_SHIFT, ref & INDEX_MASK
    base = np.array([0, counts[0], counts[0] + counts[1]], np.int64)
    return idx + base[kind]


def relabel(ref, old, new):
    """The leaf order after the counts go from old to new (triples), and the number of positions
    below the new count whose reference was written. ref: uint32 [sum(old)], a permutation of
    labels_of(old)."""
    ref = [int(r) for r in np.asarray(ref, np.uint32)]
    n = len(ref)
    assert n == sum(old) and sorted(ref) == labels_of(old), "ref is not a leaf order of the old counts"
    A = [label(k, i) for k in range(3) for i in range(old[k], new[k])]
    gone = {label(k, i) for k in range(3) for i in range(new[k], old[k])}
    H = [p for p in range(n) if ref[p] in gone]  # ascending positions
    a, h = len(A), len(H)
    written = set()
    for j in range(min(a, h)):
        ref[H[j]] = A[j]
        written.add(H[j])
    if a > h:
        for j in range(h, a):
            ref.append(A[j])
            written.add(n + j - h)
        n2 = n + a - h
    else:
        n2 = n - (h - a)
        unfilled = set(H[a:])
        B = [p for p in H[a:] if p < n2]
        M = [p for p in range(n2, n) if p not in unfilled]
        assert len(B) == len(M)
        for b, m in zip(B, M):
            ref[b] = ref[m]
            written.add(b)
        ref = ref[:n2]
    assert n2 == sum(new) and len(ref) == n2
    return np.array(ref, np.uint32), sum(1 for p in written if p < n2)


def order_of(ref, counts) -> np.ndarray:
    """A leaf order as bvh_ref.build_nodes takes it: position -> global collider index."""
    return global_index(ref, counts)


def check(ref_before, old, new, ref_after, bounds, nodes):
    """The structural check of one step: the device's leaf order is the rule applied to the order
    before the step, and its nodes are the unions over that order, bit for bit. Returns the count
    of rewritten positions (art_collider_resize_stats.relabelled)."""
    want, written = relabel(ref_before, old, new)
    assert np.array_equal(np.asarray(ref_after, np.uint32), want), "leaf order differs from the relabel rule"
    order = order_of(ref_after, new)
    bad = bvh_ref.check_tree(bounds, order, nodes)
    assert bad.size == 0, f"nodes {bad[:8].tolist()} differ from build_nodes"
    return written

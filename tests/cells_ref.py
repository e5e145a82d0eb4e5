"""A float64 reference of the muffle direction-cell lists (csrc/art_cells.hip), for the structural tests.

Plain NumPy written from the documented rule (the header of art_cells.hip, the
cone-table comment of art_frame.cpp), not from the kernels' float code. The rule: around each target
lies a cube map of G x G cells per face; the list of (target, cell) must hold every collider not owned
by the target that a segment ending at the target and arriving through the cell can meet, with a near
bound that is not above the distance from the target to any point of the collider.

The reference states that from the shapes themselves: it samples points of each shape (the points a
segment can be blocked at), takes the cell of the direction from the target to each point, and requires
the collider in that cell's list (`required`). The cell lookup of the device rounds in float32, so a
sample near a cell edge may be looked up in the neighbour: `cells_near` returns the cells of the
direction and of its 26 perturbations by +-2e-5 per component (2e-5 sqrt(3) rad, below the 1e-4 rad the
cell cones carry for exactly this rounding), and a correct build lists the collider in all of them. No
sample is ever left out. The other direction (`justified`) bounds what a build may list: only cells whose
cone comes within the angular radius of the collider's widened bounding sphere, taken with an upper
bound of every margin the build may apply.

Shapes are decoded from the ABI records as the oracle decodes them: halves to float, a sphere by
|radius| (the test squares it), a box by centre +- |size| (the slab test orders each axis' planes
itself), an OBB's local frame by local = q (P - centre) with q the normalised half quaternion, so its
world points are centre + R^T local.
"""
import numpy as np

G = 32                      # cells per cube-face axis
CELLS = 6 * G * G           # cells per target
PERTURB = 2e-5              # cells_near: the lookup's rounding, per component
CONE_SLACK = 1e-4           # each cell cone's slack over its corners (rad)
COS_SLACK = 2e-5            # justified: twice the enumeration's cosine tolerance
SLACK_REL, SLACK_ABS = 0.1, 0.2   # cell_slack(r) = 0.1 r + 0.2: the motion slack of a listed collider
ETA = 2e-6                  # relative deviation of a float muffle ray from its exact segment
FACTOR = {0: 4e-3, 1: 1e-4, 2: 1e-3}  # the broad-phase margin factors by kind (§5 item 8)
SPHERE, AABB, OBB = 0, 1, 2
_OFFS = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * PERTURB


def cell_slack(r):
    return SLACK_REL * r + SLACK_ABS


def _half(bits) -> np.ndarray:
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


# ------------------------------------------------------------------------------------------------
# Cells and their cones
# ------------------------------------------------------------------------------------------------
def cell_of(v) -> np.ndarray:
    """The cube-map cell of directions v [..., 3]: the major axis m (x before y before z on ties), face
    f = 2 m + (v[m] < 0), i from u = v[(m+1)%3] / |v[m]|, j from w = v[(m+2)%3] / |v[m]|, each cell
    covering 2 / G of [-1, 1]; cell = (f G + j) G + i."""
    v = np.asarray(v, np.float64)
    a = np.abs(v)
    m = np.where((a[..., 0] >= a[..., 1]) & (a[..., 0] >= a[..., 2]), 0, np.where(a[..., 1] >= a[..., 2], 1, 2))
    vm = np.take_along_axis(v, m[..., None], -1)[..., 0]
    vu = np.take_along_axis(v, ((m + 1) % 3)[..., None], -1)[..., 0]
    vw = np.take_along_axis(v, ((m + 2) % 3)[..., None], -1)[..., 0]
    with np.errstate(all="ignore"):
        n = np.abs(vm)
        i = np.clip(np.floor((vu / n + 1.0) * (0.5 * G)), 0, G - 1)
        j = np.clip(np.floor((vw / n + 1.0) * (0.5 * G)), 0, G - 1)
    f = 2 * m + (vm < 0)
    return ((f * G + j.astype(np.int64)) * G + i.astype(np.int64)).astype(np.int64)


def cells_near_all(v) -> np.ndarray:
    """Cells of v / |v| and of its 26 perturbations, [..., 27] (with repeats)."""
    v = np.asarray(v, np.float64)
    u = v / np.linalg.norm(v, axis=-1, keepdims=True)
    return cell_of(u[..., None, :] + _OFFS)


def cells_near(v) -> np.ndarray:
    """The set of cells of one direction v and of its 26 perturbations by +-2e-5 per component."""
    return np.unique(cells_near_all(np.asarray(v, np.float64).reshape(3)))


def _cones():
    """Each cell's cone in float64: the normalised sum of its four corner directions, and the largest angle
    from it to a corner (the farthest point of a convex spherical quadrilateral from an inner point)."""
    axis, alpha = np.zeros((CELLS, 3)), np.zeros(CELLS)
    f, j, i = np.meshgrid(np.arange(6), np.arange(G), np.arange(G), indexing="ij")
    f, j, i = f.ravel(), j.ravel(), i.ravel()
    m, sg = f >> 1, np.where(f & 1, -1.0, 1.0)
    corners = []
    for k in range(4):
        d = np.zeros((CELLS, 3))
        d[np.arange(CELLS), m] = sg
        d[np.arange(CELLS), (m + 1) % 3] = -1.0 + 2.0 * (i + (k & 1)) / G
        d[np.arange(CELLS), (m + 2) % 3] = -1.0 + 2.0 * (j + (k >> 1)) / G
        corners.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    axis = sum(corners)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    for c in corners:
        alpha = np.maximum(alpha, np.arccos(np.minimum(1.0, (axis * c).sum(1))))
    return axis, alpha


CONE_AXIS, CONE_ALPHA = _cones()   # (without the slack; cell order (f G + j) G + i)
ALPHA_MAX = float(CONE_ALPHA.max()) + CONE_SLACK


# ------------------------------------------------------------------------------------------------
# Shapes
# ------------------------------------------------------------------------------------------------
def _fibonacci(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)


_FIB32 = _fibonacci(32)
_POLES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
_CORNERS = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], np.float64)
# the 12 edges: the axis the edge runs along and the signs of the other two
_EDGES = [(ax, s1, s2) for ax in range(3) for s1 in (-1, 1) for s2 in (-1, 1)]
_EDGE_MID = np.zeros((12, 3))
for _e, (_ax, _s1, _s2) in enumerate(_EDGES):
    _EDGE_MID[_e, (_ax + 1) % 3], _EDGE_MID[_e, (_ax + 2) % 3] = _s1, _s2


class Shapes:
    """The colliders of a scene in float64, global order (spheres, AABBs, OBBs): kind, centre, r (the
    bounding radius: |radius| or |size|_2), h1 (3 r or |size|_1), half extents and the world-from-local
    rotation (boxes), owner."""

    def __init__(self, spheres, aabbs, obbs):
        ns, na, no = spheres.size, aabbs.size, obbs.size
        n = ns + na + no
        self.n, self.counts = n, (ns, na, no)
        self.kind = np.concatenate([np.full(ns, SPHERE), np.full(na, AABB), np.full(no, OBB)]).astype(np.int64)
        self.index = np.concatenate([np.arange(ns), np.arange(na), np.arange(no)]).astype(np.int64)
        self.centre = np.concatenate([_half(a["center"]).reshape(-1, 3) for a in (spheres, aabbs, obbs)])
        self.tid = np.concatenate([a["audio_target_id"].astype(np.int64) for a in (spheres, aabbs, obbs)])
        self.half = np.zeros((n, 3))
        self.half[ns:] = np.abs(np.concatenate([_half(a["size"]).reshape(-1, 3) for a in (aabbs, obbs)]))
        rad = np.abs(_half(spheres["radius"]).reshape(ns))
        self.r = np.concatenate([rad, np.linalg.norm(self.half[ns:], axis=1)])
        self.h1 = np.concatenate([3.0 * rad, self.half[ns:].sum(1)])
        self.rot = np.tile(np.eye(3), (n, 1, 1))   # world = centre + rot @ local
        if no:
            q = _half(obbs["rot"]).reshape(no, 3)
            w = np.sqrt(np.maximum(0.0, 1.0 - (q * q).sum(1)))
            q = np.concatenate([q, w[:, None]], 1)
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            x, y, z, w = q.T
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]).transpose(2, 0, 1)
            self.rot[ns + na:] = R.transpose(0, 2, 1)   # local = R (P - c), so world = c + R^T local
        self.code = (self.kind << 28) | self.index      # the order code of a list entry

    def finite(self):
        return np.isfinite(self.centre).all(1) & np.isfinite(self.r)


def _sphere_samples(c, r, target):
    """[n, 72, 3]: the centre, 6 axis poles, 32 Fibonacci surface points, 32 points of the silhouette
    circle as seen from the target (the tangent rim) and the point nearest the target; inside [n]."""
    n = c.shape[0]
    w = c - target
    D = np.linalg.norm(w, axis=1)
    inside = D <= r
    with np.errstate(all="ignore"):
        wh = np.where(D[:, None] > 0, w / D[:, None], np.array([1.0, 0.0, 0.0]))
        # two unit vectors orthogonal to wh
        a = np.where((np.abs(wh[:, 0]) < 0.9)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
        e1 = np.cross(wh, a)
        e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
        e2 = np.cross(wh, e1)
        q = np.where(inside, 0.0, r / np.where(D > 0, D, 1.0))     # sin of the angular radius
        rim_c = c - wh * (r * q)[:, None]                          # the tangent circle: centre, radius
        rim_r = r * np.sqrt(np.maximum(0.0, 1.0 - q * q))
    ang = (np.arange(32) + 0.25) * (2.0 * np.pi / 32)
    rim = rim_c[:, None, :] + rim_r[:, None, None] * (np.cos(ang)[None, :, None] * e1[:, None, :] +
                                                       np.sin(ang)[None, :, None] * e2[:, None, :])
    P = np.concatenate([c[:, None, :], c[:, None, :] + r[:, None, None] * _POLES[None],
                        c[:, None, :] + r[:, None, None] * _FIB32[None], rim,
                        (c - wh * r[:, None])[:, None, :]], 1)
    assert P.shape == (n, 72, 3)
    return P, inside


def _box_samples(c, h, rot, target):
    """[n, 60, 3]: the centre, 8 corners, 12 edge midpoints, 6 face centres, 32 points on the silhouette
    edges as seen from the target (an edge between a face turned to the target and one turned away) and the
    point nearest the target; inside [n]."""
    n = c.shape[0]
    p = np.einsum("nji,nj->ni", rot, target - c)       # the target in the box's frame (rot^T (t - c))
    inside = (np.abs(p) <= h).all(1)
    front = np.stack([p > h, p < -h], -1)              # [n, axis, (plus, minus)]
    local = [np.zeros((n, 1, 3)), np.broadcast_to(_CORNERS, (n, 8, 3)) * h[:, None, :],
             np.broadcast_to(_EDGE_MID, (n, 12, 3)) * h[:, None, :], np.broadcast_to(_POLES, (n, 6, 3)) * h[:, None, :]]
    sil = np.zeros((n, 12), bool)
    for e, (ax, s1, s2) in enumerate(_EDGES):          # the edge's two faces: axis ax+1 sign s1, axis ax+2 sign s2
        f1 = front[:, (ax + 1) % 3, 0 if s1 > 0 else 1]
        f2 = front[:, (ax + 2) % 3, 0 if s2 > 0 else 1]
        sil[:, e] = f1 != f2
    sil[~sil.any(1)] = True                            # (the target inside or in a face plane: every edge)
    order = np.argsort(~sil, axis=1, kind="stable")    # the silhouette edges first
    ne = sil.sum(1)
    k = np.arange(32)
    edge = np.take_along_axis(order, (k[None, :] % ne[:, None]), 1)            # [n, 32]
    per = (32 + ne - 1) // ne
    t = ((k[None, :] // ne[:, None]) + 0.5) / per[:, None] * 2.0 - 1.0        # along the edge, in (-1, 1)
    mid = _EDGE_MID[edge]                                                      # [n, 32, 3]
    along = np.eye(3)[np.array([ax for ax, _, _ in _EDGES])][edge]
    local.append((mid + along * t[..., None]) * h[:, None, :])
    local.append(np.clip(p, -h, h)[:, None, :])
    L = np.concatenate(local, 1)
    assert L.shape == (n, 60, 3)
    return c[:, None, :] + np.einsum("nij,nsj->nsi", rot, L), inside


class Ref:
    """The reference for one scene: its colliders (ABI records) and targets [T, 3]."""

    def __init__(self, spheres, aabbs, obbs, targets):
        self.shapes = Shapes(spheres, aabbs, obbs)
        self.targets = np.asarray(targets, np.float64).reshape(-1, 3)

    # -- samples -------------------------------------------------------------------------------
    def samples_many(self, t, gs):
        """For colliders gs (global indices, one kind at a time or mixed): a list of (gs of a kind, points
        [m, S, 3], inside [m]) as seen from target t."""
        sh, tg = self.shapes, self.targets[t]
        gs = np.asarray(gs, np.int64)
        out = []
        sp = gs[sh.kind[gs] == SPHERE]
        if sp.size:
            out.append((sp, *_sphere_samples(sh.centre[sp], sh.r[sp], tg)))
        bx = gs[sh.kind[gs] != SPHERE]
        if bx.size:
            out.append((bx, *_box_samples(sh.centre[bx], sh.half[bx], sh.rot[bx], tg)))
        return out

    def shape_samples(self, t, g):
        (_, P, inside), = self.samples_many(t, [g])
        return P[0], bool(inside[0])

    # -- required ------------------------------------------------------------------------------
    def required_many(self, t, gs, chunk=2048):
        """(pairs, dmin): pairs = the sorted unique keys g * CELLS + cell of the cells every collider of gs
        must be listed in for target t, dmin [len(gs)] = the smallest distance from the target to a sample
        (0 with the target inside the shape, which requires every cell). Colliders with non-finite records
        are the caller's to leave out."""
        gs = np.asarray(gs, np.int64)
        tg = self.targets[t]
        keys, dmin = [], np.zeros(self.shapes.n)
        for lo in range(0, gs.size, chunk):
            for g, P, inside in self.samples_many(t, gs[lo:lo + chunk]):
                v = P - tg
                d = np.linalg.norm(v, axis=2)
                dmin[g] = np.where(inside, 0.0, d.min(1))
                out = ~inside
                if out.any():
                    assert (d[out] > 0).all()
                    cells = cells_near_all(v[out]).reshape(int(out.sum()), -1)
                    keys.append(np.unique(g[out][:, None] * CELLS + cells))
                if inside.any():
                    keys.append((g[inside][:, None] * CELLS + np.arange(CELLS)[None, :]).ravel())
        pairs = np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
        return pairs, dmin[gs]

    def required(self, t, g):
        """(cells, dmin) of one collider: the union of cells_near(p - target_t) over its samples."""
        pairs, dmin = self.required_many(t, [g])
        return pairs - g * CELLS, float(dmin[0])

    def dmin_many(self, t, gs):
        """The distance from target t to the nearest point of each shape of gs (0 inside): what
        required_many's dmin equals, since the nearest point is one of the samples, without the samples."""
        sh, tg = self.shapes, self.targets[t]
        gs = np.asarray(gs, np.int64)
        w = tg - sh.centre[gs]
        p = np.einsum("nji,nj->ni", sh.rot[gs], w)
        box = np.linalg.norm(p - np.clip(p, -sh.half[gs], sh.half[gs]), axis=1)
        return np.where(sh.kind[gs] == SPHERE, np.maximum(0.0, np.linalg.norm(w, axis=1) - sh.r[gs]), box)

    # -- justified -----------------------------------------------------------------------------
    def rho_hi(self, g, factor, far):
        """An upper bound of the radius the build may give collider g's widened bounding sphere: the plain
        margin factor (far + r + h1 + 1) times 1 (sphere) or sqrt(3) (box), the ray deviation 2 (eta far +
        1e-6), 1e-6 |c|_1 and the motion slack, times 1.001."""
        sh = self.shapes
        g = np.asarray(g, np.int64)
        r, widen = sh.r[g], np.where(sh.kind[g] == SPHERE, 1.0, np.sqrt(3.0))
        return (r + widen * factor * (far + r + sh.h1[g] + 1.0) + 2.0 * (ETA * far + 1e-6) +
                1e-6 * np.abs(sh.centre[g]).sum(-1) + cell_slack(r)) * 1.001

    def justified(self, t, cell, g, factor, far):
        """Whether a build may list collider(s) g in cell(s) `cell` of target t: the direction u to the
        centre satisfies u . axis_c >= cos(alpha_c + asin(min(1, rho_hi / D))) - 2e-5; D <= rho_hi
        justifies every cell."""
        g, cell = np.asarray(g, np.int64), np.asarray(cell, np.int64)
        w = self.shapes.centre[g] - self.targets[t]
        D = np.linalg.norm(w, axis=-1)
        rho = self.rho_hi(g, factor, far)
        with np.errstate(all="ignore"):
            every = ~(D > rho) | ~np.isfinite(D) | ~np.isfinite(rho)
            u = w / np.where(D > 0, D, 1.0)[..., None]
            ang = CONE_ALPHA[cell] + CONE_SLACK + np.arcsin(np.minimum(1.0, rho / np.where(D > 0, D, 1.0)))
            ok = (u * CONE_AXIS[cell]).sum(-1) >= np.cos(np.minimum(ang, np.pi)) - COS_SLACK
        return every | ok

    def far64(self, t, lo, hi):
        """The distance from target t to the farthest corner of the box [lo, hi]."""
        tg = self.targets[t]
        with np.errstate(all="ignore"):
            d = np.maximum(np.abs(np.asarray(lo, np.float64) - tg), np.abs(np.asarray(hi, np.float64) - tg))
        return float(np.sqrt((d * d).sum()))

    def scene_box(self):
        """The union of the colliders' exact bounds (spheres c +- r, boxes by their corners): a box inside
        the device's union of cull bounds, for the CPU tests."""
        sh = self.shapes
        ext = np.where((sh.kind == SPHERE)[:, None], sh.r[:, None], np.einsum("nij,nj->ni", np.abs(sh.rot), sh.half))
        return (sh.centre - ext).min(0), (sh.centre + ext).max(0)


# ------------------------------------------------------------------------------------------------
# The rectangle rule (face_range's comment), restated: which cells of a face the enumeration visits at
# all for a cone of half-angle gamma around unit direction a. Used by the CPU tests to show what the
# coverage assertion sees when the rule is narrowed.
# ------------------------------------------------------------------------------------------------
def face_rects(a, gamma, margin=1):
    """Per face (i0, i1, j0, j1), empty when i0 > i1: the gnomonic coordinate u = (p . e_u) / (p . n) over the
    cone is bounded by the roots of (a_n^2 - s) u^2 - 2 a_u a_n u + (a_u^2 - s) = 0, s = sin^2 gamma; the
    whole axis when a_n^2 - s <= 1e-3 (the conic is no ellipse, or nearly none), nothing when the cone
    stays behind the face (a_n <= -sin gamma); the cell range of [lo, hi] is widened by `margin` cells."""
    a = np.asarray(a, np.float64)
    out = np.zeros((6, 4), np.int64)
    wide = gamma >= 1.5
    sg = np.sin(min(gamma, np.pi / 2))
    s = sg * sg

    def rng(a_u, a_n):
        den, disc = a_n * a_n - s, s * (a_u * a_u + a_n * a_n - s)
        if not den > 1e-3 or not disc >= 0:
            return 0, G - 1
        r0, r1 = (a_u * a_n - np.sqrt(disc)) / den, (a_u * a_n + np.sqrt(disc)) / den
        lo, hi = min(r0, r1), max(r0, r1)
        if not (lo <= 1.0 and hi >= -1.0):
            return 1, 0
        i0 = int(np.floor((max(lo, -1.0) + 1.0) * (0.5 * G))) - margin
        i1 = int(np.floor((min(hi, 1.0) + 1.0) * (0.5 * G))) + margin
        return max(i0, 0), min(i1, G - 1)

    for f in range(6):
        ax, sgn = f >> 1, -1.0 if f & 1 else 1.0
        a_n, a_u, a_v = sgn * a[ax], a[(ax + 1) % 3], a[(ax + 2) % 3]
        if wide:
            out[f] = 0, G - 1, 0, G - 1
        elif a_n <= -sg:
            out[f] = 1, 0, 1, 0
        else:
            out[f] = (*rng(a_u, a_n), *rng(a_v, a_n))
    return out


def rect_cells(rects) -> np.ndarray:
    """The cells of face_rects' rectangles."""
    cells = []
    for f, (i0, i1, j0, j1) in enumerate(rects):
        if i0 <= i1 and j0 <= j1:
            jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
            cells.append(((f * G + jj) * G + ii).ravel())
    return np.concatenate(cells) if cells else np.zeros(0, np.int64)

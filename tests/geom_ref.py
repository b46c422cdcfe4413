"""Float64 geometry of convex polygons, circles and sweeps: the model tests/geom_cases.py holds hk_geom.h's
primitives to.  TEST INFRASTRUCTURE ONLY.  numpy and float64 only; it imports neither the package, the oracle nor the
host build, and it is written from the definitions (distance between convex sets, separating axes, rigid motion),
not from hk_geom.h.

Polygons are float32 vertex arrays [n, 2] in counter-clockwise order (n == 1: a point, the core of a circle); a
transform is the raw (px, py, s, c) the probe is given, so the model evaluates the same rigid map.  Every function
is batched over a leading axis T (poses of a sweep): world vertices are [T, n, 2].
"""
import numpy as np

LINEAR_SLOP = 0.005
POLY_RADIUS = 2 * LINEAR_SLOP
TOI_TOL = LINEAR_SLOP / 4


def toi_target(total_radius):
    """Box2D's time-of-impact target separation, from its constants."""
    return max(LINEAR_SLOP, total_radius - 3 * LINEAR_SLOP)


def world(verts, x):
    """verts [n, 2] under x = (px, py, s, c) -> [1, n, 2] float64."""
    v = np.asarray(verts, np.float64)
    px, py, s, c = (float(k) for k in x)
    return np.stack([c * v[:, 0] - s * v[:, 1] + px, s * v[:, 0] + c * v[:, 1] + py], 1)[None]


def _pt_seg(P, A, B):
    """P [T, k, 2] against segments A -> B [T, e, 2]: distance [T, k, e] and the segment parameter u in [0, 1]."""
    P, A, B = P[:, :, None, :], A[:, None, :, :], B[:, None, :, :]
    ab, ap = B - A, P - A
    den = (ab * ab).sum(-1)
    u = np.clip(np.where(den > 0, (ap * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0), 0.0, 1.0)
    d = ap - u[..., None] * ab
    return np.sqrt((d * d).sum(-1)), u


def _edges(P):
    return P, np.roll(P, -1, axis=1)


def face_normals(P):
    A, B = _edges(P)
    e = B - A
    n = np.stack([e[..., 1], -e[..., 0]], -1)
    return n / np.sqrt((n * n).sum(-1))[..., None]


def face_seps(P, Q):
    """Separation of Q from each face of the polygon P (n >= 3): min over Q's vertices of n_i . (q - p_i); [T, n]."""
    n = face_normals(P)
    return np.einsum("tik,tijk->tij", n, Q[:, None, :, :] - P[:, :, None, :]).min(-1)


def sat(P, Q):
    """Largest face separation of either polygon: > 0 exactly when the convex sets are disjoint; -sat is the
    overlap depth.  A point (n == 1) has no faces."""
    best = np.full(P.shape[0], -np.inf)
    if P.shape[1] >= 3:
        best = np.maximum(best, face_seps(P, Q).max(-1))
    if Q.shape[1] >= 3:
        best = np.maximum(best, face_seps(Q, P).max(-1))
    return best


def vertex_edge(P, Q):
    """All vertex-segment distances: (dPQ [T, n, mE], uPQ) of P's vertices against Q's edges and the reverse."""
    qa, qb = _edges(Q)
    pa, pb = _edges(P)
    return _pt_seg(P, qa, qb), _pt_seg(Q, pa, pb)


def distance(P, Q):
    """Exact distance between the convex sets [T]: 0 where they overlap (a crossing edge or a contained vertex, i.e.
    no separating face), else the smallest vertex-segment distance.  Also returns sat(P, Q)."""
    (dpq, _), (dqp, _) = vertex_edge(P, Q)
    dmin = np.minimum(dpq.min((1, 2)), dqp.min((1, 2)))
    s = sat(P, Q)
    return np.where(s <= 0.0, 0.0, dmin), s


def closest_class(P, Q, eps=1e-5, end=0.02):
    """Closest-feature class of one disjoint pose (T == 1): 'vv', 'a_on_b' (a vertex of P in the interior of an edge
    of Q), 'b_on_a', 'par' (two or more such vertex-edge pairs: parallel edges).  `end` is the fraction of an edge
    next to its ends that still counts as the vertex."""
    (dpq, upq), (dqp, uqp) = vertex_edge(P, Q)
    d = min(dpq.min(), dqp.min())
    nab = int(((dpq <= d + eps) & (upq > end) & (upq < 1 - end)).sum()) if Q.shape[1] >= 2 else 0
    nba = int(((dqp <= d + eps) & (uqp > end) & (uqp < 1 - end)).sum()) if P.shape[1] >= 2 else 0
    if nab + nba >= 2:
        return "par"
    if nab == 1:
        return "a_on_b"
    if nba == 1:
        return "b_on_a"
    return "vv"


def _seg_seg(a0, a1, b0, b1):
    """Distance between two segments (either may be a point), one pose; 0 when they cross."""
    f = lambda p, q0, q1: _pt_seg(p[None, None, :], q0[None, None, :], q1[None, None, :])[0][0, 0, 0]
    d = min(f(a0, b0, b1), f(a1, b0, b1), f(b0, a0, a1), f(b1, a0, a1))
    cr = lambda u, v: u[0] * v[1] - u[1] * v[0]
    da, db = a1 - a0, b1 - b0
    den = cr(da, db)
    if den != 0.0:
        t, u = cr(b0 - a0, db) / den, cr(b0 - a0, da) / den
        if 0.0 <= t <= 1.0 and 0.0 <= u <= 1.0:
            return 0.0
    return d


def feature_distance(P, ia, Q, ib):
    """Distance between the features a simplex cache names (one pose: P, Q are [n, 2]): ia / ib are the cache's index
    lists; one distinct index is a vertex, two a segment, three the triangle (only of an overlap: returns 0)."""
    if len(ia) > 2:
        return 0.0
    ia, ib = sorted(set(ia)), sorted(set(ib))
    a0, a1 = P[ia[0]], P[ia[-1]]
    b0, b1 = Q[ib[0]], Q[ib[-1]]
    return _seg_seg(a0, a1, b0, b1)


def boundary_distance(P, x):
    """Distance of the point x [2] from the boundary of polygon P [n, 2] (one pose)."""
    a, b = _edges(P[None])
    return _pt_seg(x[None, None, :], a, b)[0].min()


# ---------------------------------------------------------------------------------------------- sweeps
def sweep_world(verts, sw, t):
    """World vertices [T, n, 2] of a body's shape at times t [T]: the centre moves c0 -> c, the angle a0 -> a, the
    origin is the centre minus R(angle) lc.  sw = (lcx, lcy, c0x, c0y, cx, cy, a0, a); true sin / cos."""
    v = np.asarray(verts, np.float64)
    lcx, lcy, c0x, c0y, cx, cy, a0, a = (float(k) for k in sw)
    t = np.asarray(t, np.float64)
    ang = (1 - t) * a0 + t * a
    s, c = np.sin(ang), np.cos(ang)
    px = (1 - t) * c0x + t * cx - (c * lcx - s * lcy)
    py = (1 - t) * c0y + t * cy - (s * lcx + c * lcy)
    return np.stack([c[:, None] * v[None, :, 0] - s[:, None] * v[None, :, 1] + px[:, None],
                     s[:, None] * v[None, :, 0] + c[:, None] * v[None, :, 1] + py[:, None]], -1)


class SweepModel:
    """S(t), the core distance along two sweeps, sampled on a grid over [0, 1] and refined on demand."""

    GRID = 513

    def __init__(self, va, swa, vb, swb):
        self.va, self.swa, self.vb, self.swb = va, swa, vb, swb
        self.tg = np.linspace(0.0, 1.0, self.GRID)
        self.sg = self.S(self.tg)

    def S(self, t):
        t = np.atleast_1d(np.asarray(t, np.float64))
        return distance(sweep_world(self.va, self.swa, t), sweep_world(self.vb, self.swb, t))[0]

    def _refine(self, lo, hi, n=65):
        t = np.linspace(max(0.0, lo), min(1.0, hi), n)
        return t, self.S(t)

    def min_upto(self, t_end):
        """min of S over [0, t_end]: grid points, t_end itself, and a refinement around the smallest sample."""
        h = 1.0 / (self.GRID - 1)
        m = self.tg <= t_end
        ts = np.concatenate([self.tg[m], [t_end]])
        ss = np.concatenate([self.sg[m], self.S([t_end])])
        k = int(np.argmin(ss))
        tr, sr = self._refine(ts[k] - h, min(ts[k] + h, t_end))
        return float(min(ss.min(), sr.min()))

    def first_below(self, level):
        """An upper bound of the first time S < level (None if no sample is): the first grid sample below it,
        refined between that sample and the one before."""
        idx = np.nonzero(self.sg < level)[0]
        if idx.size == 0:
            return None
        k = int(idx[0])
        if k == 0:
            return 0.0
        tr, sr = self._refine(self.tg[k - 1], self.tg[k])
        return float(tr[np.nonzero(sr < level)[0][0]])

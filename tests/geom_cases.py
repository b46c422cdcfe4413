"""Seeded cases and float64 laws for hk_geom.h's four primitives (gjk_distance, time_of_impact, collide_polygons,
collide_poly_circle), run through the geometry probe (tests/native/geom_probe.h).  TEST INFRASTRUCTURE ONLY.

  * the probe's three builds behind one call shape: oracle_probe() (oracle/hk_oracle.c's static functions),
    host_probe() (hk_geom.h under g++), gpu_probe() (hk_geom.h on gfx950, one lane per case);
  * Cases(seed): the fixture table (the compiled-in scene's 13 fixtures, read from the code itself, plus synthetic
    convex polygons of 3..8 vertices) and the families D (distance), M (manifolds) and T (time of impact).  Every case
    is aimed with the float64 model (tests/geom_ref.py) and drawn again if the model does not put it in its group;
  * check(cases, outputs): the laws D1-D2, M1-M3, T1-T3 on one build's own outputs, with coverage counts.

Tolerances follow the project's rule: TOL holds 4 x the worst deviation of the CPU ORACLE's probe outputs from the
float64 model over seeds 1000-1009 and the committed seed 0 (python tests/geom_cases.py --measure), never of the host
or GPU build.  A case whose float64 figure is within `bar` of a deciding threshold is left out of that law
(at most MAX_DROPPED of the group).
"""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np

import geom_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hockey-env_amd", "csrc")
LIBDIR = os.path.join(ROOT, "hockey-env_amd", "hockey_amd", "_lib")
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SRC = os.path.join(ROOT, "tests", "native", "geom_probe_oracle.c")
ORACLE_LIB = os.path.join(ORACLE_DIR, "libhk_geom_probe.so")

MAX_DROPPED = 0.10
SLOP = G.LINEAR_SLOP
K_TOL = 0.1 * SLOP  # collide_polygons' reference-face tie-break
MAX_TRANSLATION, MAX_ROTATION = 2.0, 0.5 * np.pi
FAILED, OVERLAPPED, TOUCHING, SEPARATED = 1, 2, 3, 4

# 4 x the CPU oracle's worst deviation from the float64 model over seeds 1000-1009 and seed 0 (measured value beside
# each; --measure prints them).  bar: metres, the float32 rounding allowance of a distance in rink coordinates.
# ubar: dimensionless, unit normals.  T1-T3 need neither on any seed: the root finder stays strictly inside tol.
TOL = {
    "bar": 7.8e-6,   # 4 x 1.93e-6 (D1, |dist - d64|, seed 1004's batch; D1 with radii 1.76e-6, D2 9.5e-7, M3 boundary 8.6e-7)
    "ubar": 5.8e-7,  # 4 x 1.43e-7 (M2, | |n| - 1 |; the normal against the float64 face normal 1.2e-7)
}
# coverage minimums: about half of what the oracle yields on seed 0 (FAILED never occurs: no minimum)
MIN_COVER = {
    "D_vv": 125, "D_a_on_b": 125, "D_b_on_a": 125, "D_par": 125, "D_touch": 125, "D_shallow": 125, "D_deep": 125,
    "D_gap": 124, "D_simplex1": 170, "D_simplex2": 520, "D_simplex3": 300,
    "M_count0": 390, "M_count1": 370, "M_count2": 450, "M_refA": 580, "M_refB": 240, "M_refB_racket_count1": 80,
    "M_flat_count2": 140, "M_tilted_count1": 115, "M_tie_A": 360, "M_end_count1": 60, "M_rackets_count2": 50,
    "M3_min_sep_n": 750, "Mc_c_face_count1": 50, "Mc_c_vertex_lo_count1": 50, "Mc_c_vertex_hi_count1": 50,
    "Mc_c_inside_count1": 99, "Mc_count0": 110, "Mc_face": 59, "Mc_vertex": 125, "Mc_inside": 99,
    "T_state2": 165, "T_state3": 580, "T_state4": 235, "T3_n": 139, "T_fast_state3": 160, "T_near_state4": 80,
    "T_near_state3": 80,
}

F32 = np.float32
FIX = np.dtype([("circle", "i4"), ("count", "i4"), ("radius", "f4"), ("pad", "f4"), ("vx", "f4", 8), ("vy", "f4", 8),
                ("nx", "f4", 8), ("ny", "f4", 8)])
POSE = np.dtype([("fA", "i4"), ("fB", "i4"), ("xa", "f4", 4), ("xb", "f4", 4)])
TOI = np.dtype([("fA", "i4"), ("fB", "i4"), ("sA", "f4", 8), ("sB", "f4", 8), ("tMax", "f4")])
DOUT = np.dtype([("dist", "f4"), ("dist_radii", "f4"), ("metric", "f4"), ("count", "i4"), ("iA", "i4", 3),
                 ("iB", "i4", 3)])
TOUT = np.dtype([("state", "i4"), ("t", "f4")])
MOUT = np.dtype([("type", "i4"), ("count", "i4"), ("ln", "f4", 2), ("lp", "f4", 2), ("p0", "f4", 2), ("p1", "f4", 2),
                 ("id0", "u4"), ("id1", "u4")])
assert (FIX.itemsize, POSE.itemsize, TOI.itemsize, DOUT.itemsize, TOUT.itemsize, MOUT.itemsize) == (144, 40, 76, 40, 8, 48)
NSCENE = 13
F_P1, F_P2, F_PK = 10, 11, 12
STATICS = (0, 1, 2, 3, 4, 5, 7, 9)  # two walls, four posts, the two solid goal boxes (6 and 8 are their sensor twins)
SENTINEL = 0x7FC5A5A5  # a NaN as float, a recognisable word as int: the prefill of every output word


# ------------------------------------------------------------------------------------------------ the three builds
def _bind(path):
    L = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    L.gp_scene.restype = None
    L.gp_scene.argtypes = [vp, vp]
    for name in ("gp_distance", "gp_toi", "gp_manifold"):
        getattr(L, name).restype = ctypes.c_int
        getattr(L, name).argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int64]
    return L


@functools.lru_cache(None)
def oracle_probe():
    """The oracle build, compiled next to the oracle library with the oracle Makefile's flags."""
    srcs = [ORACLE_SRC, os.path.join(ORACLE_DIR, "hk_oracle.c"), os.path.join(ORACLE_DIR, "hk_oracle.h"),
            os.path.join(ROOT, "tests", "native", "geom_probe.h")]
    if not (os.path.exists(ORACLE_LIB) and os.path.getmtime(ORACLE_LIB) >= max(os.path.getmtime(s) for s in srcs)):
        mk = open(os.path.join(ORACLE_DIR, "Makefile")).read()
        cflags = re.search(r"^CFLAGS\s*=\s*(.*)$", mk, re.M).group(1).split()
        tmp = ORACLE_LIB + ".%d.tmp" % os.getpid()
        subprocess.check_call([os.environ.get("CC", "gcc"), *cflags, "-shared", "-o", tmp, ORACLE_SRC, "-lm"])
        os.replace(tmp, ORACLE_LIB)
    return _bind(ORACLE_LIB)


@functools.lru_cache(None)
def host_probe():
    lib = os.environ.get("GP_HOST_LIB")  # a scratch mutation run points this at its own build
    if not lib:
        subprocess.check_call(["make", "-s", "-C", CSRC, "geom-probe-host"])
        lib = os.path.join(LIBDIR, "libhockey_geom_probe_host.so")
    return _bind(lib)


@functools.lru_cache(None)
def gpu_probe():
    subprocess.check_call(["make", "-s", "-C", CSRC, "geom-probe", "ARCH=gfx950"])
    return _bind(os.path.join(LIBDIR, "libhockey_geom_probe.so"))


def scene_table(L):
    fx, body = np.zeros(NSCENE, FIX), np.zeros((NSCENE, 4), F32)
    L.gp_scene(fx.ctypes.data, body.ctypes.data)
    return fx, body


def prefilled(n, dtype):
    return np.full(n * dtype.itemsize // 4, SENTINEL, np.uint32).view(dtype)


def run(L, table, cases, kind):
    """One call of one primitive over all its cases, into outputs prefilled with the sentinel word."""
    fn, dt = {"D": (L.gp_distance, DOUT), "T": (L.gp_toi, TOUT), "M": (L.gp_manifold, MOUT)}[kind]
    cases = np.ascontiguousarray(cases)
    out = prefilled(len(cases), dt)
    rc = fn(table.ctypes.data, len(table), cases.ctypes.data, out.ctypes.data, len(cases))
    assert rc == 0, (kind, "probe returned", rc)
    return out


def run_all(L, c):
    return {"D": run(L, c.table, c.D, "D"), "M": run(L, c.table, c.M, "M"), "T": run(L, c.table, c.T, "T")}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)


# ------------------------------------------------------------------------------------------------ shapes
def _f32_normals(v):
    """Edge normals as Box2D's polygon set-up computes them, in float32."""
    n = np.zeros_like(v)
    for i in range(len(v)):
        e = v[(i + 1) % len(v)] - v[i]
        x, y = F32(e[1]), F32(-e[0])
        inv = F32(1.0) / np.sqrt(F32(x * x + y * y))
        n[i] = (x * inv, y * inv)
    return n


def synthetic_polygon(rng, count):
    """A convex polygon: `count` points on an ellipse (semi-axes 0.15-0.45 m), counter-clockwise, float32."""
    while True:
        ang = np.sort(rng.uniform(0, 2 * np.pi, count))
        gaps = np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))
        if gaps.min() > 0.35 and gaps.max() < 2.8:
            break
    a, b = rng.uniform(0.15, 0.45, 2)
    rot = rng.uniform(0, 2 * np.pi)
    x, y = a * np.cos(ang), b * np.sin(ang)
    return np.stack([np.cos(rot) * x - np.sin(rot) * y, np.sin(rot) * x + np.cos(rot) * y], 1).astype(F32)


def _rot(th):
    return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def _ang(v):
    return np.arctan2(v[1], v[0])


def _normals64(P):
    return G.face_normals(P[None])[0]


def _cone_dir(N, i, f):
    """A direction inside the normal cone of vertex i (between the normals of edges i-1 and i), at fraction f."""
    a0 = _ang(N[i - 1])
    da = (_ang(N[i]) - a0) % (2 * np.pi)
    a = a0 + f * da
    return np.array([np.cos(a), np.sin(a)])


class Shape:
    def __init__(self, fx):
        self.count = int(fx["count"])
        self.radius = float(fx["radius"])
        self.circle = int(fx["circle"])
        self.v32 = np.stack([fx["vx"][: self.count], fx["vy"][: self.count]], 1).astype(F32)
        self.v = self.v32.astype(np.float64)
        self.N = _normals64(self.v) if self.count >= 3 else None


def aim(rng, PA, NA, B, cls, g, tilt=0.0, end_off=None, cone=None):
    """Pose (theta, p) of shape B whose closest-feature class against the world polygon PA is `cls` at gap g (aimed;
    the caller checks with the model).  Returns (theta, p, u): u is the aimed direction from A to B."""
    nA = len(PA)
    pt = B.count == 1
    f = rng.uniform(0.12, 0.88) if cone is None else cone
    if cls in ("vv", "a_on_b"):
        a = rng.integers(nA)
        u = _cone_dir(NA, a, f)
        X = PA[a] + g * u
    else:  # b_on_a, par: a point of one of A's edges
        e = rng.integers(nA)
        u = NA[e]
        ea, eb = PA[e], PA[(e + 1) % nA]
        L = np.linalg.norm(eb - ea)
        if end_off is not None:  # next to the face's end: end_off metres beyond it (negative: inside)
            X0 = (eb + end_off * (eb - ea) / L) if rng.random() < 0.5 else (ea - end_off * (eb - ea) / L)
        else:
            X0 = ea + rng.uniform(0.12, 0.88) * (eb - ea)
        X = X0 + g * u
    if pt:
        th, q = rng.uniform(-np.pi, np.pi), B.v[0]
    elif cls in ("vv", "b_on_a"):
        b = rng.integers(B.count)
        dB = _cone_dir(B.N, b, rng.uniform(0.12, 0.88))
        th, q = _ang(-u) - _ang(dB), B.v[b]
    else:  # a_on_b, par: a point of one of B's edges
        e = rng.integers(B.count) if B.pick_edge is None else B.pick_edge(rng)
        th = _ang(-u) - _ang(B.N[e]) + tilt
        lam = rng.uniform(0.15, 0.85) if cls == "a_on_b" else rng.uniform(0.35, 0.65)
        q = B.v[e] + lam * (B.v[(e + 1) % B.count] - B.v[e])
    p = X - _rot(th) @ q
    return th, p, u


def pose32(th, p):
    return np.array([p[0], p[1], np.sin(th), np.cos(th)], F32)


def in_rink(p, margin=1.0):
    return -margin <= p[0] <= 10.0 + margin and -margin <= p[1] <= 8.0 + margin


# ------------------------------------------------------------------------------------------------ the generator
class Cases:
    ND, NT = 250, 110  # cases per group: D's eight groups, T's 3 rotation classes x 6 kinds (M's are listed below)

    def __init__(self, seed=0, probe=None):
        rng = self.rng = np.random.default_rng([seed, 0x6E0])
        L = probe or oracle_probe()
        scene, self.body = scene_table(L)
        syn = []
        for k in range(12):  # two of each count 3..8
            v = synthetic_polygon(rng, 3 + k // 2)
            fx = np.zeros((), FIX)
            fx["count"], fx["radius"] = len(v), F32(G.POLY_RADIUS)
            fx["vx"][: len(v)], fx["vy"][: len(v)] = v[:, 0], v[:, 1]
            n = _f32_normals(v)
            fx["nx"][: len(v)], fx["ny"][: len(v)] = n[:, 0], n[:, 1]
            syn.append(fx)
        self.table = np.concatenate([scene, np.array(syn, FIX)])
        self.shapes = [Shape(f) for f in self.table]
        for s in self.shapes:
            s.pick_edge = None
        self.SYN = tuple(range(NSCENE, len(self.table)))
        self.POLYB = (F_P1, F_P2) + self.SYN
        self.D, self.Dgroup = self._family_D()
        self.M, self.Mgroup = self._family_M()
        self.T, self.Tgroup, self.Trot = self._family_T()
        for fam in (self.D, self.M, self.T):
            assert len(fam) % 64 != 0  # a partial last wave

    # A's world pose: a static sits at its body's origin, unrotated; a racket as A gets a random pose in the rink
    def _pose_A(self, fA):
        if fA < NSCENE and fA not in (F_P1, F_P2):
            return np.array([self.body[fA, 0], self.body[fA, 1], 0.0, 1.0], F32)
        rng = self.rng
        return pose32(rng.uniform(-np.pi, np.pi), rng.uniform([1.5, 1.5], [8.5, 6.5]))

    def _try(self, fA, fB, cls, g, accept, **kw):
        """Draw poses until the float64 model accepts: returns a POSE record and the model's figures."""
        A, B = self.shapes[fA], self.shapes[fB]
        for _ in range(200):
            xa = self._pose_A(fA)
            PA = G.world(A.v32, xa)
            gg = g() if callable(g) else g
            th, p, u = aim(self.rng, PA[0], _normals64(PA[0]), B, cls, gg, **{k: (v() if callable(v) else v) for k, v in kw.items()})
            if not in_rink(p):
                continue
            xb = pose32(th, p)
            PB = G.world(B.v32, xb)
            d, s = G.distance(PA, PB)
            if accept(PA, PB, float(d[0]), float(s[0])):
                rec = np.zeros((), POSE)
                rec["fA"], rec["fB"], rec["xa"], rec["xb"] = fA, fB, xa, xb
                return rec
        raise AssertionError(("no accepted draw", fA, fB, cls))

    def _shuffle(self, recs, groups, *more):
        order = self.rng.permutation(len(recs))
        out = [np.array(recs)[order], np.array(groups)[order]]
        return out + [np.array(m)[order] for m in more]

    # ---- family D
    def _family_D(self):
        rng = self.rng
        recs, groups = [], []
        logu = lambda lo, hi: (lambda: float(np.exp(rng.uniform(np.log(lo), np.log(hi)))))
        cls_ok = lambda c: (lambda PA, PB, d, s: d > 5e-4 and G.closest_class(PA, PB) == c)
        spec = {
            "vv": ("vv", logu(1e-3, 0.5), cls_ok("vv")),
            "a_on_b": ("a_on_b", logu(1e-3, 0.5), cls_ok("a_on_b")),
            "b_on_a": ("b_on_a", logu(1e-3, 0.5), cls_ok("b_on_a")),
            "par": ("par", logu(1e-3, 0.5), cls_ok("par")),
            "touch": (None, lambda: rng.uniform(-1e-6, 1e-6), lambda PA, PB, d, s: abs(s) < 3e-6),
            "shallow": (None, lambda: rng.uniform(-2 * SLOP, 0), lambda PA, PB, d, s: -2 * SLOP < s < -1e-4),
            "deep": (None, lambda: rng.uniform(-0.25, -0.03), lambda PA, PB, d, s: s < -0.02),
            "gap": (None, lambda: rng.uniform(0.5, 3.0), lambda PA, PB, d, s: d > 0.3),
        }
        for name, (cls, g, acc) in spec.items():
            for k in range(self.ND):
                fA = STATICS[k % len(STATICS)]
                fB = ((F_P1, F_P2, F_PK) + self.SYN)[rng.integers(3 + len(self.SYN))]
                c = cls or ("vv", "a_on_b", "b_on_a", "par")[rng.integers(4)]
                if fB == F_PK and c in ("a_on_b", "par"):  # a point has no edge
                    if cls is None:
                        c = ("vv", "b_on_a")[rng.integers(2)]
                    else:
                        fB = self.POLYB[rng.integers(len(self.POLYB))]
                recs.append(self._try(fA, fB, c, g, acc))
                groups.append(name)
        recs.pop()  # a partial last wave
        groups.pop()
        return self._shuffle(recs, groups)

    # ---- family M
    def _family_M(self):
        rng = self.rng
        recs, groups = [], []
        total = 2 * G.POLY_RADIUS
        gap = lambda: total + rng.uniform(-0.05, 0.03)
        anyc = lambda PA, PB, d, s: d < 0.08
        longest = lambda sh: (lambda r: int(np.argmax(np.linalg.norm(np.roll(sh.v, -1, 0) - sh.v, axis=1))))

        def tie(PA, PB, d, s):
            return abs(G.face_seps(PA, PB).max() - G.face_seps(PB, PA).max()) < K_TOL and s < total

        def add(name, n, fAs, fBs, cls, g, acc, **kw):
            for k in range(n):
                fA, fB = fAs[k % len(fAs)], fBs[rng.integers(len(fBs))]
                c = cls if isinstance(cls, str) else cls[rng.integers(len(cls))]
                recs.append(self._try(fA, fB, c, g, acc, **kw))
                groups.append(name)

        add("flat", 450, STATICS, self.POLYB, "par", gap, anyc, tilt=lambda: rng.uniform(-1e-4, 1e-4))
        add("tilted", 450, STATICS, self.POLYB, "b_on_a", gap, anyc)
        for f in (F_P1, F_P2):  # the static polygon's vertex on the racket's long face: the racket is the reference
            self.shapes[f].pick_edge = longest(self.shapes[f])
        add("refB_racket", 250, STATICS[2:], (F_P1, F_P2), "a_on_b", gap, anyc)
        for f in (F_P1, F_P2):
            self.shapes[f].pick_edge = None
        add("refB", 200, STATICS, self.POLYB, "a_on_b", gap, anyc)
        add("tie", 350, STATICS, self.POLYB, "par", lambda: total + rng.uniform(-0.05, -0.001), tie,
            tilt=lambda: rng.choice([-1, 1]) * float(np.exp(rng.uniform(np.log(1e-5), np.log(3e-3)))))
        add("end", 300, STATICS, self.POLYB, "b_on_a", gap, anyc, end_off=lambda: rng.uniform(-0.03, 0.03))
        add("vertex", 150, STATICS, self.POLYB, "vv", gap, anyc)
        add("rackets", 300, (F_P1,), (F_P2,), ("par", "b_on_a", "a_on_b", "vv"), gap, anyc)
        # the puck against every static fixture and both rackets
        ctot = G.POLY_RADIUS + self.shapes[F_PK].radius
        cgap = lambda: ctot + rng.uniform(-0.05, 0.03)
        CA = STATICS + (F_P1, F_P2)
        add("c_face", 200, CA, (F_PK,), "b_on_a", cgap, lambda PA, PB, d, s: G.closest_class(PA, PB) == "b_on_a")
        vtx = lambda PA, PB, d, s: d > 1e-3 and G.closest_class(PA, PB) == "vv"
        add("c_vertex_lo", 200, CA, (F_PK,), "vv", cgap, vtx, cone=lambda: rng.uniform(0.03, 0.47))
        add("c_vertex_hi", 200, CA, (F_PK,), "vv", cgap, vtx, cone=lambda: rng.uniform(0.53, 0.97))
        add("c_inside", 199, CA, (F_PK,), "b_on_a", lambda: rng.uniform(-0.1, -1e-4), lambda PA, PB, d, s: s < -5e-5)
        return self._shuffle(recs, groups)

    # ---- family T
    def _family_T(self):
        rng = self.rng
        recs, groups, rots = [], [], []
        tol = G.TOI_TOL
        for rot_cls, rmax in (("none", 0.0), ("half", 0.5), ("max", MAX_ROTATION)):
            for kind in ("hit", "near", "miss", "start_in", "start_over", "fast"):
                for k in range(self.NT):
                    fA = STATICS[k % len(STATICS)]
                    fB = (F_PK, F_P1, F_P2)[rng.integers(3)]
                    A, B = self.shapes[fA], self.shapes[fB]
                    target = G.toi_target(A.radius + B.radius)
                    lc = self.body[fB, 2:4].astype(np.float64)
                    xa = self._pose_A(fA)
                    PA = G.world(A.v32, xa)[0]
                    NA = _normals64(PA)
                    poly_cls = ("vv", "b_on_a") if fB == F_PK else ("vv", "b_on_a", "a_on_b", "par")
                    for _ in range(200):
                        cls = poly_cls[rng.integers(len(poly_cls))]
                        tstar = rng.uniform(0.1, 0.9)
                        perp = lambda u: np.array([-u[1], u[0]]) * rng.choice([-1, 1])
                        if kind == "hit":
                            g, length = target, rng.uniform(0.1, MAX_TRANSLATION)
                            dirf = lambda u: _rot(rng.uniform(-1, 1)) @ (-u)
                        elif kind == "near":
                            cls, g = "vv", target + rng.choice([-1, 1]) * 4 * tol
                            length, dirf = rng.uniform(0.2, MAX_TRANSLATION), perp
                        elif kind == "miss":
                            cls, g = "vv", rng.uniform(0.1, 1.0)
                            length, dirf = rng.uniform(0.2, MAX_TRANSLATION), perp
                        elif kind == "start_in":
                            tstar, g = 0.0, rng.uniform(0.1 * target, target + tol)
                            length, dirf = rng.uniform(0.0, 1.0), lambda u: _rot(rng.uniform(-np.pi, np.pi)) @ u
                        elif kind == "start_over":
                            tstar, g = 0.0, rng.uniform(-0.1, -0.001)
                            length, dirf = rng.uniform(0.0, 1.0), lambda u: _rot(rng.uniform(-np.pi, np.pi)) @ u
                        else:  # fast: from in front of a face right through A
                            cls, tstar, g = "b_on_a", 0.0, rng.uniform(0.2, 0.8)
                            length, dirf = rng.uniform(1.5, MAX_TRANSLATION), lambda u: -u
                        th, p, u = aim(rng, PA, NA, B, cls, g)
                        delta = length * dirf(u)
                        dth = rng.uniform(-rmax, rmax)
                        cstar = p + _rot(th) @ lc
                        c0, c1 = cstar - tstar * delta, cstar + (1 - tstar) * delta
                        if not (in_rink(c0, 1.5) and in_rink(c1, 1.5)):
                            continue
                        rec = np.zeros((), TOI)
                        rec["fA"], rec["fB"], rec["tMax"] = fA, fB, 1.0
                        rec["sA"] = (0, 0, xa[0], xa[1], xa[0], xa[1], 0, 0)
                        rec["sB"] = (lc[0], lc[1], c0[0], c0[1], c1[0], c1[1], th - tstar * dth, th + (1 - tstar) * dth)
                        if rmax == 0.0:
                            rec["sB"][7] = rec["sB"][6]
                        recs.append(rec)
                        groups.append(kind)
                        rots.append(rot_cls)
                        break
                    else:
                        raise AssertionError(("no accepted sweep", fA, fB, kind))
        recs.pop()
        groups.pop()
        rots.pop()
        return self._shuffle(recs, groups, rots)


@functools.lru_cache(None)
def committed():
    """The committed batch (seed 0) and the sweep models of its T cases: computed once, shared, never changed."""
    c = Cases(0)
    return c, models(c)


def models(c):
    out = []
    for r in c.T:
        out.append(G.SweepModel(c.shapes[r["fA"]].v32, r["sA"], c.shapes[r["fB"]].v32, r["sB"]))
    return out


# ------------------------------------------------------------------------------------------------ the laws
class Dev(dict):
    """Worst deviation per law (what `bar` / `ubar` must cover) and counts."""

    def worst(self, key, x):
        self[key] = max(self.get(key, 0.0), float(x))

    def count(self, key, n=1):
        self[key] = self.get(key, 0) + int(n)


def _xf(x, v):
    px, py, s, c = (float(k) for k in x)
    v = np.asarray(v, np.float64)
    return np.array([c * v[0] - s * v[1] + px, s * v[0] + c * v[1] + py])


def _rotv(x, v):
    s, c = float(x[2]), float(x[3])
    return np.array([c * v[0] - s * v[1], s * v[0] + c * v[1]])


def check_D(c, out, dev, bar):
    bad = []
    for i, (r, o) in enumerate(zip(c.D, out)):
        A, B = c.shapes[r["fA"]], c.shapes[r["fB"]]
        PA, PB = G.world(A.v32, r["xa"]), G.world(B.v32, r["xb"])
        d, s = (float(k[0]) for k in G.distance(PA, PB))
        dist, distr, n = float(o["dist"]), float(o["dist_radii"]), int(o["count"])
        dev.worst("D1_dist", abs(dist - d))
        if dist != 0.0 and s < 0:
            dev.worst("D1_overlap", -s)  # an overlap this deep still got a non-zero distance
        exp = max(0.0, d - A.radius - B.radius)
        dev.worst("D1_radii", abs(distr - exp))
        if not (1 <= n <= 3) or not all(0 <= o["iA"][k] < A.count and 0 <= o["iB"][k] < B.count for k in range(n)):
            bad.append(("D2 cache", i, n))
            continue
        # D2: the cache names features whose own float64 distance is d64 (three pairs: an overlap, d64 = 0)
        d2 = d if n == 3 else abs(G.feature_distance(PA[0], list(o["iA"][:n]), PB[0], list(o["iB"][:n])) - d)
        dev.worst("D2_feature", d2)
        if bar is not None and d2 > bar:
            bad.append(("D2", i, str(c.Dgroup[i]), n, d2))
        dev.count("D_simplex%d" % n)
        g = str(c.Dgroup[i])
        dev.count("D_" + g)
        if bar is not None:
            ok = abs(dist - d) <= bar and (dist == 0.0 or -s <= bar) and abs(distr - exp) <= bar
            if not ok:
                bad.append(("D1", i, g, dist, distr, d, s))
    return bad


def _ids_ok(idw, nA, nB):
    ia, ib, ta, tb = idw & 0xFF, (idw >> 8) & 0xFF, (idw >> 16) & 0xFF, (idw >> 24) & 0xFF
    return ia < nA and ib < nB and ta in (0, 1) and tb in (0, 1)


def check_M(c, out, dev, bar, ubar):
    bad = []
    for i, (r, o) in enumerate(zip(c.M, out)):
        A, B = c.shapes[r["fA"]], c.shapes[r["fB"]]
        g = str(c.Mgroup[i])
        PA, PB = G.world(A.v32, r["xa"]), G.world(B.v32, r["xb"])
        d, s = (float(k[0]) for k in G.distance(PA, PB))
        total = A.radius + B.radius
        n, typ = int(o["count"]), int(o["type"])
        ln, lp = o["ln"].astype(np.float64), o["lp"].astype(np.float64)
        fail = lambda law, *a: bad.append((law, i, g) + a)
        if B.circle:
            # M1: one point exactly when the centre is within the total radius of the core polygon
            if n == 0:
                dev.worst("M1c", total - d)
            else:
                dev.worst("M1c", d - total)
            if bar is not None and abs(d - total) <= bar:
                dev.count("M_dropped_" + g)
            elif bar is not None and n != (1 if d < total else 0):
                fail("M1 circle", n, d - total)
            dev.count("Mc_count%d" % n)
            dev.count("Mc_%s_count%d" % (g, n))
            if n == 0:
                continue
            if n != 1 or typ != 1 or int(o["id0"]) != 0 or not np.array_equal(o["p0"], B.v32[0]):
                fail("M3 circle point", n, typ)
            dev.worst("M2_unit", abs(np.hypot(*ln) - 1))
            nw = _rotv(r["xa"], ln)
            C = PB[0, 0]
            (dqp, uqp) = G.vertex_edge(PA, PB)[1]
            e = int(np.argmin(dqp[0, 0]))
            ea, eb = PA[0, e], PA[0, (e + 1) % A.count]
            closest = ea + uqp[0, 0, e] * (eb - ea)
            lpw = _xf(r["xa"], lp)
            dev.worst("M3_boundary", G.boundary_distance(PA[0], lpw))
            if s > 1e-4:  # outside: the unit vector from the closest core point to the centre
                dev.worst("M2c_normal", np.linalg.norm(nw - (C - closest) / d) * d)
                dev.worst("M3c_lp", abs(np.dot(closest - lpw, nw)))
                dev.count("Mc_vertex" if uqp[0, 0, e] in (0.0, 1.0) else "Mc_face")
                if bar is not None and (np.linalg.norm(nw - (C - closest) / d) * d > bar or abs(np.dot(closest - lpw, nw)) > bar):
                    fail("M2 circle normal", d)
            elif s < -1e-4:  # inside: the face of least penetration
                fs = G.face_seps(PA, PB)[0]
                k = int(np.argmin(np.linalg.norm(0.5 * (A.v + np.roll(A.v, -1, 0)) - lp, axis=1)))
                dev.worst("M2_face_normal", np.linalg.norm(ln - A.N[k]))
                dev.worst("M2c_inside", fs.max() - fs[k])
                dev.count("Mc_inside")
                if bar is not None and (fs.max() - fs[k] > bar or np.linalg.norm(ln - A.N[k]) > ubar):
                    fail("M2 circle inside", fs.max() - fs[k])
            if bar is not None and (abs(np.hypot(*ln) - 1) > ubar or G.boundary_distance(PA[0], lpw) > bar):
                fail("M2 circle unit / lp")
            continue
        # ---- polygon pairs.  M1
        root2 = np.sqrt(2.0)
        if n == 0:
            dev.worst("M1", total - d)
        else:
            dev.worst("M1", d - root2 * total)
        if bar is not None:
            if abs(d - total) <= bar or abs(d - root2 * total) <= bar:
                dev.count("M_dropped_" + g)
            elif (d < total and n < 1) or (d > root2 * total and n != 0):
                fail("M1", n, d)
        dev.count("M_count%d" % n)
        if n == 0:
            continue
        if typ not in (1, 2) or n > 2:
            fail("M type / count", typ, n)
            continue
        dev.count("M_refA" if typ == 1 else "M_refB")
        dev.count("M_%s_count%d" % (g, n))
        R, I, xr, xi = (A, B, r["xa"], r["xb"]) if typ == 1 else (B, A, r["xb"], r["xa"])
        PR, PI = (PA, PB) if typ == 1 else (PB, PA)
        # M2: unit; the chosen reference face's normal; from A to B; the tie-break's interval
        k = int(np.argmin(np.linalg.norm(0.5 * (R.v + np.roll(R.v, -1, 0)) - lp, axis=1)))
        u_unit, u_face = abs(np.hypot(*ln) - 1), np.linalg.norm(ln - R.N[k])
        dev.worst("M2_unit", u_unit)
        dev.worst("M2_face_normal", u_face)
        nref = _rotv(xr, ln)
        nab = nref if typ == 1 else -nref
        fsR, fsI = G.face_seps(PR, PI)[0], G.face_seps(PI, PR)[0]
        sref = float(fsR[k])
        sep_ab = float((PB[0] @ nab).min() - (PA[0] @ nab).max())
        m2_ab = abs(sep_ab - sref)
        dev.worst("M2_a_to_b", m2_ab)
        sA, sB = (fsR.max(), fsI.max()) if typ == 1 else (fsI.max(), fsR.max())
        m2_best = float(fsR.max() - sref)  # the reference face is its polygon's best face
        m2_tie = float((sB - sA) - K_TOL) if typ == 1 else float(K_TOL - (sB - sA))  # B only if sB > sA + k_tol
        dev.worst("M2_best_face", m2_best)
        dev.worst("M2_tiebreak", m2_tie)
        if abs(sB - sA) < K_TOL:
            dev.count("M_tie_A" if typ == 1 else "M_tie_B")
        elif abs(sB - sA) < 2 * K_TOL:
            dev.count("M_neartie_A" if typ == 1 else "M_neartie_B")
        # M3: the points
        ids = [int(o["id0"]), int(o["id1"])][:n]
        if not all(_ids_ok(w, A.count, B.count) for w in ids) or (n == 2 and ids[0] == ids[1]):
            fail("M3 ids", ids)
        pts = [_xf(xi, o["p0"]), _xf(xi, o["p1"])][:n]
        vk = PR[0, k]
        seps = [float(np.dot(x - vk, nref)) for x in pts]
        m3_b = max(G.boundary_distance(PI[0], x) for x in pts)
        m3_r = max(seps) - total
        dev.worst("M3_boundary", m3_b)
        dev.worst("M3_within_radius", m3_r)
        # the smallest point separation is the face's SAT separation, when a deepest incident vertex is inside the
        # side planes (the reference face's ends pushed out by the total radius)
        tang = np.array([-nref[1], nref[0]])
        Lk = float(np.dot(PR[0, (k + 1) % R.count] - vk, tang))
        depth = (PI[0] - vk) @ nref
        tau = (PI[0] - vk) @ tang
        lo, hi = min(0.0, Lk) - total, max(0.0, Lk) + total
        deepest = depth <= depth.min() + 1e-6
        margin = 1e-4
        inside = deepest & (tau > lo + margin) & (tau < hi - margin)
        m3_s = None
        if inside.any():
            m3_s = abs(min(seps) - sref)
            dev.worst("M3_min_sep", m3_s)
            dev.count("M3_min_sep_n")
        else:
            dev.count("M3_min_sep_premise_not_met_" + g)
        if bar is not None:
            if u_unit > ubar or u_face > ubar:
                fail("M2 unit / face normal", u_unit, u_face)
            if m2_ab > bar:
                fail("M2 A to B", sep_ab, sref)
            if m2_best > bar or m2_tie > bar:
                fail("M2 tie-break", typ, sA, sB, sref)
            if m3_b > bar or m3_r > bar:
                fail("M3 boundary / radius", m3_b, m3_r)
            if m3_s is not None and m3_s > bar:
                fail("M3 min sep", min(seps), sref)
    return bad


def check_T(c, out, mods, dev, bar):
    bad = []
    tol = G.TOI_TOL
    for i, (r, o, m) in enumerate(zip(c.T, out, mods)):
        A, B = c.shapes[r["fA"]], c.shapes[r["fB"]]
        target = G.toi_target(A.radius + B.radius)
        g, rot = str(c.Tgroup[i]), str(c.Trot[i])
        st, t = int(o["state"]), float(o["t"])
        S0, S1 = float(m.sg[0]), float(m.sg[-1])
        fail = lambda law, *a: bad.append((law, i, g, rot, st, t) + a)
        dev.count("T_state%d" % st)
        dev.count("T_%s_state%d" % (g, st))
        if not (st in (FAILED, OVERLAPPED, TOUCHING, SEPARATED) and 0.0 <= t <= 1.0):
            fail("T state / t")
            continue
        smin = None
        if st == TOUCHING and t > 0:
            St = float(m.S([t])[0])
            smin = m.min_upto(t)
            dev.worst("T1_at_t", abs(St - target) - tol)
            dev.count("T1_n_" + rot)
            if bar is not None and abs(St - target) > tol + bar:
                fail("T1", St - target)
            if rot == "none":  # no earlier penetration: every separation function is linear in t
                dev.worst("T1_before_t", (target - tol) - smin)
                if bar is not None and smin < target - tol - bar:
                    fail("T1 before t", smin - target)
            elif smin < target - tol - (bar or 1e-5):
                # a rotating B can dip under the target between two root-finder samples and come back (the same
                # property of Box2D's algorithm as the rotating tunnel): counted, capped at MAX_DROPPED below
                dev.count("T_rot_touching_after_dip_" + rot)
        elif st == TOUCHING:
            dev.worst("T2_touching0", S0 - (target + tol))
            if bar is not None and not S0 < target + tol + bar:
                fail("T2 touching at 0", S0)
        elif st == SEPARATED:
            dev.worst("T2_separated", (target + tol) - S1)
            if bar is not None and not (S1 > target + tol - bar and t == 1.0):
                fail("T2 separated", S1)
        elif st == OVERLAPPED:
            dev.worst("T2_overlapped", S0)
            if bar is not None and not (S0 <= bar and t == 0.0):
                fail("T2 overlapped", S0)
        # T3 and the rotating classes' record
        full_min = m.min_upto(1.0)
        b = bar if bar is not None else 0.0
        crossed = S0 > target + tol + b and full_min < target - tol - b
        if rot == "none":
            if crossed:
                dev.count("T3_n")
                first = m.first_below(target - tol - b)
                if st != TOUCHING or (first is not None and t > first):
                    dev.count("T3_tunnel")
                    if bar is not None:
                        fail("T3", S0, full_min, first)
            elif bar is not None and (abs(S0 - target - tol) <= bar or abs(full_min - target + tol) <= bar):
                dev.count("T_dropped_T3")
            if st == FAILED:
                dev.count("T_failed_none")
        else:
            if st == SEPARATED and crossed:
                dev.count("T_rot_separated_but_crossed_" + rot)
            if st == FAILED:
                dev.count("T_rot_failed_" + rot)
    return bad


def check(c, outs, mods, tol=TOL, assert_laws=True):
    """All laws on one build's outputs; returns the figures.  tol=None only measures (no law is asserted)."""
    dev = Dev()
    bar, ubar = (None, None) if tol is None else (tol["bar"], tol["ubar"])
    bad = check_D(c, outs["D"], dev, bar) + check_M(c, outs["M"], dev, bar, ubar) + check_T(c, outs["T"], mods, dev, bar)
    if tol is not None:
        for g in np.unique(c.Mgroup):  # cases within `bar` of a deciding threshold
            n = int((c.Mgroup == g).sum())
            assert dev.get("M_dropped_" + str(g), 0) <= MAX_DROPPED * n, (g, dev.get("M_dropped_" + str(g)), n)
        assert dev.get("T_dropped_T3", 0) <= MAX_DROPPED * max(1, dev.get("T3_n", 0)), dev.get("T_dropped_T3")
        for rot in ("half", "max"):
            dip = dev.get("T_rot_touching_after_dip_" + rot, 0)
            assert dip <= MAX_DROPPED * dev.get("T1_n_" + rot, 0), (rot, dip)
        for key, least in MIN_COVER.items():
            assert dev.get(key, 0) >= least, ("coverage", key, dev.get(key, 0), least)
    if assert_laws:
        assert not bad, (len(bad), bad[:12])
    dev["violations"] = bad
    return dev


def rotating_record(dev):
    return {k: v for k, v in dev.items() if k.startswith("T_rot_")}


if __name__ == "__main__":
    if "--measure" in sys.argv:
        worst = Dev()
        for seed in [0] + list(range(1000, 1010)):
            c = Cases(seed)
            dv = check(c, run_all(oracle_probe(), c), models(c), tol=None, assert_laws=False)
            for k, v in dv.items():
                if isinstance(v, float):
                    worst.worst(k, v)
            print(seed, {k: (round(v, 9) if isinstance(v, float) else v) for k, v in sorted(dv.items()) if k != "violations"},
                  flush=True)
        print("WORST", {k: v for k, v in sorted(worst.items())})

"""Seeded scenes for the float64 rigid-body laws of tests/physics_ref.py, and the figures measured on them.

A scene is one arena's raw state put in place with set_state after a reset, then K steps with `debug`.  Families:
  A   free flight: everything well apart, random velocities, spins and angles
  B1  puck into player 1's racket, B2 into player 2's (random angle, velocity, spin; some with a fast-spinning puck)
  C   racket into racket across the centre line (polygon-polygon, the two-point block solver)
  D   puck into the top / bottom wall, zero actions, a few on either side of the restitution threshold
  E   head-on 1-D hit on a racket at rest, both rackets, six speeds
  F   puck fired at a wall at 30-60 m/s (continuous collision)
measure() reduces a trajectory to worst deviations and coverage counts; check() holds them to the tolerances below.
Both the CPU test (oracle, host build of the kernel source) and the GPU test use the same two functions.  numpy only.
"""
import numpy as np

import physics_ref as P

K = 6
E_SPEEDS = (0.5, 0.9, 1.2, 3.0, 8.0, 20.0)
HOME = ((2.0, 4.0), (8.0, 4.0))  # where a parked racket stands
PUCK_PARK = (5.0, 1.6)

# Tolerances: 4 x the worst deviation of the CPU oracle from the float64 model, measured over ten batches of other
# seeds (1000-1009: ten times the committed sample) and the test's own seed 0; DESIGN.md "Float64 rigid-body laws"
# has the table.  The deviation is accumulated float32 rounding of <= 180 solver iterations; every variant and
# mutation the tests name sits four to five orders of magnitude above it.
TOL = {
    "A_dev": 4 * 3.2e-7,        # worst 3.2e-7 of |got - want| / max(1, |want|): a few float32 ulp
    "B_momentum": 4 * 3.8e-7,   # worst 3.8e-7
    "C_momentum": 4 * 3.4e-6,   # worst 3.4e-6 (slow rackets: a small denominator)
    "B_angular": 4 * 1.9e-7,    # worst 1.9e-7 (angular momentum about the rink's centre)
    "C_angular": 4 * 1.6e-6,    # worst 1.6e-6
    "B_energy": 4 * 9.8e-8,     # kinetic energy never rose by more than 9.8e-8 relative
    "C_energy": 4 * 2.7e-7,     # nor by more than 2.7e-7
    "D_vn": 4 * 2.5e-7,         # worst 2.5e-7 of |v_n' + e v_n| / max(1, |v_n|)
    "D_cone": 4 * 1.2e-7,       # worst 1.2e-7 of (|j_t| - mu j_n) / (m max(1, |v_t|, |omega| r))
    "D_slide_or_stick": 4 * 1.1e-6,  # worst 1.1e-6, same scale (the sticking slip weighted by min(1, |d_v_t|))
    "E_rel": 4 * 1.8e-7,        # worst 1.8e-7 relative to the incoming speed (the twelve scenes are not seeded)
    # Reasoned, not measured (the oracle's worst: ratio 0.99997, off-axis motion exactly 0).  B_coulomb: the ratio is
    # built from the puck's velocity change of at least COULOMB_MIN_DV = 0.1 m/s, each component known to an ulp of
    # 25 m/s (1.9e-6), so to 2e-5 relative per component.  E_off_axis: one float32 epsilon of the incoming speed.
    "B_coulomb": 1e-4,
    "E_off_axis": 1.2e-7,
}
# D's lever arm rho = -I d_omega / j_t is asserted inside [r - 3 linearSlop, r] (Box2D puts the contact point between
# the two skins) with no blanket slack: each bounce carries the error bar of its own float32 inputs,
# (I ulp(omega) + r m ulp(v_t)) / (m |d_v_t|), and only bounces with |d_v_t| >= RHO_MIN_DVT have an arm at all.
# F's containment (the rink shrunk by r - 3 linearSlop) has no slack either.
RHO_MIN_DVT = 0.02
COULOMB_MIN_DV = 0.1
MIN_COUNTS = {"B1_contacts": 100, "B2_contacts": 100, "C_contacts": 30, "D_sliding": 20, "D_sticking": 20,
              "B_near_cone": 10}
MAX_DROPPED = 0.10


class Batch:
    """state[N,18], aux[N,5], actions[K,N,8] and per-arena labels, the families interleaved by a seeded shuffle."""

    def __init__(self, keep_mode, seed=0, scale=1):
        rng = np.random.default_rng([seed, int(keep_mode)])
        rows = _family_a(rng, 60 * scale)
        if not keep_mode:  # B-F run without possession: no hold law may rewrite the puck before the solve
            rows += _family_b(rng, 0, 230 * scale) + _family_b(rng, 1, 230 * scale) + _family_c(rng, 220 * scale)
            rows += _family_d(rng, 150 * scale) + _family_e() + _family_f(rng, 40 * scale)
            rows += _family_a(rng, 1)  # 60 + 460 + 220 + 150 + 12 + 40 + 1 = 943 arenas: a partial last wave
        order = rng.permutation(len(rows))
        rows = [rows[i] for i in order]
        self.keep_mode = bool(keep_mode)
        self.n = len(rows)
        self.family = np.array([r[0] for r in rows])
        self.state = np.array([r[1] for r in rows], np.float32)
        self.tag = np.array([r[2] for r in rows], np.float64)  # D: +1 top / -1 bottom wall; E: the listed speed
        self.aux = np.zeros((self.n, 5), np.int32)
        self.actions = rng.uniform(-1, 1, (K, self.n, 8)).astype(np.float32)
        self.actions[:, np.isin(self.family, ("D", "E", "F"))] = 0.0
        for a in (self.state, self.aux, self.actions):
            a.setflags(write=False)


def _row(p1, p2, pk):
    return np.concatenate([p1, p2, pk])


def _parked(i):
    return np.array([HOME[i][0], HOME[i][1], 0, 0, 0, 0], np.float64)


def _family_a(rng, n):
    rows = []
    for _ in range(n):
        u = rng.uniform
        p1 = [u(2.4, 2.7), u(3, 5), u(-0.9, 0.9), u(-2, 2), u(-2, 2), u(-5, 5)]
        p2 = [u(7.3, 7.6), u(3, 5), u(-0.9, 0.9), u(-2, 2), u(-2, 2), u(-5, 5)]
        pk = [u(4.7, 5.3), u(2, 6), u(-3, 3), u(-3, 3), u(-3, 3), u(-40, 40)]
        rows.append(("A", _row(p1, p2, pk), 0.0))
    return rows


def _family_b(rng, who, n):
    rows = []
    for k in range(n):
        u = rng.uniform
        x = u(2.7, 3.8) if who == 0 else u(6.2, 7.3)
        rk = np.array([x, u(2.4, 5.6), u(-0.9, 0.9), u(-3, 3), u(-3, 3), u(-5, 5)])
        th = u(0, 2 * np.pi)
        d = np.array([np.cos(th), np.sin(th)])  # racket origin -> puck
        t = np.array([-d[1], d[0]])
        grazing = k % 2 == 0  # every other: a fast-spinning, slowly closing puck, to reach the cone's edge
        if grazing:  # just off the racket's surface (its support along d); spin below Box2D's rotation clamp, 78.5
            c, s = np.cos(rk[2]), np.sin(rk[2])
            vw = P.VERTS[who] @ np.array([[c, s], [-s, c]])
            dist = (vw @ d).max() + P.R + u(0.02, 0.08)
            spin, close, side = u(40, 70) * rng.choice([-1, 1]), u(1, 4), u(-2, 2)
        else:
            dist, spin, close, side = u(0.75, 1.1), u(-20, 20), u(0, 25), u(-4, 4)
        v = -close * d + side * t
        pk = np.concatenate([rk[:2] + dist * d, [u(-3, 3)], v, [spin]])
        rows.append(("B%d" % (who + 1), _row(rk, _parked(1), pk) if who == 0 else _row(_parked(0), rk, pk), 0.0))
    return rows


def _extent(verts, a, sign):
    c, s = np.cos(a), np.sin(a)
    return (sign * (c * verts[:, 0] - s * verts[:, 1])).max()


def _family_c(rng, n):
    """Faces at most 0.04 apart in x.  The centre-zone law reverses a racket's x velocity towards the line, so the
    closing speed comes from spin and from y motion of the tilted faces."""
    rows = []
    for _ in range(n):
        u = rng.uniform
        a1, a2 = u(-0.5, 0.5), u(-0.5, 0.5)
        line, gap = 5 + u(-0.1, 0.1), u(0.0, 0.04)
        y1 = u(3, 5)
        x1 = line - gap / 2 - _extent(P.VERTS[0], a1, +1)
        x2 = line + gap / 2 + _extent(P.VERTS[1], a2, -1)
        p1 = [x1, y1, a1, u(0, 4), u(-6, 6), u(-12, 12)]
        p2 = [x2, y1 + u(-0.5, 0.5), a2, u(-4, 0), u(-6, 6), u(-12, 12)]
        rows.append(("C", _row(p1, p2, [PUCK_PARK[0], PUCK_PARK[1], 0, 0, 0, 0]), 0.0))
    return rows


def _family_d(rng, n):
    rows = []
    for k in range(n):
        u = rng.uniform
        wall = 1.0 if k % 2 == 0 else -1.0
        if k % 10 == 8:
            vn, gap = u(0.5, 0.98), u(0.012, 0.03)  # below the restitution threshold
        elif k % 10 == 9:
            vn, gap = u(1.02, 1.5), u(0.012, 0.05)  # just above it
        else:
            vn = u(6, 24)
            gap = u(0.05, 3 * vn * P.DT)
        y = (P.Y_TOP - P.R - gap) if wall > 0 else (P.Y_BOT + P.R + gap)
        pk = [u(4.2, 5.8), y, 0.0, u(-10, 10), wall * vn, u(-40, 40)]
        rows.append(("D", _row(_parked(0), _parked(1), pk), wall))
    return rows


def _family_e():
    rows = []
    for who in (0, 1):
        sgn = 1.0 if who == 0 else -1.0  # player 1's flat face looks along +x, player 2's along -x
        for v in E_SPEEDS:
            rk = np.array([2.5 if who == 0 else 7.5, 4.0, 0, 0, 0, 0])
            gap = 1.5 * v * P.DT
            pk = [rk[0] + sgn * (0.1 + P.R + gap), 4.0 + P.LC[who, 1], 0.0, -sgn * v, 0.0, 0.0]
            rows.append(("E", _row(rk, _parked(1), pk) if who == 0 else _row(_parked(0), rk, pk), sgn * v))
    return rows


def _family_f(rng, n):
    rows = []
    for k in range(n):
        u = rng.uniform
        sp = u(30, 60)
        if k % 2 == 0:  # top / bottom wall, far from the posts
            sgn = 1.0 if k % 4 == 0 else -1.0
            y = (P.Y_TOP if sgn > 0 else P.Y_BOT) - sgn * u(0.4, 3.0)
            pk = [u(3.5, 6.5), y, 0.0, u(-5, 5), sgn * sp, u(-40, 40)]
        else:  # the posts' faces, below / above the goal mouth
            sgn = 1.0 if k % 4 == 1 else -1.0
            y = u(1.3, 2.1) if k % 8 < 4 else u(5.9, 6.7)
            x = (P.X_RIGHT if sgn > 0 else P.X_LEFT) - sgn * u(0.4, 3.0)
            pk = [x, y, 0.0, sgn * sp, u(-3, 3), u(-40, 40)]
        rows.append(("F", _row(_parked(0), _parked(1), pk), 0.0))
    return rows


# ---------------------------------------------------------------------------------------------------- measurement
def measure(batch, S, D):
    """S[K+1,N,18] the raw states before / after each step, D[K,N,13] each step's debug row -> figures and counts."""
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    fam = batch.family
    ff = np.stack([P.free_flight(S[k], D[k]) for k in range(K)])
    dev = np.stack([P.deviation(S[k + 1], ff[k]) for k in range(K)])  # [K,N]
    pre = [P.presolve(S[k], D[k]) for k in range(K)]
    free = dev <= TOL["A_dev"]
    out = {}

    a = fam == "A"
    out["A_apart"] = all((P.well_apart(S[k][a], S[k + 1][a]) & P.clear_of_walls(S[k][a], S[k + 1][a])).all()
                         for k in range(K))
    out["A_steps"] = int(a.sum()) * K
    out["A_dev"] = float(dev[:, a].max())

    n_contact = n_dropped = 0
    out["B_near_cone"] = 0
    for name in ("B1", "B2", "C"):
        sel = fam == name
        mom, ang, en, cone, count = 0.0, 0.0, -np.inf, 0.0, 0
        for k in range(K):
            hit = sel & ~free[k]
            clear = P.clear_of_walls(S[k], S[k + 1])
            n_contact += int(hit.sum())
            n_dropped += int((hit & ~clear).sum())
            hit &= clear
            if not hit.any():
                continue
            count += int(hit.sum())
            vs, ws = pre[k][0][hit], pre[k][1][hit]
            s1 = S[k + 1][hit]
            mom = max(mom, float(P.momentum_residual(s1, vs).max()))
            ang = max(ang, float(P.angular_momentum_residual(S[k][hit], s1, vs, ws).max()))
            _, _, v1, w1 = P.bodies(s1)
            en = max(en, float((P.kinetic_energy(v1, w1) / P.kinetic_energy(vs, ws) - 1).max()))
            if name != "C":
                ratio, J = P.coulomb_ratio(vs, ws, s1, P.MU_RACKET)
                ratio = ratio[J > COULOMB_MIN_DV * P.M[2]]  # a puck the step barely pushed has no direction to bound
                if len(ratio):
                    cone = max(cone, float(ratio.max()))
                    out["B_near_cone"] += int((ratio > 0.98).sum())
        out[name + "_contacts"], out[name + "_momentum"], out[name + "_energy"] = count, mom, en
        out[name + "_angular"] = ang
        if name != "C":
            out[name + "_coulomb"] = cone
    out["BC_dropped"] = n_dropped / max(n_contact, 1)

    # D: the first step that is not free flight is the bounce
    vn_err, cone, rho_lo, rho_hi, rho_out, sos = 0.0, -np.inf, np.inf, -np.inf, -np.inf, 0.0
    sliding = sticking = bounces = no_arm = 0
    d_log = []
    for i in np.nonzero(fam == "D")[0]:
        ks = np.nonzero(~free[:, i])[0]
        if not len(ks):
            continue
        k, s = int(ks[0]), batch.tag[i]
        bounces += 1
        vx, vy, w = pre[k][0][i, 2, 0], pre[k][0][i, 2, 1], pre[k][1][i, 2]
        _, _, v1, w1 = P.bodies(S[k + 1][i:i + 1])
        vx1, vy1, w1 = v1[0, 2, 0], v1[0, 2, 1], w1[0, 2]
        err = abs(vy1 - P.wall_bounce(vy)) / max(1.0, abs(vy))
        d_log.append((float(vy), float(vy1)))
        vn_err = max(vn_err, float(err))
        jn = P.M[2] * (1 + float(P.restitution(vy))) * abs(vy)
        jt = P.M[2] * (vx1 - vx)
        scale = P.M[2] * max(1.0, abs(vx), abs(w) * P.R)  # float32 resolves v_t and omega r to an ulp of themselves
        cone = max(cone, (abs(jt) - P.MU_WALL * jn) / scale)
        if abs(vx1 - vx) < RHO_MIN_DVT:
            no_arm += 1
            continue
        rho = -s * P.I[2] * (w1 - w) / jt  # contact point at s * rho above the centre: I d_omega = -s rho j_t
        rho_lo, rho_hi = min(rho_lo, rho), max(rho_hi, rho)
        bar = (P.I[2] * np.spacing(np.float32(max(abs(w), abs(w1)))) + P.R * P.M[2] * np.spacing(
            np.float32(max(abs(vx), abs(vx1))))) / abs(jt)
        rho_out = max(rho_out, P.R - 3 * P.LINEAR_SLOP - rho - bar, rho - P.R - bar)
        slip0, slip1 = vx - s * w * rho, vx1 - s * w1 * rho
        slide = abs(abs(jt) - P.MU_WALL * jn) / scale if jt * slip0 < 0 else np.inf  # friction opposes the slip
        stick = abs(slip1) * min(1.0, abs(vx1 - vx)) * P.M[2] / scale  # rho, hence the slip, is known to ~1 / |d_v_t|
        sliding += slide <= stick
        sticking += stick < slide
        sos = max(sos, float(min(slide, stick)))
    out.update(D_bounces=bounces, D_vn=vn_err, D_cone=float(cone), D_rho_lo=float(rho_lo), D_rho_hi=float(rho_hi),
               D_rho_out=float(rho_out), D_slide_or_stick=sos, D_sliding=int(sliding), D_sticking=int(sticking),
               D_no_arm=no_arm, D_log=d_log,
               D_sub_threshold=sum(1 for v, _ in d_log if abs(v) <= P.V_THRESH),
               D_near_threshold=sum(1 for v, _ in d_log if P.V_THRESH < abs(v) < 1.6))

    # E: the first step that is not free flight is the hit
    rel, off, seen, e_log = 0.0, 0.0, set(), {}
    for i in np.nonzero(fam == "E")[0]:
        ks = np.nonzero(~free[:, i])[0]
        if not len(ks):
            continue
        k = int(ks[0])
        who = 0 if batch.tag[i] > 0 else 1
        seen.add((who, abs(batch.tag[i])))
        v_in = pre[k][0][i, 2, 0]
        want_p, want_r = P.head_on(v_in, P.M[who])
        _, _, v1, w1 = P.bodies(S[k + 1][i:i + 1])
        rel = max(rel, abs(v1[0, 2, 0] - want_p) / abs(v_in), abs(v1[0, who, 0] - want_r) / abs(v_in))
        off = max(off, *(np.abs([v1[0, 2, 1], v1[0, who, 1], w1[0, 2], w1[0, who]]) / abs(v_in)))
        e_log[(who, abs(batch.tag[i]))] = (float(v_in), float(v1[0, 2, 0]), float(want_p))
    out.update(E_rel=float(rel), E_off_axis=float(off), E_seen=seen, E_log=e_log)

    # F: the puck centre stays inside the rink shrunk by r - 3 linearSlop, after every step
    f = fam == "F"
    pk = S[1:, f, 12:14]
    d = P.R - 3 * P.LINEAR_SLOP
    out["F_out"] = float(max((P.X_LEFT + d - pk[..., 0]).max(), (pk[..., 0] - (P.X_RIGHT - d)).max(),
                             (P.Y_BOT + d - pk[..., 1]).max(), (pk[..., 1] - (P.Y_TOP - d)).max())) if f.any() else 0.0
    out["F_bounces"] = int((~free[:, f]).any(0).sum())
    return out


def check(m, full=True):
    """Every law within its tolerance, and the scenes' coverage conditions.  full=False: a keep-mode batch (A only)."""
    assert m["A_apart"] and m["A_steps"] > 0, "free-flight scenes must stay apart and clear of walls"
    assert m["A_dev"] <= TOL["A_dev"], ("A free flight", m["A_dev"])
    if not full:
        return
    assert m["BC_dropped"] <= MAX_DROPPED, m["BC_dropped"]
    for k, v in MIN_COUNTS.items():
        assert m[k] >= v, (k, m[k], v)
    for name in ("B1", "B2", "C"):
        fam = name[0]
        assert m[name + "_momentum"] <= TOL[fam + "_momentum"], (name, "momentum", m[name + "_momentum"])
        assert m[name + "_angular"] <= TOL[fam + "_angular"], (name, "angular momentum", m[name + "_angular"])
        assert m[name + "_energy"] <= TOL[fam + "_energy"], (name, "kinetic energy rose", m[name + "_energy"])
    for name in ("B1", "B2"):
        assert m[name + "_coulomb"] <= 1 + TOL["B_coulomb"], (name, "Coulomb cone", m[name + "_coulomb"])
    assert m["D_bounces"] >= 0.9 * 150 and m["D_sub_threshold"] >= 5 and m["D_near_threshold"] >= 5, (
        m["D_bounces"], m["D_sub_threshold"], m["D_near_threshold"])
    assert m["D_no_arm"] <= 0.05 * m["D_bounces"], m["D_no_arm"]
    assert m["D_vn"] <= TOL["D_vn"], ("D normal velocity", m["D_vn"])
    assert m["D_cone"] <= TOL["D_cone"], ("D |j_t| <= mu j_n", m["D_cone"])
    assert m["D_rho_out"] <= 0.0, ("D lever arm outside [r - 3 slop, r]", m["D_rho_lo"], m["D_rho_hi"])
    assert m["D_slide_or_stick"] <= TOL["D_slide_or_stick"], ("D sliding or sticking", m["D_slide_or_stick"])
    assert m["E_seen"] == {(w, v) for w in (0, 1) for v in E_SPEEDS}, m["E_seen"]
    assert m["E_rel"] <= TOL["E_rel"], ("E head-on", m["E_rel"], m["E_log"])
    assert m["E_off_axis"] <= TOL["E_off_axis"], ("E rotation / y motion", m["E_off_axis"])
    assert m["F_bounces"] >= 30, m["F_bounces"]
    assert m["F_out"] <= 0.0, ("F containment", m["F_out"])


def run(env, batch, aux=False):
    """Drive an implementation (the call shapes of tests/scene_lockstep.py) through the batch: (S[K + 1, N, 18],
    D[K, N, 13]).  aux=True: also the aux rows before / after each step and each step's done flags, (S, D, A, done)."""
    env.set_state(batch.state, batch.aux)
    S, D, A, done = [batch.state.copy()], [], [batch.aux.copy()], []
    for k in range(K):
        r = env.step(batch.actions[k], debug=True)
        D.append(r.debug)
        done.append(r.done)
        st, ax = env.get_state()
        S.append(st)
        A.append(ax)
    return (np.stack(S), np.stack(D), np.stack(A), np.stack(done)) if aux else (np.stack(S), np.stack(D))

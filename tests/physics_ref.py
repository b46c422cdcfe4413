"""Float64 rigid-body laws for one world.Step of the hockey scene.  numpy only: TEST INFRASTRUCTURE.

Nothing here reads the solver (hk_solver.h / hk_velocity.h) or its CPU restatement (oracle/hk_oracle.c), and this
module must not import hockey_amd, oracle or hostcheck.  It states what ANY correct rigid-body step obeys -- the
pre-solve integration, free flight about the centre of mass, linear and angular momentum, energy, the Coulomb cone --
plus the closed forms of two scripted collisions, so that a misreading of Box2D made once in the oracle and copied
faithfully into the kernel still fails a test (tests/test_physics_ref.py, tests/test_gpu_physics_ref.py).

Layout of the arrays (include/hockey.h):
  s[N, 18]    raw state, three bodies (player 1, player 2, puck) x {x, y, angle, vx, vy, omega}, x / y the body ORIGIN
  dbg[N, 13]  the step's HK_DEBUG_DIM row {F1x, F1y, F2x, F2y, FPx, FPy, T1, T2, ld1, ld2, ldP, ad1, ad2}: the forces,
              torques and dampings the env's laws handed to world.Step (the dampings switch with speed and zone)
Mass data is the reference's own (tests/golden/g6_geometry.npz); the wall faces and material constants are numbers.
"""
import os

import numpy as np

_G6 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g6_geometry.npz")
with np.load(_G6, allow_pickle=False) as _z:
    _mass = np.stack([_z["player1_mass"][:6], _z["player2_mass"][:6], _z["puck_mass"][:6]]).astype(np.float64)
    R = float(_z["puck_mass"][6])  # puck radius
    VERTS = (_z["player1_verts"].astype(np.float64), _z["player2_verts"].astype(np.float64))

# per body (player 1, player 2, puck); I is the inertia about the centre of mass
M, INV_M, LC, I, INV_I = _mass[:, 0], _mass[:, 1], _mass[:, 2:4], _mass[:, 4], _mass[:, 5]
CIRCUM = float(max(np.linalg.norm(v, axis=1).max() for v in VERTS))  # racket circumradius about its origin, ~0.447

DT = float(np.float32(0.02))  # world.Step's float32 time step
LINEAR_SLOP = 0.005
E_REST, V_THRESH = 0.95, 1.0  # max(0.95, 0) restitution of every puck contact; Box2D's velocity threshold
MU_WALL = 0.1  # sqrt(0.1 * 0.1)
MU_RACKET = float(np.sqrt(0.1 * 1.0))
# inner faces of the rink: top / bottom walls, and the goal posts' faces left and right (outside the goal mouths)
Y_TOP, Y_BOT = 7.5 - 1.0 / 6, 0.5 + 1.0 / 6
X_LEFT, X_RIGHT = 5 - (245.0 / 60 - 1.0 / 6), 5 + (245.0 / 60 - 1.0 / 6)
MARGIN = 0.05  # clear_of_walls: five skins (2 * linearSlop) beyond touching
POLY_RADIUS = 0.01  # b2_polygonRadius = 2 * linearSlop: the skin of every polygon
BAUMGARTE, MAX_CORRECTION, POSITION_ITERATIONS = 0.2, 0.2, 60  # b2_baumgarte, b2_maxLinearCorrection, world.Step's
# goal boxes (sensor and solid fixture alike): half-size 10/60 x 75/60, centred at x = 5 -+ 245/60 -+ 10/60, y = 4
GOAL_HALF = (10.0 / 60, 75.0 / 60)
GOAL_CENTRE = ((5 - 245.0 / 60 - 10.0 / 60, 4.0), (5 + 245.0 / 60 + 10.0 / 60, 4.0))  # left (winner -1), right (+1)
# the posts' inner faces x = X_LEFT / X_RIGHT run from the wall down / up to this height (hockey_env.py:222-319: the
# post quad's inner vertex lies 128/60 from the wall body's centre line, the outer one 135/60)
POST_Y_BOT, POST_Y_TOP = 0.5 + 128.0 / 60, 7.5 - 128.0 / 60
POST_Y_BOT_OUTER, POST_Y_TOP_OUTER = 0.5 + 135.0 / 60, 7.5 - 135.0 / 60  # ... and 20/60 further out it ends here


def post_slant_face(right, up):
    """The post quad's face towards the goal mouth (hockey_env.py:222-319: the quad (-10, 135), (10, 128), (10, -5),
    (-10, -5) / 60 about (5 -+ 245/60, 0.5), mirrored for the other three): (inner end, outer end, unit normal into
    the mouth).  It slants by atan(7 / 20) = 19.3 degrees; the goal box covers its outer half."""
    inner = np.array([X_RIGHT if right else X_LEFT, POST_Y_TOP if up else POST_Y_BOT])
    outer = np.array([inner[0] + (1.0 if right else -1.0) / 3, POST_Y_TOP_OUTER if up else POST_Y_BOT_OUTER])
    d = outer - inner
    n = np.array([-d[1], d[0]]) / np.hypot(*d)
    return inner, outer, n if (n[1] > 0) != up else -n


def bodies(s):
    """s[N,18] -> (origin[N,3,2], angle[N,3], v[N,3,2], omega[N,3]) in float64."""
    b = np.asarray(s, np.float64).reshape(-1, 3, 6)
    return b[:, :, 0:2], b[:, :, 2], b[:, :, 3:5], b[:, :, 5]


def _rot(a, v):
    c, s = np.cos(a)[..., None], np.sin(a)[..., None]
    return np.concatenate([c * v[..., 0:1] - s * v[..., 1:2], s * v[..., 0:1] + c * v[..., 1:2]], -1)


def presolve(s0, dbg):
    """Velocities after world.Step's force / damping integration and before any contact impulse:
    v* = (v + dt F / m) / (1 + dt ld), omega* = (omega + dt T / I) / (1 + dt ad).  Returns (v*[N,3,2], omega*[N,3])."""
    _, _, v, w = bodies(s0)
    d = np.asarray(dbg, np.float64)
    n = len(d)
    F = d[:, 0:6].reshape(n, 3, 2)
    T = np.concatenate([d[:, 6:8], np.zeros((n, 1))], 1)  # no torque law acts on the puck
    ld = d[:, 8:11]
    ad = np.concatenate([d[:, 11:13], np.zeros((n, 1))], 1)  # the puck's angular damping is never set
    vs = (v + DT * F / M[None, :, None]) / (1 + DT * ld)[..., None]
    ws = (w + DT * T / I[None, :]) / (1 + DT * ad)
    return vs, ws


def free_flight(s0, dbg):
    """The state after a contact-free step: the CENTRE OF MASS moves with v*, the body turns about it with omega*."""
    o, a, _, _ = bodies(s0)
    vs, ws = presolve(s0, dbg)
    c = o + _rot(a, LC[None])
    c1 = c + DT * vs
    a1 = a + DT * ws
    o1 = c1 - _rot(a1, LC[None])
    return np.concatenate([o1, a1[..., None], vs, ws[..., None]], -1).reshape(-1, 18)


def deviation(got, want):
    """Largest |got - want| / max(1, |want|) of each arena's 18 entries."""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.abs(g - w) / np.maximum(1.0, np.abs(w))).max(-1)


def _inside(p, d):
    return (p[..., 0] > X_LEFT + d) & (p[..., 0] < X_RIGHT - d) & (p[..., 1] > Y_BOT + d) & (p[..., 1] < Y_TOP - d)


def clear_of_walls(s0, s1, margin=MARGIN):
    """No wall or post can have touched a body in this step: both racket origins stay farther than the circumradius
    from every inner face, the puck centre farther than r -- at s0, at s1, and (puck) at the extrapolated
    s0 + dt v, which unmasks a mid-step bounce that starts and ends clear."""
    o0, _, v0, _ = bodies(s0)
    o1 = bodies(s1)[0]
    ok = np.ones(len(o0), bool)
    for o in (o0, o1):
        ok &= _inside(o[:, 0], CIRCUM + margin) & _inside(o[:, 1], CIRCUM + margin) & _inside(o[:, 2], R + margin)
    return ok & _inside(o0[:, 2] + DT * v0[:, 2], R + margin)


def well_apart(s0, s1, margin=MARGIN):
    """No two bodies can have touched in this step: origins / centres farther apart than the sum of the bounding
    radii at s0 and at s1 (free-flight scenes move less than a radius per step)."""
    ok = np.ones(len(s0), bool)
    rad = (CIRCUM, CIRCUM, R)
    for s in (s0, s1):
        o = bodies(s)[0]
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ok &= np.linalg.norm(o[:, i] - o[:, j], axis=1) > rad[i] + rad[j] + margin
    return ok


def momentum_residual(s1, vstar):
    """|sum m v(s1) - sum m v*|_inf / sum m |v*|_inf: contact impulses come in equal and opposite pairs."""
    v1 = bodies(s1)[2]
    m = M[None, :, None]
    num = np.abs((m * v1).sum(1) - (m * vstar).sum(1)).max(-1)
    den = (M[None] * np.abs(vstar).max(-1)).sum(1)
    return num / den


def angular_momentum_residual(s0, s1, vstar, wstar):
    """|sum m c x (v' - v*) + I (omega' - omega*)| / sum (m |c| |v*| + I |omega*|), c the centres of mass at s0 about
    the rink's centre: the two impulses of a contact act at one point, so they add no angular momentum either (this
    is what holds each body's lever arm).  Valid where no time-of-impact event moved a body before its contact."""
    o, a, _, _ = bodies(s0)
    _, _, v1, w1 = bodies(s1)
    c = o + _rot(a, LC[None]) - np.array([5.0, 4.0])
    dv = v1 - vstar
    num = (M[None] * (c[..., 0] * dv[..., 1] - c[..., 1] * dv[..., 0]) + I[None] * (w1 - wstar)).sum(1)
    den = (M[None] * np.linalg.norm(c, axis=-1) * np.linalg.norm(vstar, axis=-1) + I[None] * np.abs(wstar)).sum(1)
    return np.abs(num) / den


def kinetic_energy(v, w):
    """sum of m |v|^2 / 2 + I omega^2 / 2 over the three bodies."""
    return (0.5 * M[None] * (v ** 2).sum(-1) + 0.5 * I[None] * w ** 2).sum(1)


def coulomb_ratio(vstar, wstar, s1, mu):
    """How far into the friction cone the puck's contact impulse reaches, from velocities alone.
    J = m (v' - v*); the contact point is at most r from the centre, so I |omega' - omega*| / r bounds the tangential
    impulse from below; J_n = sqrt(|J|^2 - J_t,min^2).  Returns (J_t,min / (mu J_n), |J|): at most 1."""
    _, _, v1, w1 = bodies(s1)
    J2 = ((M[2] * (v1[:, 2] - vstar[:, 2])) ** 2).sum(-1)
    jt = I[2] * np.abs(w1[:, 2] - wstar[:, 2]) / R
    jn = np.sqrt(np.maximum(J2 - jt ** 2, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return jt / (mu * jn), np.sqrt(J2)


def restitution(v_n):
    """Box2D applies restitution only above its velocity threshold (relative normal speed of the step's v*)."""
    return np.where(np.abs(v_n) > V_THRESH, E_REST, 0.0)


def wall_bounce(v_n):
    """Normal velocity after a puck-wall hit."""
    return -restitution(v_n) * v_n


def head_on(v_in, m_racket):
    """1-D hit of the puck (v_in along the face normal, through the racket's centre of mass) on a racket at rest:
    (puck velocity, racket velocity) after the hit."""
    e = restitution(v_in)
    return v_in * (M[2] - e * m_racket) / (M[2] + m_racket), v_in * M[2] * (1 + e) / (M[2] + m_racket)


# A sequential-impulse solve rounds each velocity twice per iteration (friction row, normal row) by up to half an ulp,
# for up to 180 iterations; errors of random sign add as a random walk, sqrt(360) / 2 ~ 10 ulps.  Allow 16.
SOLVER_ULPS = 16


# ------------------------------------------------- a racket against static faces (families G, H of physics_scenes2)
def racket_world(s, who):
    """World positions of racket `who`'s vertices [N,nv,2] and of its centre of mass [N,2] at state s."""
    o, a, _, _ = bodies(s)
    verts = o[:, who, None, :] + _rot(a[:, who, None], VERTS[who][None])
    return verts, o[:, who] + _rot(a[:, who], LC[who][None])


def face_coordinates(p, q, n):
    """Points p[..., 2] in the frame of a static face through q with unit normal n pointing into the rink:
    (tau along t = (n_y, -n_x), eta above the face)."""
    d = np.asarray(p, np.float64) - np.asarray(q, np.float64)
    return d[..., 0] * n[1] - d[..., 1] * n[0], d[..., 0] * n[0] + d[..., 1] * n[1]


def racket_impulse(who, vstar, wstar, s1):
    """What the step's contacts gave racket `who`: J = m (v' - v*) [N,2] and L = I (omega' - omega*) [N]."""
    _, _, v1, w1 = bodies(s1)
    return M[who] * (v1[:, who] - vstar[:, who]), I[who] * (w1[:, who] - wstar[:, who])


def point_velocity(who, s0, s1, p):
    """Velocity after the step of the racket's material points p[N,k,2] (world positions at the START of the step,
    where Box2D takes its lever arms): v' + omega' x r, r = p - centre of mass."""
    _, com = racket_world(s0, who)
    _, _, v1, w1 = bodies(s1)
    r = p - com[:, None, :]
    return v1[:, who, None, :] + w1[:, who, None, None] * np.stack([-r[..., 1], r[..., 0]], -1)


def centre_of_pressure(who, s0, s1, vstar, wstar, q, n, eta=0.5 * POLY_RADIUS, eta_bar=2 * POLY_RADIUS):
    """Where along the face (tau) the net impulse acted, from L = r x J with the contact plane at height eta above
    the face: Box2D puts a manifold point midway between the two skins' surfaces, both within 2 * polygonRadius of
    the face.  Returns (tau[N], bar[N], J_n[N], J_t[N]); bar is the scene's own error bar: SOLVER_ULPS float32 ulps
    of each velocity that enters (v', omega', and the v*, omega* the solver held in float32), one of the position,
    plus |J_t| eta_bar of height uncertainty -- all over J_n."""
    n = np.asarray(n, np.float64)
    t = np.array([n[1], -n[0]])
    chi = t[0] * n[1] - t[1] * n[0]  # t x n
    J, L = racket_impulse(who, vstar, wstar, s1)
    Jn, Jt = J @ n, J @ t
    _, com = racket_world(s0, who)
    c_tau, c_eta = face_coordinates(com, q, n)
    _, _, v1, w1 = bodies(s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tau = c_tau + (L / chi + (eta - c_eta) * Jt) / Jn
        ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
        uv = SOLVER_ULPS * np.maximum(ulp(v1[:, who]), ulp(vstar[:, who])).max(-1)
        uw = SOLVER_ULPS * np.maximum(ulp(w1[:, who]), ulp(wstar[:, who]))
        bar = (I[who] * uw + (np.abs(eta - c_eta) + np.abs(tau - c_tau)) * M[who] * uv + np.abs(Jt) * eta_bar) / Jn
    return tau, bar + float(np.spacing(np.float32(10.0))), Jn, Jt


# ------------------------------------------------------------------------ the position solver (family P)
def position_recurrence(s):
    """Separation after one step's position solve of a lone dynamic-dynamic contact on the line of centres, both
    bodies free to move, no rotation: every iteration moves the pair apart by -C, C = clamp(baumgarte (s + linearSlop),
    -maxLinearCorrection, 0), and the loop ends after the iteration that saw s >= -3 linearSlop (that iteration's
    correction still applies), at most world.Step's 60 times."""
    s = float(s)
    for _ in range(POSITION_ITERATIONS):
        pre = s
        s -= min(max(BAUMGARTE * (s + LINEAR_SLOP), -MAX_CORRECTION), 0.0)
        if pre >= -3 * LINEAR_SLOP:
            break
    return s


# ------------------------------------------------------------------------------- the goal sensors (family Q)
def goal_separation(p, goal):
    """Euclidean distance of the points p[..., 2] from goal box `goal` (0 left, 1 right), less the puck's radius and
    the box's polygon skin: Box2D's b2TestOverlap of a circle and a polygon is true where this is negative."""
    p = np.asarray(p, np.float64)
    d = np.maximum(np.abs(p - np.array(GOAL_CENTRE[goal])) - np.array(GOAL_HALF), 0.0)
    return np.hypot(d[..., 0], d[..., 1]) - R - POLY_RADIUS

"""Seeded scenes that put bodies to sleep and wake them, for the island sleep rule of tests/sleep_ref.py.

A scene is one arena's raw state put in place with set_state after a reset, then K = 96 steps with `debug`.
"Fell asleep at step k" is OBSERVED through get_state alone: the body's speed after step k - 1 lies in (0, tolerance]
and its v and omega are all exactly 0 after step k.  A body at exact rest shows nothing, so every watched body creeps.
Families (keep_mode False; Z1 once more with keep_mode True):
  Z0  control: everything stays well above tolerance, nothing ever sleeps, free flight holds for all K steps
  Z1  isolated creep: puck and both rackets (zero action) below tolerance from step 0: all asleep at index 24, frozen
  Z2  crossing: a racket at |v| ~ 0.02 or omega ~ 0.05, or a puck at |v| in (0.0100, 0.0105), decays through the
      tolerance at model step k*: asleep at k* + 24 and not before
  Z3  force on a sleeper: rackets parked under zero action for steps 0..24 (a creeping puck certifies index 24), random
      actions from step 25 on, the first step that begins with the racket asleep: free flight holds from there
  Z4  wake by a hit, twin pairs: X's puck creeps to sleep and player 1 is driven into it from T0 = 30; Y's puck moves
      above tolerance elsewhere and a masked set_state puts it, awake, where X's sleeps: X and Y agree bit for bit
  W   sleeper at a wall: a puck (in every third arena a racket too) creeps into the top / bottom wall, or rests up to
      12 mm inside its skin, and sleeps in that contact at index 24: the puck is bit-frozen from then on.  A sleeper
      that an island walk picked up again would be pushed out by the position solver.  Before step T0 the same
      masked set_state moves each sleeping puck 5 to 30 mm further into the wall, position only: SetTransform wakes
      nothing, so it stays there, untouched by the time-of-impact pass (this last law is SURVEY's reading of
      SetTransform and SetAwake, not an external one)
  I   two-body island: a puck arrives at a parked racket at 0.1 m/s; both sleep 24 indices after the puck's first quiet
      step, the racket not at index 24 on its own
measure() reduces a trajectory to figures and counts, check() holds them; the CPU tests (oracle, host build of the
kernel source) and the GPU test share both.  numpy only.
"""
import numpy as np

import physics_ref as P
import physics_scenes as SC
import sleep_ref as Z

K = 96
T0 = 30  # Z4: player 1 is driven at the puck from this step on; before it one masked set_state places Y's and W's pucks
N_SLEEP = Z.steps_to_sleep()[0]  # 25 consecutive quiet steps: asleep at index 24
HOME = SC.HOME
TOL = {k: SC.TOL[k] for k in ("A_dev", "B_momentum", "B_angular", "B_energy", "B_coulomb")}  # the same arithmetic
AMBIGUOUS = 1e-4  # Z2: a model speed this close (relative) to a tolerance at k* - 1 or k* decides nothing
Z4_GAP = 0.83  # rim of X's puck to player 1's skin at rest: the driven racket arrives 7 to 8 steps after T0
Z4_HIT = (7, 8)
Z3_ACTION = 0.2  # scale of the random actions that wake the parked rackets
Z3_X = (3.0, 7.0)  # where they are parked
COUNTS = {"Z0": 31, "Z1": 32, "Z2": 54, "Z3": 30, "Z4": 24, "W": 14, "I": 40}  # Z4 counts pairs: 249 arenas in all
I_MIN = 20
FORCE_TOL = 2.0 ** -23  # Z3: float32(a) * 6000 and float32(a) * 400 are one float32 rounding each, relative 2^-24
LOADED = np.array([True, True, False])  # both rackets get a force and a torque with wake = true every step


def _row(p1, p2, pk):
    return np.concatenate([p1, p2, pk]).astype(np.float64)


def _parked(i, y=None):
    return np.array([HOME[i][0], HOME[i][1] if y is None else y, 0, 0, 0, 0], np.float64)


def _creep(rng, lo=0.001, hi=0.009):
    th = rng.uniform(0, 2 * np.pi)
    return rng.uniform(lo, hi) * np.array([np.cos(th), np.sin(th)])


def _sign(rng):
    return float(rng.choice([-1.0, 1.0]))


def _creeping_racket(rng, i):
    v = _creep(rng)
    return np.array([HOME[i][0] + rng.uniform(-0.3, 0.3), rng.uniform(3, 5), rng.uniform(-0.5, 0.5), v[0], v[1],
                     _sign(rng) * rng.uniform(0.002, 0.03)])


def _creeping_puck(rng, x=None, y=None):
    v = _creep(rng)
    return np.array([rng.uniform(4.5, 5.5) if x is None else x, rng.uniform(2, 6) if y is None else y, 0.0, v[0], v[1],
                     _sign(rng) * rng.uniform(0.002, 0.03)])


def _family_z0(rng, n):
    rows = []
    for _ in range(n):
        u = rng.uniform
        p1 = [2.0, u(3.5, 4.5), u(-0.3, 0.3), 0.3, 0.0, _sign(rng) * u(0.5, 1.0)]
        p2 = [8.0, u(3.5, 4.5), u(-0.3, 0.3), -0.3, 0.0, _sign(rng) * u(0.5, 1.0)]
        pk = [5.0, 4.0, 0.0, u(-0.2, 0.2), _sign(rng) * u(0.5, 0.9), _sign(rng) * u(1, 5)]
        act = np.array([0.02, 0.0, _sign(rng) * 0.02, 0.0, 0.02, 0.0, _sign(rng) * 0.02, 0.0])
        rows.append(dict(family="Z0", state=_row(p1, p2, pk), act=act))
    return rows


def _family_z1(rng, n):
    return [dict(family="Z1", state=_row(_creeping_racket(rng, 0), _creeping_racket(rng, 1), _creeping_puck(rng)))
            for _ in range(n)]


def _midway(rng, damping, lo, hi):
    """(1 + dt damping)^(n + 0.3 .. 0.7), n drawn from lo .. hi - 1: a speed this many times a tolerance is divided by
    1 + dt damping every step and passes the tolerance about midway between steps n and n + 1."""
    return (1 + P.DT * damping) ** (int(rng.integers(lo, hi)) + rng.uniform(0.3, 0.7))


def _family_z2(rng, n):
    """The watched body crosses a tolerance on the way down: linear damping 5 (a racket under zero action), angular
    damping 2, or the puck's 0.05.  Everything else in the arena is parked at exact rest.  The puck loses 0.1 % a
    step: drawn freely, one puck in five would come within AMBIGUOUS of the tolerance, so every start speed is placed
    to cross midway between two steps (the float64 model's decay, nothing of the code under test)."""
    rows = []
    for k in range(n):
        u = rng.uniform
        p1, p2, pk = _parked(0), _parked(1), np.array([5.0, 4.0, 0, 0, 0, 0], np.float64)
        kind = ("lin", "ang", "puck")[k % 3]
        who = (k // 3) % 2
        if kind == "lin":  # 0.01 * 1.1^(n + 1/2), n = 5 .. 9: 0.017 to 0.025
            r = (p1, p2)[who]
            sp = _midway(rng, 5.0, 5, 10) * Z.LIN_TOL
            r[3:5] = _creep(rng, sp, sp)
            r[5] = _sign(rng) * u(0.002, 0.02)
            body = who
        elif kind == "ang":  # 2 pi / 180 * 1.04^(n + 1/2), n = 6 .. 12: 0.045 to 0.057
            r = (p1, p2)[who]
            r[3:5] = _creep(rng)
            r[5] = _sign(rng) * _midway(rng, 2.0, 6, 13) * Z.ANG_TOL
            body = who
        else:  # 0.01 * 1.001^(n + 1/2), n = 1 .. 48: within (0.0100, 0.0105)
            sp = _midway(rng, 0.05, 1, 49) * Z.LIN_TOL
            pk[3:5] = _creep(rng, sp, sp)
            pk[5] = _sign(rng) * u(0.002, 0.03)
            body = 2
        rows.append(dict(family="Z2", state=_row(p1, p2, pk), body=body))
    return rows


def _family_z3(rng, n):
    rows = []
    for _ in range(n):
        act = np.zeros((K, 8))
        act[N_SLEEP:] = rng.uniform(-Z3_ACTION, Z3_ACTION, (K - N_SLEEP, 8))
        act[N_SLEEP] = rng.choice([-1.0, 1.0], 8) * rng.uniform(0.4 * Z3_ACTION, Z3_ACTION, 8)  # a visible wake-up
        p1, p2 = _parked(0), _parked(1)
        p1[0], p2[0] = Z3_X  # a metre and more from every wall, and outside the centre zone's force law
        rows.append(dict(family="Z3", state=_row(p1, p2, _creeping_puck(rng, 5.0, 1.6)), act=act))
    return rows


def _family_z4(rng, n):
    """n twin pairs.  Every fourth pair stands with the puck's rim 0.3 m from the top / bottom wall, the puck offset
    towards the wall so that the hit sends it there."""
    rows = []
    for k in range(n):
        u = rng.uniform
        wall = 0.0 if k % 4 else (1.0 if k % 8 == 0 else -1.0)
        a2 = u(-0.5, 0.5)
        if wall:
            yp = (P.Y_TOP - 0.3 - P.R) if wall > 0 else (P.Y_BOT + 0.3 + P.R)
            off = wall * u(0.1, 0.3)
        else:
            yp, off = u(3.0, 5.0), u(-0.3, 0.3)
        p1 = _parked(0, yp - off)
        x = HOME[0][0] + 0.1 + P.POLY_RADIUS + P.R + Z4_GAP
        v = _creep(rng)
        act = np.zeros((K, 8))
        act[T0:, 0], act[T0:, 2] = 1.0, a2
        away = np.array([6.3, 4.0, 0.0, 0.0, _sign(rng) * u(0.04, 0.06), 0.0])  # Y's puck until T0: above tolerance
        rows.append(dict(family="Z4X", state=_row(p1, _parked(1), [x, yp, 0.0, v[0], v[1], 0.0]), act=act, wall=wall,
                         pair=k))
        rows.append(dict(family="Z4Y", state=_row(p1, _parked(1), away), act=act, wall=wall, pair=k))
    return rows


def _family_w(rng, n):
    """depth: how far the body's skin reaches into the wall's at the start, -4 mm (not yet touching) to 12 mm (inside
    the 3 linearSlop = 15 mm within which the island counts as solved)."""
    rows = []
    for k in range(n):
        u = rng.uniform
        wall = 1.0 if k % 2 else -1.0
        face = P.Y_TOP if wall > 0 else P.Y_BOT
        p1 = _parked(0)
        if k % 3 == 0:
            a = u(-0.3, 0.3)
            ext = (wall * (np.sin(a) * P.VERTS[0][:, 0] + np.cos(a) * P.VERTS[0][:, 1])).max()
            p1 = np.array([2.0 + u(-0.3, 0.3), face - wall * (ext + 2 * P.POLY_RADIUS - u(-0.004, 0.012)), a,
                           u(-0.004, 0.004), wall * u(-0.002, 0.007), _sign(rng) * u(0.002, 0.02)])
        depth = u(-0.004, -0.001) if k % 4 == 3 else u(0.002, 0.012)  # every fourth puck starts short of touching
        pk = [u(3.5, 6.5), face - wall * (P.R + P.POLY_RADIUS - depth), 0.0, u(-0.004, 0.004),
              wall * u(-0.002, 0.007), _sign(rng) * u(0.002, 0.03)]
        rows.append(dict(family="W", state=_row(p1, _parked(1), pk), wall=wall, push=u(0.005, 0.03)))
    return rows


def _family_i(rng, n):
    """The puck starts 2.4 to 3.6 mm outside touching range of a parked racket's flat face and closes at 0.1 m/s:
    2 mm a step, so the contact is touching from the start of step 2."""
    rows = []
    for k in range(n):
        u = rng.uniform
        who = k % 2
        sgn = 1.0 if who == 0 else -1.0  # player 1's flat face looks along +x, player 2's along -x
        y = u(3.5, 4.5)
        x = HOME[who][0] + sgn * (0.1 + P.POLY_RADIUS + P.R + u(0.0024, 0.0036))
        pk = [x, y + u(-0.25, 0.25), 0.0, -sgn * u(0.095, 0.105), u(-0.004, 0.004), 0.0]
        p1, p2 = _parked(0, y if who == 0 else None), _parked(1, y if who == 1 else None)
        rows.append(dict(family="I", state=_row(p1, p2, pk), body=who))
    return rows


class Batch:
    """state[N,18], aux[N,5], actions[K,N,8] and per-arena labels.  kind "main": all families interleaved by a seeded
    shuffle, twins in different waves; kind "z1": 65 arenas of Z1, so that from step 25 on every lane of the first
    wave holds a sleeper and the second wave holds one lane."""

    def __init__(self, kind="main", keep_mode=False, seed=0, scale=1):
        rng = np.random.default_rng([seed, 7, int(keep_mode), kind == "main"])
        if kind == "main":
            c = {k: v * scale for k, v in COUNTS.items()}
            rows = (_family_z0(rng, c["Z0"]) + _family_z1(rng, c["Z1"]) + _family_z2(rng, c["Z2"])
                    + _family_z3(rng, c["Z3"]) + _family_z4(rng, c["Z4"]) + _family_w(rng, c["W"])
                    + _family_i(rng, c["I"]))
            rows = [rows[i] for i in rng.permutation(len(rows))]
            _separate_twins(rows)
        else:
            rows = _family_z1(rng, 65)
        self.kind, self.keep_mode, self.n = kind, bool(keep_mode), len(rows)
        self.family = np.array([r["family"] for r in rows])
        self.state = np.array([r["state"] for r in rows], np.float32)
        self.body = np.array([r.get("body", -1) for r in rows])  # Z2: the watched body; I: the racket
        self.wall = np.array([r.get("wall", 0.0) for r in rows])
        self.push = np.array([r.get("push", 0.0) for r in rows])  # W: how far the sleeping puck is moved into the wall
        pair = np.array([r.get("pair", -1) for r in rows])
        self.twin = np.full(self.n, -1)  # X's index for a Y, Y's for an X
        for p in set(pair[pair >= 0]):
            x, = np.nonzero((pair == p) & (self.family == "Z4X"))
            y, = np.nonzero((pair == p) & (self.family == "Z4Y"))
            self.twin[x[0]], self.twin[y[0]] = y[0], x[0]
        self.aux = np.zeros((self.n, 5), np.int32)
        self.actions = np.zeros((K, self.n, 8), np.float32)
        for i, r in enumerate(rows):
            if "act" in r:
                self.actions[:, i] = r["act"]
        for a in (self.state, self.aux, self.actions):
            a.setflags(write=False)

    def twin_patch(self, s):
        """The masked set_state made before step T0, from the state s[N,18] read back then: each Y's puck goes to its
        X's puck position with v = 0, each W's puck into its wall; every other entry is NaN, "setter not called" --
        the rackets, and the puck's angle and omega, which HockeyEnv.set_state never assigns.  Returns
        (state[N,18], mask[N]) or None."""
        y, = np.nonzero(self.family == "Z4Y")
        w, = np.nonzero(self.family == "W")
        if not len(y) and not len(w):
            return None
        s = np.asarray(s, np.float32)
        st = np.full((self.n, 18), np.nan, np.float32)
        st[y, 12:14] = s[self.twin[y], 12:14]
        st[y, 15:17] = 0.0
        # W: the sleeping puck is moved 5 to 30 mm further into the wall, position only: SetTransform wakes nothing
        st[w, 12] = s[w, 12]
        st[w, 13] = (s[w, 13].astype(np.float64) + self.wall[w] * self.push[w]).astype(np.float32)
        mask = np.zeros(self.n, np.uint8)
        mask[y] = 1
        mask[w] = 1
        return st, mask


def _separate_twins(rows):
    """Swap a Y that shares its X's wave with the nearest arena of another wave that belongs to no pair."""
    where = {(r["family"], r["pair"]): i for i, r in enumerate(rows) if "pair" in r}
    for (fam, p), i in sorted(where.items()):
        if fam != "Z4Y" or i // 64 != where[("Z4X", p)] // 64:
            continue
        j = next(j for j in range(len(rows)) if j // 64 != i // 64 and "pair" not in rows[j])
        rows[i], rows[j] = rows[j], rows[i]


# ---------------------------------------------------------------------------------------------------- measurement
def _first(flags):
    """Index [..] of the first True along axis 0, -1 where there is none."""
    return np.where(flags.any(0), flags.argmax(0), -1)


def observe(S):
    """fell[K,N,3]: the body's speed after step k - 1 lies in (0, tolerance] and v, omega are exactly 0 after step k."""
    b = np.asarray(S, np.float64).reshape(len(S), -1, 3, 6)[..., 3:6]
    moving = (b != 0.0).any(-1)  # [K+1,N,3]
    slow = np.stack([Z.quiet(*Z.read_speeds(s)) for s in S])
    return moving[:-1] & slow[:-1] & ~moving[1:]


def measure(batch, S, D):
    """S[K+1,N,18] the raw states before / after each step (S[T0] after the twins' set_state), D[K,N,13] each step's
    debug row -> figures and counts."""
    S32 = np.asarray(S, np.float32)
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    fam, n = batch.family, batch.n
    ff = np.stack([P.free_flight(S[k], D[k]) for k in range(K)])
    err = np.abs(S[1:] - ff) / np.maximum(1.0, np.abs(ff))
    dev = err.max(-1)  # [K,N]
    devb = err.reshape(K, n, 3, 6).max(-1)  # [K,N,3]
    free = dev <= TOL["A_dev"]
    pre = [P.presolve(S[k], D[k]) for k in range(K)]
    clear = np.stack([P.clear_of_walls(S[k], S[k + 1]) for k in range(K)])
    apart = np.stack([P.well_apart(S[k], S[k + 1]) for k in range(K)])

    # the model: float64 pre-solve speeds where the body flew free, the velocities read back where a contact acted
    mlin, mang = (np.stack(x) for x in zip(*[Z.speeds(*pre[k]) for k in range(K)]))
    rlin, rang = (np.stack(x) for x in zip(*[Z.read_speeds(S[k + 1]) for k in range(K)]))
    hit_body = devb > TOL["A_dev"]
    quiet = np.where(hit_body, Z.quiet(rlin, rang), Z.quiet(mlin, mang))
    sl = Z.Sleepers(n)
    sl.set_velocity((S[0].reshape(n, 3, 6)[..., 3:6] != 0).any(-1))
    pred = np.stack([sl.step(np.tile(LOADED, (n, 1)), quiet[k], Z.islands(S[k])) for k in range(K)])
    obs = observe(S)
    moving = (S[:-1].reshape(K, n, 3, 6)[..., 3:6] != 0).any(-1)
    # wherever the model's verdict can be seen at all (the body moved), it is what was observed; Z4 only before T0
    seen = np.ones((K, n, 1), bool)
    seen[T0:, np.isin(fam, ("Z4X", "Z4Y"))] = False
    out = {"mismatch": int(((obs != (pred & moving)) & seen).sum()), "n": n}
    first_obs, first_pred = _first(obs), _first(pred)  # [N,3]

    z = fam == "Z0"
    if z.any():
        above = np.maximum(mlin[:, z] / Z.LIN_TOL, mang[:, z] / Z.ANG_TOL)
        out.update(Z0_steps=int(z.sum()) * K, Z0_dev=float(dev[:, z].max()), Z0_above=float(above.min()),
                   Z0_clear=bool((clear[:, z] & apart[:, z]).all()),
                   Z0_slept=int(obs[:, z].sum() + pred[:, z].sum()))

    z = fam == "Z1"
    if z.any():
        frozen = (S32[N_SLEEP:, z].view(np.uint32) == S32[N_SLEEP, z].view(np.uint32)[None]).all()
        still = (S32[N_SLEEP:, z].reshape(-1, 3, 6)[..., 3:6] == 0).all()
        out.update(Z1_bodies=int(z.sum()) * 3, Z1_asleep_at_24=int((first_obs[z] == N_SLEEP - 1).sum()),
                   Z1_rackets_at_24=int((first_obs[z][:, :2] == N_SLEEP - 1).sum()),
                   Z1_model_at_24=int((first_pred[z] == N_SLEEP - 1).sum()),
                   Z1_frozen=bool(frozen), Z1_zero=bool(still),
                   Z1_puck_frozen=bool((S32[N_SLEEP:, z, 12:18].view(np.uint32)
                                        == S32[N_SLEEP, z, 12:18].view(np.uint32)[None]).all()),
                   Z1_clear=bool((clear[:, z] & apart[:, z]).all()))

    idx, = np.nonzero(fam == "Z2")
    if len(idx):
        ok = left = early = 0
        kstars = []
        for i in idx:
            b = batch.body[i]
            q = Z.quiet(mlin[:, i, b], mang[:, i, b])
            ks = int(np.argmax(q))  # the first step whose model speeds are both at or below tolerance
            assert q[ks] and ks > 0, (i, ks)
            if Z.tolerance_margin(mlin[ks - 1:ks + 1, i, b], mang[ks - 1:ks + 1, i, b]).min() < AMBIGUOUS:
                left += 1
                continue
            kstars.append(ks)
            ok += first_obs[i, b] == ks + N_SLEEP - 1
            early += int(obs[:ks + N_SLEEP - 1, i, b].any())
        out.update(Z2_scenes=len(idx), Z2_left_out=left, Z2_on_time=int(ok), Z2_early=early,
                   Z2_kstar=(min(kstars), max(kstars)) if kstars else None,
                   Z2_clear=bool((clear[:, idx] & apart[:, idx]).all()))

    z = fam == "Z3"
    if z.any():
        good = clear[N_SLEEP:, z] & apart[N_SLEEP:, z]
        d = np.where(good, dev[N_SLEEP:, z], 0.0)
        # the debug row holds what the bodies accumulated: a wake-up that dropped the force would show 0 there and fly
        # "free", so the row of the waking step is held to HockeyEnv's own law (parked at rest outside the centre zone,
        # angle 0: F = +-6000 a, T = 400 a), to one float32 rounding
        a = np.asarray(batch.actions[N_SLEEP, z], np.float64)
        law = np.concatenate([6000 * a[:, 0:2], -6000 * a[:, 4:6], 400 * a[:, [2, 6]]], 1)
        got = D[N_SLEEP][z][:, [0, 1, 2, 3, 6, 7]]
        out["Z3_wake_force"] = float((np.abs(got - law) / np.maximum(1.0, np.abs(law))).max())
        out.update(Z3_scenes=int(z.sum()), Z3_puck_at_24=int((first_obs[z][:, 2] == N_SLEEP - 1).sum()),
                   Z3_wake_clear=bool(good[0].all()), Z3_clear_share=float(good.mean()),
                   Z3_dev=float(d.max()), Z3_wake_dev=float(d[0].max()),
                   Z3_wake_speed=float(np.linalg.norm(S[N_SLEEP + 1, z].reshape(-1, 3, 6)[:, :2, 3:5], axis=-1).min()))

    xs, = np.nonzero(fam == "Z4X")
    if len(xs):
        ys = batch.twin[xs]
        equal = (S32[T0 + 1:, xs].view(np.uint32) == S32[T0 + 1:, ys].view(np.uint32)).all((0, 2))
        fig = {k: -np.inf for k in ("momentum", "angular", "energy", "coulomb")}
        offs, hit_clear, f_out, walls = [], 0, -np.inf, 0
        for i in xs:
            ks = np.nonzero(~free[T0:, i])[0]
            if not len(ks):
                offs.append(-1)
                continue
            k = T0 + int(ks[0])
            offs.append(k - T0)
            hit_clear += bool(clear[k, i])
            sel = slice(i, i + 1)
            vs, ws, s1 = pre[k][0][sel], pre[k][1][sel], S[k + 1][sel]
            _, _, v1, w1 = P.bodies(s1)
            ratio, J = P.coulomb_ratio(vs, ws, s1, P.MU_RACKET)
            fig["momentum"] = max(fig["momentum"], float(P.momentum_residual(s1, vs)[0]))
            fig["angular"] = max(fig["angular"], float(P.angular_momentum_residual(S[k][sel], s1, vs, ws)[0]))
            fig["energy"] = max(fig["energy"], float((P.kinetic_energy(v1, w1) / P.kinetic_energy(vs, ws) - 1)[0]))
            if J[0] > SC.COULOMB_MIN_DV * P.M[2]:
                fig["coulomb"] = max(fig["coulomb"], float(ratio[0]))
            if batch.wall[i]:
                walls += 1
                pk, d = S[k + 1:, i, 12:14], P.R - 3 * P.LINEAR_SLOP
                x_out = np.maximum(P.X_LEFT + d - pk[:, 0], pk[:, 0] - (P.X_RIGHT - d))
                mouth = (x_out > 0) & (pk[:, 1] > P.POST_Y_BOT) & (pk[:, 1] < P.POST_Y_TOP)
                gone = np.maximum.accumulate(mouth)  # through a goal mouth: nothing holds the puck behind it
                y_out = np.maximum(P.Y_BOT + d - pk[:, 1], pk[:, 1] - (P.Y_TOP - d))
                f_out = max(f_out, float(np.where(gone, -np.inf, np.maximum(x_out, y_out)).max()))
        waves = {(int(x) // 64, int(y) // 64) for x, y in zip(xs, ys)}
        out.update(Z4_pairs=len(xs), Z4_puck_at_24=int((first_obs[xs, 2] == N_SLEEP - 1).sum()),
                   Z4_equal=int(equal.sum()), Z4_hit_offsets=(min(offs), max(offs)), Z4_hit_clear=hit_clear,
                   Z4_wall_pairs=walls, Z4_F_out=f_out, Z4_same_wave=sum(a == b for a, b in waves),
                   Z4_y_awake=bool((np.linalg.norm(S[:T0, ys, 15:17], axis=-1) > 2 * Z.LIN_TOL).all()),
                   **{"Z4_" + k: v for k, v in fig.items()})

    z = fam == "W"
    if z.any():
        gap = np.where(batch.wall[z] > 0, P.Y_TOP - S[N_SLEEP, z, 13], S[N_SLEEP, z, 13] - P.Y_BOT) - P.R
        out.update(W_scenes=int(z.sum()), W_puck_at_24=int((first_obs[z][:, 2] == N_SLEEP - 1).sum()),
                   W_touching=int((gap < P.POLY_RADIUS).sum()),  # the puck's rim is inside the wall's skin
                   W_puck_frozen=bool((S32[N_SLEEP:T0, z, 12:18].view(np.uint32)
                                       == S32[N_SLEEP, z, 12:18].view(np.uint32)[None]).all()),
                   W_moved_frozen=bool((S32[T0:, z, 12:18].view(np.uint32)
                                        == S32[T0, z, 12:18].view(np.uint32)[None]).all()),
                   W_moved=float(np.abs(S[T0, z, 13] - S[T0 - 1, z, 13]).min()))

    idx, = np.nonzero(fam == "I")
    if len(idx):
        qual = on_time = alone = 0
        touch, slept = set(), set()
        for i in idx:
            who = batch.body[i]
            sep = np.stack([Z.puck_racket_separation(S[k, i:i + 1], who)[0] for k in range(K + 1)])
            qk = Z.quiet(rlin[:, i], rang[:, i])  # [K,3] from the velocities read back: a contact acts here
            loud = np.nonzero(~qk[:, 2])[0]
            q = int(loud[-1]) + 1 if len(loud) else 0  # the puck's first quiet step
            end = q + N_SLEEP - 1
            alone += int(first_obs[i, who] == N_SLEEP - 1)
            if not (0 < q and end < K and (sep[q:end + 1] < 0).all() and qk[:end + 1, who].all()
                    and qk[q:end + 1, 2].all()):
                continue
            qual += 1
            touch.add(int(np.argmax(sep < 0)))
            slept.update((int(first_obs[i, who]), int(first_obs[i, 2])))
            on_time += int(first_obs[i, who] == end and first_obs[i, 2] == end)
        out.update(I_scenes=len(idx), I_qualifying=qual, I_together=on_time, I_racket_alone_at_24=alone,
                   I_touch_index=sorted(touch), I_sleep_index=sorted(slept))
    return out


def check(m, batch):
    """Every law, and the scenes' coverage conditions."""
    assert m["mismatch"] == 0, ("observed sleep events differ from the float32-timer model's", m["mismatch"])
    if "Z0_steps" in m:
        assert m["Z0_clear"] and m["Z0_steps"] > 0, "Z0 must stay apart and clear of walls"
        assert m["Z0_above"] >= 2.0, ("Z0 must stay well above tolerance", m["Z0_above"])
        assert m["Z0_slept"] == 0, ("Z0: nothing may fall asleep", m["Z0_slept"])
        assert m["Z0_dev"] <= TOL["A_dev"], ("Z0 free flight", m["Z0_dev"])
    assert m["Z1_clear"] and m["Z1_bodies"] > 0
    assert m["Z1_model_at_24"] == m["Z1_bodies"], ("Z1: the model itself", m["Z1_model_at_24"])
    assert m["Z1_rackets_at_24"] == m["Z1_bodies"] // 3 * 2, (
        "Z1: a racket woken while awake keeps its timer and sleeps at index 24", m["Z1_rackets_at_24"])
    assert m["Z1_asleep_at_24"] == m["Z1_bodies"], ("Z1: every body asleep at index 24", m["Z1_asleep_at_24"])
    assert m["Z1_zero"] and m["Z1_puck_frozen"] and m["Z1_frozen"], (
        "Z1: exactly zero and frozen from index 24 on", m["Z1_zero"], m["Z1_puck_frozen"], m["Z1_frozen"])
    if batch.kind != "main":
        assert batch.n == 65
        return
    assert m["Z2_clear"]
    assert m["Z2_left_out"] == 0, ("Z2: the seed leaves no scene out", m["Z2_left_out"])
    assert m["Z2_early"] == 0, ("Z2: asleep before k* + 24", m["Z2_early"])
    assert m["Z2_on_time"] == m["Z2_scenes"] - m["Z2_left_out"], ("Z2: asleep at k* + 24", m["Z2_on_time"])
    assert m["Z3_puck_at_24"] == m["Z3_scenes"], ("Z3: the puck certifies index 24", m["Z3_puck_at_24"])
    assert m["Z3_wake_clear"] and m["Z3_clear_share"] >= 0.9, (m["Z3_wake_clear"], m["Z3_clear_share"])
    assert m["Z3_wake_speed"] > 10 * Z.LIN_TOL, ("Z3: the waking force must be visible", m["Z3_wake_speed"])
    assert m["Z3_wake_force"] <= FORCE_TOL, ("Z3: the force of the waking step is the action's", m["Z3_wake_force"])
    assert m["Z3_wake_dev"] <= TOL["A_dev"], ("Z3: the force acts in the step that wakes the body", m["Z3_wake_dev"])
    assert m["Z3_dev"] <= TOL["A_dev"], ("Z3 free flight after the wake", m["Z3_dev"])
    assert m["Z4_puck_at_24"] == m["Z4_pairs"] and m["Z4_y_awake"], (m["Z4_puck_at_24"], m["Z4_y_awake"])
    assert m["Z4_same_wave"] == 0, "Z4: twins sit in different waves"
    assert Z4_HIT[0] <= m["Z4_hit_offsets"][0] and m["Z4_hit_offsets"][1] <= Z4_HIT[1] < N_SLEEP - 1, (
        "Z4: the hit lands 7 to 8 steps after T0", m["Z4_hit_offsets"])
    assert m["Z4_hit_clear"] == m["Z4_pairs"], ("Z4: no wall in the hit step", m["Z4_hit_clear"])
    assert m["Z4_equal"] == m["Z4_pairs"], ("Z4: X and Y differ after T0", m["Z4_equal"])
    assert m["Z4_momentum"] <= TOL["B_momentum"], ("Z4 momentum", m["Z4_momentum"])
    assert m["Z4_angular"] <= TOL["B_angular"], ("Z4 angular momentum", m["Z4_angular"])
    assert m["Z4_energy"] <= TOL["B_energy"], ("Z4 kinetic energy rose", m["Z4_energy"])
    assert m["Z4_coulomb"] <= 1 + TOL["B_coulomb"], ("Z4 Coulomb cone", m["Z4_coulomb"])
    assert m["Z4_wall_pairs"] * 4 == m["Z4_pairs"] and m["Z4_F_out"] <= 0.0, ("Z4 containment", m["Z4_F_out"])
    assert m["W_puck_at_24"] == m["W_scenes"] and m["W_touching"] >= 0.7 * m["W_scenes"], (
        "W: asleep at index 24, most in touch with the wall", m["W_puck_at_24"], m["W_touching"])
    assert m["W_puck_frozen"], "W: a puck asleep against a wall stays where it fell asleep, bit for bit"
    assert m["W_moved"] > 0.004 and m["W_moved_frozen"], (
        "W: a sleeper that set_state moves into the wall stays asleep where it was put", m["W_moved"])
    assert m["I_qualifying"] >= I_MIN, ("I: qualifying scenes", m["I_qualifying"])
    assert m["I_together"] == m["I_qualifying"], ("I: both asleep 24 indices after the puck's first quiet step",
                                                  m["I_together"], m["I_sleep_index"])
    assert m["I_racket_alone_at_24"] == 0, ("I: the racket slept on its own timer", m["I_racket_alone_at_24"])


def run(env, batch, first=0, last=K):
    """Drive an implementation (the call shapes of tests/scene_lockstep.py) through steps first .. last - 1 of the
    batch (first = 0 puts the batch's state in place; a later first continues from the context's own).  Returns
    (S[last - first + 1, N, 18], D[last - first, N, 13])."""
    if first == 0:
        env.set_state(batch.state, batch.aux)
    S, D = [np.array(batch.state) if first == 0 else env.get_state()[0]], []
    for k in range(first, last):
        if k == T0:
            patch = batch.twin_patch(S[-1])
            if patch is not None:
                env.set_state(patch[0], None, patch[1])
                S[-1] = env.get_state()[0]
        D.append(env.step(batch.actions[k], debug=True).debug)
        S.append(env.get_state()[0])
    return np.stack(S), np.stack(D)

"""Box2D 2.3's island sleep rule as a plain numpy model.  numpy only: TEST INFRASTRUCTURE.

Like physics_ref, this module must not import hockey_amd, oracle or hostcheck, and reads neither hk_world.h nor
oracle/hk_oracle.c.  It holds the rule as SURVEY.md records it ("Island solve" step 9 and the ApplyForceToCenter note):

  * after the position solve a body with omega^2 > (2 pi / 180)^2 or |v|^2 > 0.01^2 gets sleep time 0, any other body
    sleepTime += h;
  * the island sleeps when the minimum over its bodies has reached 0.5 s (and its positions are solved: every scene
    of sleep_scenes is contact-free or rests in a contact far shallower than 3 linearSlop);
  * sleeping zeroes v, omega, force and torque;
  * waking an awake body (a force applied with wake = true, a contact that begins, the island walk) does not restart
    its timer; waking a sleeping one starts it at 0;
  * a force applied to a sleeping body wakes it and acts in that very step.

THE 25 STEPS.  The timer is a float32 and h = float32(0.02) = 0.0199999995529651641845703125.  The float32 RUNNING SUM
of h reaches 0.50000006 on the 25th add (the additions round up on the way: 24 adds give 0.48000008), so a body
falls asleep at the end of its 25th consecutive quiet step, index 24 when it is quiet from step 0.  The exact product
25 * float32(0.02) = 0.49999998882... is BELOW 0.5: a float64 timer, or a timer computed as n * h, says 26.  The model
therefore keeps the timer as the float32 running sum (steps_to_sleep() states both numbers).

Speeds are the float64 pre-solve velocities of physics_ref (presolve on the step's debug row): in a contact-free step
they are the velocities the rule sees.  Where a contact acted the caller hands in the velocities read back instead.
"""
import numpy as np

import physics_ref as P

LIN_TOL = 0.01  # b2_linearSleepTolerance, m/s
ANG_TOL = 2.0 / 180.0 * np.pi  # b2_angularSleepTolerance, rad/s
TIME_TO_SLEEP = 0.5  # b2_timeToSleep, s
H32 = np.float32(0.02)  # world.Step's float32 time step: what the timer adds


def steps_to_sleep():
    """(consecutive quiet steps until the float32 running sum reaches 0.5 s, the same for an exact timer)."""
    t, n = np.float32(0.0), 0
    while t < np.float32(TIME_TO_SLEEP):
        t = np.float32(t + H32)
        n += 1
    exact = int(np.ceil(TIME_TO_SLEEP / float(H32)))
    return n, exact


def speeds(v, w):
    """(|v|[...], |omega|[...]) in float64 of velocities v[..., 2], w[...]."""
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    return np.sqrt((v ** 2).sum(-1)), np.abs(w)


def model_speeds(s0, dbg):
    """The float64 pre-solve speeds (|v*|[N,3], |omega*|[N,3]) of one step from state s0 under debug row dbg."""
    return speeds(*P.presolve(s0, dbg))


def read_speeds(s1):
    """(|v|[N,3], |omega|[N,3]) of a state read back."""
    _, _, v, w = P.bodies(s1)
    return speeds(v, w)


def quiet(lin, ang):
    """The rule's comparison: NOT (omega^2 > tol^2 or |v|^2 > tol^2)."""
    return ~((np.asarray(ang) ** 2 > ANG_TOL ** 2) | (np.asarray(lin) ** 2 > LIN_TOL ** 2))


def tolerance_margin(lin, ang):
    """How close a body's speeds come to a tolerance, relative: min(|lin / LIN_TOL - 1|, |ang / ANG_TOL - 1|).  A
    float32 engine and the float64 model may disagree about `quiet` only where this is a few float32 ulp."""
    return np.minimum(np.abs(np.asarray(lin) / LIN_TOL - 1.0), np.abs(np.asarray(ang) / ANG_TOL - 1.0))


def puck_racket_separation(s, who):
    """Distance [N] between the puck's rim and racket `who`'s skin (the polygon grown by b2_polygonRadius), float64.
    Box2D's manifold of a circle and a polygon has a point, so the contact is touching, where this is negative."""
    verts, _ = P.racket_world(s, who)  # [N,nv,2]
    c = P.bodies(s)[0][:, 2]  # puck centre [N,2]
    a, b = verts, np.roll(verts, -1, axis=1)
    ab, ac = b - a, c[:, None, :] - a
    t = np.clip((ab * ac).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    d = np.linalg.norm(ac - t[..., None] * ab, axis=-1).min(1)
    return d - P.R - P.POLY_RADIUS


def islands(s0):
    """Island label [N,3] of each body at the start of a step: its own index, except that a puck touching a racket
    takes that racket's (the scenes never bring the two rackets together)."""
    lab = np.tile(np.arange(3), (len(s0), 1))
    for who in (0, 1):
        lab[puck_racket_separation(s0, who) < 0.0, 2] = who
    return lab


class Sleepers:
    """awake[N,3] and the float32 timers[N,3] of N arenas' three bodies after a reset: all awake, timers 0."""

    def __init__(self, n):
        self.awake = np.ones((n, 3), bool)
        self.timer = np.zeros((n, 3), np.float32)

    def set_velocity(self, nonzero):
        """SetLinearVelocity / SetAngularVelocity wake a body only when handed a non-zero velocity."""
        self._wake(np.asarray(nonzero, bool))

    def _wake(self, who):
        asleep = who & ~self.awake
        self.timer[asleep] = np.float32(0.0)  # an awake body keeps its timer
        self.awake |= who

    def step(self, loaded, is_quiet, island):
        """One world.Step.  loaded[N,3]: a force or torque was applied with wake = true (any value, zero included);
        is_quiet[N,3]: the rule's comparison on the velocities after the solve; island[N,3]: islands() of the state
        the step starts from.  Returns fell[N,3]: the body was put to sleep at the end of this step."""
        self._wake(np.asarray(loaded, bool))
        n = len(self.awake)
        same = island[:, :, None] == island[:, None, :]  # [N,3,3]
        live = (same & self.awake[:, None, :]).any(-1)  # an island is built from every awake body; it wakes the rest
        self._wake(live)
        t = np.where(is_quiet, (self.timer + H32).astype(np.float32), np.float32(0.0)).astype(np.float32)
        self.timer = np.where(self.awake, t, self.timer).astype(np.float32)
        big = np.float32(np.finfo(np.float32).max)
        tmin = np.where(same & self.awake[:, None, :], self.timer[:, None, :], big).min(-1)  # min over the island
        fell = self.awake & (tmin >= np.float32(TIME_TO_SLEEP))
        self.awake &= ~fell
        self.timer[fell] = np.float32(0.0)
        assert self.timer.shape == (n, 3)
        return fell

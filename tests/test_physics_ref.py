"""world.Step held to float64 rigid-body laws that are not derived from our solver (tests/physics_ref.py).

Every parity test compares the kernel with oracle/hk_oracle.c, our own restatement of Box2D 2.3: a misreading made
once there and copied faithfully into hk_solver.h / hk_velocity.h passes them all.  Here the CPU oracle AND the host
build of the kernel source are each held, on seeded scenes (tests/physics_scenes.py), to the closed form of a
contact-free step, momentum, energy and the Coulomb cone of a contact, and the closed forms of a puck-wall bounce and
a head-on puck-racket hit.  The oracle's deliberately wrong variants must each fail the law named for it.
"""
import numpy as np
import pytest

import physics_scenes as SC
from hostcheck import HostVec


class OracleWorlds:
    """N OracleWorld arenas behind the three calls physics_scenes.run makes."""

    def __init__(self, oracle, n, keep_mode):
        self.ws = [oracle.OracleWorld(keep_mode, 0) for _ in range(n)]

    def set_state(self, st, aux):
        for w, s, x in zip(self.ws, st, aux):
            w.set_raw(s, x)

    def step_debug(self, actions):
        return np.stack([w.step(a)[4] for w, a in zip(self.ws, actions)])

    def get_state(self):
        return np.stack([w.get_raw()[0] for w in self.ws])


class HostArenas:
    def __init__(self, n, keep_mode):
        self.env = HostVec(n, keep_mode=keep_mode, mode=0, auto_reset=False)

    def set_state(self, st, aux):
        self.env.set_state(st, aux)

    def step_debug(self, actions):
        return self.env.step(actions, debug=True).debug

    def get_state(self):
        return self.env.get_state()[0]


@pytest.fixture(scope="module")
def batches():
    return {keep: SC.Batch(keep) for keep in (False, True)}


def _measure(oracle, which, batch):
    env = OracleWorlds(oracle, batch.n, batch.keep_mode) if which == "oracle" else HostArenas(batch.n, batch.keep_mode)
    return SC.measure(batch, *SC.run(env, batch))


@pytest.mark.parametrize("which", ["oracle", "hostcheck"])
def test_laws_hold(oracle, batches, which):
    """A-F on the pinned restatement and on the kernel source: every figure within 4 x the oracle's float32 rounding,
    and the scenes' coverage conditions (contacts per family, sliding and sticking bounces, steps at the cone's
    edge)."""
    m = _measure(oracle, which, batches[False])
    print({k: v for k, v in m.items() if not k.endswith("_log")})
    SC.check(m)
    assert batches[False].n % 64 != 0


@pytest.mark.parametrize("which", ["oracle", "hostcheck"])
def test_free_flight_with_possession_laws_on(oracle, batches, which):
    m = _measure(oracle, which, batches[True])
    SC.check(m, full=False)


def _variant(oracle, flag, batch):
    oracle.set_variant(flag)  # read when a world is created (contact mixing) and at every step
    try:
        return _measure(oracle, "oracle", batch)
    finally:
        oracle.set_variant(0)


WIDE = 1000  # a wrong law misses its tolerance by orders of magnitude, not by rounding


def test_power_restitution_threshold(oracle, batches):
    """VAR_REST_THRESH0 (restitution applied below Box2D's velocity threshold): E at 0.5 m/s and D's slow bounces."""
    m = _variant(oracle, oracle.VAR_REST_THRESH0, batches[False])
    for who in (0, 1):
        v_in, got, want = m["E_log"][(who, 0.5)]
        assert abs(got - want) > 0.4 * abs(v_in), (v_in, got, want)  # the puck bounces back instead of stopping
    assert m["E_rel"] > WIDE * SC.TOL["E_rel"]
    slow = [(v, v1) for v, v1 in m["D_log"] if abs(v) <= 1.0]
    assert len(slow) >= 5 and all(abs(v1) > 0.9 * abs(v) for v, v1 in slow), slow
    assert m["D_vn"] > WIDE * SC.TOL["D_vn"]
    with pytest.raises(AssertionError):
        SC.check(m)


def test_power_restitution_mix(oracle, batches):
    """VAR_REST_MIN (restitution mixed by min: 0 against a racket): E at 8 m/s leaves with the racket, not off it."""
    m = _variant(oracle, oracle.VAR_REST_MIN, batches[False])
    for who in (0, 1):
        v_in, got, want = m["E_log"][(who, 8.0)]
        assert abs(got - want) > 0.9 * abs(v_in), (v_in, got, want)
    assert m["E_rel"] > WIDE * SC.TOL["E_rel"]


def test_power_friction_mix(oracle, batches):
    """VAR_ARITH_FRIC (arithmetic-mean friction, 0.55 instead of 0.316): B's impulses leave the Coulomb cone."""
    m = _variant(oracle, oracle.VAR_ARITH_FRIC, batches[False])
    assert max(m["B1_coulomb"], m["B2_coulomb"]) > 1.5, (m["B1_coulomb"], m["B2_coulomb"])
    assert min(m["B1_coulomb"], m["B2_coulomb"]) - 1 > WIDE * SC.TOL["B_coulomb"]


def test_power_continuous_collision(oracle, batches):
    """VAR_NO_TOI (SolveTOI skipped): F's pucks leave the rink."""
    m = _variant(oracle, oracle.VAR_NO_TOI, batches[False])
    assert m["F_out"] > 1.0, m["F_out"]

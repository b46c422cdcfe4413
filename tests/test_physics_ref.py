"""world.Step held to float64 rigid-body laws that are not derived from our solver (tests/physics_ref.py).

Every parity test compares the kernel with oracle/hk_oracle.c, our own restatement of Box2D 2.3: a misreading made
once there and copied faithfully into hk_solver.h / hk_velocity.h passes them all.  Here the CPU oracle AND the host
build of the kernel source are each held, on seeded scenes (tests/physics_scenes.py), to the closed form of a
contact-free step, momentum, energy and the Coulomb cone of a contact, and the closed forms of a puck-wall bounce and
a head-on puck-racket hit; and on a second batch (tests/physics_scenes2.py) to non-approach, the friction cone, the
centre of pressure and energy of a racket against a wall, a rink corner and a goal box, to the position solver's closed
form, and to when a goal is scored.  The oracle's deliberately wrong variants must each fail the law named for it.
"""
import pytest

import physics_scenes as SC
import physics_scenes2 as S2
from hostcheck import HostVec
from scene_lockstep import OracleWorlds


@pytest.fixture(scope="module")
def batches():
    return {keep: SC.Batch(keep) for keep in (False, True)}


@pytest.fixture(scope="module")
def batch2():
    return S2.Batch2()


def _measure(oracle, which, batch):
    env = OracleWorlds(oracle, batch.n, batch.keep_mode) if which == "oracle" else HostVec(batch.n,
                                                                                         keep_mode=batch.keep_mode)
    if isinstance(batch, S2.Batch2):
        return S2.measure(batch, *S2.run(env, batch)[:3])
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


# --------------------------------------------------- G, H, P, Q: racket-static contacts, position solver, goal sensors
BATCH_AF_SHA256 = ("a0241c9635f5f5bd7488bf56d28259f258b9683d41dc78f6fed2a02241288cfa",
                   "aee5f7e69d48505b699c2d17069d14ef2b8192525ab944ecd4af5a2bad6293ad")


def test_first_batch_is_unchanged(batches):
    """TOL of physics_scenes was measured on exactly these arrays; the second batch draws from its own generator."""
    import hashlib

    b = batches[False]
    assert (hashlib.sha256(b.state.tobytes()).hexdigest(), hashlib.sha256(b.actions.tobytes()).hexdigest()) == (
        BATCH_AF_SHA256)


@pytest.mark.parametrize("which", ["oracle", "hostcheck"])
def test_laws_hold_second_batch(oracle, batch2, which):
    """G, H, P, Q on the pinned restatement and on the kernel source."""
    m = _measure(oracle, which, batch2)
    print({k: v for k, v in m.items() if not k.endswith("_log")})
    S2.check(m)
    assert batch2.n % 64 != 0


def test_power_iterations(oracle, batch2):
    """VAR_ITERS_8_3 (world.Step(dt, 8, 3)): three position iterations leave the deep overlaps of P where sixty
    bring them to the exit, and eight velocity iterations leave the puck squeezed between racket and wall in S
    closing at 2.6 m/s.  (Eight velocity iterations leave a racket wedged in a corner of H closing at 0.019 m/s
    on this batch, 0.009 to 0.125 on others: at H's tolerance, not above it -- H does not resolve this variant.)"""
    m = _variant(oracle, oracle.VAR_ITERS_8_3, batch2)
    for who in (0, 1):
        for s in (-0.09, -0.14, -0.19):
            _, got, want = m["P_log"][(who, s, 0)]
            assert got < want - 0.01, (who, s, got, want)  # centimetres short of the closed form
    assert m["P_recurrence"] > WIDE * S2.TOL["P_recurrence"]
    assert m["S_approach"] > 10 * S2.TOL["S_approach"], m["S_approach"]  # the squeezed puck still closes at m/s
    with pytest.raises(AssertionError):
        S2.check(m)


def _q_wrong(m):
    return {(kind, probe) for _, kind, probe in m["Q_wrong"]}


def test_power_sensor_skin_plus(oracle, batch2):
    """VAR_SENSOR_SKIN_PLUS (fires a skin early): every probe that ends a step just outside scores a step early."""
    wrong = _q_wrong(_variant(oracle, oracle.VAR_SENSOR_SKIN_PLUS, batch2))
    assert {(k, p) for k in ("face", "corner") for p in (1e-3, 5e-3)} <= wrong, wrong
    assert {("graze", 1e-3), ("graze", 5e-3), ("along", 1e-3), ("along", 5e-3)} <= wrong, wrong  # these never score


def test_power_sensor_skin_minus(oracle, batch2):
    """VAR_SENSOR_SKIN_MINUS (the sensor's skin dropped): every probe that ends a step just inside scores late."""
    wrong = _q_wrong(_variant(oracle, oracle.VAR_SENSOR_SKIN_MINUS, batch2))
    assert {(k, p) for k in ("face", "corner", "along") for p in (-1e-3, -5e-3)} <= wrong, wrong


def test_power_sensor_core(oracle, batch2):
    """VAR_SENSOR_CORE (the puck's centre must be inside the box): late or never, on every scoring scene."""
    m = _variant(oracle, oracle.VAR_SENSOR_CORE, batch2)
    wrong = _q_wrong(m)
    assert {(k, p) for k in ("face", "corner") for p in S2.Q_PROBES} <= wrong, wrong
    assert {("along", -1e-3), ("along", -5e-3)} <= wrong, wrong


def test_power_sensor_swept(oracle, batch2):
    """VAR_SENSOR_SWEPT (the sensor tested along the sweep): the pucks that jump the box between two steps score."""
    m = _variant(oracle, oracle.VAR_SENSOR_SWEPT, batch2)
    kinds = [kind for _, kind, _ in m["Q_wrong"]]
    assert kinds.count("tunnel") == int((batch2.kind == "tunnel").sum()) > 0, kinds

"""Sleeping and wake-up held to Box2D's island rule (tests/sleep_ref.py) and to the float64 laws of physics_ref.

No lockstep game is known to put a body to sleep, so the awake-conditioned code of the step (the sequential narrow
phase of a lane with a sleeper, the island seeds, the TOI eligibility, SetAwake(false), the stores of changed sleep
words) was compared with the oracle only by accident, and the oracle's own reading of the rule with nothing.  Here the
CPU oracle AND the host build of the kernel source run seeded scenes that put bodies to sleep and wake them
(tests/sleep_scenes.py); each is held to the rule -- 25 quiet steps of a float32 timer, the island minimum, exact zero
velocities, a timer that waking an awake body does not restart, a force that acts in the step that wakes -- and the
two must agree bit for bit.  The oracle's deliberately wrong variants must each fail the law named for it.
"""
import numpy as np
import pytest

import sleep_ref as Z
import sleep_scenes as ZS
from hostcheck import HostVec
from scene_lockstep import OracleWorlds, same_bits

WIDE = 1000  # a wrong law misses its tolerance by orders of magnitude, not by rounding


BATCHES = {"main": ("main", False), "z1": ("z1", False), "z1_keep": ("z1", True)}


@pytest.fixture(scope="module")
def batches():
    return {k: ZS.Batch(*v) for k, v in BATCHES.items()}


@pytest.fixture(scope="module")
def runs(oracle, batches):
    """(S, D) of every batch on the oracle and on the host build, computed once and left unchanged."""
    out = {}
    for name, b in batches.items():
        for which in ("oracle", "hostcheck"):
            env = OracleWorlds(oracle, b.n, b.keep_mode) if which == "oracle" else HostVec(b.n, keep_mode=b.keep_mode)
            out[name, which] = ZS.run(env, b)
            for a in out[name, which]:
                a.setflags(write=False)
    return out


def test_the_25_steps():
    """The float32 running sum of float32(0.02) reaches 0.5 on the 25th add; the exact product does not."""
    assert Z.steps_to_sleep() == (25, 26)
    assert 25 * float(Z.H32) < 0.5 < 26 * float(Z.H32)
    assert ZS.N_SLEEP == 25 and ZS.T0 > ZS.N_SLEEP and ZS.T0 + ZS.Z4_HIT[1] < ZS.T0 + ZS.N_SLEEP - 1


def test_batches(batches):
    b = batches["main"]
    assert 240 <= b.n <= 253 and b.n % 64 != 0 and ZS.K == 96
    fams = [set(b.family[w:w + 64]) for w in range(0, b.n, 64)]
    assert all(len(f) >= 3 for f in fams), fams  # every wave mixes scene families
    x, = np.nonzero(b.family == "Z4X")
    assert len(x) == ZS.COUNTS["Z4"] and (x // 64 != b.twin[x] // 64).all()  # twins in different waves
    assert (b.family[b.twin[x]] == "Z4Y").all() and (b.twin[b.twin[x]] == x).all()
    assert batches["z1"].n == 65 and set(batches["z1"].family) == {"Z1"} and batches["z1_keep"].keep_mode


@pytest.mark.parametrize("which", ["oracle", "hostcheck"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_laws_hold(batches, runs, name, which):
    """Every family's law and every coverage minimum, on the pinned restatement and on the kernel source."""
    m = ZS.measure(batches[name], *runs[name, which])
    print(m)
    ZS.check(m, batches[name])
    if name == "main":  # what the scenes were built to show, on this seed
        assert m["I_touch_index"] == [2] and m["I_sleep_index"] == [26], (m["I_touch_index"], m["I_sleep_index"])
        assert m["Z1_asleep_at_24"] == m["Z1_bodies"] and m["Z2_left_out"] == 0 and m["I_qualifying"] >= ZS.I_MIN


@pytest.mark.parametrize("name", list(BATCHES))
def test_oracle_and_kernel_source_agree_bit_for_bit(batches, runs, name):
    for want, got, what in zip(runs[name, "oracle"], runs[name, "hostcheck"], ("state before", "debug row of")):
        same_bits(got, want, "%s: host build's %s" % (name, what), batches[name].family)


# ------------------------------------------------------------------------------------ the wrong variants
def _variant(oracle, flag, batch):
    oracle.set_variant(flag)
    try:
        m = ZS.measure(batch, *ZS.run(OracleWorlds(oracle, batch.n, batch.keep_mode), batch))
    finally:
        oracle.set_variant(0)
    with pytest.raises(AssertionError):
        ZS.check(m, batch)
    return m


def test_power_no_sleep(oracle, batches):
    """VAR_NO_SLEEP: nothing of Z1 is asleep at index 24, or ever."""
    m = _variant(oracle, oracle.VAR_NO_SLEEP, batches["main"])
    assert m["Z1_asleep_at_24"] == 0 and not m["Z1_zero"]


def test_power_wake_resets_timer(oracle, batches):
    """VAR_WAKE_RESETS_TIMER: the rackets, handed a zero force with wake = true every step, never sleep; the pucks,
    which nothing loads, still do."""
    m = _variant(oracle, oracle.VAR_WAKE_RESETS_TIMER, batches["main"])
    assert m["Z1_rackets_at_24"] == 0 and m["Z1_asleep_at_24"] == m["Z1_bodies"] // 3 and m["Z1_puck_frozen"]


def test_power_sleep_keeps_velocity(oracle, batches):
    """VAR_SLEEP_KEEPS_VELOCITY: asleep, but not exactly zero (the pucks stand still with a velocity) nor frozen (the
    rackets, woken by the next step's force, creep on)."""
    m = _variant(oracle, oracle.VAR_SLEEP_KEEPS_VELOCITY, batches["main"])
    assert not m["Z1_zero"] and not m["Z1_frozen"] and m["Z1_asleep_at_24"] == 0


def test_power_sleep_per_body(oracle, batches):
    """VAR_SLEEP_PER_BODY: I's racket sleeps at index 24 on its own timer, not with the puck.  Z1-Z4 hold lone
    bodies, whose island minimum is their own timer: they do not see this variant."""
    m = _variant(oracle, oracle.VAR_SLEEP_PER_BODY, batches["main"])
    assert m["I_racket_alone_at_24"] == m["I_scenes"] and m["I_together"] == 0
    assert m["Z1_asleep_at_24"] == m["Z1_bodies"] and m["Z2_on_time"] == m["Z2_scenes"]


def test_power_sleeper_drops_force(oracle, batches):
    """VAR_SLEEPER_DROPS_FORCE: Z3's rackets stay put in the step that wakes them."""
    m = _variant(oracle, oracle.VAR_SLEEPER_DROPS_FORCE, batches["main"])
    assert m["Z3_wake_force"] > 0.99 and m["Z3_wake_speed"] == 0.0  # the whole force is lost, relative error 1
    assert m["Z1_asleep_at_24"] == m["Z1_bodies"] and m["Z3_puck_at_24"] == m["Z3_scenes"]

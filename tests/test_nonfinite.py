"""Values that are not finite numbers, on the CPU: the kernel source's host build and the oracle held to the
contract of include/hockey.h ("Non-finite values") over the scenarios of tests/nonfinite_cases.py.

External values (actions, phase increments) are sanitised where the step fetches them: the host build equals the
oracle bit for bit on every output, the final state and the counters; both equal a twin run that is fed what the
value must act as; HK_CNT_BAD_ACTION equals the number of arena-steps that carried such a value; the state stays
finite.  Non-finite state is not sanitised: the step terminates, no other arena changes, and a masked reset restores
the affected arenas -- each scenario in a child process under a flat limit, which is a hang detector, not a timing
(a scenario takes well under a second)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nonfinite_cases as C
from hostcheck import HostVec
from vec_lockstep import FIELDS, first_mismatch

N_ARENAS = 128
CNT_BAD_ACTION = 9
HANG_LIMIT_S = 60


def _run(oracle, x):
    """Host build and oracle through scenario inputs x, in lockstep: every output field of every arena and step,
    the final state and the counters the oracle keeps are equal; the state is finite.  Returns the host build's
    per-step outputs, final state and counters."""
    kw = dict(keep_mode=True, mode=x.mode, policies=x.policies, auto_reset=True, seed=x.seed)
    env, ov = HostVec(x.n, **kw), oracle.OracleVec(x.n, **kw)
    got = C.run_steps(env, x, C.host_step)
    want = C.run_steps(ov, x, C.oracle_step)
    for t in range(C.STEPS):
        bad = first_mismatch(t, got[t], want[t], fields=FIELDS)
        assert bad is None, bad
        assert all(np.isfinite(got[t][f]).all() for f in ("obs", "obs2", "reward", "reward2", "info", "info2")), t
    st, aux = env.get_state()
    ost, oaux = ov.get_state()
    assert np.array_equal(st.view(np.uint32), ost.view(np.uint32)) and np.array_equal(aux, oaux)
    assert np.isfinite(st).all()
    c, oc = env.counters().astype(np.int64), ov.counters()
    assert np.array_equal(c[:5], oc[:5]), (c, oc)
    assert c[CNT_BAD_ACTION] == oc[CNT_BAD_ACTION] == x.count, (c, oc, x.count)
    assert c[5] == 0 and c[7] == 0, c  # no capacity overflow, no bad policy id
    env.close()
    ov.close()
    return got, (st, aux), c


def _assert_twin(run, twin, x):
    """The run that carried the value equals its twin bit for bit, apart from HK_CNT_BAD_ACTION."""
    fields = tuple(f for f in FIELDS if f not in x.twin_fields_differ)
    for t in range(C.STEPS):
        bad = first_mismatch(t, run[0][t], twin[0][t], fields=fields)
        assert bad is None, ("twin", bad)
    assert np.array_equal(run[1][0].view(np.uint32), twin[1][0].view(np.uint32))
    assert np.array_equal(run[1][1], twin[1][1])
    assert np.array_equal(run[2][:CNT_BAD_ACTION], twin[2][:CNT_BAD_ACTION]), (run[2], twin[2])
    assert twin[2][CNT_BAD_ACTION] == 0


@pytest.mark.parametrize("kind", list(C.ACTION_KINDS))
@pytest.mark.parametrize("mode", C.MODES)
def test_action_values(oracle, mode, kind):
    """Every action value in each of the 8 components (five placements per batch, nonfinite_cases.C0S), at lanes
    0, 5, 63, 64 and 127 of 128 arenas, 10 clean then 60 affected steps.  NaN of any sign or payload acts as 0,
    +-Inf and +-3e38 as +-1; a denormal and -0.0 are ordinary values."""
    for c0 in C.C0S:
        twins = {}
        for value, (_, acts_as) in C.ACTION_VALUES.items():
            x = C.action_inputs(N_ARENAS, kind, mode, value, c0, seed=mode)
            run = _run(oracle, x)
            if acts_as is None:
                continue
            if acts_as not in twins:  # the twin's inputs depend on what the value acts as only
                twins[acts_as] = _run(oracle, C.twin_of(x))
            _assert_twin(run, twins[acts_as], x)


@pytest.mark.parametrize("kind", list(C.INC_KINDS))
@pytest.mark.parametrize("mode", C.MODES)
def test_phase_increment_values(oracle, mode, kind):
    """NaN and +-Inf BasicOpponent phase increments act as 0 (the phase stands still) and are counted, whether or
    not a bot reads that increment in that step."""
    twin = None
    for value in C.INC_VALUES:
        x = C.inc_inputs(N_ARENAS, kind, mode, value, seed=mode)
        run = _run(oracle, x)
        if twin is None:
            twin = _run(oracle, C.twin_of(x))
        _assert_twin(run, twin, x)


def test_one_count_per_arena_step(oracle):
    """An arena-step with several sanitised values -- two NaN components and a non-finite increment -- counts once."""
    x = C.inc_inputs(N_ARENAS, "ext_strong", 0, "nan", seed=5)
    for a in C.lanes(N_ARENAS):
        x.acts[C.CLEAN:, a, 1] = np.nan
        x.acts[C.CLEAN:, a, 6] = np.nan  # player 2 is the fused bot here: not read, still counted
    x.acts[3, 17, 2] = np.nan  # one more arena-step, outside the schedule
    x.count += 1
    _run(oracle, x)


def test_single_world_oracle_mirrors_the_rule(oracle):
    """OracleWorld (hko_step): a NaN component acts as 0 and bad_action() reports the step; +-Inf clips."""
    a, b = oracle.OracleWorld(True, 0), oracle.OracleWorld(True, 0)
    p6 = np.array([7.0, 4.5, 3.0, 4.2, 0.0, 0.0], np.float32)
    a.reset(p6, 250)
    b.reset(p6, 250)
    rng = np.random.default_rng(3)
    for t in range(40):
        act = rng.uniform(-1, 1, 8).astype(np.float32)
        twin = act.copy()
        k = t % 8
        act[k], twin[k] = (np.nan, 0.0) if t % 3 else (np.inf, 1.0)
        o1, r1, d1, i1, _ = a.step(act)
        o2, r2, d2, i2, _ = b.step(twin)
        assert a.bad_action() == (1 if t % 3 else 0) and b.bad_action() == 0
        assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and r1 == r2 and d1 == d2
        assert np.array_equal(i1, i2) and np.isfinite(o1).all()


@pytest.mark.parametrize("name", list(C.STATE_CASES))
def test_state_borne_values_are_contained(oracle, name):
    """+-Inf positions, angles and velocities, velocities that overflow within a step, and NaN / Inf placement
    params in the affected arenas: the run ends within the hang limit, the unaffected arenas equal the clean twin
    and the oracle bit for bit at every step, and after a masked reset the whole batch equals the oracle for 60
    more steps.  Nothing is asserted about the affected arenas' values while they hold such state."""
    HostVec(1).close()  # the libraries are built before the clock starts
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nonfinite_cases.py")
    p = subprocess.run([sys.executable, script, name], capture_output=True, text=True, timeout=HANG_LIMIT_S)
    assert p.returncode == 0, (name, p.stdout[-2000:], p.stderr[-2000:])

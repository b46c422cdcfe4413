"""The TOI event path on the CPU: the event waves of tests/toi_lean_zoo.py through the host build of the kernel
source, against the oracle at tolerance zero.  solve_toi sends every one-contact event down
toi_island_solve_one and every other event down toi_island_solve -- both routines run
here, and the host build's lean-path counter says how often.

The comparisons pin what the event path computes, not which routine computes it: they hold for a library built
without the lean routine as well (only the counter assertions need it).
"""
import ctypes

import numpy as np
import pytest

import toi_lean_zoo as Z
import wave_zoo as W
from hostcheck import HostVec, lib
from vec_lockstep import first_mismatch

FIELDS = ("obs", "obs2", "reward", "reward2", "done", "info", "info2")


def lean_events():
    """TOI events that took the lean path since the last call (read and cleared)."""
    L = lib()
    L.hkh_toi_lean.restype = ctypes.c_ulonglong
    L.hkh_toi_lean.argtypes = []
    return int(L.hkh_toi_lean())


@pytest.fixture(scope="module")
def batch():
    return Z.lean_batch()


def _lockstep(oracle, state, aux, actions, toi, describe):
    n = state.shape[0]
    env = HostVec(n)
    ov = oracle.OracleVec(n, policies=("external", "external"), auto_reset=False)
    env.set_state(state, aux)
    ov.set_state(state, aux)
    for t in range(W.K):
        got = vars(env.step(actions[t], with_agent_two=True))
        want = ov.step(actions[t], with_agent_two=True)
        bad = first_mismatch(t, got, want, fields=FIELDS)
        assert bad is None, (bad, describe(bad["arena"], t) if "arena" in bad else "")
    st, ax = env.get_state()
    ost, oax = ov.get_state()
    assert np.array_equal(st.view(np.uint32), ost.view(np.uint32)) and np.array_equal(ax, oax)
    c, oc = env.counters().astype(np.int64), ov.counters()
    assert np.array_equal(c[:5], oc[:5]) and c[5] == 0
    assert c[4] == toi.sum()  # the TOI counter against the labels
    assert c[6] == 0  # no solve on the HBM slot file
    env.close()
    ov.close()


def test_event_waves_host_build_vs_oracle(oracle, batch):
    """The composed batch, lane by lane; the lean routine took exactly the one-contact events of the labels."""
    lean_events()
    _lockstep(oracle, batch.state, batch.aux, batch.actions, batch.toi, batch.describe)
    assert lean_events() == batch.toi_one.sum() > 0


def test_one_contact_scenario_takes_the_lean_path(oracle, batch):
    """The single toi1 scenario as a one-arena context: bit-exact, and every event of it on the lean path."""
    state, aux, actions, toi = batch.one(batch.single)
    lean_events()
    _lockstep(oracle, state, aux, actions, toi, lambda a, t: "the single toi1 scenario")
    assert lean_events() == toi.sum() > 0


def test_two_contact_scenario_takes_the_generic_path(oracle, batch):
    """A scenario whose only TOI event builds a two-contact mini-island: bit-exact, and nothing on the lean path."""
    arena = 64 + 13  # wave 1's toim2 lane
    state, aux, actions, toi = batch.one(arena)
    assert batch.idx[arena] in batch.m2 and toi.sum() == 1 and batch.toi_one[arena].sum() == 0
    lean_events()
    _lockstep(oracle, state, aux, actions, toi, lambda a, t: "the toim2 scenario")
    assert lean_events() == 0

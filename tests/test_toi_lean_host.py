"""The TOI event path on the CPU: the event waves of tests/toi_lean_zoo.py through the host build of the kernel
source, against the oracle at tolerance zero.  solve_toi sends every one-contact event down
toi_island_solve_one and every other event down toi_island_solve -- both routines run
here, and the host build's lean-path counter says how often.

The comparisons pin what the event path computes, not which routine computes it: they hold for a library built
without the lean routine as well (only the counter assertions need it).
"""
import ctypes

import pytest

import toi_lean_zoo as Z
from hostcheck import HostVec, lib
from scene_lockstep import check_run, oracle_run, scene_env


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
    """W.K steps of the host build against the oracle: outputs, final state, counters 0 to 4, the TOI counter against
    the labels, no overflow and no solve on the HBM slot file."""
    want = oracle_run(oracle, state, aux, actions)
    check_run(scene_env(HostVec, state, aux), actions, "hk_step", want, "host build", describe=describe, toi=toi,
              large=0)


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

"""The work-list overflow batch on the CPU (tests/wave_list_scenes.py): every lane is certain to list the items
that send its wave round the cooperative drains a second time, and the oracle steps the batch to finite states
through at least one TOI event, and the kernel source's host build steps it bit for bit like the oracle.  The waves
themselves run only on the GPU (tests/test_gpu_wave_list.py): the host build steps one lane at a time."""
import numpy as np
import pytest

import wave_list_scenes as L
from hostcheck import HostVec
from scene_lockstep import check_run, oracle_run, scene_env


@pytest.fixture(scope="module")
def batch():
    return L.Batch()


def test_scene_data_parses_to_the_pair_table():
    S = L.scene()
    assert S["pairA"].shape == S["pbodyB"].shape == S["sensor"].shape == (27,)
    assert S["fx_aabb"].shape == (13, 4) and S["rcore"].shape == (3,) and S["lc"].shape == (3, 2)
    assert (S["pbodyA"] != L.B_PK).all() and (S["pbodyB"] <= L.B_PK).all()
    assert S["circle"].tolist() == [0] * 12 + [1] and S["rcore"][L.B_PK] == 0.0


def test_every_lane_is_certain_to_list_enough_items(batch):
    """At least 3 items per lane of the full wave and 4 per lane of the 37-lane wave, in each of the two lists:
    192 and 148 items, both above the list's 128, so each wave takes the overflow round in each drain."""
    collide, toi = L.near_counts(batch.state, L.scene())
    assert batch.n == 101 and L.N_FULL == 64 and L.N_PART == 37
    for name, cnt in (("collide", collide), ("toi", toi)):
        full, part = cnt[:L.N_FULL], cnt[L.N_FULL:]
        assert (full >= L.MIN_FULL).all(), (name, np.nonzero(full < L.MIN_FULL)[0], full)
        assert (part >= L.MIN_PART).all(), (name, np.nonzero(part < L.MIN_PART)[0], part)
        assert full.sum() > L.WAVE_Q and part.sum() > L.WAVE_Q and len(part) < 64, (name, full.sum(), part.sum())
    assert len(set(collide[:L.N_FULL].tolist())) > 1, "queue lengths vary across the full wave's lanes"


def test_oracle_steps_the_batch_to_finite_states_with_toi_events(oracle, batch):
    ov = oracle.OracleVec(batch.n, policies=("external", "external"), auto_reset=False)
    ov.set_state(batch.state, batch.aux)
    for t in range(L.K):
        out = ov.step(batch.actions[t], with_agent_two=True)
        for f in ("obs", "obs2", "reward", "info"):
            assert np.isfinite(out[f]).all(), (t, f)
    st, _ = ov.get_state()
    toi = int(ov.counters()[4])
    ov.close()
    assert np.isfinite(st).all()
    assert toi >= 1, toi


def test_batch_host_build_vs_oracle(oracle, batch):
    """The batch through the host build for L.K steps: every step output, the final state and aux rows, counters 0
    to 4 and no overflow, against the oracle.  Lane by lane: this checks the scenarios, not the waves.  The host
    build takes the large-island path on some of these lanes, which the oracle does not count, and the scenes carry
    no TOI labels: neither counter is held here."""
    want = oracle_run(oracle, batch.state, batch.aux, batch.actions)
    assert len(want["steps"]) == L.K
    check_run(scene_env(HostVec, batch.state, batch.aux), batch.actions, "hk_step", want, "host build",
              describe=batch.describe, toi=None, large=None)

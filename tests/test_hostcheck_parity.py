"""The kernel's per-arena source (hk_step.h -> hk_arena.h / hk_solver.h / hk_velocity.h / hk_geom.h), compiled for the host
CPU by tests/hostcheck.py, held bit-for-bit to the oracle -- on the CPU, without a GPU.

This catches logic errors in the device code before a GPU run; the GPU parity tests (test_gpu_parity.py)
then hold the gfx950 binary of the same source to the same oracle.  The harness is test infrastructure
(never loaded by the product package).
"""
from functools import partial

import numpy as np
import pytest

from hostcheck import HostVec, velocity_diag
from scene_lockstep import batched_lockstep, world_lockstep
from vec_lockstep import first_mismatch

# the two game locksteps of tests/scene_lockstep.py on the host build (test_gpu_parity.py: the same two on the GPU)
_lockstep = partial(world_lockstep, HostVec)
_vec_lockstep = partial(batched_lockstep, HostVec)


@pytest.mark.parametrize("mode,seed", [(0, 1), (1, 3), (2, 4)])
def test_kernel_source_lockstep_vs_oracle(oracle, mode, seed):
    out = _lockstep(oracle, mode, n=48, steps=200, seed=seed)
    assert "field" not in out, out
    if mode == 0:
        assert out["n_toi"] > 0


def test_large_island_solver_vs_oracle(oracle):
    """diag_flags=HK_DIAG_LARGE_ISLANDS routes every island / TOI solve through the HBM slot file (HbmSlots,
    the path of islands with more contacts than the register slots) -- it must be bit-identical as well."""
    out = _lockstep(oracle, 1, n=32, steps=150, seed=3, diag_flags=1)
    assert "field" not in out, out
    assert out["counters"][6] > 0  # large-island solves were taken


def test_fused_opponents_autoreset_run(oracle):
    """Fused strong/weak BasicOpponent with device auto-reset: counters consistent, no overflow."""
    env = HostVec(256, policies=("strong", "weak"), auto_reset=True, seed=7)
    for _ in range(300):
        env.step(None)
    c = env.counters()
    assert c[0] == 256 * 300 and c[5] == 0
    assert c[1] > 0 and c[2] + c[3] <= c[1]


# ------------------------------------------------------------------------------------------------ batched contract
@pytest.mark.parametrize("mode,steps", [(0, 560), (1, 200), (2, 200)])
def test_bench_path_vs_oracle_vec(oracle, mode, steps):
    """The benchmarked workload (strong vs strong, in-kernel Philox phase increments, auto-reset with device
    placement): every arena rolls over at least twice in every mode."""
    out = _vec_lockstep(oracle, 64, steps, mode, ("strong", "strong"), seed=5 + mode)
    assert "field" not in out, out
    assert out["counters"][1] >= 2 * 64


def test_random_and_external_policies_vs_oracle_vec(oracle):
    out = _vec_lockstep(oracle, 48, 300, 0, ("random", "weak"), seed=21, offset=1000)
    assert "field" not in out, out
    out = _vec_lockstep(oracle, 48, 300, 2, ("external", "strong"), seed=22, external=True)
    assert "field" not in out, out


def test_per_step_opponent_mix_vs_oracle_vec(oracle):
    """Player 2's opponent drawn per arena and step (hk_step_io.policy2, rl/training/opponent_manager.py:62-91):
    external (self-play actions), weak bot and strong bot, each bot with its own phase."""
    out = _vec_lockstep(oracle, 48, 300, 0, ("external", "external"), seed=23, external=True, mix=True)
    assert "field" not in out, out
    out = _vec_lockstep(oracle, 32, 200, 1, ("strong", "weak"), seed=24, external=True, mix=True)
    assert "field" not in out, out


def test_island_retirement_and_slot_swaps_vs_oracle(oracle):
    """Islands of one lane retire one by one inside the shared velocity loop (hk_velocity.h vgen / vtwo), and
    the live contacts are swapped into the one- and two-contact slots: both paths run in a bit-exact lockstep
    of the strong-vs-strong workload against the oracle (which solves island by island, like Box2D)."""
    velocity_diag()
    out = _vec_lockstep(oracle, 256, 400, 0, ("strong", "strong"), seed=31)
    assert "field" not in out, out
    d = velocity_diag()
    assert d[0] > 0 and d[1] > 0, d


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_keep_mode_false_with_physics_vs_oracle_vec(oracle, mode):
    """Hockey-v0 with keep_mode=False (hockey_env.py:91): 6-dim joint action, player 2's action at index 3
    (:663), no hold / shoot (:668-680) -- with world.Step running, external random actions and the fused
    BasicOpponent(keep_mode=False) in every mode."""
    out = _vec_lockstep(oracle, 48, 260, mode, ("external", "strong"), seed=41 + mode, external=True,
                        keep_mode=False)
    assert "field" not in out, out
    out = _vec_lockstep(oracle, 48, 200, mode, ("weak", "strong"), seed=44 + mode, keep_mode=False)
    assert "field" not in out, out


def test_live_velocity_semantics_with_physics_vs_oracle_vec(oracle):
    """SURVEY App. B Q1 live-reference velocity getters (vel_ref_semantics=1, hockey_env.py:425-432) with
    world.Step running: random external actions (boundary hits) and the strong-vs-strong workload."""
    out = _vec_lockstep(oracle, 48, 300, 0, ("external", "external"), seed=47, external=True, vel_ref=True)
    assert "field" not in out, out
    out = _vec_lockstep(oracle, 48, 300, 1, ("strong", "strong"), seed=48, vel_ref=True)
    assert "field" not in out, out


def test_step_record_matches_outputs_and_state(oracle):
    """hk_step_io.record (the single-env facade's one-copy step result): float64 info / info2 / rewards whose
    float32 roundings are the step's float outputs (oracle-checked), and has_puck / time / done / winner equal
    to the state after the step -- over a strong-vs-strong run with goals and holds."""
    n = 64
    env = HostVec(n, policies=("strong", "strong"), auto_reset=False, seed=9)
    ov = oracle.OracleVec(n, policies=("strong", "strong"), auto_reset=False, seed=9)
    held = 0
    for t in range(300):
        got = env.step(None, with_agent_two=True, record=True)
        want = ov.step(with_agent_two=True)
        rec = got.record
        assert first_mismatch(t, {"info": rec[:, 0:4].astype(np.float32), "info2": rec[:, 4:8].astype(np.float32),
                                  "reward": rec[:, 8].astype(np.float32), "reward2": rec[:, 9].astype(np.float32)},
                              want, fields=("info", "info2", "reward", "reward2")) is None
        _, aux = env.get_state()
        assert np.array_equal(rec[:, 10:15].astype(np.int32), aux), t
        assert np.array_equal(rec[:, 13].astype(np.uint8), got.done) and np.all(rec[:, 15] == 0)
        held += int((aux[:, 0] > 0).sum())
    assert aux[:, 3].sum() > 0 and held > 0  # goals and holds happened



def test_shape_families_vs_oracle(oracle):
    """The tail's shape-specialised velocity loops (r06, hk_velocity.h): the S2 two-contact chunk (contact 1's body B
    aliased to contact 0's body A, contact 1 static-A) and the S3 three-contact family (wall-puck, player-puck,
    wall-player with the two dynamic bodies in locals) both run in a bit-exact lockstep of the strong-vs-strong
    bench workload against the oracle.  (The host build runs one lane at a time, so the riders and mixed waves of
    those loops run on the GPU only: tests/test_gpu_wave_zoo.py composes them lane by lane from the table in
    tests/wave_zoo.py.)"""
    velocity_diag()
    out = _vec_lockstep(oracle, 1024, 400, 0, ("strong", "strong"), seed=41)
    assert "field" not in out, out
    d = velocity_diag()
    assert d[2] > 0 and d[3] > 0, d

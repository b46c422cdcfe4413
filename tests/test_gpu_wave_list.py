"""The cooperative drains' overflow round and partial-wave worker count on the GPU (hk_collide.h collide_near_wave,
hk_world.h toi_drain_wave).

tests/wave_list_scenes.py builds 101 arenas: a full wave whose lanes are certain to list 192 items or more in each
of the two drains (Collide's narrow phases, SolveTOI's b2TimeOfImpact calls) at step 0, and a wave of 37 lanes
certain to list 148 or more -- both above the list's 128 items, so each wave goes round again, the second with
fewer than 64 workers (tests/test_wave_list_scenes.py proves the counts on the CPU).  The batch runs through
hk_step, through hk_rollout (step_kernel<true>, its own instantiation) and with the lanes of every wave permuted
(another listing order, other owners per worker), each against one oracle run at tolerance zero: per-step outputs,
final state and the TOI counter.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from scene_lockstep import GpuVec, check_run, oracle_run, require_gfx950, scene_env, wave_permutation  # noqa: E402
import wave_list_scenes as L  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


@pytest.fixture(scope="module")
def batch():
    return L.Batch()


@pytest.fixture(scope="module")
def want(oracle, batch):
    """The oracle's answer, computed once: per-step outputs, final state, counters."""
    out = oracle_run(oracle, batch.state, batch.aux, batch.actions)
    assert len(out["steps"]) == L.K and out["counters"][N.CNT_TOI] >= 1
    return out


def _check(batch, want, path, how, rows=None):
    """Outputs, final state, counters 0 to 4 (the TOI counter among them) and no overflow.  The scenes carry no TOI
    or large-island labels."""
    rows_ = slice(None) if rows is None else rows
    check_run(scene_env(GpuVec, batch.state[rows_], batch.aux[rows_]), batch.actions, path, want, how, rows,
              batch.describe)


def test_wave_list_hk_step_vs_oracle(batch, want):
    _check(batch, want, "hk_step", "hk_step")


def test_wave_list_hk_rollout_vs_oracle(batch, want):
    _check(batch, want, "hk_rollout", "hk_rollout")


def test_wave_list_permuted_lanes_vs_oracle(batch, want):
    """The lanes of each wave permuted (fixed seed): every arena keeps its wave, so both waves still overflow."""
    perm = wave_permutation(batch.n)
    assert (perm != range(batch.n)).any()
    _check(batch, want, "hk_step", "hk_step, permuted lanes", perm)

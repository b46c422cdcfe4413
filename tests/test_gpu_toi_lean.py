"""The TOI event path on the GPU: solve_toi's choice between toi_island_solve_one (a lane whose mini-island has one
contact on register slots) and toi_island_solve, under controlled lane mixes.

The batch of tests/toi_lean_zoo.py -- a full wave of one-contact events, a wave where a two-contact lane shares the
round with one-contact lanes, a wave whose later rounds have fewer event lanes, a last wave of 37 lanes with a single
event lane -- is driven 4 steps through hk_step and hk_rollout against one oracle run at tolerance zero, once more with the lanes
of every wave permuted, and the single event scenario as a one-arena context (lane 0 alone).  The TOI counter is held
to the fixture's labels.

These comparisons pin what the event path computes, not which routine computes it: they pass on a library built
without the lean routine as well.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from scene_lockstep import GpuVec, check_run, oracle_run, require_gfx950, scene_env  # noqa: E402
import toi_lean_zoo as Z  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


@pytest.fixture(scope="module")
def batch():
    return Z.lean_batch()


@pytest.fixture(scope="module")
def want(oracle, batch):
    """The oracle's answer for the composed batch, computed once: per-step outputs, final state, counters."""
    return oracle_run(oracle, batch.state, batch.aux, batch.actions)


def _check(batch, want, path, how, rows=None):
    """The batch's arenas `rows` (all when None) as one context through `path` against the oracle: outputs, final
    state, counters (0 to 4 for the whole batch), the TOI counter against the labels, no large-island solve."""
    rows_ = slice(None) if rows is None else rows
    check_run(scene_env(GpuVec, batch.state[rows_], batch.aux[rows_]), batch.actions, path, want, how, rows,
              batch.describe, toi=batch.toi, large=0)


def test_event_waves_hk_step_vs_oracle(batch, want):
    _check(batch, want, "hk_step", "hk_step")


def test_event_waves_hk_rollout_vs_oracle(batch, want):
    _check(batch, want, "hk_rollout", "hk_rollout")


@pytest.mark.parametrize("path", ["hk_step", "hk_rollout"])
def test_event_waves_permuted_vs_oracle(batch, want, path):
    """The lanes of every wave permuted: the event lanes sit elsewhere (and lane 0 is another lane), each arena's
    answer is still the oracle's."""
    _check(batch, want, path, path + ", lanes permuted", batch.permutation())


@pytest.mark.parametrize("path", ["hk_step", "hk_rollout"])
def test_single_event_arena_alone_vs_oracle(batch, want, path):
    """The last wave's event scenario as a one-arena context: lane 0 is the only lane."""
    assert batch.toi[batch.single].sum() > 0
    _check(batch, want, path, path + ", one-arena context", np.array([batch.single]))

"""Wave-composition zoo on the GPU: the velocity-family dispatch of hk_velocity.h under controlled lane mixes.

velocity_iterations / vtwo_family / vone_family pick one of about 25 loop variants from what ALL 64 lanes of a wave
hold, re-pick at every chunk boundary, let riders discard updates through selects, swap slots and save / restore
retired contacts' impulses.  Every variant must be bit-identical, lane by lane, to the generic loop -- and whether
it is depends on the mix.  tests/wave_zoo.py composes that mix: each wave of the batch is one row of its TABLE (the
arm or event the row exists for is named there, and tests/test_wave_zoo.py proves on the CPU that the rows cover
every arm), built from the one-arena scenarios of tests/golden/wave_zoo.npz.

The batch is driven through hk_step, hk_rollout (step_kernel<true>, its own instantiation) and the
HK_DIAG_LARGE_ISLANDS path against one oracle run, with tolerance zero, and once more with the lanes of every wave
permuted: a lane's result must not depend on its neighbours.  Needs neither the probe nor a compiler.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from scene_lockstep import (STEP_FIELDS, GpuVec, check_run, oracle_run, require_gfx950, scene_env,  # noqa: E402
                            wave_permutation)
from vec_lockstep import first_mismatch  # noqa: E402
import wave_zoo as W  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


@pytest.fixture(scope="module")
def batch():
    return W.Batch(W.Zoo())


@pytest.fixture(scope="module")
def want(oracle, batch):
    """The oracle's answer for the composed batch, computed once: per-step outputs, final state, counters."""
    return oracle_run(oracle, batch.state, batch.aux, batch.actions)


def _check(batch, want, path, how, large, **kw):
    """The batch through `path` against the oracle: outputs, final state, counters, the fixture's TOI labels."""
    check_run(scene_env(GpuVec, batch.state, batch.aux, **kw), batch.actions, path, want, how,
              describe=batch.describe, toi=batch.toi, large=large)


def test_zoo_hk_step_vs_oracle(batch, want):
    """(i) K hk_step launches.  The large-island counter equals what the fixture's labels predict: lanes with more
    island contacts than register slots, TOI mini-islands with more than two."""
    _check(batch, want, "hk_step", "hk_step", batch.large)


def test_zoo_hk_rollout_vs_oracle(batch, want):
    """(ii) a fresh context through one hk_rollout(K): step_kernel<true>, a separate instantiation."""
    _check(batch, want, "hk_rollout", "hk_rollout", batch.large)


def test_zoo_large_island_path_vs_oracle(batch, want):
    """(iii) HK_DIAG_LARGE_ISLANDS: every solve of every lane on the HBM slot file."""
    _check(batch, want, "hk_step", "hk_step, large-island path", lambda c: c > batch.large,
           diag_flags=N.DIAG_LARGE_ISLANDS)


def test_zoo_lane_permutation_invariance(batch):
    """A lane's result does not depend on its neighbours: with the lanes of every wave permuted (fixed seed), each
    arena's outputs equal those of its unpermuted twin bit for bit.  GPU against GPU, no oracle."""
    perm = wave_permutation(batch.n)
    a, b = scene_env(GpuVec, batch.state, batch.aux), scene_env(GpuVec, batch.state[perm], batch.aux[perm])
    for t in range(W.K):
        ra = vars(a.step(batch.actions[t], with_agent_two=True))
        rb = vars(b.step(batch.actions[t][perm], with_agent_two=True))
        twin = {f: ra[f][perm] for f in STEP_FIELDS}
        bad = first_mismatch(t, rb, twin, fields=STEP_FIELDS)
        if bad:
            i = int(perm[bad["arena"]])
            pytest.fail("permuted lane %d (arena %d of the table) differs from its twin: %s\n%s" % (
                bad["arena"], i, bad, batch.describe(i, t)))
    (sa, xa), (sb, xb) = a.get_state(), b.get_state()
    assert np.array_equal(sa[perm].view(np.uint32), sb.view(np.uint32)) and np.array_equal(xa[perm], xb)
    assert np.array_equal(a.counters()[:8], b.counters()[:8])
    a.close()
    b.close()

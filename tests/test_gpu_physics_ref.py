"""The gfx950 step kernel held to the float64 rigid-body laws of tests/physics_ref.py, and to the oracle bit for bit
on the same scenes.

All scenes of a keep mode (tests/physics_scenes.py: free flight, puck-racket, racket-racket, wall bounces, head-on
hits, fast pucks) share ONE context, interleaved by a seeded shuffle: 943 arenas, so the waves mix scene families and
the last wave is partial -- the wave-composition dispatch of hk_velocity.h sees high-speed, set_state-injected contacts
that the lockstep games rarely visit.  The laws and the coverage counts are re-asserted on the GPU's own data, once
more on the HK_DIAG_LARGE_ISLANDS path, and every state is compared with OracleVec's with tolerance zero.

A second context of 619 arenas holds tests/physics_scenes2.py's families (racket against wall, corner, goal box and
slanted post face; the squeezed puck; the position solver; the goal sensors) to their laws in the same way, once more through hk_rollout, and compares the aux
rows and done flags as well.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from scene_lockstep import GpuVec, oracle_run, require_gfx950, same_bits  # noqa: E402
import physics_scenes as SC  # noqa: E402
import physics_scenes2 as S2  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


@pytest.fixture(scope="module")
def batches():
    return {keep: SC.Batch(keep) for keep in (False, True)}


@pytest.fixture(scope="module")
def want(oracle, batches):
    """OracleVec's states after every step of both batches, computed once."""
    return {keep: oracle_run(oracle, b.state, b.aux, b.actions, keep_mode=keep, every_step_state=True)["states"]
            for keep, b in batches.items()}


def _run(batch, want, full, **kw):
    g = GpuVec(batch.n, keep_mode=batch.keep_mode, **kw)
    S, D = SC.run(g, batch)
    counters = g.counters()
    g.close()
    m = SC.measure(batch, S, D)
    if full:
        print({k: v for k, v in m.items() if not k.endswith("_log")})
    SC.check(m, full=full)
    same_bits(S[1:], want, "state after", batch.family)
    assert counters[N.CNT_OVERFLOW] == 0
    return counters


def test_laws_and_oracle_bits_one_mixed_context(batches, want):
    b = batches[False]
    assert 900 <= b.n <= 1100 and b.n % 64 != 0
    fams = {tuple(sorted(set(b.family[w:w + 64]))) for w in range(0, b.n, 64)}
    assert all(len(f) >= 4 for f in fams), fams  # every wave mixes scene families
    c = _run(b, want[False], True)
    assert c[N.CNT_TOI] > 0


def test_free_flight_with_possession_laws_on(batches, want):
    _run(batches[True], want[True], False)


def test_laws_and_oracle_bits_large_island_path(batches, want):
    """HK_DIAG_LARGE_ISLANDS: every solve of every lane through the HBM slot file."""
    c = _run(batches[False], want[False], True, diag_flags=N.DIAG_LARGE_ISLANDS)
    assert c[N.CNT_LARGE_ISLANDS] > 0


# --------------------------------------------------- G, H, P, Q: racket-static contacts, position solver, goal sensors
@pytest.fixture(scope="module")
def batch2():
    return S2.Batch2()


@pytest.fixture(scope="module")
def want2(oracle, batch2):
    """OracleVec's states, aux rows and done flags after every step of the second batch, computed once."""
    b = batch2
    run = oracle_run(oracle, b.state, b.aux, b.actions, keep_mode=False, every_step_state=True)
    done = np.stack([s["done"] for s in run["steps"]])
    done.setflags(write=False)
    return run["states"], run["auxs"], done


def _label(batch):
    return ["family %s %s" % fk for fk in zip(batch.family, batch.kind)]


def _run2(batch, want, **kw):
    g = GpuVec(batch.n, keep_mode=False, **kw)
    S, D, A, done = S2.run(g, batch)
    counters = g.counters()
    g.close()
    m = S2.measure(batch, S, D, A)
    print({k: v for k, v in m.items() if not k.endswith("_log")})
    S2.check(m)
    same_bits(S[1:], want[0], "state after", _label(batch))
    same_bits(A[1:], want[1], "aux (has_puck, time, done, winner) after", _label(batch))
    same_bits(done, want[2], "done of", _label(batch))
    assert counters[N.CNT_OVERFLOW] == 0
    return counters, S, A, done


def test_second_batch_one_mixed_context(batch2, want2):
    """G, H, P, Q shuffled into one context: the laws and coverage counts on the GPU's own states and aux rows, and
    every state, aux row and done flag equal to OracleVec's bit for bit."""
    b = batch2
    assert 300 <= b.n <= 700 and b.n % 64 != 0
    assert (b.kind == "post").sum() >= 40 and (b.family == "S").sum() >= 40
    fams = {tuple(sorted(set(b.family[w:w + 64]))) for w in range(0, b.n, 64)}
    assert all(len(f) >= 4 for f in fams), fams  # every wave mixes scene families
    _run2(b, want2)


def test_second_batch_large_island_path(batch2, want2):
    c = _run2(batch2, want2, diag_flags=N.DIAG_LARGE_ISLANDS)[0]
    assert c[N.CNT_LARGE_ISLANDS] > 0


def test_second_batch_rollout(batch2, want2):
    """hk_rollout: the six steps in one launch.  It returns each step's done flag and leaves the final state, nothing
    per step, so G, H, S and P are held here only THROUGH the final state: it must be the oracle's bit for bit, hence
    the step-by-step run's, whose per-step laws the tests above hold.  The goal law is re-asserted on the rollout's own
    done flags and final winner."""
    b = batch2
    g = GpuVec(b.n, keep_mode=False)
    g.set_state(b.state, b.aux)
    done = np.stack([r["done"] for r in g.rollout(b.actions)])
    st, aux = g.get_state()
    counters = g.counters()
    g.close()
    same_bits(done, want2[2], "done of", _label(b))
    same_bits(st[None], want2[0][-1:], "final state, rollout", _label(b))
    same_bits(aux[None], want2[1][-1:], "final aux, rollout", _label(b))
    assert counters[N.CNT_OVERFLOW] == 0
    # Q from the rollout's flags: done in step j exactly when an earlier step's end state overlapped the sensor
    import physics_ref as P

    S = np.concatenate([b.state[None], want2[0]]).astype(np.float64)  # bit-equal to the GPU's, asserted above
    for i in np.nonzero(b.family == "Q")[0]:
        sep = P.goal_separation(S[:, i, 12:14], int(b.goal[i]))
        inside = np.nonzero(sep[1:] < 0)[0]
        want_done = np.zeros(SC.K, np.uint8)
        if len(inside):
            want_done[int(inside[0]) + 1:] = 1
        assert (done[:, i] == want_done).all(), (i, b.kind[i], sep, done[:, i])
        assert aux[i, 4] == (0 if not want_done.any() else (-1 if b.goal[i] == 0 else 1))

"""The gfx950 step kernel held to Box2D's island sleep rule (tests/sleep_ref.py) and to the oracle bit for bit on
scenes that put bodies to sleep and wake them (tests/sleep_scenes.py).

One context of 249 arenas holds every family, interleaved by a seeded shuffle, so a lane with a sleeper takes the
sequential narrow phase of collide() while its wave-mates stay on the wave-wide one, the twins of Z4 sit in different
waves, and the last wave is partial.  A second context of 65 arenas, all Z1, has every lane of its first wave on the
sequential path from step 25 on and one lane in its second.  In each run the laws and the coverage counts are
re-asserted on the GPU's own data and every state word of every step equals OracleVec's.  The main batch runs once
more through hk_rollout (two launches split at T0), once more on the HK_DIAG_LARGE_ISLANDS path, and once more through
a snapshot taken while pucks sleep and restored into a fresh context.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from scene_lockstep import GpuVec, oracle_run, require_gfx950, same_bits  # noqa: E402
import sleep_scenes as ZS  # noqa: E402

BATCHES = {"main": ("main", False), "z1": ("z1", False), "z1_keep": ("z1", True)}
SNAP_AT = 40


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gfx950()


@pytest.fixture(scope="module")
def batches():
    return {k: ZS.Batch(*v) for k, v in BATCHES.items()}


@pytest.fixture(scope="module")
def want(oracle, batches):
    """OracleVec's state after every step of every batch (S[T0] after the twins' set_state), its observation after
    every step, and the state before that set_state; computed once."""
    out = {}
    for name, b in batches.items():
        run = oracle_run(oracle, b.state, b.aux, b.actions, keep_mode=b.keep_mode, every_step_state=True,
                         patch=lambda k, st, b=b: b.twin_patch(st) if k == ZS.T0 else None)
        S = np.concatenate([b.state[None], run["states"]])
        before, S[ZS.T0] = run["patched"].get(ZS.T0, (S[ZS.T0], S[ZS.T0]))
        out[name] = (S, np.stack([s["obs"] for s in run["steps"]]), before)
        for a in out[name]:
            a.setflags(write=False)
    return out


def _run(batch, want, **kw):
    g = GpuVec(batch.n, keep_mode=batch.keep_mode, **kw)
    S, D = ZS.run(g, batch)
    counters = g.counters()
    g.close()
    m = ZS.measure(batch, S, D)
    print(m)
    ZS.check(m, batch)
    same_bits(S, want[0], "state before", batch.family)
    assert counters[N.CNT_OVERFLOW] == 0
    return S, counters


@pytest.fixture(scope="module")
def main_run(batches, want):
    """The main batch through hk_step, uninterrupted: laws, coverage, oracle bits.  The snapshot test compares to it."""
    S, _ = _run(batches["main"], want["main"])
    S.setflags(write=False)
    return S


def test_main_batch_laws_and_oracle_bits(batches, main_run):
    b = batches["main"]
    assert 240 <= b.n <= 253 and b.n % 64 != 0
    fams = [set(b.family[w:w + 64]) for w in range(0, b.n, 64)]
    assert all(len(f) >= 3 for f in fams), fams  # every wave mixes scene families
    assert main_run.shape == (ZS.K + 1, b.n, 18)


@pytest.mark.parametrize("name", ["z1", "z1_keep"])
def test_whole_wave_of_sleepers(batches, want, name):
    """65 arenas of Z1: from step 25 on every lane of the first wave holds a sleeper, the second wave has one lane."""
    _run(batches[name], want[name])


def test_main_batch_large_island_path(batches, want):
    """HK_DIAG_LARGE_ISLANDS: every solve of every lane through the HBM slot file."""
    _, c = _run(batches["main"], want["main"], diag_flags=N.DIAG_LARGE_ISLANDS)
    assert c[N.CNT_LARGE_ISLANDS] > 0


def test_main_batch_rollout_in_two_launches(batches, want):
    """hk_rollout, split at T0 for the twins' set_state.  It returns each step's observation and leaves the final
    state: the observations (positions, the rackets' angles, every velocity but the puck's spin) must be the oracle's
    bit for bit at every step, and so must the raw states at T0 and at the end -- hence the step-by-step run's, whose
    per-step laws the tests above hold."""
    b = batches["main"]
    S, obs, before = want["main"]
    g = GpuVec(b.n, keep_mode=b.keep_mode)
    g.set_state(b.state, b.aux)
    o1 = [r["obs"] for r in g.rollout(b.actions[:ZS.T0])]
    mid = g.get_state()[0]
    patch = b.twin_patch(mid)
    g.set_state(patch[0], None, patch[1])
    mid2 = g.get_state()[0]
    o2 = [r["obs"] for r in g.rollout(b.actions[ZS.T0:])]
    end = g.get_state()[0]
    counters = g.counters()
    g.close()
    same_bits(np.stack(o1 + o2), obs, "observation after", b.family)
    same_bits(np.stack([mid, mid2, end]), np.stack([before, S[ZS.T0], S[-1]]), "state (0: T0, 1: T0 patched, 2: end),",
              b.family)
    assert counters[N.CNT_OVERFLOW] == 0


def test_snapshot_with_sleeping_pucks_continues_bit_for_bit(batches, main_run):
    """Snapshot at step 40, when Z1's, Z2's and Z3's pucks sleep; restore into a fresh context; finish the run."""
    b = batches["main"]
    z1 = b.family == "Z1"
    assert (main_run[SNAP_AT][z1, 15:18] == 0).all() and (main_run[ZS.N_SLEEP - 1][z1, 15:17] != 0).any(-1).all()
    g = GpuVec(b.n, keep_mode=b.keep_mode)
    head, _ = ZS.run(g, b, 0, SNAP_AT)
    snap = g.env.snapshot()
    g.close()
    h = GpuVec(b.n, keep_mode=b.keep_mode)
    h.env.restore(snap)
    tail, _ = ZS.run(h, b, SNAP_AT, ZS.K)
    counters = h.counters()
    h.close()
    same_bits(head, main_run[:SNAP_AT + 1], "state before", b.family, 0, "the uninterrupted run's")
    same_bits(tail, main_run[SNAP_AT:], "state before", b.family, SNAP_AT, "the uninterrupted run's")
    assert counters[N.CNT_OVERFLOW] == 0

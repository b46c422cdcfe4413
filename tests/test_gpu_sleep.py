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
import sleep_scenes as ZS  # noqa: E402

BATCHES = {"main": ("main", False), "z1": ("z1", False), "z1_keep": ("z1", True)}
SNAP_AT = 40


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def _env(batch, **kw):
    from hockey_amd.vec_env import VecHockeyEnv

    return VecHockeyEnv(batch.n, keep_mode=batch.keep_mode, mode=0, device="cuda:0",
                        policies=("external", "external"), auto_reset=False, **kw)


class GpuArenas:
    """VecHockeyEnv behind the three calls sleep_scenes.run makes."""

    def __init__(self, batch, **kw):
        self.env = _env(batch, **kw)
        self.dbg = torch.zeros((batch.n, N.DEBUG_DIM), dtype=torch.float32, device="cuda:0")

    def set_state(self, st, aux, mask):
        c = lambda a: None if a is None else np.array(a)  # noqa: E731  (the batch's arrays are read-only)
        self.env.set_state(c(st), c(aux), c(mask))

    def step_debug(self, actions):
        self.env.step(torch.as_tensor(np.array(actions), device="cuda:0"), debug=self.dbg)
        return self.dbg.cpu().numpy()

    def get_state(self):
        return self.env.get_state()[0].cpu().numpy()


@pytest.fixture(scope="module")
def batches():
    return {k: ZS.Batch(*v) for k, v in BATCHES.items()}


@pytest.fixture(scope="module")
def want(oracle, batches):
    """OracleVec's state after every step of every batch (S[T0] after the twins' set_state), its observation after
    every step, and the state before that set_state; computed once."""
    out = {}
    for name, b in batches.items():
        ov = oracle.OracleVec(b.n, keep_mode=b.keep_mode, policies=("external", "external"), auto_reset=False)
        ov.set_state(b.state, b.aux)
        S, obs, before = [np.array(b.state)], [], None
        for k in range(ZS.K):
            if k == ZS.T0:
                before = S[-1]
                patch = b.twin_patch(S[-1])
                if patch is not None:
                    ov.set_state(patch[0], None, patch[1])
                    S[-1] = ov.get_state()[0]
            obs.append(ov.step(b.actions[k])["obs"])
            S.append(ov.get_state()[0])
        ov.close()
        out[name] = (np.stack(S), np.stack(obs), before)
        for a in out[name]:
            a.setflags(write=False)
    return out


def _same_bits(batch, got, want, what, first=0, ref="the oracle's"):
    same = (got.view(np.uint32) == want.view(np.uint32)).all(-1)
    if not same.all():
        k, i = (int(x[0]) for x in np.nonzero(~same))
        pytest.fail("%s %d, arena %d (family %s): differs from %s\n%s\n%s" % (
            what, k + first, i, batch.family[i], ref, got[k, i], want[k, i]))


def _run(batch, want, **kw):
    g = GpuArenas(batch, **kw)
    S, D = ZS.run(g, batch)
    counters = np.asarray(g.env.counters())
    g.env.close()
    m = ZS.measure(batch, S, D)
    print(m)
    ZS.check(m, batch)
    _same_bits(batch, S, want[0], "state before step")
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
    env = _env(b)
    env.set_state(np.array(b.state), np.array(b.aux))
    acts = torch.as_tensor(np.array(b.actions), device="cuda:0")
    o1 = env.rollout(ZS.T0, acts[:ZS.T0]).obs.cpu().numpy()
    mid = env.get_state()[0].cpu().numpy()
    patch = b.twin_patch(mid)
    env.set_state(patch[0], None, patch[1])
    mid2 = env.get_state()[0].cpu().numpy()
    o2 = env.rollout(ZS.K - ZS.T0, acts[ZS.T0:]).obs.cpu().numpy()
    end = env.get_state()[0].cpu().numpy()
    counters = np.asarray(env.counters())
    env.close()
    _same_bits(b, np.concatenate([o1, o2]), obs, "observation after step")
    _same_bits(b, np.stack([mid, mid2, end]), np.stack([before, S[ZS.T0], S[-1]]), "state (T0, T0 patched, end)")
    assert counters[N.CNT_OVERFLOW] == 0


def test_snapshot_with_sleeping_pucks_continues_bit_for_bit(batches, main_run):
    """Snapshot at step 40, when Z1's, Z2's and Z3's pucks sleep; restore into a fresh context; finish the run."""
    b = batches["main"]
    z1 = b.family == "Z1"
    assert (main_run[SNAP_AT][z1, 15:18] == 0).all() and (main_run[ZS.N_SLEEP - 1][z1, 15:17] != 0).any(-1).all()
    g = GpuArenas(b)
    head, _ = ZS.run(g, b, 0, SNAP_AT)
    snap = g.env.snapshot()
    g.env.close()
    h = GpuArenas(b)
    h.env.restore(snap)
    tail, _ = ZS.run(h, b, SNAP_AT, ZS.K)
    counters = np.asarray(h.env.counters())
    h.env.close()
    _same_bits(b, head, main_run[:SNAP_AT + 1], "state before step", 0, "the uninterrupted run's")
    _same_bits(b, tail, main_run[SNAP_AT:], "state before step", SNAP_AT, "the uninterrupted run's")
    assert counters[N.CNT_OVERFLOW] == 0

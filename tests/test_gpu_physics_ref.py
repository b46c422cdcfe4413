"""The gfx950 step kernel held to the float64 rigid-body laws of tests/physics_ref.py, and to the oracle bit for bit
on the same scenes.

All scenes of a keep mode (tests/physics_scenes.py: free flight, puck-racket, racket-racket, wall bounces, head-on
hits, fast pucks) share ONE context, interleaved by a seeded shuffle: 943 arenas, so the waves mix scene families and
the last wave is partial -- the wave-composition dispatch of hk_velocity.h sees high-speed, set_state-injected contacts
that the lockstep games rarely visit.  The laws and the coverage counts are re-asserted on the GPU's own data, once
more on the HK_DIAG_LARGE_ISLANDS path, and every state is compared with OracleVec's with tolerance zero.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
import physics_scenes as SC  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


class GpuArenas:
    """VecHockeyEnv behind the three calls physics_scenes.run makes."""

    def __init__(self, n, keep_mode, **kw):
        from hockey_amd.vec_env import VecHockeyEnv

        self.env = VecHockeyEnv(n, keep_mode=keep_mode, mode=0, device="cuda:0", policies=("external", "external"),
                                auto_reset=False, **kw)
        self.dbg = torch.zeros((n, N.DEBUG_DIM), dtype=torch.float32, device="cuda:0")

    def set_state(self, st, aux):
        self.env.set_state(np.array(st), np.array(aux))  # the batch's arrays are read-only: torch wants its own

    def step_debug(self, actions):
        self.env.step(torch.as_tensor(np.array(actions), device="cuda:0"), debug=self.dbg)
        return self.dbg.cpu().numpy()

    def get_state(self):
        return self.env.get_state()[0].cpu().numpy()


@pytest.fixture(scope="module")
def batches():
    return {keep: SC.Batch(keep) for keep in (False, True)}


@pytest.fixture(scope="module")
def want(oracle, batches):
    """OracleVec's states after every step of both batches, computed once."""
    out = {}
    for keep, b in batches.items():
        ov = oracle.OracleVec(b.n, keep_mode=keep, policies=("external", "external"), auto_reset=False)
        ov.set_state(b.state, b.aux)
        states = []
        for k in range(SC.K):
            ov.step(b.actions[k])
            states.append(ov.get_state()[0])
        ov.close()
        out[keep] = np.stack(states)
        out[keep].setflags(write=False)
    return out


def _run(batch, want, full, **kw):
    g = GpuArenas(batch.n, batch.keep_mode, **kw)
    S, D = SC.run(g, batch)
    counters = np.asarray(g.env.counters())
    g.env.close()
    m = SC.measure(batch, S, D)
    if full:
        print({k: v for k, v in m.items() if not k.endswith("_log")})
    SC.check(m, full=full)
    same = (S[1:].view(np.uint32) == want.view(np.uint32)).all(-1)
    if not same.all():
        k, i = (int(x[0]) for x in np.nonzero(~same))
        pytest.fail("step %d, arena %d (family %s): state differs from the oracle's\n%s\n%s" % (
            k, i, batch.family[i], S[k + 1, i], want[k, i]))
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

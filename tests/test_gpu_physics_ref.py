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
import physics_scenes as SC  # noqa: E402
import physics_scenes2 as S2  # noqa: E402


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
        self.done = []

    def set_state(self, st, aux):
        self.env.set_state(np.array(st), np.array(aux))  # the batch's arrays are read-only: torch wants its own

    def step_debug(self, actions):
        r = self.env.step(torch.as_tensor(np.array(actions), device="cuda:0"), debug=self.dbg)
        self.done.append(r.done.cpu().numpy().copy())
        return self.dbg.cpu().numpy()

    def get_state(self):
        st, aux = self.env.get_state()
        self._aux = aux.cpu().numpy()
        return st.cpu().numpy()

    def get_aux(self):
        return self._aux  # of the get_state just made


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


# --------------------------------------------------- G, H, P, Q: racket-static contacts, position solver, goal sensors
@pytest.fixture(scope="module")
def batch2():
    return S2.Batch2()


@pytest.fixture(scope="module")
def want2(oracle, batch2):
    """OracleVec's states, aux rows and done flags after every step of the second batch, computed once."""
    b = batch2
    ov = oracle.OracleVec(b.n, keep_mode=False, policies=("external", "external"), auto_reset=False)
    ov.set_state(b.state, b.aux)
    states, auxs, dones = [], [], []
    for k in range(SC.K):
        dones.append(ov.step(b.actions[k])["done"])
        st, aux = ov.get_state()
        states.append(st)
        auxs.append(aux)
    ov.close()
    out = (np.stack(states), np.stack(auxs), np.stack(dones))
    for a in out:
        a.setflags(write=False)
    return out


def _same_bits(batch, got, want, what):
    same = (got.view(np.uint32 if got.dtype.itemsize == 4 else got.dtype) == want.view(
        np.uint32 if want.dtype.itemsize == 4 else want.dtype)).reshape(got.shape[0], got.shape[1], -1).all(-1)
    if not same.all():
        k, i = (int(x[0]) for x in np.nonzero(~same))
        pytest.fail("step %d, arena %d (family %s %s): %s differs from the oracle's\n%s\n%s" % (
            k, i, batch.family[i], batch.kind[i], what, got[k, i], want[k, i]))


def _run2(batch, want, **kw):
    g = GpuArenas(batch.n, False, **kw)
    S, D, A = S2.run(g, batch)
    counters = np.asarray(g.env.counters())
    done = np.stack(g.done)
    g.env.close()
    m = S2.measure(batch, S, D, A)
    print({k: v for k, v in m.items() if not k.endswith("_log")})
    S2.check(m)
    _same_bits(batch, S[1:], want[0], "state")
    _same_bits(batch, A[1:].astype(np.int32), want[1], "aux (has_puck, time, done, winner)")
    _same_bits(batch, done, want[2], "done")
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
    from hockey_amd.vec_env import VecHockeyEnv

    b = batch2
    env = VecHockeyEnv(b.n, keep_mode=False, mode=0, device="cuda:0", policies=("external", "external"),
                       auto_reset=False)
    env.set_state(np.array(b.state), np.array(b.aux))
    r = env.rollout(SC.K, torch.as_tensor(np.array(b.actions), device="cuda:0"))
    done = r.done.cpu().numpy()
    st, aux = (t.cpu().numpy() for t in env.get_state())
    counters = np.asarray(env.counters())
    env.close()
    _same_bits(b, done, want2[2], "done")
    _same_bits(b, st[None], want2[0][-1:], "final state")
    _same_bits(b, aux[None], want2[1][-1:], "final aux")
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

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
from vec_lockstep import first_mismatch  # noqa: E402
import wave_zoo as W  # noqa: E402

FIELDS = ("obs", "obs2", "reward", "reward2", "done", "info", "info2")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


@pytest.fixture(scope="module")
def batch():
    return W.Batch(W.Zoo())


@pytest.fixture(scope="module")
def want(oracle, batch):
    """The oracle's answer for the composed batch, computed once: per-step outputs, final state, counters."""
    ov = oracle.OracleVec(batch.n, policies=("external", "external"), auto_reset=False)
    ov.set_state(batch.state, batch.aux)
    steps = [ov.step(batch.actions[t], with_agent_two=True) for t in range(W.K)]
    out = {"steps": steps, "state": ov.get_state(), "counters": ov.counters()}
    ov.close()
    for s in steps:
        for v in s.values():
            v.setflags(write=False)
    return out


def _env(batch, perm=None, **kw):
    from hockey_amd.vec_env import VecHockeyEnv

    env = VecHockeyEnv(batch.n, keep_mode=True, mode=0, device="cuda:0", policies=("external", "external"),
                       auto_reset=False, **kw)
    sel = slice(None) if perm is None else perm
    env.set_state(batch.state[sel], batch.aux[sel])
    return env


def _np(res, t=None):
    return {f: (getattr(res, f) if t is None else getattr(res, f)[t]).detach().cpu().numpy() for f in FIELDS}


def _check_step(batch, t, got, want_t, how):
    bad = first_mismatch(t, got, want_t, fields=FIELDS)
    if bad:
        ctx = batch.describe(bad["arena"], t) if "arena" in bad else ""
        pytest.fail("%s: %s\n%s" % (how, bad, ctx))


def _check_end(batch, env, want, how, large):
    st, aux = env.get_state()
    st, aux = st.cpu().numpy(), aux.cpu().numpy()
    ost, oaux = want["state"]
    ok = (st.view(np.uint32) == ost.view(np.uint32)).all(1) & (aux == oaux).all(1)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        pytest.fail("%s: final state of arena %d differs\n%s" % (how, i, batch.describe(i, W.K - 1)))
    c = np.asarray(env.counters()).astype(np.int64)
    assert np.array_equal(c[:5], want["counters"][:5]), (how, c[:8], want["counters"][:5])
    assert c[N.CNT_TOI] == batch.toi.sum(), how  # the fixture's TOI labels: every TOI row's event counts
    assert c[N.CNT_OVERFLOW] == 0, how
    large(int(c[N.CNT_LARGE_ISLANDS]))


def _eq(a, b):
    assert a == b, (a, b)


def test_zoo_hk_step_vs_oracle(batch, want):
    """(i) K hk_step launches.  The large-island counter equals what the fixture's labels predict: lanes with more
    island contacts than register slots, TOI mini-islands with more than two."""
    env = _env(batch)
    for t in range(W.K):
        res = env.step(torch.as_tensor(batch.actions[t], device="cuda:0"), with_agent_two=True)
        _check_step(batch, t, _np(res), want["steps"][t], "hk_step")
    _check_end(batch, env, want, "hk_step", lambda c: _eq(c, batch.large))
    env.close()


def test_zoo_hk_rollout_vs_oracle(batch, want):
    """(ii) a fresh context through one hk_rollout(K): step_kernel<true>, a separate instantiation."""
    env = _env(batch)
    ro = env.rollout(W.K, actions=torch.as_tensor(batch.actions, device="cuda:0"), with_agent_two=True)
    for t in range(W.K):
        _check_step(batch, t, _np(ro, t), want["steps"][t], "hk_rollout")
    _check_end(batch, env, want, "hk_rollout", lambda c: _eq(c, batch.large))
    env.close()


def test_zoo_large_island_path_vs_oracle(batch, want):
    """(iii) HK_DIAG_LARGE_ISLANDS: every solve of every lane on the HBM slot file."""
    env = _env(batch, diag_flags=N.DIAG_LARGE_ISLANDS)
    for t in range(W.K):
        res = env.step(torch.as_tensor(batch.actions[t], device="cuda:0"), with_agent_two=True)
        _check_step(batch, t, _np(res), want["steps"][t], "hk_step, large-island path")

    def more(c):
        assert c > batch.large, (c, batch.large)

    _check_end(batch, env, want, "hk_step, large-island path", more)
    env.close()


def test_zoo_lane_permutation_invariance(batch):
    """A lane's result does not depend on its neighbours: with the lanes of every wave permuted (fixed seed), each
    arena's outputs equal those of its unpermuted twin bit for bit.  GPU against GPU, no oracle."""
    rng = np.random.default_rng(64)
    perm = np.concatenate([w0 + rng.permutation(min(64, batch.n - w0)) for w0 in range(0, batch.n, 64)])
    assert np.array_equal(np.sort(perm), np.arange(batch.n)) and (perm // 64 == np.arange(batch.n) // 64).all()
    a, b = _env(batch), _env(batch, perm=perm)
    for t in range(W.K):
        ra = _np(a.step(torch.as_tensor(batch.actions[t], device="cuda:0"), with_agent_two=True))
        rb = _np(b.step(torch.as_tensor(batch.actions[t][perm], device="cuda:0"), with_agent_two=True))
        twin = {f: ra[f][perm] for f in FIELDS}
        bad = first_mismatch(t, rb, twin, fields=FIELDS)
        if bad:
            i = int(perm[bad["arena"]])
            pytest.fail("permuted lane %d (arena %d of the table) differs from its twin: %s\n%s" % (
                bad["arena"], i, bad, batch.describe(i, t)))
    sa, xa = a.get_state()
    sb, xb = b.get_state()
    p = torch.as_tensor(perm, device="cuda:0")
    assert torch.equal(sa[p].view(torch.int32), sb.view(torch.int32)) and torch.equal(xa[p], xb)
    assert np.array_equal(np.asarray(a.counters())[:8], np.asarray(b.counters())[:8])
    a.close()
    b.close()

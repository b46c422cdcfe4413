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

from hockey_amd import _native as N  # noqa: E402
from vec_lockstep import first_mismatch  # noqa: E402
import toi_lean_zoo as Z  # noqa: E402
import wave_zoo as W  # noqa: E402

FIELDS = ("obs", "obs2", "reward", "reward2", "done", "info", "info2")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


@pytest.fixture(scope="module")
def batch():
    return Z.lean_batch()


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


def _env(state, aux):
    from hockey_amd.vec_env import VecHockeyEnv

    env = VecHockeyEnv(state.shape[0], keep_mode=True, mode=0, device="cuda:0", policies=("external", "external"),
                       auto_reset=False)
    env.set_state(state, aux)
    return env


def _np(res, t=None):
    return {f: (getattr(res, f) if t is None else getattr(res, f)[t]).detach().cpu().numpy() for f in FIELDS}


def _sel(x, sel):
    return x if sel is None else x[sel]


def _check_step(batch, t, got, want_t, how, sel=None):
    bad = first_mismatch(t, got, {f: _sel(want_t[f], sel) for f in FIELDS}, fields=FIELDS)
    if bad:
        ctx = ""
        if "arena" in bad:
            ctx = batch.describe(int(bad["arena"] if sel is None else np.arange(batch.n)[sel][bad["arena"]]), t)
        pytest.fail("%s: %s\n%s" % (how, bad, ctx))


def _check_end(batch, env, want, how, sel=None):
    st, aux = env.get_state()
    st, aux = st.cpu().numpy(), aux.cpu().numpy()
    ost, oaux = (_sel(x, sel) for x in want["state"])
    ok = (st.view(np.uint32) == ost.view(np.uint32)).all(1) & (aux == oaux).all(1)
    assert ok.all(), "%s: final state of arena %d differs" % (how, int(np.nonzero(~ok)[0][0]))
    c = np.asarray(env.counters()).astype(np.int64)
    if sel is None or len(st) == batch.n:  # the whole batch: every counter the oracle keeps
        assert np.array_equal(c[:5], want["counters"][:5]), (how, c[:8], want["counters"][:5])
    assert c[N.CNT_TOI] == _sel(batch.toi, sel).sum(), how  # the fixture's TOI labels
    assert c[N.CNT_OVERFLOW] == 0, how
    assert c[N.CNT_LARGE_ISLANDS] == 0, how


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def test_event_waves_hk_step_vs_oracle(batch, want):
    env = _env(batch.state, batch.aux)
    for t in range(W.K):
        res = env.step(_dev(batch.actions[t]), with_agent_two=True)
        _check_step(batch, t, _np(res), want["steps"][t], "hk_step")
    _check_end(batch, env, want, "hk_step")
    env.close()


def test_event_waves_hk_rollout_vs_oracle(batch, want):
    env = _env(batch.state, batch.aux)
    ro = env.rollout(W.K, actions=_dev(batch.actions), with_agent_two=True)
    for t in range(W.K):
        _check_step(batch, t, _np(ro, t), want["steps"][t], "hk_rollout")
    _check_end(batch, env, want, "hk_rollout")
    env.close()


@pytest.mark.parametrize("path", ["hk_step", "hk_rollout"])
def test_event_waves_permuted_vs_oracle(batch, want, path):
    """The lanes of every wave permuted: the event lanes sit elsewhere (and lane 0 is another lane), each arena's
    answer is still the oracle's."""
    perm = batch.permutation()
    env = _env(batch.state[perm], batch.aux[perm])
    how = path + ", lanes permuted"
    if path == "hk_step":
        for t in range(W.K):
            res = env.step(_dev(batch.actions[t][perm]), with_agent_two=True)
            _check_step(batch, t, _np(res), want["steps"][t], how, perm)
    else:
        ro = env.rollout(W.K, actions=_dev(batch.actions[:, perm]), with_agent_two=True)
        for t in range(W.K):
            _check_step(batch, t, _np(ro, t), want["steps"][t], how, perm)
    _check_end(batch, env, want, how, perm)
    env.close()


@pytest.mark.parametrize("path", ["hk_step", "hk_rollout"])
def test_single_event_arena_alone_vs_oracle(batch, want, path):
    """The last wave's event scenario as a one-arena context: lane 0 is the only lane."""
    sel = np.array([batch.single])
    state, aux, actions, toi = batch.one(batch.single)
    assert toi.sum() > 0
    env = _env(state, aux)
    how = path + ", one-arena context"
    if path == "hk_step":
        for t in range(W.K):
            res = env.step(_dev(actions[t]), with_agent_two=True)
            _check_step(batch, t, _np(res), want["steps"][t], how, sel)
    else:
        ro = env.rollout(W.K, actions=_dev(actions), with_agent_two=True)
        for t in range(W.K):
            _check_step(batch, t, _np(ro, t), want["steps"][t], how, sel)
    _check_end(batch, env, want, how, sel)
    env.close()

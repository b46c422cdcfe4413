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
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from hockey_amd import _native as N  # noqa: E402
from vec_lockstep import first_mismatch  # noqa: E402
import wave_list_scenes as L  # noqa: E402

FIELDS = ("obs", "obs2", "reward", "reward2", "done", "info", "info2")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


@pytest.fixture(scope="module")
def batch():
    return L.Batch()


@pytest.fixture(scope="module")
def want(oracle, batch):
    """The oracle's answer, computed once: per-step outputs, final state, counters."""
    ov = oracle.OracleVec(batch.n, policies=("external", "external"), auto_reset=False)
    ov.set_state(batch.state, batch.aux)
    steps = [ov.step(batch.actions[t], with_agent_two=True) for t in range(L.K)]
    out = {"steps": steps, "state": ov.get_state(), "counters": ov.counters()}
    ov.close()
    for s in steps:
        for v in s.values():
            v.setflags(write=False)
    assert out["counters"][N.CNT_TOI] >= 1
    return out


def _env(batch, perm):
    from hockey_amd.vec_env import VecHockeyEnv

    env = VecHockeyEnv(batch.n, keep_mode=True, mode=0, device="cuda:0", policies=("external", "external"),
                       auto_reset=False)
    env.set_state(batch.state[perm], batch.aux[perm])
    return env


def _np(res, t=None):
    return {f: (getattr(res, f) if t is None else getattr(res, f)[t]).detach().cpu().numpy() for f in FIELDS}


def _check_step(batch, perm, t, got, want_t, how):
    bad = first_mismatch(t, got, {f: want_t[f][perm] for f in FIELDS}, fields=FIELDS)
    if bad:
        ctx = batch.describe(int(perm[bad["arena"]]), t) if "arena" in bad else ""
        pytest.fail("%s: %s\n%s" % (how, bad, ctx))


def _check_end(batch, perm, env, want, how):
    st, aux = env.get_state()
    st, aux = st.cpu().numpy(), aux.cpu().numpy()
    ost, oaux = want["state"]
    ok = (st.view(np.uint32) == ost[perm].view(np.uint32)).all(1) & (aux == oaux[perm]).all(1)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        pytest.fail("%s: final state of lane %d differs\n%s" % (how, i, batch.describe(int(perm[i]), L.K - 1)))
    c = np.asarray(env.counters()).astype(np.int64)
    assert np.array_equal(c[:5], want["counters"][:5]), (how, c[:8], want["counters"][:5])
    assert c[N.CNT_OVERFLOW] == 0, how


IDENTITY = np.arange(L.N)


def test_wave_list_hk_step_vs_oracle(batch, want):
    env = _env(batch, IDENTITY)
    for t in range(L.K):
        res = env.step(torch.as_tensor(batch.actions[t], device="cuda:0"), with_agent_two=True)
        _check_step(batch, IDENTITY, t, _np(res), want["steps"][t], "hk_step")
    _check_end(batch, IDENTITY, env, want, "hk_step")
    env.close()


def test_wave_list_hk_rollout_vs_oracle(batch, want):
    env = _env(batch, IDENTITY)
    ro = env.rollout(L.K, actions=torch.as_tensor(batch.actions, device="cuda:0"), with_agent_two=True)
    for t in range(L.K):
        _check_step(batch, IDENTITY, t, _np(ro, t), want["steps"][t], "hk_rollout")
    _check_end(batch, IDENTITY, env, want, "hk_rollout")
    env.close()


def test_wave_list_permuted_lanes_vs_oracle(batch, want):
    """The lanes of each wave permuted (fixed seed): every arena keeps its wave, so both waves still overflow."""
    rng = np.random.default_rng(64)
    perm = np.concatenate([w0 + rng.permutation(min(64, batch.n - w0)) for w0 in range(0, batch.n, 64)])
    assert np.array_equal(np.sort(perm), IDENTITY) and (perm // 64 == IDENTITY // 64).all()
    assert not np.array_equal(perm, IDENTITY)
    env = _env(batch, perm)
    for t in range(L.K):
        res = env.step(torch.as_tensor(batch.actions[t][perm], device="cuda:0"), with_agent_two=True)
        _check_step(batch, perm, t, _np(res), want["steps"][t], "hk_step, permuted lanes")
    _check_end(batch, perm, env, want, "hk_step, permuted lanes")
    env.close()

"""The laws built on the device random draws, held to numpy -- not to the oracle's restatement of them.

Philox4x32-10 itself is pinned to the Random123 known answer (tests/learner_ref.py, tests/test_learner_ref.py).  What
hk_step.h builds on it -- which counter words, which words make which uniform, the placement formulas -- was compared
only between the kernel and the oracle, two restatements by the same hands.  Here the expected values come from
learner_ref.philox4x32_10 and from hockey_amd.placement.placement (pinned to the reference's reset by golden G1),
and every comparison is bit-exact:

  counter = (arena id lo, arena id hi, c2, purpose), key = the context seed
  purpose 3 + 0x100 j  reset placement, c2 = the arena's episode counter; uniforms (x,y), (z,w) of blocks j = 0, 1 and
                       (x,y) of block 2, in the order reset() draws; u = ((a >> 5) 2^26 + (b >> 6)) / 2^53
  purpose 1 + 0x10 p   RANDOM policy of player p, c2 = the step counter: a_k = 2 float32((w_k >> 8) 2^-24) - 1
  purpose 2 + 0x10 p   BasicOpponent phase increment 0.2 u(x,y), c2 = the step counter
  purpose 4 + 0x10 p   BasicOpponent initial phase pi u(x,y), c2 = 0 (p = 2: player 2's weak bot under an override)

Arena ids straddle 2^32 (arena_offset = 2^32 - 100, 200 arenas), so the high id word matters.
"""
import numpy as np
import pytest

from hockey_amd.placement import placement
from hostcheck import HostVec
from learner_ref import philox4x32_10

N_ARENAS, OFFSET, SEED = 200, 2 ** 32 - 100, 0x9E3779B97F4A7C15
RESET, ACTION, PHASE, PHASE0 = 3, 1, 2, 4


def _words(c2, purpose):
    ga = np.arange(N_ARENAS, dtype=np.uint64) + np.uint64(OFFSET)
    ctr = np.stack([ga & np.uint64(0xFFFFFFFF), ga >> np.uint64(32), np.full(N_ARENAS, c2, np.uint64),
                    np.full(N_ARENAS, purpose, np.uint64)], -1)
    assert (ctr[:, 1] == 0).any() and (ctr[:, 1] == 1).any()
    return philox4x32_10(np.uint64(SEED), ctr)


def _u53(a, b):
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) / 2.0 ** 53


class _Stub:
    """The Generator placement() draws from: uniform(lo, hi, 1) = lo + (hi - lo) u_k, numpy's own formula."""

    def __init__(self, us):
        self.us, self.k = us, 0

    def uniform(self, lo, hi, size):
        assert size == 1
        self.k += 1
        return np.array([lo + (hi - lo) * self.us[self.k - 1]])


def expected_reset_state(mode, one_starts, episode):
    """([N,18] state, [N,2] initial puck force) of a device reset."""
    w = [_words(episode, RESET + 0x100 * j) for j in range(3)]
    us = np.stack([_u53(w[0][:, 0], w[0][:, 1]), _u53(w[0][:, 2], w[0][:, 3]), _u53(w[1][:, 0], w[1][:, 1]),
                   _u53(w[1][:, 2], w[1][:, 3]), _u53(w[2][:, 0], w[2][:, 1])], 1)
    st = np.zeros((N_ARENAS, 18), np.float32)
    force = np.zeros((N_ARENAS, 2), np.float32)
    for i in range(N_ARENAS):
        p, _ = placement(mode, bool(one_starts[i]), _Stub(us[i]))
        st[i, 0:2] = (2.0, 4.0)  # player 1 stands at (W / 5, H / 2) in every mode
        st[i, 6:8], st[i, 12:14], force[i] = p[0:2], p[2:4], p[4:6]
    return st, force


def expected_actions(step):
    w = np.concatenate([_words(step, ACTION + 0x10 * p) for p in (0, 1)], 1)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.float32(2.0) * u - np.float32(1.0)


def expected_phase0():
    return np.stack([np.pi * _u53(*_words(0, PHASE0 + 0x10 * p)[:, :2].T) for p in range(3)], 1)


def expected_increment(step):
    return np.stack([0.2 * _u53(*_words(step, PHASE + 0x10 * p)[:, :2].T) for p in range(2)], 1)


# -------------------------------------------------------------------------------------------------- the three contexts
class _Oracle:
    def __init__(self, oracle, mode, policies):
        self.v = oracle.OracleVec(N_ARENAS, mode=mode, auto_reset=True, policies=policies, seed=SEED,
                                  arena_offset=OFFSET)
        self.rows = 2

    def reset(self, one):
        self.v.reset(one_starts=one)

    def state(self):
        return self.v.get_state()[0]

    def set_aux(self, aux):
        self.v.set_state(None, aux)

    def step(self):
        return self.v.step(np.zeros((N_ARENAS, 8), np.float32))["actions"], None

    def phase(self):
        return self.v.phase()


class _Host:
    def __init__(self, oracle, mode, policies):
        self.v = HostVec(N_ARENAS, mode=mode, auto_reset=True, policies=policies, seed=SEED, arena_offset=OFFSET)
        self.rows = 3

    def reset(self, one):
        self.v.reset(one_starts=one)

    def state(self):
        return self.v.get_state()[0]

    def set_aux(self, aux):
        self.v.set_state(None, aux)

    def step(self):
        r = self.v.step(np.zeros((N_ARENAS, 8), np.float32), record_actions=True, debug=True)
        return r.actions, r.debug

    def phase(self):
        return self.v.phase()


class _Gpu:
    def __init__(self, oracle, mode, policies):
        import torch
        from hockey_amd.vec_env import VecHockeyEnv

        assert torch.cuda.is_available(), "GPU tests need the MI355X (gfx950)"
        self.torch = torch
        self.v = VecHockeyEnv(N_ARENAS, mode=mode, device="cuda:0", auto_reset=True, policies=policies, seed=SEED,
                              arena_offset=OFFSET)
        self.dbg = torch.zeros((N_ARENAS, 13), dtype=torch.float32, device="cuda:0")
        self.rows = 3

    def reset(self, one):
        self.v.reset(one_starting=one.astype(bool))

    def state(self):
        return self.v.get_state()[0].cpu().numpy()

    def set_aux(self, aux):
        self.v.set_state(aux=aux)

    def step(self):
        r = self.v.step(self.torch.zeros((N_ARENAS, 8), device="cuda:0"), record_actions=True, debug=self.dbg)
        return r.actions.cpu().numpy(), self.dbg.cpu().numpy()

    def phase(self):
        return self.v.opponent_phase(rows=3).cpu().numpy()


CONTEXTS = [pytest.param(_Oracle, id="oracle"), pytest.param(_Host, id="hostcheck"),
            pytest.param(_Gpu, id="gpu", marks=pytest.mark.gpu)]


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    bad = np.nonzero(got.view(u) != want.view(u))
    assert not len(bad[0]), (bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("make", CONTEXTS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_device_placement(oracle, make, mode):
    """An explicit reset with both one_starts values, then two auto-resets of every arena: episodes 1, 2 and 3 (episode
    0 is the context's own first reset); NORMAL mode toggles the puck side at each auto-reset."""
    env = make(oracle, mode, ("external", "external"))
    one = (np.arange(N_ARENAS) % 2).astype(np.uint8)
    env.reset(one)
    st, force = expected_reset_state(mode, one, 1)
    _same_bits(env.state(), st)
    if mode == 2:
        assert (force != 0).all()
    expired = np.tile(np.array([0, 0, 1000, 0, 0], np.int32), (N_ARENAS, 1))  # time >= max_timesteps: done at this step
    for episode in (2, 3):
        env.set_aux(expired)
        _, dbg = env.step()
        if dbg is not None and episode == 2:  # the ended episode's first step saw the reset's initial shot
            _same_bits(dbg[:, 4:6], force)
        one = 1 - one if mode == 0 else one
        st, force = expected_reset_state(mode, one, episode)
        _same_bits(env.state(), st)


@pytest.mark.parametrize("make", CONTEXTS)
def test_random_policy_actions(oracle, make):
    env = make(oracle, 0, ("random", "random"))
    for step in (0, 1):
        actions, _ = env.step()
        _same_bits(actions, expected_actions(step))


@pytest.mark.parametrize("make", CONTEXTS)
def test_basic_opponent_phases(oracle, make):
    """Initial phases pi u (all three rows where the context exposes them) and one step's advance by 0.2 u."""
    env = make(oracle, 0, ("weak", "strong"))
    ph0 = expected_phase0()
    _same_bits(env.phase(), ph0[:, :env.rows])
    env.step()
    want = ph0.copy()
    want[:, :2] += expected_increment(0)
    _same_bits(env.phase(), want[:, :env.rows])

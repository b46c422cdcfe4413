"""Shared cases of tests/test_arena_copy.py (host build) and tests/test_gpu_arena_copy.py (GPU): the composed zoo
batch with the oracle's uninterrupted run, the interrupted run, the fork case and the lookahead case, each over an
implementation of tests/scene_lockstep.py.  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
import pytest

import wave_zoo as W
from hockey_amd import _native as N
from scene_lockstep import STEP_FIELDS, check_step, oracle_run, run_batch
from vec_lockstep import first_mismatch

N_ARENAS = 101  # one full wave and one of 37 lanes


@pytest.fixture(scope="module")
def scen():
    """101 zoo scenarios whose arena holds a touching island of two or more contacts at steps 1 AND 2 -- across the
    point where the tests interrupt the run -- so the step after the interruption warm-starts from stored impulses."""
    z = W.Zoo()
    nc = z.d["ncont"]
    ids = [i for i in range(z.n) if nc[i, 1] >= 2 and nc[i, 2] >= 2]
    assert len(ids) >= 8, "the fixture holds multi-contact scenarios"
    ids = np.array([ids[k % len(ids)] for k in range(N_ARENAS)])
    return {"state": z.d["state"][ids], "aux": z.d["aux"][ids],
            "actions": np.ascontiguousarray(z.d["actions"][ids].transpose(1, 0, 2))}  # [K, n, 8]


@pytest.fixture(scope="module")
def want(oracle, scen):
    """The oracle's uninterrupted 4 steps of the composed batch, and its final state."""
    return oracle_run(oracle, scen["state"], scen["aux"], scen["actions"])


def state_equal(env, want_state):
    """Per arena: the state words and aux rows equal want_state's."""
    st, aux = env.get_state()
    return (st.view(np.uint32) == want_state[0].view(np.uint32)).all(1) & (aux == want_state[1]).all(1)


def no_bad_index(*envs):
    for e in envs:
        c = e.counters()
        assert c[N.CNT_BAD_INDEX] == 0 and c[N.CNT_OVERFLOW] == 0


def _rows_equal(got, want, rows, want_rows):
    return all((got[f][rows].reshape(len(rows), -1).view(np.uint8)
                == want[f][want_rows].reshape(len(rows), -1).view(np.uint8)).all() for f in STEP_FIELDS)


def interrupted(env, scen, want, path, save, load):
    """env (the scenarios in place): 2 steps in lockstep with the oracle, save(env), every arena reset and stepped,
    load(env, saved), 2 more steps.  Returns per arena whether every output of steps 2..3 and the final state equal
    the oracle's; closes env."""
    for t, got in enumerate(run_batch(env, scen["actions"][:2], path)):
        check_step(t, got, want["steps"][t], path)
    saved = save(env)
    env.reset()  # a device-placement reset, then one step of it: every arena overwritten
    env.step(np.zeros((env.n, 8), np.float32))
    assert not state_equal(env, want["state"]).any()
    load(env, saved)
    ok = np.ones(env.n, bool)
    for t, got in enumerate(run_batch(env, scen["actions"][2:], path), start=2):
        for f in STEP_FIELDS:
            g, w = got[f].reshape(env.n, -1), want["steps"][t][f].reshape(env.n, -1)
            ok &= (g.view(np.uint8) == w.view(np.uint8)).all(1)
    ok &= state_equal(env, want["state"])
    no_bad_index(env)
    env.close()
    return ok


def fork_follows_the_oracle(oracle, env, path, fork):
    """env (128 arenas): arenas 64..127 live another history for 3 steps, then fork(env, src, dst) gives them arenas
    0..63 through a permuted destination list; from there all 128 arenas equal the oracle, whose arenas 64..127 lived
    0..63's history from the reset.  Then one source arena into 37 destinations.  Closes env."""
    params, max_t, actions, other = fork_case()
    ov = oracle.OracleVec(128, policies=("external", "external"), auto_reset=False)
    ov.reset(params=params, max_t=max_t)
    env.reset_params(params, max_t=max_t)
    pre = actions[:3].copy()
    pre[:, 64:] = other
    got = run_batch(env, pre, path)
    touched, first = 0, np.arange(64)
    for t in range(3):
        w = ov.step(actions[t], with_agent_two=True)
        assert _rows_equal(got[t], w, first, first), t
        touched += int((w["info"][:, 2] != 0).sum())
    assert touched > 0, "the case holds player-puck contacts"
    assert not state_equal(env, ov.get_state())[64:].all()
    perm = np.random.default_rng(7).permutation(64)
    fork(env, perm, 64 + perm)
    assert state_equal(env, ov.get_state()).all()
    got = run_batch(env, actions[3:6], path)
    for t in range(3, 6):
        bad = first_mismatch(t, got[t - 3], ov.step(actions[t], with_agent_two=True), fields=STEP_FIELDS)
        assert bad is None, bad
    assert state_equal(env, ov.get_state()).all()
    # K-way replication: arena 5 into 37 destinations, which then take arena 5's action
    dst = np.arange(70, 107)
    fork(env, np.full(37, 5), dst)
    a = np.random.default_rng(8).uniform(-1, 1, (128, 8)).astype(np.float32)
    a[dst] = a[5]
    w = ov.step(a, with_agent_two=True)
    assert _rows_equal(vars(env.step(a, with_agent_two=True)), w, dst, np.full(37, 5))
    five = tuple(x[np.full(128, 5)] for x in ov.get_state())
    assert state_equal(env, five)[dst].all()
    no_bad_index(env)
    env.close()
    ov.close()


def fork_case():
    """128 arenas; 64..127 are given arenas 0..63's reset parameters and actions.  The puck starts overlapping a
    player so contacts (and stored impulses) exist from the first step."""
    rng = np.random.default_rng(1103)
    p = np.zeros((64, 6), np.float32)
    p[:, 0] = rng.uniform(6.5, 8.5, 64)
    p[:, 1] = rng.uniform(2.5, 5.5, 64)
    near1 = rng.random(64) < 0.5  # the puck at player 1 (2, 4) or at player 2
    ang, rad = rng.uniform(0, 2 * np.pi, 64), rng.uniform(0.3, 0.9, 64)
    p[:, 2] = np.where(near1, 2.0, p[:, 0]) + rad * np.cos(ang)
    p[:, 3] = np.where(near1, 4.0, p[:, 1]) + rad * np.sin(ang)
    params = np.concatenate([p, p])
    a = rng.uniform(-1, 1, (6, 64, 8)).astype(np.float32)
    actions = np.concatenate([a, a], axis=1)
    other = rng.uniform(-1, 1, (3, 64, 8)).astype(np.float32)  # the host build's arenas 64..127 before the fork
    return params, np.full(128, 250, np.int32), actions, other


def lookahead_case(oracle, M=5, K=8, H=6, n_live=8, hist=2):
    """A live env of n_live arenas (player 2 a fused weak bot with given phase increments) `hist` steps after its
    reset, M of its arenas as lookahead sources with K branches of H steps, and the oracle's answer: a batch of
    M * K arenas whose histories duplicate the sources' (oracle arena m * K + k = branch k of source m).
    Source 1 (live arena 3) has the puck behind player 1, flying into player 1's goal: every branch of it ends
    inside the horizon with steps to spare."""
    rng = np.random.default_rng(99)
    c = {"M": M, "K": K, "H": H, "n_live": n_live, "hist": hist, "policies": ("external", "weak")}
    params = np.zeros((n_live, 6), np.float32)
    params[:, 0], params[:, 1] = rng.uniform(6.5, 8.5, n_live), rng.uniform(2.5, 5.5, n_live)
    params[:, 2], params[:, 3] = rng.uniform(3.0, 7.0, n_live), rng.uniform(2.0, 6.0, n_live)
    params[3] = [8.0, 4.0, 1.2, 4.0, -40.0, 0.0]
    c["params"], c["max_t"] = params, np.full(n_live, 250, np.int32)
    c["phase"] = rng.uniform(0, np.pi, (n_live, 2))
    c["h_act"] = rng.uniform(-1, 1, (hist, n_live, 8)).astype(np.float32)
    c["h_act"][:, 3] = 0.0
    c["h_inc"] = rng.uniform(0, 0.2, (hist, n_live, 2))
    c["src"] = np.array([6, 3, 0, 7, 2])[:M]
    c["acts"] = rng.uniform(-1, 1, (H, M, K, 8)).astype(np.float32)
    c["incs"] = rng.uniform(0, 0.2, (H, M, K, 2))
    dup = np.repeat(c["src"], K)
    ov = oracle.OracleVec(M * K, policies=c["policies"], auto_reset=False)
    ov.reset(params=params[dup], max_t=c["max_t"][dup])
    ov.phase(c["phase"][dup])
    for t in range(hist):
        ov.step(c["h_act"][t][dup], c["h_inc"][t][dup])
    c["rewards"], c["dones"] = np.zeros((H, M * K), np.float32), np.zeros((H, M * K), np.uint8)
    for t in range(H):
        w = ov.step(c["acts"][t].reshape(M * K, 8), c["incs"][t].reshape(M * K, 2))
        c["rewards"][t], c["dones"][t] = w["reward"], w["done"]
    c["winner"] = ov.get_state()[1][:, 4].copy()
    ov.close()
    return c

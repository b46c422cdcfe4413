"""Shared cases of tests/test_arena_copy.py (host build) and tests/test_gpu_arena_copy.py (GPU): the composed zoo
batch with the oracle's uninterrupted run, the fork case and the lookahead case.  TEST INFRASTRUCTURE ONLY.
"""
import numpy as np
import pytest

import wave_zoo as W

FIELDS = ("obs", "obs2", "reward", "reward2", "done", "info", "info2")
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
    ov = oracle.OracleVec(N_ARENAS, policies=("external", "external"), auto_reset=False)
    ov.set_state(scen["state"], scen["aux"])
    steps = [ov.step(scen["actions"][t], with_agent_two=True) for t in range(W.K)]
    out = {"steps": steps, "state": ov.get_state()}
    ov.close()
    for s in steps:
        for v in s.values():
            v.setflags(write=False)
    return out


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

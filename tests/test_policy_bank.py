"""The policy bank (hockey_amd/policy_bank.py, hkl_act of include/hockey_learner.h) and what is built on it -- per-arena
self-play (OpponentMix(sampling="arena")) and the cross-play tournament's host functions -- on the CPU: the binding,
the torch reference backend, the draws' statistics and the outcome bookkeeping.  tests/test_gpu_policy_bank.py holds
the kernel itself to a float64 forward."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from hockey_amd import learner_hip as LH
from hockey_amd.evaluate import Actor, tournament_fold, tournament_pairs
from hockey_amd.opponents import OpponentMix, SelfPlayPool
from hockey_amd.policy_bank import PolicyBank


def _actor(seed):
    torch.manual_seed(seed)
    return Actor().eval()


def test_library_exports_hkl_act_and_the_struct_sizes_agree():
    """The cross-compiled libhockey_learner.so exports hkl_act, and hkl_act_io as ctypes lays it out has the size
    the library compiled (hkl_act_io_size; dlopen needs no GPU)."""
    assert os.path.exists(LH.LIB_PATH), "build() compiles libhockey_learner.so"
    L = ctypes.CDLL(LH.LIB_PATH)
    assert hasattr(L, "hkl_act")
    assert L.hkl_act_io_size() == ctypes.sizeof(LH.ActIO)
    assert LH.ACT_PARAM_FLOATS == sum(p.numel() for p in Actor().parameters())
    # bad scalars are refused on the host, before anything touches a device
    L.hkl_act.argtypes = [ctypes.POINTER(LH.ActIO), ctypes.c_void_p]
    ok = dict(n_policies=3, n_rows=5, params=8, packs=8, obs=8, obs_ld=18, out=8, out_ld=8, out_col=4)
    for bad in (dict(n_policies=0), dict(n_policies=65), dict(n_rows=-1), dict(obs_ld=17), dict(out_ld=7),
                dict(out_col=-1), dict(policy=8)):  # the last: a policy without scratch
        io = LH.ActIO(**{**ok, **bad})
        assert L.hkl_act(ctypes.byref(io), None) == 1, bad
    assert L.hkl_act(ctypes.byref(LH.ActIO(**{**ok, "n_rows": 0})), None) == 0  # nothing to do, nothing launched


def test_torch_backend_equals_per_slot_actor_forward():
    """PolicyBank.act(backend="torch") on the CPU: every row carries its slot's Actor forward, rows at -1 and the
    other columns of ``out`` keep their contents; policy=None runs slot 0; policy_fn(slot) that slot."""
    actors = [_actor(s) for s in range(3)]
    bank = PolicyBank(5, "cpu")
    assert [bank.add(a) for a in actors[:2]] == [0, 1]
    bank.free(0)
    assert bank.add(actors[0]) == 0 and bank.replace(3, actors[2]) == 3 and bank.slots() == [0, 1, 3]
    g = torch.Generator().manual_seed(1)
    n = 300
    obs = torch.randn(n, 18, generator=g) * 2
    policy = torch.tensor([-1, 0, 1, 3], dtype=torch.int32)[torch.randint(0, 4, (n,), generator=g)]
    out = torch.full((n, 8), 7.5)
    ret = bank.act(obs, policy, out=out, out_col=4, backend="torch")
    assert ret is out and torch.all(out[:, :4] == 7.5)
    with torch.no_grad():
        for slot, a in ((0, actors[0]), (1, actors[1]), (3, actors[2])):
            rows = policy == slot
            assert rows.any() and torch.equal(out[rows, 4:], a(obs)[rows])
            assert torch.equal(bank.policy_fn(slot, backend="torch")(obs), a(obs))
        assert torch.all(out[policy == -1] == 7.5) and (policy == -1).any()
        assert torch.equal(bank.act(obs, backend="torch"), actors[0](obs))
    with pytest.raises(ValueError):
        bank.replace(2, torch.nn.Linear(18, 4))
    with pytest.raises(ValueError):
        PolicyBank(65, "cpu")


def _mix3(n, p_self, scores):
    mix = OpponentMix(n, [(1.0, 0.3, 0.7 - p_self, p_self)], pool_size=4, device="cpu", seed=9, sampling="arena")
    for s in range(3):
        mix.pool.add_snapshot(_actor(10 + s))
    mix.pool.scores[:] = scores
    return mix


def test_arena_sampling_draws_score_weighted_snapshots_and_charges_them():
    """OpponentMix(sampling="arena") at 20 000 arenas, p_self = 0.5, three snapshots of scores (1, 2, 5): each
    snapshot's share of the self-play arenas lies within 4 binomial standard deviations of score / sum, the bots
    split the rest as under "step", the actions are each arena's own snapshot's, and outcomes fed through
    register_outcomes / end_round land on the snapshot the arena faced, as update_difficulty applied by hand."""
    from hockey_amd import _native as N

    n, scores = 20000, [1.0, 2.0, 5.0]
    mix = _mix3(n, 0.5, scores)
    g = torch.Generator().manual_seed(2)
    obs2 = torch.randn(n, 18, generator=g)
    act8 = torch.full((n, 8), -3.0)
    p2, out, policy = mix.select(obs2, out=act8)
    assert out is act8 and policy.dtype == torch.int32
    sp = p2 == N.POLICY_EXTERNAL
    m = int(sp.sum())
    assert abs(m - 0.5 * n) < 4 * math.sqrt(n * 0.25)
    assert torch.equal(policy >= 0, sp) and torch.all(policy[~sp] == -1)
    slots = mix.pool.slots
    assert sorted(slots) == [0, 1, 2]
    for i, s in enumerate(scores):
        p = s / sum(scores)
        k = int((policy == slots[i]).sum())
        assert abs(k - m * p) < 4 * math.sqrt(m * p * (1 - p)), (i, k, m)
    # the bots among the rest: strong with probability p_strong, as the per-step mode draws them
    rest = n - m
    strong = int((p2 == N.POLICY_BASIC_STRONG).sum())
    assert strong + int((p2 == N.POLICY_BASIC_WEAK).sum()) == rest
    assert abs(strong - rest * 0.3) < 4 * math.sqrt(rest * 0.3 * 0.7)
    # actions: each self-play arena's own snapshot; every other float of the buffer untouched
    assert torch.all(act8[:, :4] == -3.0) and torch.all(act8[~sp, 4:] == -3.0)
    with torch.no_grad():
        for i in range(3):
            rows = policy == slots[i]
            assert torch.equal(act8[rows, 4:], mix.pool.pool[i](obs2)[rows])
    # outcomes: two steps; a done self-play arena is an agent win when its reward is positive
    faced = torch.stack([(policy == slots[i]) for i in range(3)])
    want = list(scores)
    hand = SelfPlayPool(pool_size=4)
    hand.pool, hand.scores = [None] * 3, want
    counts = np.zeros(3, np.int64)
    for step in range(2):
        if step:
            p2, _, policy = mix.select(obs2, out=act8)
            sp = p2 == N.POLICY_EXTERNAL
            faced = torch.stack([(policy == slots[i]) for i in range(3)])
        done = (torch.rand(n, generator=g) < 0.004 * (1 + step)).to(torch.uint8)
        reward = torch.randn(n, generator=g)
        mix.register_outcomes(done, reward)
        for i in range(3):
            d = (done != 0) & faced[i]
            w = int((d & (reward > 0)).sum())
            hand.update_difficulty(i, w, int(d.sum()) - w)
            counts[i] += int(faced[i].sum())
    stats = mix.end_round()
    assert mix.pool.scores == hand.scores and mix.pool.scores != scores
    assert stats["snapshots"] == counts.tolist() and sum(stats["snapshots"]) == stats["self_play"]


def test_pool_mirrors_snapshots_into_bank_slots():
    """SelfPlayPool with a bank: snapshot i lives in bank slot slots[i]; dropping the oldest frees its slot, which
    the next snapshot takes."""
    mix = OpponentMix(8, "stage3", pool_size=2, device="cpu", sampling="arena")
    assert mix.bank.capacity == 3
    for s in range(4):
        mix.pool.add_snapshot(_actor(s))
        assert len(mix.pool) == len(mix.pool.slots) == min(s + 1, 2) == len(mix.bank)
    assert mix.pool.slots == [2, 0]  # slots 0 and 1 were dropped in turn; 0 was free again for the 4th
    for i, slot in enumerate(mix.pool.slots):
        for k, v in mix.pool.pool[i].state_dict().items():
            assert torch.equal(mix.bank.state_dict(slot)[k], v)
    with pytest.raises(ValueError):
        OpponentMix(8, "stage3", device="cpu", sampling="game")


def test_step_sampling_is_the_default_and_keeps_its_stream():
    """sampling="step" is the default: no bank, the three-tuple of before, and the same draws as a mix built without
    the argument."""
    a, b = (OpponentMix(64, "stage3", device="cpu", seed=4, **kw) for kw in ({}, {"sampling": "step"}))
    assert a.bank is None and a.sampling == "step"
    for m in (a, b):
        m.update_schedule(0.9)
        m.pool.add_snapshot(_actor(0))
    obs2 = torch.randn(64, 18)
    for _ in range(3):
        (pa, aa, ia), (pb, ab, ib) = a.select(obs2), b.select(obs2)
        assert torch.equal(pa, pb) and torch.equal(aa, ab) and ia == ib == 0 and aa.shape == (64, 4)
    assert set(a.end_round()) == {"strong", "weak", "self_play"}


def test_tournament_pairing_table_and_fold():
    """Every ordered pair and bot column appears exactly ``games`` times, game indices 0..games-1 each; a hand-made
    winner vector folds to the expected matrices."""
    k, games = 3, 4
    p1, p2, g = tournament_pairs(k, games, include_bots=True)
    assert len(p1) == k * (k + 2) * games
    seen = {}
    for a, (i, j, gg) in enumerate(zip(p1.tolist(), p2.tolist(), g.tolist())):
        seen.setdefault((i, j), []).append(gg)
    assert set(seen) == {(i, j) for i in range(k) for j in (0, 1, 2, -1, -2)}
    assert all(v == list(range(games)) for v in seen.values())
    q1, q2, _ = tournament_pairs(k, games, include_bots=False)
    assert len(q1) == k * k * games and q2.min() == 0
    # actor 0 wins everything, actor 1 draws everything, actor 2: against column j, wins the first j games and
    # loses the rest (columns 3 / 4 = weak / strong bot)
    col = np.where(p2 >= 0, p2, k - 1 - p2)
    winner = np.where(p1 == 0, 1, np.where(p1 == 1, 0, np.where(g < col, 1, -1)))
    length = 10 * (p1 + 1) + col
    out = tournament_fold(winner, length, k, games)
    frac = np.arange(k + 2) / games
    np.testing.assert_array_equal(out["win"], np.stack([np.ones(5), np.zeros(5), frac]))
    np.testing.assert_array_equal(out["draw"], np.stack([np.zeros(5), np.ones(5), np.zeros(5)]))
    np.testing.assert_array_equal(out["loss"], np.stack([np.zeros(5), np.zeros(5), 1 - frac]))
    np.testing.assert_array_equal(out["score"], out["win"] + 0.5 * out["draw"])
    np.testing.assert_array_equal(out["mean_length"], 10.0 * np.arange(1, 4)[:, None] + np.arange(5)[None, :])
    np.testing.assert_array_equal(out["win"] + out["draw"] + out["loss"], np.ones((3, 5)))


def test_train_round_with_per_arena_self_play_on_host_build():
    """One train() round on the kernel source's host build with self_play_sampling="arena" and a pool seeded with
    two snapshots: self-play arenas read the bank's actions, and the round reports the arena-steps per snapshot."""
    from hostcheck import HostTorchEnv

    from hockey_amd.td3 import TD3Config, train

    n, steps = 8, 30
    env = HostTorchEnv(n, policies=("external", "external"))
    mix = OpponentMix(n, [(1.0, 0.25, 0.25, 0.5)], self_play_interval=10 ** 9, pool_size=4, device="cpu", seed=3,
                      sampling="arena")
    for s in range(2):
        mix.pool.add_snapshot(_actor(20 + s))
    seen = []
    cfg = TD3Config(max_steps=steps, start_steps=10 ** 9, batch_size=32)
    agent, st = train(n_arenas=n, rounds=1, cfg=cfg, device="cpu", seed=3, env=env, graphs=False, updates_per_round=0,
                      self_play_sampling="arena", mix=mix,
                      on_step=lambda o, a, r, o2, d, res: seen.append(res.actions.clone()))
    o = st["opponents"][0]
    assert o["strong"] + o["weak"] + o["self_play"] == steps * n and len(seen) == steps
    assert len(o["snapshots"]) == 2 and sum(o["snapshots"]) == o["self_play"] > 0 and min(o["snapshots"]) > 0
    assert all(torch.isfinite(a).all() and a.abs().max() <= 1 for a in seen)
    with pytest.raises(ValueError):
        train(n_arenas=n, rounds=0, cfg=cfg, device="cpu", env=env, mix=mix, self_play_sampling="step")

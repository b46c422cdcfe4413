"""Marker actors and the isolation run shared by tests/test_population_selfplay.py (CPU, torch backend) and
tests/test_gpu_population_selfplay.py (hip backend).

A marker actor has fc3.weight = 0 and fc3.bias = atanh(c): its four actions are c whatever it observes, so an action
names the (member, snapshot) that produced it."""
import math

import torch

from hockey_amd import _native as N
from hockey_amd.evaluate import Actor
from hockey_amd.opponents import PopulationOpponentMix
from hockey_amd.td3 import TD3Config

SENTINEL = -7.5
TABLE = [(1.0, 0.25, 0.25, 0.5)]  # one curriculum row: P(strong), P(weak), P(self-play) = 0.5


def marker(member, snapshot):
    return 0.1 * (member + 1) + 0.005 * (snapshot + 1)  # up to 19 snapshots stay inside the member's tenth


def marker_actor(c, device="cpu"):
    a = Actor()
    with torch.no_grad():
        a.fc3.weight.zero_()
        a.fc3.bias.fill_(math.atanh(c))
    return a.to(device)


def make_mix(S, n, device, sampling, backend, snapshots, no_self_play=(), seed=0, **cfg_kw):
    """A PopulationOpponentMix of S members x n arenas; member j (not in ``no_self_play``) is pre-seeded with
    ``snapshots[j]`` marker snapshots.  cfg_kw: per-member lists of TD3Config fields."""
    cfgs = []
    for j in range(S):
        kw = {k: v[j] for k, v in cfg_kw.items()}
        cfgs.append(TD3Config(use_self_play=j not in no_self_play, curriculum_name="stage3", **kw))
    mix = PopulationOpponentMix(cfgs, [seed + 10 * j for j in range(S)], n, device, sampling, backend=backend,
                                curriculum=TABLE)
    for j in range(S):
        for i in range(snapshots.get(j, 0)):
            mix.snapshot([j], [marker_actor(marker(j, i), device)])
    return mix


def isolation_run(mix, calls, seed=0):
    """``calls`` select() calls on random observations.  Asserts per call: a self-play arena's actions are a marker
    of a snapshot in its own member's pool, and the one its returned bank slot names; a member without a pool never
    gets POLICY_EXTERNAL; every other float of the action buffer keeps the sentinel.  Returns (the recount per member
    from the returned policy2 / policy tensors, end_round()'s result)."""
    S, n, dev = mix.S, mix.n_per, mix.device
    g = torch.Generator().manual_seed(seed)
    member_of = torch.arange(S * n) // n
    recount = [{"strong": 0, "weak": 0, "self_play": 0, "snapshots": [0] * len(p) if p is not None else []}
               for p in mix.pools]
    for _ in range(calls):
        obs2 = (torch.rand((S * n, 18), generator=g) * 2 - 1).to(dev)
        act8 = torch.full((S * n, 8), SENTINEL, device=dev)
        p2, out, policy = mix.select(obs2, act8)
        assert out is act8
        p2, policy, a = p2.cpu(), policy.cpu(), act8.cpu()
        sp = p2 == N.POLICY_EXTERNAL
        assert torch.all(a[:, :4] == SENTINEL) and torch.all(a[~sp][:, 4:] == SENTINEL)
        assert torch.all(policy[~sp] == -1)
        for i in range(S * n):
            j = int(member_of[i])
            key = {N.POLICY_BASIC_STRONG: "strong", N.POLICY_BASIC_WEAK: "weak", N.POLICY_EXTERNAL: "self_play"}
            recount[j][key[int(p2[i])]] += 1
            if not sp[i]:
                continue
            pool = mix.pools[j]
            assert pool is not None and len(pool) > 0, (i, j)
            slot = int(policy[i])
            assert j * mix.stride <= slot < (j + 1) * mix.stride and slot in pool.slots, (i, j, slot)
            idx = pool.slots.index(slot)
            want = float(torch.tanh(pool.pool[idx].fc3.bias[0]))  # the marker of that snapshot
            assert torch.all((a[i, 4:] - want).abs() < 1e-5), (i, j, idx, a[i, 4:], want)
            # ... which is one of member j's own markers and nobody else's
            assert 0.1 * (j + 1) + 0.0025 < want < 0.1 * (j + 1) + 0.0975, (i, j, want)
            recount[j]["snapshots"][idx] += 1
    return recount, mix.end_round()

"""Population self-play on the CPU: hockey_amd.opponents.PopulationOpponentMix on the PolicyBank's torch backend,
train_population(self_play=...) on the kernel source's host build, and hkl_act_wide's host-side argument checks."""
import ctypes
import math

import pytest
import torch

import selfplay_cases as C
from hockey_amd import _native as N
from hockey_amd.opponents import SelfPlayPool
from hockey_amd.population import train_population
from hockey_amd.td3 import TD3Config


def _mix(sampling="arena", seed=0, **kw):
    # S = 3 members x 8 arenas; member 1 does not use self-play, members 0 and 2 hold 2 and 3 marker snapshots
    return C.make_mix(3, 8, "cpu", sampling, "torch", {0: 2, 2: 3}, no_self_play=(1,), seed=seed, **kw)


@pytest.mark.parametrize("sampling", ["arena", "step"])
def test_self_play_arenas_face_their_own_members_snapshots(sampling):
    mix = _mix(sampling)
    assert mix.bank.capacity == 3 * 13 and mix.pool_sizes() == [2, 0, 3]
    recount, got = C.isolation_run(mix, 200)
    assert got == recount
    assert recount[1]["self_play"] == 0 and recount[1]["snapshots"] == []
    assert recount[0]["self_play"] > 0 and recount[2]["self_play"] > 0
    assert all(sum(r["snapshots"]) == r["self_play"] for r in recount)
    assert all(r["strong"] + r["weak"] + r["self_play"] == 200 * 8 for r in recount)


def test_a_member_with_an_empty_pool_falls_through_to_the_bots():
    mix = C.make_mix(2, 8, "cpu", "arena", "torch", {1: 1})  # member 0 uses self-play, but holds no snapshot yet
    recount, got = C.isolation_run(mix, 50)
    assert got == recount and recount[0]["self_play"] == 0 and recount[1]["self_play"] > 0


@pytest.mark.parametrize("sampling", ["arena", "step"])
def test_snapshots_are_drawn_by_their_members_scores(sampling):
    """Scores [1, 3] and [2, 2, 4]: each snapshot's share of its member's draws lies within 5 binomial standard
    deviations, sqrt(n p (1 - p)) at the counted n draws, of its score share.  "arena": one draw per self-play
    arena-step; "step": one per member and step (counted on the steps where the member has a self-play arena)."""
    mix = _mix(sampling, seed=3)
    mix.pools[0].scores[:] = [1.0, 3.0]
    mix.pools[2].scores[:] = [2.0, 2.0, 4.0]
    g = torch.Generator().manual_seed(1)
    counts = {0: [0, 0], 2: [0, 0, 0]}
    for _ in range(400):
        _, _, policy = mix.select(torch.rand((24, 18), generator=g))
        for j in (0, 2):
            rows = policy[8 * j:8 * j + 8]
            rows = rows[rows >= 0].tolist()
            for slot in (rows if sampling == "arena" else rows[:1]):
                counts[j][mix.pools[j].slots.index(slot)] += 1
            assert sampling == "arena" or len(set(rows)) <= 1
    for j, scores in ((0, [1.0, 3.0]), (2, [2.0, 2.0, 4.0])):
        n = sum(counts[j])
        assert n > 300
        for c, s in zip(counts[j], scores):
            p = s / sum(scores)
            print(sampling, j, c, n, p, abs(c - n * p) / math.sqrt(n * p * (1 - p)))
            assert abs(c - n * p) <= 5.0 * math.sqrt(n * p * (1 - p)), (j, counts[j])


def test_outcomes_charge_the_snapshot_each_arena_faced():
    """Hand-made done / reward tensors over 12 steps: the scores equal SelfPlayPool.update_difficulty applied by hand
    to the (member, snapshot) each done self-play arena faced, step by step, and both clips (0.1 and 10) are met."""
    mix = _mix("arena", seed=5)
    start = {0: [9.0, 9.0], 2: [0.104, 0.104, 0.104]}  # one loss from the upper clip, one win from the lower
    ref = {}
    for j, s in start.items():
        mix.pools[j].scores[:] = s
        ref[j] = SelfPlayPool()
        ref[j].scores = list(s)
    g = torch.Generator().manual_seed(2)
    charged, clipped = set(), set()
    for t in range(12):
        p2, _, policy = mix.select(torch.rand((24, 18), generator=g))
        done = (torch.arange(24) + t) % 3 != 0  # two thirds of the arenas end an episode at this step
        reward = torch.where((torch.arange(24) + t) % 2 == 0, 1.0, -1.0) * ((torch.arange(24) % 5) != 0)  # win / loss / 0
        mix.register_outcomes(done.to(torch.uint8), reward)
        tally = {}
        for i in range(24):
            if p2[i] == N.POLICY_EXTERNAL and done[i]:
                j = i // 8
                key = (j, mix.pools[j].slots.index(int(policy[i])))
                w, o = tally.get(key, (0, 0))
                tally[key] = (w + 1, o) if reward[i] > 0 else (w, o + 1)
        for (j, idx), (w, o) in tally.items():
            ref[j].update_difficulty(idx, w, o)
            charged.add((j, idx))
            clipped.add(ref[j].scores[idx])
    mix.end_round()
    for j in (0, 2):
        assert mix.pools[j].scores == ref[j].scores, j
    assert mix.pools[0].scores != start[0] and mix.pools[2].scores != start[2] and len(charged) == 5
    assert 10.0 in clipped and 0.1 in clipped  # both clips were met on the way
    # a second round without outcomes leaves the scores alone
    mix.select(torch.rand((24, 18), generator=g))
    mix.end_round()
    assert all(mix.pools[j].scores == ref[j].scores for j in (0, 2))


def test_snapshots_follow_each_members_interval_and_stay_in_its_slots():
    """Intervals 16 (member 0, pool of 2) and 24 (member 2, pool of 3) at 8 episodes per round: the first snapshots
    appear after rounds 2 and 3; at the pool size the oldest leaves and its slot is the next one used; a snapshot of
    one member leaves every other member's slots byte-unchanged."""
    mix = C.make_mix(3, 8, "cpu", "arena", "torch", {}, no_self_play=(1,), self_play_interval=[16, 16, 24],
                     self_play_pool_size=[2, 2, 3])
    assert mix.pmax == 3 and mix.stride == 4 and mix.bank.capacity == 12
    sizes, slots0, faced = [], [], []
    for rnd in range(1, 10):
        actors = [C.marker_actor(C.marker(j, rnd - 1)) for j in range(3)]  # this round's weights
        before = mix.bank.params.clone()
        mix.select(torch.zeros((24, 18)))
        out = mix.end_round(actors, 8)
        faced.append([len(o["snapshots"]) for o in out])
        sizes.append(mix.pool_sizes())
        slots0.append(list(mix.pools[0].slots))
        took0, took2 = rnd % 2 == 0, rnd % 3 == 0
        changed = (mix.bank.params != before).any(1).view(3, 4).any(1).tolist()
        assert changed == [took0, False, took2], rnd
        if took0:  # the newest snapshot holds this round's weights, in the bank too
            sd = mix.bank.state_dict(mix.pools[0].slots[-1])
            assert torch.allclose(torch.tanh(sd["fc3.bias"]), torch.full((4,), C.marker(0, rnd - 1)), atol=1e-6)
            assert torch.all(sd["fc3.weight"] == 0)
    assert [s[0] for s in sizes] == [0, 1, 1, 2, 2, 2, 2, 2, 2]
    assert [s[1] for s in sizes] == [0] * 9
    assert [s[2] for s in sizes] == [0, 0, 1, 1, 1, 2, 2, 2, 3]
    # member 0: slots 0 and 1 fill, the third snapshot (round 6) goes to slot 2 and frees 0, which round 8 reuses
    assert slots0[1] == [0] and slots0[3] == [0, 1] and slots0[5] == [1, 2] and slots0[7] == [2, 0]
    assert all(4 * 2 <= k < 4 * 3 for k in mix.pools[2].slots) and len(mix.bank) == 5
    # "snapshots" lists the pool as it stood during the round
    assert faced[0] == [0, 0, 0] and faced[2] == [1, 0, 0] and faced[8] == [2, 0, 2]


def _members():
    kw = dict(batch_size=32, use_self_play=True, curriculum_name="stage3", max_steps=40, start_steps=50,
              self_play_interval=4, self_play_pool_size=3)
    return [(TD3Config(noise_mode="gaussian", **kw), 3), (TD3Config(noise_mode="ornstein-uhlenbeck", lr_q=1e-3, **kw), 11)]


@pytest.mark.parametrize("sampling", ["arena", "step"])
def test_train_population_with_self_play_on_host_build(sampling):
    from hostcheck import HostTorchEnv

    S, n = 2, 4
    env = HostTorchEnv(S * n, policies=("external", "external"))
    agents, st = train_population(_members(), n_arenas=n, rounds=3, device="cpu", env=env, updates_per_round=2,
                                  graphs=False, self_play=sampling)
    for j, ag in enumerate(agents):
        assert st[j]["pool_size"] == [1, 2, 3]  # interval 4 = one round's episodes
        assert len(st[j]["opponents"]) == 3 and all("snapshots" in o for o in st[j]["opponents"])
        assert [len(o["snapshots"]) for o in st[j]["opponents"]] == [0, 1, 2]
        assert all(o["strong"] + o["weak"] + o["self_play"] == n * 40 for o in st[j]["opponents"])
        assert st[j]["opponents"][0]["self_play"] == 0  # the pool was empty (and stage3 starts without self-play)
        assert all(torch.isfinite(p).all() for p in ag.actor.parameters())
        assert st[j]["updates"] == 6
    # stage3 reaches a self-play share of 0.1 in round 2 and 0.3 in round 3: 320 arena-steps with a pool
    assert sum(o["self_play"] for s in st for o in s["opponents"]) > 0
    assert st[0]["opponents"] != st[1]["opponents"]  # each member's own counts


def test_train_population_still_refuses_self_play_by_default():
    with pytest.raises(ValueError, match="self-play") as e:
        train_population(_members(), n_arenas=4, rounds=1, device="cpu")
    assert "self_play" in str(e.value)
    with pytest.raises(ValueError, match="self_play"):
        train_population(_members(), n_arenas=4, rounds=1, device="cpu", self_play="round")


def test_members_with_and_without_self_play_share_a_population():
    from hostcheck import HostTorchEnv

    ms = _members()
    ms[1] = (TD3Config(batch_size=32, use_self_play=False, curriculum_name="stage3", max_steps=40, start_steps=50), 11)
    env = HostTorchEnv(8, policies=("external", "external"))
    _, st = train_population(ms, n_arenas=4, rounds=3, device="cpu", env=env, updates_per_round=0, graphs=False,
                             self_play="arena")
    assert st[0]["pool_size"] == [1, 2, 3] and st[1]["pool_size"] == [0, 0, 0]
    assert all(o["self_play"] == 0 and o["snapshots"] == [] for o in st[1]["opponents"])


def test_policy_bank_replace_many_and_wide_capacities_on_the_torch_backend():
    from hockey_amd.learner_hip import ACT_WIDE_MAX_POLICIES
    from hockey_amd.policy_bank import PolicyBank

    assert ACT_WIDE_MAX_POLICIES == 4096
    bank = PolicyBank(130, "cpu", wide=True)
    bank.replace_many([0, 64, 129], [C.marker_actor(c) for c in (0.2, 0.4, 0.6)])
    assert bank.slots() == [0, 64, 129]
    policy = torch.tensor([129, -1, 64, 0, 5], dtype=torch.int32)  # 5: a free slot, untouched on this backend
    out = bank.act(torch.zeros((5, 18)), policy, out=torch.full((5, 8), C.SENTINEL), out_col=4, backend="torch")
    want = torch.tensor([0.6, C.SENTINEL, 0.4, 0.2, C.SENTINEL])
    assert torch.allclose(out[:, 4:], want[:, None].expand(5, 4), atol=1e-6) and torch.all(out[:, :4] == C.SENTINEL)
    with pytest.raises(ValueError):
        PolicyBank(ACT_WIDE_MAX_POLICIES + 1, "cpu", wide=True)
    with pytest.raises(ValueError):
        bank.replace_many([1, 1], [C.marker_actor(0.1)] * 2)
    PolicyBank(ACT_WIDE_MAX_POLICIES, "cpu", wide=True)
    with pytest.raises(ValueError, match="wide=True"):
        PolicyBank(65, "cpu")  # without the switch the limit is hkl_act's


def test_act_wide_checks_its_arguments_on_the_host():
    """hkl_act_wide refuses K outside [1, 4096], a negative n_rows, obs_ld < 18, out_ld < out_col + 4 and null
    scratch with policy given with HKL_E_INVALID before any launch, and n_rows = 0 is HKL_OK: no GPU is needed."""
    from hockey_amd import learner_hip as LH

    L = LH.lib()
    fake = 256  # a non-null "device" address: never dereferenced

    def io(**kw):
        x = LH.ActWideIO()
        x.n_policies, x.n_rows = 130, 0
        x.params = x.packs = x.obs = x.policy = x.out = x.order = x.counts = x.offsets = x.tiles = fake
        x.obs_ld, x.out_ld, x.out_col = 18, 8, 4
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    assert L.hkl_act_wide_io_size() == ctypes.sizeof(LH.ActWideIO)
    assert L.hkl_act_wide(ctypes.byref(io()), None) == 0  # n_rows = 0
    assert L.hkl_act_wide(ctypes.byref(io(n_policies=4096)), None) == 0
    bad = [dict(n_policies=0), dict(n_policies=4097), dict(n_rows=-1), dict(obs_ld=17), dict(out_ld=7),
           dict(out_col=-1), dict(tiles=None), dict(order=None), dict(counts=None), dict(offsets=None),
           dict(params=None), dict(packs=None), dict(obs=None), dict(out=None)]
    for kw in bad:
        assert L.hkl_act_wide(ctypes.byref(io(**kw)), None) == 1, kw
    assert L.hkl_act_wide(None, None) == 1
    assert L.hkl_act_wide(ctypes.byref(io(policy=None, order=None, counts=None, offsets=None, tiles=None)), None) == 0

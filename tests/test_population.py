"""hockey_amd.population without a GPU: the ragged ring against S ReplayRings, train_population's collection on the
kernel source's host build (eager fallback learners), the members it refuses, and the grouped calls' host-side
argument checks (they return before any launch)."""
import ctypes

import pytest
import torch

from hockey_amd.population import PopulationLearner, PopulationRing, train_population
from hockey_amd.td3 import TD3, ReplayRing, TD3Config


def test_population_ring_push_equals_member_rings():
    """S = 3, cap 64: ragged pushes of 0-8 rows per member (a member with none included) until every member has
    wrapped twice; all five columns and the fill levels equal those of three ReplayRings pushed in member order."""
    S, cap = 3, 64
    g = torch.Generator().manual_seed(7)
    pop = PopulationRing(S, cap, device="cpu")
    refs = [ReplayRing(cap, device="cpu") for _ in range(S)]
    pushed = [0] * S
    step, saw_empty = 0, False
    while min(pushed) < 2 * cap + 8:
        counts = torch.randint(0, 9, (S,), generator=g).tolist()
        counts[step % S] = 0 if step % 4 == 0 else counts[step % S]  # regularly a member without a row
        step += 1
        saw_empty |= 0 in counts
        n = sum(counts)
        member = torch.cat([torch.full((c,), j, dtype=torch.int64) for j, c in enumerate(counts)])
        perm = torch.randperm(n, generator=g)  # members interleaved; a member's rows keep their relative order
        member = member[perm]
        s, a = torch.randn(n, 18, generator=g), torch.randn(n, 4, generator=g)
        r, s2 = torch.randn(n, generator=g), torch.randn(n, 18, generator=g)
        d = torch.randint(0, 2, (n,), generator=g).to(torch.uint8)
        pop.push(member, s, a, r, s2, d)
        for j in range(S):
            rows = member == j
            refs[j].push(s[rows], a[rows], r[rows], s2[rows], d[rows])
            pushed[j] += counts[j]
    assert saw_empty
    for j in range(S):
        v = pop.member(j)
        assert len(v) == len(refs[j]) == cap and int(pop.size_t[j]) == int(refs[j].size_t)
        assert int(pop.pos_t[j]) == refs[j].pos
        for k in ("s", "a", "r", "s2", "d"):
            assert torch.equal(getattr(v, k), getattr(refs[j], k)), (j, k)
    with pytest.raises(ValueError):
        pop.push(torch.zeros(cap + 1, dtype=torch.int64), *[torch.zeros(cap + 1, w) for w in (18, 4)],
                 torch.zeros(cap + 1), torch.zeros(cap + 1, 18), torch.zeros(cap + 1))


def test_population_ring_fill_levels_before_wrap():
    pop = PopulationRing(3, 16, device="cpu")
    member = torch.tensor([2, 0, 2, 2], dtype=torch.int64)
    x = torch.arange(4, dtype=torch.float32)
    pop.push(member, x[:, None].expand(4, 18), x[:, None].expand(4, 4), x, x[:, None].expand(4, 18), x)
    assert pop.size_t.tolist() == [1, 0, 3] and [len(pop.member(j)) for j in range(3)] == [1, 0, 3]
    assert pop.member(2).r[:3].tolist() == [0.0, 2.0, 3.0] and pop.member(0).r[0].item() == 1.0


def _cfgs(**kw):
    base = dict(batch_size=32, use_self_play=False, curriculum_name="stage1")
    base.update(kw)
    return [TD3Config(noise_mode="gaussian", **base), TD3Config(noise_mode="ornstein-uhlenbeck", lr_q=1e-3, **base)]


def test_train_population_collection_on_host_build():
    """episode_end="max_steps", S = 2 x 8 arenas on the host build: per member, the stored actions are the applied ones
    (clipped), transitions chain within an episode, every arena of the member is stored at every step, total_steps
    equals the stored rows, and the noise scale in use is TD3.noise_scale() of the member's total_steps."""
    from hostcheck import HostTorchEnv

    S, n, steps = 2, 8, 40
    env = HostTorchEnv(S * n, policies=("external", "external"))
    seen = []

    def on_step(member, arena, obs, a, r, o2, d, res):
        seen.append((member.clone(), arena.clone(), obs.clone(), a.clone(), o2.clone(), res.actions.clone()))

    cfgs = _cfgs(max_steps=steps, start_steps=100)
    # member 1 leaves the random phase in round 1, member 0 (start_steps 100 of 8 x 40 steps per round) too
    agents, st = train_population([(cfgs[0], 3), (cfgs[1], 11)], n_arenas=n, rounds=2, device="cpu", env=env,
                                  on_step=on_step, updates_per_round=4, graphs=False)
    assert len(seen) == 2 * steps
    for t, (member, arena, obs, a, o2, applied) in enumerate(seen):
        assert torch.equal(arena, torch.arange(S * n)) and torch.equal(member, arena // n), t
        assert torch.equal(applied[:, :4], torch.clamp(a, -1, 1)), t
        assert torch.all(applied[:, 4:7].abs().sum(1) > 0)  # the fused weak bot acts for player 2
        if t % steps:
            assert torch.equal(obs, seen[t - 1][4]), t
    for j, ag in enumerate(agents):
        assert st[j]["replay_size"] == st[j]["env_steps"] == ag.total_steps == 2 * steps * n
        assert st[j]["updates"] == 8 and st[j]["skipped_rounds"] == 0 and ag.train_step == 8
        assert ag.current_noise_scale == ag.noise_scale() == st[j]["noise_scale"][-1]
        assert ag.noise_scale() < ag.cfg.action_noise_scale  # annealed: the schedule ran on this member's count
        assert len(st[j]["critic_loss"]) == 2 and all(torch.isfinite(p).all() for p in ag.actor.parameters())
    # the eager learners trained each member on its own slice: the actors have left their (different) initial weights
    assert not torch.equal(agents[0].actor.fc3.weight, agents[1].actor.fc3.weight)


def test_train_population_episode_end_done():
    """episode_end="done", per member: an arena's transitions stop at its done step, the member's total_steps counts
    only its running arenas, and the round ends once every member's episodes have."""
    from hostcheck import HostTorchEnv

    S, n = 2, 8
    env = HostTorchEnv(S * n, policies=("external", "external"))
    seen = []
    cfgs = _cfgs(max_steps=400, start_steps=10 ** 9)
    agents, st = train_population([(cfgs[0], 5), (cfgs[1], 6)], n_arenas=n, rounds=1, device="cpu", env=env,
                                  updates_per_round=0, episode_end="done", graphs=False,
                                  on_step=lambda m, ar, o, a, r, o2, d, res: seen.append((m.clone(), ar.clone(),
                                                                                          d.clone())))
    for j, ag in enumerate(agents):
        stored = sum(int((m == j).sum()) for m, _, _ in seen)
        assert st[j]["replay_size"] == stored == st[j]["env_steps"] == ag.total_steps
        running = set(range(j * n, (j + 1) * n))
        for m, ar, d in seen:
            assert set(ar[m == j].tolist()) == running  # exactly the member's arenas not yet done
            running -= set(ar[(m == j) & (d != 0)].tolist())
        assert not running
    assert len(seen) <= 251 and torch.all(seen[-1][2] != 0)
    # updates_per_round=0: the learner ran no update
    assert all(s["updates"] == 0 for s in st)


def test_train_population_refuses_unsupported_members():
    ok = TD3Config(batch_size=32, use_self_play=False, curriculum_name="stage1", max_steps=10)
    sp = TD3Config(batch_size=32, use_self_play=True, curriculum_name="stage3", max_steps=10)
    per = TD3Config(batch_size=32, use_self_play=False, curriculum_name="stage1", max_steps=10,
                    prioritized_replay=True)
    longer = TD3Config(batch_size=32, use_self_play=False, curriculum_name="stage1", max_steps=11)
    with pytest.raises(ValueError, match="self-play"):
        train_population([(ok, 0), (sp, 1)], n_arenas=2, rounds=1, device="cpu")
    with pytest.raises(ValueError, match="prioritized_replay"):
        train_population([(ok, 0), (per, 1)], n_arenas=2, rounds=1, device="cpu")
    with pytest.raises(ValueError, match="max_steps"):
        train_population([(ok, 0), (longer, 1)], n_arenas=2, rounds=1, device="cpu")
    # use_self_play on a curriculum without a self-play share is the same training: accepted (checked, not run)
    from hockey_amd.population import _check_members

    assert len(_check_members([(TD3Config(use_self_play=True, curriculum_name="stage1"), 0)])) == 1


def test_population_learner_refuses_unequal_members():
    a = TD3(TD3Config(batch_size=32), device="cpu", seed=0)
    b = TD3(TD3Config(batch_size=64), device="cpu", seed=1)
    c = TD3(TD3Config(batch_size=32, policy_update_freq=3), device="cpu", seed=2)
    pop = PopulationRing(2, 16, device="cpu")
    rings = [pop.member(0), pop.member(1)]
    with pytest.raises(ValueError, match="batch_size"):
        PopulationLearner([a, b], rings, 32)
    with pytest.raises(ValueError, match="policy_update_freq"):
        PopulationLearner([a, c], rings, 32)
    with pytest.raises(ValueError, match="members"):
        PopulationLearner([], [], 32)


def test_group_calls_check_their_arguments_on_the_host():
    """Every grouped call refuses n_members outside [1, 64], a null device array and a zeroed member (batch 0, null
    pointers) with HKL_E_INVALID and a message, before any launch: no GPU is needed to see it."""
    from hockey_amd import learner_hip as LH

    L = LH.lib()
    fake = ctypes.c_void_p(256)  # a non-null "device" address: never dereferenced, the checks fail first
    calls = {
        "hkl_sample_group": lambda n, dev: L.hkl_sample_group((LH.SampleIO * 65)(), dev, n, None),
        "hkl_critic_step_group": lambda n, dev: L.hkl_critic_step_group((LH.CriticIO * 65)(), dev, n, None),
        "hkl_actor_step_group": lambda n, dev: L.hkl_actor_step_group((LH.ActorIO * 65)(), dev, n, None),
        "hkl_adam_group": lambda n, dev: L.hkl_adam_group((LH.AdamIO * 65)(), dev, n, None),
        "hkl_pack_group": lambda n, dev: L.hkl_pack_group((LH.PackIO * 65)(), dev, 2, n, None),
        "hkl_wgrad_pair_group": lambda n, dev: L.hkl_wgrad_pair_group((LH.WgJob * 130)(), dev, 2, (LH.WgJob * 130)(),
                                                                      dev, 2, 256, n, None),
    }
    for name, call in calls.items():
        for n, dev in ((0, fake), (65, fake), (3, None), (3, fake)):
            assert call(n, dev) == 1, (name, n)
            msg = L.hkl_last_error().decode()
            assert msg.startswith(name) and len(msg) > len(name) + 2, (name, n, msg)
        assert "member 0" in L.hkl_last_error().decode(), name

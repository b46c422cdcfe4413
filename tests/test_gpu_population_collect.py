"""hkl_opp_draw + hkl_collect under graph capture, and train_population with collect="device" on a VecHockeyEnv: a
member's whole run does not depend on the population, nor on how often the host polls the survivors.

These take streams from torch's pool (a capture, the learners' warm-up pairs), so they stand in a file that runs after
tests/test_gpu_facade.py, as tests/test_gpu_population_explore.py does; the kernels' own tests are
tests/test_gpu_collect.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_population_explore as GP  # noqa: E402
from hockey_amd import collect as C  # noqa: E402
from hockey_amd import population as POP  # noqa: E402
from hockey_amd.opponents import PopulationOpponentMix  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"
STATE = ("policy2", "policy", "snap", "opp_inc", "counts", "snap_counts", "calls", "obs", "obs2", "alive",
         "ep_reward", "push_pos", "push_n", "count", "steps", "live")


def _collector(S, n, cap, episode_end):
    cfg = TD3Config(use_self_play=True, self_play_pool_size=3, curriculum_name="stage3")
    mix = PopulationOpponentMix([cfg] * S, [5, 6, 7][:S], n, DEV, sampling="arena")
    col = C.Collector(None, None, mix, POP.PopulationRing(S, cap, device=DEV), None, [5, 6, 7][:S], n, backend="hip",
                      episode_end=episode_end)
    g = torch.Generator().manual_seed(1)
    col.begin_round(torch.randn(S * n, 18, generator=g).to(DEV), torch.randn(S * n, 18, generator=g).to(DEV), 8)
    # pools as if two of the members held snapshots (the draw reads these buffers only)
    col.len_t.copy_(torch.tensor([3, 0, 2][:S], dtype=torch.int32))
    col.scores.copy_(torch.tensor([[1.0, 2.0, 5.0]] * S))
    col.probs.copy_(torch.tensor([[0.5, 0.5]] * S))
    return col


@pytest.mark.parametrize("episode_end", ["done", "max_steps"])
def test_graph_replay_of_a_draw_and_collect_pair_equals_eager_pairs(episode_end):
    """One hkl_opp_draw + hkl_collect pair (S = 3 x 65 rows, rings of 68) captured once and replayed three times
    against three eager pairs of a twin: the draw's outputs, the rings, every counter and accumulator, bit for bit --
    the call counters, write positions, survivors and kept observations advance on the device.  The captured graph is a
    straight line of kernel nodes: the draw and its counter's advance, then count / scan / store ("done") or the one
    store launch ("max_steps")."""
    S, n = 3, 65
    cap_c, twin = (_collector(S, n, n + 3, episode_end) for _ in range(2))
    g = torch.Generator().manual_seed(2)
    o2, o22 = (torch.randn(S * n, 18, generator=g).to(DEV) for _ in range(2))
    r = torch.randn(S * n, generator=g).to(DEV)
    d = (torch.rand(S * n, generator=g) < 0.15).to(DEV).to(torch.uint8)
    for col in (cap_c, twin):
        col.act8.copy_(torch.randn(S * n, 8, generator=torch.Generator().manual_seed(3)).to(DEV))

    def pair(col):
        col.draw()
        col.store(o2, o22, r, d)

    pair(cap_c)  # warm-up: the structs exist and the kernels are loaded before the capture
    pair(twin)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        pair(cap_c)
    order, line = GP._graph_shape(graph)
    assert line, order
    assert order == [GP.KERNEL] * (5 if episode_end == "done" else 3), order
    for _ in range(3):
        graph.replay()
        pair(twin)
    torch.cuda.synchronize()
    bits = lambda t: t.cpu().contiguous().view(torch.uint8).numpy()  # noqa: E731
    for k in STATE:
        assert np.array_equal(bits(getattr(cap_c, k)), bits(getattr(twin, k))), k
    for k in ("s", "a", "r", "s2", "d", "pos_t", "size_t"):
        assert np.array_equal(bits(getattr(cap_c.ring, k)), bits(getattr(twin.ring, k))), k
    # the replays charged the captured step's tally row, the eager calls one row each
    assert torch.equal(cap_c.tally[1:].sum(0), twin.tally[1:].sum(0)) and torch.equal(cap_c.tally[0], twin.tally[0])
    assert cap_c.calls.tolist() == [4] * S and int(cap_c.snap_counts.sum()) > 0
    assert int(cap_c.ring.size_t.max()) == n + 3  # the rings wrapped


def _cfg(noise, **kw):
    base = dict(batch_size=256, use_self_play=False, curriculum_name="stage3", max_steps=40, start_steps=100,
                noise_mode=noise, self_play_interval=8, buffer_size=2000)
    base.update(kw)
    return TD3Config(**base)


def _run(members, monkeypatch, **kw):
    """train_population(explore="device", collect="device") on its own env; returns (agents, stats, the ring)."""
    rings = []
    for name in ("PopulationRing", "PopulationPrioritizedRing"):
        cls = getattr(POP, name)

        def make(*a, _cls=cls, **k):
            rings.append(_cls(*a, **k))
            return rings[-1]

        monkeypatch.setattr(POP, name, make)
    agents, st = POP.train_population(members, n_arenas=8, device=DEV, explore="device", collect="device",
                                      updates_per_round=4, **kw)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return agents, st, rings[-1]


def _same_member(a, b):
    """(agent, stats, ring, index) twice: ring bytes, stats and every actor / critic parameter, bit for bit."""
    (ag_a, st_a, ring_a, ja), (ag_b, st_b, ring_b, jb) = a, b
    bits = lambda t: t.detach().cpu().contiguous().view(torch.uint8).numpy()  # noqa: E731
    ma, mb = ring_a.member(ja), ring_b.member(jb)
    for k in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(bits(getattr(ma, k)), bits(getattr(mb, k))), k
    assert int(ring_a.pos_t[ja]) == int(ring_b.pos_t[jb]) and int(ma.size_t) == int(mb.size_t)
    if hasattr(ma, "w"):
        assert np.array_equal(bits(ma.w), bits(mb.w))
    assert st_a == st_b
    for net in ("actor", "critic", "target_actor", "target_critic"):
        for (name, p), (_, q) in zip(getattr(ag_a, net).named_parameters(), getattr(ag_b, net).named_parameters()):
            assert np.array_equal(bits(p), bits(q)), (net, name)


def test_a_members_run_does_not_depend_on_the_population(monkeypatch):
    """Three members (gaussian, uniform replay, no self-play; Ornstein-Uhlenbeck, prioritized, a pool of 2; pink, a
    pool of 3) x 8 arenas x 3 rounds of 40 steps at batch 256, then the middle member alone: its ring bytes, priorities,
    stats and final actor and critic parameters are equal bit for bit.  The curriculum reaches a self-play share in
    rounds 2 and 3, against the snapshots the pools took after round 1."""
    members = [(_cfg("gaussian"), 21), (_cfg("ornstein-uhlenbeck", use_self_play=True, self_play_pool_size=2,
                                             prioritized_replay=True, start_steps=200), 34),
               (_cfg("pink", use_self_play=True, self_play_pool_size=3, lr_q=1e-3), 55)]
    agents, st, ring = _run(members, monkeypatch, rounds=3, self_play="arena")
    solo_agents, solo_st, solo_ring = _run(members[1:2], monkeypatch, rounds=3, self_play="arena")
    assert st[1]["updates"] == 12 and st[1]["env_steps"] == 3 * 40 * 8 and st[1]["pool_size"] == [1, 2, 2]
    assert st[1]["opponents"][2]["self_play"] > 0 and sum(st[1]["opponents"][2]["snapshots"]) > 0
    assert st[0]["opponents"] != st[1]["opponents"]
    _same_member((agents[1], st[1], ring, 1), (solo_agents[0], solo_st[0], solo_ring, 0))


def test_results_do_not_depend_on_poll_every(monkeypatch):
    """episode_end="done" with the survivors read every step and never (poll_every 1 and 1 000), two members x 8
    arenas x 2 rounds of up to 270 steps (every episode ends by the env's 250-step limit): the same rings, stats and
    parameters; the polled run stopped early, so the call counters were set back to the same values."""
    members = [(_cfg("gaussian", max_steps=270), 3), (_cfg("ornstein-uhlenbeck", max_steps=270, start_steps=500), 4)]
    runs = [_run(members, monkeypatch, rounds=2, episode_end="done", poll_every=p) for p in (1, 1000)]
    for j in range(2):
        _same_member(*[(ag[j], st[j], ring, j) for ag, st, ring in runs])
    assert 0 < runs[0][1][0]["env_steps"] <= 2 * 250 * 8

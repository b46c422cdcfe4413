"""Population self-play on the GPU: PopulationOpponentMix on the hip backend over a wide bank (hkl_act_wide),
train_population(self_play="arena") with graphs on, and the wide acting call replayed from a captured graph (the
rest of hkl_act_wide's tests are in tests/test_gpu_act_wide.py, whose docstring says why this one is here)."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import selfplay_cases as C  # noqa: E402
from hockey_amd.learner_hip import ACT_MAX_POLICIES  # noqa: E402
from hockey_amd.population import train_population  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"


def test_self_play_arenas_face_their_own_members_snapshots_on_the_wide_bank():
    """The marker-actor isolation run of tests/test_population_selfplay.py at S = 5 x 8 arenas: 5 x 13 = 65 slots,
    one more than hkl_act holds, so every select acts through hkl_act_wide."""
    mix = C.make_mix(5, 8, DEV, "arena", "hip", {0: 2, 2: 3, 3: 12, 4: 1}, no_self_play=(1,))
    assert mix.bank.capacity == 65 > ACT_MAX_POLICIES
    recount, got = C.isolation_run(mix, 200)
    assert got == recount
    assert recount[1]["self_play"] == 0 and all(recount[j]["self_play"] > 0 for j in (0, 2, 3, 4))
    assert all(sum(r["snapshots"]) == r["self_play"] for r in recount)


def test_train_population_with_self_play_and_prioritized_members():
    kw = dict(batch_size=256, use_self_play=True, curriculum_name="stage3", max_steps=50, start_steps=50,
              self_play_interval=8, self_play_pool_size=12)
    ms = [(TD3Config(prioritized_replay=j < 2, **kw), 20 + j) for j in range(4)]
    agents, st = train_population(ms, n_arenas=8, rounds=2, device=DEV, updates_per_round=8, graphs=True,
                                  self_play="arena")
    for j, ag in enumerate(agents):
        assert st[j]["pool_size"] == [1, 2]
        assert all(bool(torch.isfinite(p).all()) for p in ag.actor.parameters())
        assert st[j]["updates"] == 16 and len(st[j]["opponents"]) == 2
        assert all(o["strong"] + o["weak"] + o["self_play"] == 8 * 50 for o in st[j]["opponents"])


def test_wide_bank_graph_replay():
    """One act at K = 130 captured in a (linear) graph; policy and obs are overwritten in place before each of two
    replays, and each replay equals the eager call on the same contents bit for bit (sentinels included)."""
    import test_gpu_act_wide as W

    wide, _ = W._bank130()
    n = 1000
    obs, policy, out = W._obs(n).clone(), W._policy130(n).clone(), W._out(n)
    wide.act(obs, policy, out=out, out_col=4, backend="hip")  # warm-up: the scratch buffers exist before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wide.act(obs, policy, out=out, out_col=4, backend="hip")
    for r in (1, 2):
        new_p = W._policy130(n)[torch.randperm(n, generator=torch.Generator().manual_seed(r)).to(DEV)]
        obs.copy_(W._obs(n, seed=10 + r))
        policy.copy_(new_p)
        out.fill_(W.SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager = wide.act(obs.clone(), policy.clone(), out=W._out(n), out_col=4, backend="hip")
        assert torch.equal(out, eager), r
        assert int((out[:, 4] != W.SENTINEL).sum()) == int(((policy >= 0) & (policy < 130)).sum())

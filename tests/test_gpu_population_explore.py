"""hkl_explore under graph capture, and train / train_population with explore="device" on a VecHockeyEnv.

These take streams from torch's pool (a capture, the learners' warm-up pairs), so they stand in a file that runs after
tests/test_gpu_facade.py, as tests/test_gpu_population_selfplay.py's graph test does; the kernel's own tests are
tests/test_gpu_explore.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_explore as G  # noqa: E402
from hockey_amd import explore as X  # noqa: E402
from hockey_amd.td3 import TD3Config  # noqa: E402

DEV = "cuda:0"
KERNEL = 0  # hipGraphNodeTypeKernel


def _hip():
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def _graph_shape(graph):
    """(node types in order along the line, True when every node has at most one dependency and one dependent and
    exactly one node has none) of a captured graph kept with keep_graph=True."""
    hip, vp = _hip(), ctypes.c_void_p
    g, n = vp(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (vp * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kinds, parent = {}, {}
    for node in nodes:
        t, k = ctypes.c_int(-1), ctypes.c_size_t(0)
        assert hip.hipGraphNodeGetType(vp(node), ctypes.byref(t)) == 0
        assert hip.hipGraphNodeGetDependencies(vp(node), None, ctypes.byref(k)) == 0
        deps = (vp * max(k.value, 1))()
        if k.value:
            assert hip.hipGraphNodeGetDependencies(vp(node), deps, ctypes.byref(k)) == 0
        kinds[node], parent[node] = t.value, [deps[i] for i in range(k.value)]
    roots = [v for v in nodes if not parent[v]]
    line = len(roots) == 1 and all(len(p) <= 1 for p in parent.values())
    children = [p[0] for p in parent.values() if p]
    line = line and len(set(children)) == len(children)
    order, cur = [], roots[0] if roots else None
    while cur is not None:
        order.append(kinds[cur])
        nxt = [v for v in nodes if parent[v] == [cur]]
        cur = nxt[0] if nxt else None
    return order, line and len(order) == len(nodes)


@pytest.mark.parametrize("S", [3, 1])
def test_graph_replay_equals_eager_calls(S):
    """One hkl_explore call (S = 3: gaussian / OU / uniform through the grouping; S = 1: OU on slot 0, no grouping)
    captured once and replayed 4 times against 4 eager calls of a twin: out after every call, and x, z_out, scale_out,
    total and calls at the end, bit for bit -- the counters and the OU state advance on the device.  The captured
    graph is a straight line of kernel nodes: two for S = 1, six for S = 3 (the counters' zeroing, hkl_act's three
    grouping kernels, the acting kernel, the counters' advance)."""
    n = 20
    b = G.bank(S)
    kinds = ("gaussian", "ornstein-uhlenbeck", "uniform") if S == 3 else ("ornstein-uhlenbeck",)
    pk, _ = G.members_for(S, kinds, start=(0, 30, 0) if S == 3 else (30,))
    obs = G.observations(S * n, 5)
    count = torch.full((S,), n - 1, dtype=torch.int32, device=DEV)
    cap, twin = (X.Explorer(b, pk, n, backend="hip", keep_draws=True) for _ in range(2))
    out_c, out_t = torch.zeros(S * n, 4, device=DEV), torch.zeros(S * n, 4, device=DEV)
    cap.explore(obs, out_c, 0, count=count)  # warm-up: the bank's scratch exists before the capture
    torch.cuda.synchronize()
    for t in (cap.total, cap.calls, cap.x):
        t.zero_()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        cap.explore(obs, out_c, 0, count=count)
    order, line = _graph_shape(graph)
    assert line, order
    assert order == [KERNEL] * (6 if S == 3 else 2), order
    for r in range(4):
        G.nan_fill(cap)
        out_c.fill_(float("nan"))
        graph.replay()
        twin.explore(obs, out_t, 0, count=count)
        torch.cuda.synchronize()
        assert np.array_equal(G.bits(out_c), G.bits(out_t)), r
    for a, t in ((cap.x, twin.x), (cap.z, twin.z), (cap.scale, twin.scale)):
        assert np.array_equal(G.bits(a), G.bits(t))
    assert cap.total.tolist() == twin.total.tolist() == [4 * (n - 1)] * S and cap.calls.tolist() == [4] * S
    assert cap.x.abs().sum() > 0


class _Recording:
    """A VecHockeyEnv whose every step records the actions the kernel received (res.actions)."""

    def __init__(self, env):
        self._env = env

    def __getattr__(self, name):
        return getattr(self._env, name)

    def step(self, actions, **kw):
        return self._env.step(actions, record_actions=True, **kw)


def _cfg(noise, **kw):
    base = dict(batch_size=256, use_self_play=False, curriculum_name="stage1", max_steps=20, start_steps=60,
                noise_mode=noise)
    base.update(kw)
    return TD3Config(**base)


def test_train_explore_device_on_the_gpu():
    """train(explore="device"), 16 arenas x two rounds of 20 steps: the stored action is act8[:, :4] as the step kernel
    received it, lies in [-1, 1], the agent's total_steps is the arena-steps played, its noise scale noise_scale() of
    that count, and both rounds' updates ran (320 arena-steps exceed the batch of 256)."""
    from hockey_amd.td3 import train
    from hockey_amd.vec_env import VecHockeyEnv

    n, seen = 16, []
    env = _Recording(VecHockeyEnv(n, device=DEV, policies=("external", "external"), auto_reset=False, seed=4))
    agent, st = train(n_arenas=n, rounds=2, cfg=_cfg("ornstein-uhlenbeck"), device=DEV, env=env, seed=4,
                      explore="device", updates_per_round=2,
                      on_step=lambda o, a, r, o2, d, res: seen.append((a.clone(), res.actions.clone())))
    torch.cuda.synchronize()
    env.close()
    assert len(seen) == 40
    for a, applied in seen:
        assert torch.equal(applied[:, :4], a) and a.abs().max() <= 1
    assert torch.stack([a for a, _ in seen]).std() > 0.05
    assert agent.total_steps == st["env_steps"] == st["replay_size"] == 2 * 20 * n
    assert agent.current_noise_scale == agent.noise_scale() < agent.cfg.action_noise_scale
    assert st["updates"] == 4 and all(torch.isfinite(p).all() for p in agent.actor.parameters())


@pytest.mark.parametrize("episode_end", ["max_steps", "done"])
def test_train_population_explore_device_on_the_gpu(episode_end):
    """train_population(explore="device"), S = 3 (gaussian / OU / pink; start_steps 0, 60, 120) x 8 arenas, two rounds
    of 20 steps: per member the stored actions are the step kernel's, total_steps equals the stored rows
    (episode_end="done": counted on the device from the arenas still running) and the noise scale follows the
    member's own count."""
    from hockey_amd.population import train_population
    from hockey_amd.vec_env import VecHockeyEnv

    S, n, seen = 3, 8, []
    kinds = ("gaussian", "ornstein-uhlenbeck", "pink")
    members = [(_cfg(k, start_steps=60 * j, lr_q=4e-4 * (j + 1)), 7 + j) for j, k in enumerate(kinds)]
    env = _Recording(VecHockeyEnv(S * n, device=DEV, policies=("external", "external"), auto_reset=False, seed=7))
    agents, st = train_population(members, n_arenas=n, rounds=2, device=DEV, env=env, explore="device",
                                  updates_per_round=2, episode_end=episode_end,
                                  on_step=lambda m, ar, o, a, r, o2, d, res: seen.append(
                                      (m.clone(), ar.clone(), a.clone(), res.actions.clone())))
    torch.cuda.synchronize()
    env.close()
    for m, ar, a, applied in seen:
        assert torch.equal(applied[ar, :4], a) and a.abs().max() <= 1
    for j, ag in enumerate(agents):
        stored = sum(int((m == j).sum()) for m, _, _, _ in seen)
        assert ag.total_steps == st[j]["env_steps"] == st[j]["replay_size"] == stored
        if episode_end == "max_steps":
            assert stored == 2 * 20 * n and st[j]["updates"] == 2 and st[j]["skipped_rounds"] == 1
        assert ag.current_noise_scale == ag.noise_scale() == st[j]["noise_scale"][-1]
        assert ag.noise_scale() < ag.cfg.action_noise_scale

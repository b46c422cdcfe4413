"""One law for both collectors of a training round (hockey_amd.host_round): ``TorchCollector`` and
``hockey_amd.collect.Collector`` are driven through ``begin_round`` / ``run_round`` / ``end_round`` only, S = 2 members x
n = 4 arenas on a one-slot-per-member bank and a ``PopulationRing`` of n * max_steps rows per member, and held to the
same integer identities: what ``end_round`` reports is what the ring holds, an arena's episode is stored up to its done
step and no further, and the explorer is told how many arenas of each member still run.

On the CPU the env is the kernel source's host build and the device Collector runs its numpy laws; the GPU twin runs the
kernels (``backend="hip"``) and ``TorchCollector`` on a VecHockeyEnv of the same 8 arenas.

SEEDS = (3, 4), chosen together with TABLE (mostly the strong bot) and ``start_steps=10``: with them at least one member
has an episode end inside 120 steps under every collector here, on the host build and on the GPU (``min(steps) <
n * 120`` asserts it), so the "done" identities are tested on rounds in which episodes did end."""
import pytest

torch = pytest.importorskip("torch")

from hockey_amd.collect import Collector  # noqa: E402
from hockey_amd.constants import Mode  # noqa: E402
from hockey_amd.explore import Explorer, Member  # noqa: E402
from hockey_amd.host_round import PopulationExplorer, TorchCollector  # noqa: E402
from hockey_amd.opponents import PopulationOpponentMix  # noqa: E402
from hockey_amd.policy_bank import PolicyBank  # noqa: E402
from hockey_amd.population import PopulationRing  # noqa: E402
from hockey_amd.td3 import TD3, TD3Config, reset_round  # noqa: E402

S, N_PER = 2, 4
SEEDS = (3, 4)
TABLE = [(1.0, 0.7, 0.3, 0.0)]  # mostly the strong bot: goals inside 120 steps
KINDS = ("torch_host_explorer", "torch_device_explorer", "device")


class Recording:
    """In the explorer's place: passes every call on and keeps (the count it was given, the members' arenas still
    running according to the collector's ``alive`` before the step)."""

    def __init__(self, explorer):
        self.inner, self.count_on_device, self.seen, self.collector = explorer, explorer.count_on_device, [], None

    def __getattr__(self, name):  # calls, total, ...: the device Collector's round-end bookkeeping
        return getattr(self.inner, name)

    def explore(self, obs, out, out_col=0, count=None):
        running = (self.collector.alive != 0).view(S, N_PER).sum(1).tolist()
        given = [N_PER] * S if count is None else [int(c) for c in count]
        self.seen.append((given, running))
        return self.inner.explore(obs, out, out_col, count=count)


def run_round(kind, device, episode_end, max_steps):
    """One round of ``kind``'s collector; returns (steps, ep_reward, opp, ring, collector, recording explorer, the
    agents' total_steps after the round)."""
    dev = torch.device(device)
    N = S * N_PER
    if dev.type == "cpu":
        from hostcheck import HostTorchEnv

        env = HostTorchEnv(N, policies=("external", "external"))
    else:
        from hockey_amd.vec_env import VecHockeyEnv

        env = VecHockeyEnv(N, device=dev, policies=("external", "external"), auto_reset=False, seed=SEEDS[0])
    backend = "hip" if dev.type == "cuda" else "torch"
    cfg = TD3Config(max_steps=max_steps, start_steps=10, use_self_play=False, noise_mode="gaussian")
    agents = [TD3(cfg, dev, s, max_total_steps=4 * max_steps * N_PER, n_envs=1) for s in SEEDS]
    bank = PolicyBank(S, dev)
    bank.replace_many(range(S), [ag.actor for ag in agents])
    if kind == "torch_host_explorer":
        explorer = PopulationExplorer(agents, bank, N_PER)
    else:
        explorer = Explorer(bank, [Member.from_agent(ag) for ag in agents], N_PER, backend=backend)
    explorer = Recording(explorer)
    mix = PopulationOpponentMix([cfg] * S, list(SEEDS), N_PER, dev, sampling="arena", curriculum=TABLE)
    ring = PopulationRing(S, N_PER * max_steps, device=dev)
    args = (env, bank, mix, ring, explorer, list(SEEDS), N_PER)
    if kind == "device":
        col = Collector(*args, backend=backend, episode_end=episode_end, poll_every=5)
    else:
        col = TorchCollector(*args, episode_end=episode_end)
    explorer.collector = col
    obs, obs2 = reset_round(env, "seeded", Mode.NORMAL, 0, N_PER, list(SEEDS))
    explorer.reset_noise()
    col.begin_round(obs, obs2, max_steps)
    col.run_round()
    explorer.sync(agents)
    steps, ep_reward, opp = col.end_round([ag.actor for ag in agents], N_PER)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    env.close()
    return steps, ep_reward, opp, ring, col, explorer, [ag.total_steps for ag in agents]


def check_max_steps(kind, device):
    steps, ep_reward, opp, ring, col, rec, totals = run_round(kind, device, "max_steps", 6)
    assert list(steps) == [N_PER * 6] * S == ring.size_t.tolist() == totals
    assert ep_reward.shape == (S * N_PER,) and len(opp) == S
    assert len(rec.seen) == 6 and all(given == [N_PER] * S for given, _ in rec.seen)


def check_done(kind, device):
    T = 120
    steps, ep_reward, opp, ring, col, rec, totals = run_round(kind, device, "done", T)
    sizes = ring.size_t.tolist()
    ended = (N_PER - (col.alive != 0).view(S, N_PER).sum(1)).tolist()  # per member: the arenas whose episode ended
    assert list(steps) == sizes == totals
    assert min(steps) < N_PER * T
    for m in range(S):
        d = ring.d[m * ring.cap:m * ring.cap + sizes[m]]
        assert int((d == 1).sum()) == ended[m] <= N_PER
    # the explorer was told, at every step, how many arenas of each member still ran before it ...
    assert all(given == running for given, running in rec.seen)
    # ... which is also what the step stored: the counts add up to the arena-steps (a step with nobody alive, which the
    # device Collector may run between two polls, counts nothing)
    assert [sum(given[m] for given, _ in rec.seen) for m in range(S)] == list(steps)


@pytest.mark.parametrize("kind", KINDS)
def test_round_max_steps_on_the_host_build(kind):
    check_max_steps(kind, "cpu")


@pytest.mark.parametrize("kind", KINDS)
def test_round_done_on_the_host_build(kind):
    check_done(kind, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_round_max_steps_on_the_gpu(kind):
    check_max_steps(kind, "cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_round_done_on_the_gpu(kind):
    check_done(kind, "cuda:0")

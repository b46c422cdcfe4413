"""A training round's collection: one collector interface with an explorer in front of it, on the host or the device.

``hockey_amd.td3.train`` (S = 1 member) and ``hockey_amd.population.train_population`` build one *explorer* (player 1's
actions with exploration) and one *collector* (the rest of a collection step) and drive them, per round::

    obs, obs2 = reset_round(...); explorer.reset_noise()
    collector.begin_round(obs, obs2, max_steps); collector.run_round(); explorer.sync(agents)
    steps, ep_reward, opp = collector.end_round(actors, episodes)    # per member: arena-steps, opponent record

A collector's ``step()`` is four pieces: the explorer's ``explore`` into ``act8[:, :4]``, ``draw()`` (player 2: bot or
self-play, which snapshot, its actions into ``act8[:, 4:]``), ``env.step`` and ``store(...)`` (the replay ring, episode
rewards, outcome tally, survivors).  Member m owns arenas [m n, (m + 1) n).

explore="torch" (default): this module's ``AgentExplorer`` (``train``: ``TD3.act``) or ``PopulationExplorer``, which
restates ``TD3.act`` per arena for S members acting through a PolicyBank (one ``hkl_act`` launch): each member's
total_steps advances by its running arenas, its annealed scale is ``TD3.noise_scale()`` of that count, and arena i of the
member draws a uniform action while (total_steps before the step + 1 + i) < start_steps or the whole step lies in the
random phase; one noise generator per distinct ``noise_mode`` covers that mode's arenas (unit scale, seeded by the
mode's first member, multiplied by the arena's scale) and advances on every step in which one of its members is past the
all-random phase.  explore="device": a ``hockey_amd.explore.Explorer`` on the acting bank (refreshed after each round's
updates): ONE ``hkl_explore`` call per step writes player 1's columns of the step kernel's input; the step counts and
noise state live on the device and reach ``agent.total_steps`` / ``current_noise_scale`` in ``sync``.  The law is
``TD3.act``'s; the draws are Philox's, keyed by the member's seed, its arenas' indices inside the member and its own
call counter, so they do not depend on the population (hockey_amd.explore lists the batched differences).

collect="torch" (default): ``TorchCollector``.  The opponent draws come from the mix's torch generator over all arenas
and the step kernel's device draws are keyed by the global arena id, so a member's trajectory depends on its position
in the population and on its size; ``episode_end="done"`` costs one host sync per step.  collect="device" (needs
explore="device", a snapshot per arena and step, no ``on_step``): a ``hockey_amd.collect.Collector``, whose module
docstring states a step's calls: nothing is read back but, under "done", the survivors' count every ``poll_every``
steps (the results do not depend on it).  Player 2 is then a ``PopulationOpponentMix`` and the ring a
``PopulationRing``; every draw is keyed by the member's seed, so member j's trajectories, ring and weights are the same
bits alone and in any population (hockey_amd.collect lists the batched differences).
"""
import time

import numpy as np
import torch

from .evaluate import reset_params
from .noise import make_noise


def check_collect_args(explore, collect, per_step_snapshots, on_step):
    """The ``explore`` / ``collect`` arguments of ``train`` and ``train_population`` and what collect="device" refuses
    (per_step_snapshots: the caller asked for one self-play snapshot per step)."""
    if explore not in ("torch", "device"):
        raise ValueError("explore must be 'torch' or 'device'")
    if collect not in ("torch", "device"):
        raise ValueError("collect must be 'torch' or 'device'")
    if collect == "device":
        if explore != "device":
            raise ValueError("collect='device' runs behind hkl_explore: it needs explore='device'")
        if per_step_snapshots:
            raise ValueError("collect='device' draws a snapshot per arena and step: 'step' sampling is not supported "
                             "on the device, ask for 'arena'")
        if on_step is not None:
            raise ValueError("collect='device' stores the transitions on the device without materialising a step's "
                             "rows: on_step is not supported")


def reset_round(env, reset, mode, rnd, n, seeds):
    """(obs, obs2) after resetting ``env`` for round ``rnd`` of ``train`` / ``train_population``: one block of ``n``
    arenas per entry of ``seeds``, whose arena i plays episode e = rnd * n + i + 1 of that seed's run, placed like
    ``reset(seed=seed + e)`` with the puck side toggling per reset.  reset: "seeded" (drawn by the kernel where the
    env has ``reset_seeded``, else on the host), "seeded_host", or "device" (the kernel's Philox placement)."""
    if reset == "device":
        pair = env.reset()
    elif reset == "seeded" and hasattr(env, "reset_seeded"):
        # the same episodes as below, drawn by the kernel: seeds and puck sides are reset_params' own
        e = np.arange(rnd * n, (rnd + 1) * n, dtype=np.int64)
        st = torch.cat([torch.arange(s + 1 + rnd * n, s + 1 + (rnd + 1) * n, device=env.device) for s in seeds])
        pair = env.reset_seeded(st, one_starting=np.tile((e % 2) == 1, len(seeds)))
    else:
        env.reset_params(np.concatenate([reset_params(n, s + rnd * n + 1, mode, first_reset=rnd * n)[0]
                                         for s in seeds]))
        pair = env.observe()
    return tuple(t.clone() for t in pair)


def store_step(store, mix, stop_at_done, alive, ep_reward, res, obs, a, r, o2, d):
    """A collection step's bookkeeping for both ``episode_end`` values: ``store(rows, res, obs, a, r, o2, d)`` gets
    the transitions to keep (rows: their arena indices, or None for all arenas), ``mix`` the step's outcomes, and
    ``ep_reward`` the rewards.  episode_end="done" keeps only the arenas still ``alive`` and clears the flag of those
    that ended (in place); the caller counts the survivors."""
    if stop_at_done:  # only the transitions of episodes that were still running are stored
        idx = torch.nonzero(alive).squeeze(1)
        store(idx, res, obs[idx], a[idx], r[idx], o2[idx], d[idx])
        mix.register_outcomes(d & alive, r)
        ep_reward += torch.where(alive, r, torch.zeros_like(r))
        alive &= d == 0
    else:
        store(None, res, obs, a, r, o2, d)
        mix.register_outcomes(d, r)
        ep_reward += r


class RoundClock:
    """A training round's wall-clock marks (with ``timing``: a device synchronise before each) and the evaluation
    schedule, every ``eval_interval`` episodes."""

    def __init__(self, device, timing, eval_interval):
        self.device, self.timing, self.interval, self.next_eval = device, timing, eval_interval, eval_interval

    def mark(self):
        if self.timing:
            torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def start(self):
        self.t0 = self.mark()

    def collected(self):
        self.t1 = self.mark()

    def updated(self, stats):
        """Append (collection seconds, update seconds) to every dict's "round_time" (with ``timing``)."""
        t2 = self.mark()
        if self.timing:
            for st in stats:
                st["round_time"].append((self.t1 - self.t0, t2 - self.t1))

    def eval_due(self, episodes):
        due = episodes >= self.next_eval
        if due:
            self.next_eval = (episodes // self.interval + 1) * self.interval
        return due


# ---------------------------------------------------------------------------------------------------- host explorers
class HostExplorer:
    """What the host explorers share, shaped like ``hockey_amd.explore.Explorer``: ``explore`` takes the members'
    running arenas as a host list [S] (None: all) and returns the actions as a tensor of their own; the agents advance
    as they act, so ``sync`` has nothing to do."""

    count_on_device = False

    def sync(self, agents):
        pass


class AgentExplorer(HostExplorer):
    """``train``'s explore="torch": ``TD3.act`` of one agent on all rows."""

    def __init__(self, agent):
        self.agent = agent

    def reset_noise(self):
        self.agent.reset_noise()

    def explore(self, obs, out, out_col=0, count=None):
        a = self.agent.act(obs, count=None if count is None else count[0])
        out[:, out_col:out_col + 4] = a
        return a


class PopulationExplorer(HostExplorer):
    """``train_population``'s explore="torch" (module docstring): ``TD3.act`` restated per arena for the S ``agents``,
    member j on ``rows_per_member`` rows through slot j of ``bank``."""

    def __init__(self, agents, bank, rows_per_member):
        self.agents, self.bank = list(agents), bank
        S, n, dev = len(self.agents), int(rows_per_member), bank.device
        self.S, self.n, self.N = S, n, S * n
        self.member_of = torch.arange(self.N, device=dev) // n  # [N] int64
        self.policy = self.member_of.to(torch.int32)
        self.local = (torch.arange(self.N, device=dev) % n).to(torch.float64)  # an arena's index inside its member
        # one generator per noise mode over that mode's arenas (unit scale: the arena's own scale multiplies the draw)
        modes = {}
        for j, ag in enumerate(self.agents):
            modes.setdefault(ag.cfg.noise_mode, []).append(j)
        self.gens = {}
        for mname, js in modes.items():
            rows = torch.cat([torch.arange(j * n, (j + 1) * n, device=dev) for j in js])
            first = self.agents[js[0]]
            self.gens[mname] = (make_noise(mname, rows.numel(), 4, 1.0, first.cfg.max_steps, dev, first.seed), rows, js)
        self.start_t = torch.tensor([float(ag.cfg.start_steps) for ag in self.agents], dtype=torch.float64, device=dev)

    def reset_noise(self):
        for g, _, _ in self.gens.values():
            g.reset()

    def explore(self, obs, out, out_col=0, count=None):
        agents, dev, N, member_of = self.agents, self.bank.device, self.N, self.member_of
        # ---- TD3.act per member: count, random phase, annealed scale (host scalars -> [S] tensors)
        first = [ag.total_steps + 1 for ag in agents]
        for ag, k in zip(agents, [self.n] * self.S if count is None else count):
            ag.total_steps += k
        all_random = [ag.total_steps < ag.cfg.start_steps for ag in agents]
        for ag, rnd_phase in zip(agents, all_random):
            if not rnd_phase:
                ag.current_noise_scale = ag.noise_scale()
        scale_t = torch.tensor([ag.current_noise_scale for ag in agents], dtype=torch.float32, device=dev)
        first_t = torch.tensor(first, dtype=torch.float64, device=dev)
        allr_t = torch.tensor(all_random, dtype=torch.bool, device=dev)
        a = self.bank.act(obs, self.policy)
        noise = torch.zeros((N, 4), device=dev)
        for g, rows, js in self.gens.values():
            if not all(all_random[j] for j in js):
                noise[rows] = g().float()
        a = torch.clamp(a + noise * scale_t[member_of][:, None], -1, 1)
        if any(f < ag.cfg.start_steps for f, ag in zip(first, agents)):
            rnd_rows = allr_t[member_of] | ((self.local + first_t[member_of]) < self.start_t[member_of])
            a = torch.where(rnd_rows[:, None], torch.rand((N, 4), device=dev) * 2 - 1, a)
        out[:, out_col:out_col + 4] = a
        return a


# ---------------------------------------------------------------------------------------------------- TorchCollector
class TorchCollector:
    """collect="torch": ``hockey_amd.collect.Collector``'s constructor and round interface in torch ops, for S =
    len(members) members of ``rows_per_member`` arenas each (``bank`` and the members' seeds are not used here).  mix: an
    ``OpponentMix`` over all arenas or a ``PopulationOpponentMix`` of the S members.  Under episode_end="done" the
    explorer gets the members' running arenas in the form its ``count_on_device`` asks for (int32 [S] on the device, or
    a host list).  store(rows, res, obs, a, r, o2, d) keeps a step's transitions (rows: their arena indices, None for
    all; res: the env's step result); the default pushes them ragged into ``ring``, a ``PopulationRing``."""

    def __init__(self, env, bank, mix, ring, explorer, members, rows_per_member, episode_end="max_steps", store=None):
        if episode_end not in ("max_steps", "done"):
            raise ValueError("episode_end must be 'max_steps' or 'done'")
        self.env, self.mix, self.ring, self.explorer = env, mix, ring, explorer
        self.S, self.n = len(members), int(rows_per_member)
        self.N, self.device = self.S * self.n, torch.device(ring.device)
        self.stop_at_done = episode_end == "done"
        self.member_of = torch.arange(self.N, device=self.device) // self.n  # [N] int64
        self.act8 = torch.zeros((self.N, 8), device=self.device)
        self.keep = store  # None: push (not bound here: the collector would hold a cycle to itself)

    def push(self, rows, res, *row):
        """The default ``store``: the ragged push over the members; returns the rows' members."""
        m = self.member_of if rows is None else self.member_of[rows]
        self.ring.push(m, *row)
        return m

    # ------------------------------------------------------------------ a round
    def begin_round(self, obs, obs2, max_steps):
        """Start a round of at most ``max_steps`` steps from the reset observations."""
        self.obs, self.obs2, self.max_steps = obs, obs2, int(max_steps)
        self.ep_reward = torch.zeros(self.N, device=self.device)
        self.alive = torch.ones(self.N, dtype=torch.bool, device=self.device)  # episode_end="done": not yet done
        self.n_alive, self.steps, self.count = [self.n] * self.S, [0] * self.S, None

    def run_round(self):
        """``step()`` until ``max_steps`` or, under episode_end="done", until nobody is alive."""
        for _ in range(self.max_steps):
            self.step()
            if not any(self.n_alive):
                break

    def end_round(self, actors=None, episodes=0):
        """Close the round through the mix's round-end fold (the snapshots precede the updates).  Returns (arena-steps
        per member as a list, ep_reward [N] on the device, one opponent dict per member: a ``PopulationOpponentMix``'s
        own, or S times the one of an ``OpponentMix`` over all arenas)."""
        if hasattr(self.mix, "pools"):
            opp = self.mix.end_round(actors, episodes)
        else:  # one pool at most, which follows the only member there is
            opp = [self.mix.end_round(actors[0] if actors and self.S == 1 else None, episodes)] * self.S
        return self.steps, self.ep_reward, opp

    # ------------------------------------------------------------------ one step
    def step(self):
        """One collection step of every arena; returns the env's step result."""
        a = self.explorer.explore(self.obs, self.act8, 0, count=self.count)[:, :4]
        policy2 = self.draw()
        res = self.env.step(self.act8, with_agent_two=True, policy2=policy2)
        self.store(a, res)
        return res

    def draw(self):
        """Player 2's draw for this step; returns ``policy2``.  Every mix is asked to write the self-play arenas'
        actions into ``act8[:, 4:]``; one that returns actions of its own (one snapshot per step) has them copied."""
        policy2, a2, _ = self.mix.select(self.obs2, out=self.act8)
        if a2 is not None and a2 is not self.act8:
            self.act8[:, 4:] = a2
        return policy2

    def store(self, a, res):
        """The step's transitions (``obs``, a, reward, next obs, done) of the running arenas into the store, the
        bookkeeping, the survivors, and ``obs`` / ``obs2`` := the step's.  Its three parts can be called one by one."""
        row = self.clones(res)
        self.store_rows(a, res, *row[:3])
        if self.stop_at_done:
            self.survivors()
        self.obs, self.obs2 = row[0], row[3]

    def clones(self, res):  # (next obs, reward, done, next obs2): the next step overwrites the result's buffers
        return res.obs.clone(), res.reward.clone(), res.done.clone(), res.obs2.clone()

    def store_rows(self, a, res, o2, r, d):
        for j in range(self.S):
            self.steps[j] += self.n_alive[j]
        store_step(self.keep or self.push, self.mix, self.stop_at_done, self.alive, self.ep_reward, res, self.obs, a, r,
                   o2, d)

    def survivors(self):  # episode_end="done": the running arenas per member, the step's one host sync
        left = self.alive.view(self.S, self.n)
        count_t = left.sum(1, dtype=torch.int32) if self.explorer.count_on_device else None
        self.n_alive = left.sum(1).tolist()
        self.count = self.n_alive if count_t is None else count_t

"""Player-2 opponents of the batched TD3 loop (BASELINE config C5).

Batched form of the reference's opponent machinery, device-resident and free of per-step host syncs:

* ``CURRICULA`` -- the stage tables of rl/training/curricula.py: rows (progress threshold, P(strong bot),
  P(weak bot), P(self-play)); ``OpponentMix.update_schedule`` picks the first row whose threshold exceeds
  the training progress (opponent_manager.py:38-51).
* ``SelfPlayPool`` -- rl/training/self_play.py:20-68: frozen actor snapshots taken every ``interval``
  episodes, at most ``pool_size`` kept (oldest dropped), a difficulty score per snapshot (start 1.0, x1.2 on
  an outcome that is not an agent win, x0.95 on a win, clipped to [0.1, 10]) and score-weighted sampling.
* ``OpponentMix.select`` -- opponent_manager.py:62-91, per arena and per step: with probability P(self-play)
  (only once the pool holds a snapshot) the opponent is the snapshot sampled for this step, evaluated as
  ONE batched ``PolicyOpponent`` forward (hockey_env.py:908-922) over every arena's agent-two observation;
  otherwise a second draw picks the strong bot below P(strong) and the weak bot above it.  The choice goes
  to the kernel as ``hk_step_io.policy2`` (external for self-play arenas, whose actions fill
  ``actions[:, 4:8]``; the fused BasicOpponent for the bots, each bot kind with its own phase, as the
  reference's manager holds one ``BasicOpponent`` of each kind).

Batched differences (by design, documented): the draws come from a torch generator on the device instead of
the process-global ``np.random``; under ``sampling="step"`` (the default) the snapshot is sampled once per step
for all arenas (the reference samples one per step for its single env); ``register_outcome`` counts the done
steps of self-play arenas against the snapshot they faced (the reference charges the last sampled snapshot for
every done step of any opponent), tallied per step on the device and folded into the scores step by step at the
end of the round (within one step, the non-win outcomes are applied before the wins; clipping follows every
outcome as in the reference).

``sampling="arena"`` removes the snapshot difference: every self-play arena draws its OWN snapshot at every step,
score-weighted (``torch.multinomial`` on the mix's device generator), as the reference does for every env-step of
its single env (opponent_manager.py:62-91, self_play.py).  The pool mirrors its snapshots into a
``hockey_amd.policy_bank.PolicyBank`` and ONE ``PolicyBank.act`` call (``hkl_act`` on the GPU: rows grouped by
snapshot on the device) writes the self-play arenas' actions into ``actions[:, 4:8]``; there is no forward per
pool member and no mask multiply.  Each done step is charged to the snapshot that arena faced at that step, as a
per-step [pool][2] scatter-add on the device; ``end_round`` folds the steps in order (the snapshots' scores do
not depend on each other, so the order across snapshots within a step is immaterial).

``PopulationOpponentMix`` is the same for ``hockey_amd.population.train_population``: one pool per member, all of
them in one wide PolicyBank, one ``select`` and one acting call per step for the whole population.
"""
import copy
import math

import numpy as np
import torch

from . import _native as N

# rl/training/curricula.py (threshold, strong, weak, self_play)
CURRICULA = {
    "stage1": [(1.00, 0.00, 1.00, 0.00)],
    "stage2": [(0.33, 0.55, 0.45, 0.00), (0.66, 0.45, 0.45, 0.10), (1.00, 0.50, 0.40, 0.10)],
    "stage3": [(0.15, 0.30, 0.70, 0.00), (0.70, 0.60, 0.30, 0.10), (1.00, 0.35, 0.35, 0.30)],
    "noise_study": [(1.0, 0.5, 0.5, 0.0)],
}
CURRICULA["ablation"] = CURRICULA["stage2"]

SCORE_MIN, SCORE_MAX, SCORE_LOSS, SCORE_WIN = 0.1, 10.0, 1.2, 0.95


class SelfPlayPool:
    """Frozen actor snapshots with difficulty scores (rl/training/self_play.py)."""

    def __init__(self, interval=100, pool_size=40, seed=0, bank=None):
        """bank: a PolicyBank with at least ``pool_size`` + 1 slots that mirrors the snapshots (``slots[i]`` is the
        bank slot of ``pool[i]``; a dropped snapshot's slot is freed)."""
        self.interval, self.pool_size = int(interval), int(pool_size)
        self.episode_counter = 0
        self.pool, self.scores = [], []
        self.bank, self.slots = bank, []
        self.rng = np.random.default_rng(seed)

    def step(self, actor, episodes=1):
        """Count `episodes` finished training episodes; snapshot the actor when an interval boundary is crossed
        (at most one snapshot per call: a batched round crosses several boundaries with the same weights)."""
        if self.advance(episodes):
            self.add_snapshot(actor)

    def advance(self, episodes):
        """Count ``episodes`` finished training episodes; True when an interval boundary was crossed."""
        before = self.episode_counter // self.interval
        self.episode_counter += int(episodes)
        return self.episode_counter // self.interval > before

    def add_snapshot(self, actor, slot=None):
        """Append a frozen copy of ``actor`` (score 1.0) and drop the oldest snapshot past ``pool_size``, freeing its
        bank slot.  slot: the bank slot the caller chose and writes itself (default: the bank's first free slot,
        written here).  Returns the copy."""
        snap = copy.deepcopy(actor).eval()
        for p in snap.parameters():
            p.requires_grad_(False)
        self.pool.append(snap)
        self.scores.append(1.0)
        if self.bank is not None:
            self.slots.append(self.bank.add(snap) if slot is None else slot)
        if len(self.pool) > self.pool_size:
            self.pool.pop(0)
            self.scores.pop(0)
            if self.bank is not None:
                self.bank.free(self.slots.pop(0))
        return snap

    def update_difficulty(self, idx, wins, others):
        """One step's outcomes against snapshot ``idx``: ``others`` outcomes that are not agent wins (x1.2 each)
        then ``wins`` agent wins (x0.95 each), clipped to [0.1, 10] after EVERY outcome as the reference does
        (self_play.py:45-55).  Both runs are monotone, so clipping after each factor equals clipping the run's
        product once: min(10, s * 1.2^others), then max(0.1, s * 0.95^wins)."""
        s = self.scores[idx]
        if others:
            s = min(SCORE_MAX, math.exp(min(math.log(s) + others * math.log(SCORE_LOSS), 50.0)))
        if wins:
            s = max(SCORE_MIN, math.exp(math.log(s) + wins * math.log(SCORE_WIN)))
        self.scores[idx] = float(np.clip(s, SCORE_MIN, SCORE_MAX))

    def sample(self):
        """Score-weighted snapshot index (get_opponent), or None with an empty pool."""
        if not self.pool:
            return None
        w = np.asarray(self.scores, np.float64)
        return int(self.rng.choice(len(self.pool), p=w / w.sum()))

    def __len__(self):
        return len(self.pool)


def _draw(mix, can_sp):
    """A step's bot-or-self-play draw for OpponentMix and PopulationOpponentMix: ``u_sp`` and then ``u_bot`` from
    ``mix.gen``, self-play where u_sp < P(self-play) and ``can_sp`` allows it (a bool, or [N] bool on the device),
    else the strong bot below P(strong) and the weak one above.  Fills ``mix._policy2``, adds the arena counts to
    ``mix._counts`` ([rows, 3], the arenas split evenly over the rows) and returns the self-play mask."""
    n, dev = mix.n, mix.device
    u_sp = torch.rand(n, device=dev, generator=mix.gen)
    u_bot = torch.rand(n, device=dev, generator=mix.gen)
    if torch.is_tensor(can_sp):
        sp = (u_sp < mix.p_self) & can_sp
    else:
        sp = (u_sp < mix.p_self) if can_sp else torch.zeros(n, dtype=torch.bool, device=dev)
    strong = ~sp & (u_bot < mix.p_strong)
    weak = ~sp & ~strong
    p2 = mix._policy2
    p2.fill_(N.POLICY_BASIC_WEAK)
    p2.masked_fill_(strong, N.POLICY_BASIC_STRONG)
    p2.masked_fill_(sp, N.POLICY_EXTERNAL)
    mix._counts += torch.stack([strong, weak, sp]).view(3, mix._counts.shape[0], -1).sum(2).t()
    mix._sp_mask = sp
    return sp


def _bank_act(mix, obs2, policy, out):
    """One ``PolicyBank.act`` for the step's self-play arenas into ``out[:, 4:8]`` (``out``: the caller's [N, 8]
    action buffer, or one kept by the mix); returns the buffer."""
    if out is None:
        if getattr(mix, "_act8", None) is None:
            mix._act8 = torch.zeros((mix.n, 8), dtype=torch.float32, device=mix.device)
        out = mix._act8
    mix.bank.act(obs2, policy, out=out, out_col=4, backend=mix.backend)
    return out


def _outcomes(mix, done, reward):
    """(agent wins, other outcomes) of this step's self-play arenas as [N] int64 masks."""
    d = (done != 0) & mix._sp_mask
    win = d & (reward > 0)
    return win.to(torch.int64), (d & ~win).to(torch.int64)


def _tally(mix, done, reward, size):
    """A step's outcomes charged to the snapshot each arena faced (``mix._snap``): [size][wins, others] int64."""
    tally = torch.zeros((size, 2), dtype=torch.int64, device=mix.device)
    for col, hit in enumerate(_outcomes(mix, done, reward)):
        tally[:, col].scatter_add_(0, mix._snap, hit)
    return tally


class OpponentMix:
    """Per-arena, per-step opponent selection for player 2 (rl/training/opponent_manager.py)."""

    def __init__(self, n_arenas, curriculum="stage3", use_self_play=True, self_play_interval=100, pool_size=40,
                 device="cuda:0", seed=0, sampling="step", backend="auto"):
        """sampling: "step" -- one snapshot per step for all self-play arenas; "arena" -- one per arena and step,
        through a PolicyBank (module docstring; ``backend`` is its ``act`` backend)."""
        if sampling not in ("step", "arena"):
            raise ValueError("sampling must be 'step' or 'arena'")
        self.n = int(n_arenas)
        self.device = torch.device(device)
        self.sampling, self.backend = sampling, backend
        self.table = CURRICULA[curriculum] if isinstance(curriculum, str) else [tuple(r) for r in curriculum]
        self.bank = None
        if use_self_play and sampling == "arena":
            from .policy_bank import PolicyBank

            # one slot more than the pool keeps: a new snapshot is added before the oldest is dropped
            self.bank = PolicyBank(int(pool_size) + 1, self.device)
        self.pool = SelfPlayPool(self_play_interval, pool_size, seed, self.bank) if use_self_play else None
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed) + 0x5EED)
        self.p_strong, self.p_weak, self.p_self = 0.0, 1.0, 0.0
        self.update_schedule(0.0)
        self._policy2 = torch.empty(self.n, dtype=torch.uint8, device=self.device)
        self.reset_stats()

    def update_schedule(self, progress):
        for threshold, strong, weak, self_play in self.table:
            if progress < threshold:
                if strong + weak + self_play <= 0:
                    raise ValueError("Bot probabilities must sum to > 0")
                self.p_strong, self.p_weak, self.p_self = strong, weak, self_play
                return

    def reset_stats(self):
        self._counts = torch.zeros((1, 3), dtype=torch.int64, device=self.device)  # strong, weak, self-play
        self._outcomes = []  # per step: device tensor [snapshot index, wins, others] ("arena": [pool][wins, others])
        if self.bank is not None:  # arena-steps each snapshot (by pool index) was faced in this round
            self._snap_counts = torch.zeros(self.pool.pool_size, dtype=torch.int64, device=self.device)
        self._snap = None

    def _pool_tensors(self):
        """The pool's scores and bank slots on the device, rebuilt when either changed on the host."""
        key = (tuple(self.pool.scores), tuple(self.pool.slots))
        if getattr(self, "_pool_key", None) != key:
            self._pool_key = key
            self._scores_t = torch.tensor(self.pool.scores, dtype=torch.float32, device=self.device)
            self._slots_t = torch.tensor(self.pool.slots, dtype=torch.int32, device=self.device)
        return self._scores_t, self._slots_t

    def _select_arena(self, obs2, out):
        """sampling="arena": (policy2 [N] uint8, actions [N,8] or None, bank slot per arena [N] int32 or None).
        The self-play arenas' player-2 actions are written into ``out[:, 4:8]`` (``out``: the caller's [N,8] action
        buffer, or one kept here); every other float of it is left alone."""
        dev = self.device
        sp = _draw(self, len(self.pool) > 0)
        p2, self._snap = self._policy2, None
        if not len(self.pool):
            return p2, None, None
        scores, slots = self._pool_tensors()
        snap = torch.multinomial(scores, self.n, replacement=True, generator=self.gen)  # pool index per arena
        policy = torch.where(sp, slots[snap], torch.full((), -1, dtype=torch.int32, device=dev))
        out = _bank_act(self, obs2, policy, out)
        self._snap = snap
        self._snap_counts.scatter_add_(0, snap, sp.to(torch.int64))
        return p2, out, policy

    def select(self, obs2, out=None):
        """(policy2 [N] uint8, player-2 actions [N,4] or None, snapshot index or None) for this step.
        obs2: [N,18] agent-two observations (device).  sampling="arena": see _select_arena (``out`` is used by
        that mode only)."""
        if self.sampling == "arena" and self.pool is not None:
            return self._select_arena(obs2, out)
        idx = self.pool.sample() if self.pool is not None else None  # numpy's draw precedes the device draws
        sp = _draw(self, idx is not None)
        act = None
        if idx is not None:
            with torch.no_grad():
                act = self.pool.pool[idx](obs2)  # one batched PolicyOpponent forward for the step
            act = act * sp.unsqueeze(1)
        self._idx = idx
        return self._policy2, act, idx

    def register_outcomes(self, done, reward):
        """Done steps of this step's self-play arenas: agent win (reward > 0) or not (opponent_manager
        register_outcome -> update_difficulty).  Tallied per step on the device; end_round() applies the steps in
        order, clipping after every outcome."""
        if self.bank is not None:
            if self._snap is not None:
                self._outcomes.append(_tally(self, done, reward, self.pool.pool_size))
        elif self._idx is not None:
            win, other = _outcomes(self, done, reward)
            self._outcomes.append(torch.stack([torch.full((), self._idx, dtype=torch.int64, device=self.device),
                                               win.sum(), other.sum()]))

    def end_round(self, actor=None, episodes=0):
        """Fold the round's outcomes into the snapshot scores, advance the self-play episode counter (taking a
        snapshot on an interval boundary) and return the round's opponent counts."""
        counts = self._counts[0].cpu().tolist()
        out = {"strong": counts[0], "weak": counts[1], "self_play": counts[2]}
        if self.pool is not None:
            if self.bank is not None:
                out["snapshots"] = self._snap_counts[:len(self.pool)].cpu().tolist()
                if self._outcomes:
                    for step in torch.stack(self._outcomes).cpu().tolist():
                        for idx, (w, o) in enumerate(step[:len(self.pool)]):
                            if w or o:
                                self.pool.update_difficulty(idx, w, o)
            elif self._outcomes:
                for idx, w, o in torch.stack(self._outcomes).cpu().tolist():
                    if idx < len(self.pool) and (w or o):
                        self.pool.update_difficulty(idx, w, o)
            if actor is not None and episodes:
                self.pool.step(actor, episodes)
        self.reset_stats()
        return out


class PopulationOpponentMix:
    """``OpponentMix`` for a population (``hockey_amd.population.train_population(self_play=...)``): member j owns
    arenas [j n, (j + 1) n) and, if its config has ``use_self_play``, its own ``SelfPlayPool`` -- interval and size
    from its config, seeded by its seed, scores and snapshots its own.  All pools mirror into ONE wide ``PolicyBank``
    of S x (Pmax + 1) slots (Pmax: the largest pool size; member j's slots lie in [j (Pmax + 1), (j + 1) (Pmax + 1)))
    and one ``PolicyBank.act`` call per step acts for every self-play arena of every member (``hkl_act_wide`` on the
    GPU once the bank exceeds 64 slots).  The curriculum row is shared: the members share ``curriculum_name``
    (``curriculum``: a name or a table, default the first member's).

    The bot-or-self-play draws are ``OpponentMix``'s (``_draw``), from one generator over the population (seeded
    by the first member's seed); an arena can draw self-play only if its member uses it and that member's pool
    holds a snapshot, otherwise it falls through to the bots.  sampling="arena": every arena draws its snapshot from
    its own member's scores (one 2-D ``torch.multinomial`` over the [S, Pmax] score matrix; empty rows carry a dummy
    weight and are masked out).  sampling="step": one snapshot per member and step.  Nothing is read back per step."""

    update_schedule = OpponentMix.update_schedule

    def __init__(self, members_cfg, seeds, n_arenas_per_member, device="cuda:0", sampling="arena", backend="auto",
                 curriculum=None):
        if sampling not in ("step", "arena"):
            raise ValueError("sampling must be 'step' or 'arena'")
        cfgs, seeds = list(members_cfg), [int(s) for s in seeds]
        if not cfgs or len(cfgs) != len(seeds):
            raise ValueError("one seed per member config")
        self.S, self.n_per = len(cfgs), int(n_arenas_per_member)
        self.n = self.S * self.n_per
        self.device = dev = torch.device(device)
        self.sampling, self.backend = sampling, backend
        curriculum = cfgs[0].curriculum_name if curriculum is None else curriculum
        self.table = CURRICULA[curriculum] if isinstance(curriculum, str) else [tuple(r) for r in curriculum]
        self.pools = [SelfPlayPool(c.self_play_interval, c.self_play_pool_size, s) if c.use_self_play else None
                      for c, s in zip(cfgs, seeds)]
        self.pmax = max([p.pool_size for p in self.pools if p is not None] + [1])
        self.stride = self.pmax + 1  # one slot more than a pool keeps: a snapshot is added before the oldest leaves
        self.bank = None
        if any(p is not None for p in self.pools):
            from .policy_bank import PolicyBank

            self.bank = PolicyBank(self.S * self.stride, dev, wide=True)
            for p in self.pools:
                if p is not None:
                    p.bank = self.bank  # the pool frees its dropped snapshots' slots; snapshot() picks the new ones
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seeds[0] + 0x5EED)
        self.p_strong, self.p_weak, self.p_self = 0.0, 1.0, 0.0
        self.update_schedule(0.0)
        self.member_of = torch.arange(self.n, device=dev) // self.n_per  # [N] int64
        self._policy2 = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self._minus1 = torch.full((), -1, dtype=torch.int32, device=dev)
        self._pool_key = None
        self.reset_stats()

    # ------------------------------------------------------------------ pools
    def pool_sizes(self):
        return [len(p) if p is not None else 0 for p in self.pools]

    def snapshot(self, members, actors):
        """Append a snapshot of ``actors[i]`` to member ``members[i]``'s pool (score 1.0; the oldest is dropped past
        the pool size and its slot freed for reuse); all bank slots are written by one ``replace_many``."""
        slots, snaps = [], []
        for j, actor in zip(members, actors):
            pool = self.pools[j]
            if pool is None:
                raise ValueError(f"member {j} does not use self-play")
            lo = j * self.stride
            slots.append(next(k for k in range(lo, lo + pool.pool_size + 1) if k not in pool.slots))
            snaps.append(pool.add_snapshot(actor, slots[-1]))
        if slots:
            self.bank.replace_many(slots, snaps)

    def _pool_tensors(self):
        """([S, Pmax] scores with a dummy weight in empty rows, [S, Pmax] bank slots, [S] bool: the member can draw
        self-play) on the device, rebuilt when a pool changed on the host."""
        key = tuple((tuple(p.scores), tuple(p.slots)) if p is not None else None for p in self.pools)
        if self._pool_key != key:
            self._pool_key = key
            scores = np.zeros((self.S, self.pmax), np.float32)
            slots = np.full((self.S, self.pmax), -1, np.int32)
            have = np.zeros(self.S, bool)
            for j, p in enumerate(self.pools):
                if p is not None and len(p):
                    scores[j, :len(p)] = p.scores
                    slots[j, :len(p)] = p.slots
                    have[j] = True
                else:
                    scores[j, 0] = 1.0  # never used: the row's arenas cannot draw self-play
            self._any = bool(have.any())
            self._scores_t = torch.from_numpy(scores).to(self.device)
            self._slots_t = torch.from_numpy(slots).to(self.device)
            self._have_t = torch.from_numpy(have).to(self.device)
        return self._scores_t, self._slots_t, self._have_t

    # ------------------------------------------------------------------ per step
    def reset_stats(self):
        dev = self.device
        self._counts = torch.zeros((self.S, 3), dtype=torch.int64, device=dev)  # per member: strong, weak, self-play
        self._snap_counts = torch.zeros(self.S * self.pmax, dtype=torch.int64, device=dev)
        self._outcomes = []  # per step: [S * Pmax][wins, others]
        self._snap = None

    def select(self, obs2, out=None):
        """(policy2 [N] uint8, actions [N, 8] or None, bank slot per arena [N] int32 or None) for this step.  The
        self-play arenas' player-2 actions are written into ``out[:, 4:8]`` (``out``: the caller's [N, 8] action
        buffer, or one kept here); every other float of it is left alone."""
        n, S = self.n, self.S
        scores, slots, have = self._pool_tensors()
        sp = _draw(self, have[self.member_of])
        p2, self._snap = self._policy2, None
        if not self._any:
            return p2, None, None
        if self.sampling == "arena":  # pool index per arena, from the arena's own member's scores
            snap = torch.multinomial(scores, self.n_per, replacement=True, generator=self.gen).reshape(n)
        else:  # one per member and step
            snap = torch.multinomial(scores, 1, generator=self.gen).expand(S, self.n_per).reshape(n)
        policy = torch.where(sp, slots[self.member_of, snap], self._minus1)
        out = _bank_act(self, obs2, policy, out)
        self._snap = self.member_of * self.pmax + snap  # the (member, snapshot) each arena faces, flat
        self._snap_counts.scatter_add_(0, self._snap, sp.to(torch.int64))
        return p2, out, policy

    def register_outcomes(self, done, reward):
        """Done steps of this step's self-play arenas, charged to the (member, snapshot) the arena faced: agent win
        (reward > 0) or not.  Tallied on the device; end_round() applies the steps in order."""
        if self._snap is not None:
            self._outcomes.append(_tally(self, done, reward, self.S * self.pmax))

    def end_round(self, actors=None, episodes=0):
        """Per member: fold the round's outcomes, in step order, through its pool's ``update_difficulty``, advance its
        pool by ``episodes`` (an int, or one per member) and snapshot ``actors[j]`` where an interval boundary was
        crossed -- all crossing members in one ``replace_many``.  Returns one dict per member: its "strong" / "weak" /
        "self_play" arena-steps and "snapshots", the arena-steps per snapshot of its pool (empty without a pool)."""
        S, P = self.S, self.pmax
        counts = self._counts.cpu().tolist()
        faced = self._snap_counts.view(S, P).cpu().tolist()
        out = []
        for j, pool in enumerate(self.pools):
            out.append({"strong": counts[j][0], "weak": counts[j][1], "self_play": counts[j][2],
                        "snapshots": faced[j][:len(pool)] if pool is not None else []})
        if self._outcomes:
            steps = torch.stack(self._outcomes).cpu().numpy()  # [T][S * P][2]
            for t, idx in zip(*np.nonzero(steps.any(-1))):  # row-major: the steps in order
                j, i = divmod(int(idx), P)
                pool = self.pools[j]
                if pool is not None and i < len(pool):
                    pool.update_difficulty(i, int(steps[t, idx, 0]), int(steps[t, idx, 1]))
        if actors is not None:
            eps = list(episodes) if isinstance(episodes, (list, tuple)) else [episodes] * S
            crossed = [j for j, pool in enumerate(self.pools) if pool is not None and eps[j] and pool.advance(eps[j])]
            self.snapshot(crossed, [actors[j] for j in crossed])
        self.reset_stats()
        return out

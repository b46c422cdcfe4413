"""Population TD3: up to 64 independent agents trained in one process on grouped learner kernels.

A seed study runs the same small job many times: one ``hockey_amd.td3.train`` per (config, seed) on 4-20 arenas at the
reference's learner batch of 256, where the fused learner's kernels launch 4 workgroups each on a 256-CU chip.  Here
the S members share every launch instead:

* ``PopulationLearner`` -- one ``FusedLearner`` per member (flat parameter buffers, Adam state, operand packs and
  fixed-pointer io structs, all unchanged); their structs are gathered into host arrays, uploaded once, and every call
  of ``FusedLearner.update`` is replaced by its ``_group`` form (include/hockey_learner.h): member m runs in slice m of
  the grid.  An update is 5 (+ 4 on actor updates) launches whatever S is, and member m's results are bit for bit
  those of its own FusedLearner, whatever the other members are.  Members with prioritized replay draw through
  ``hkl_per_sample_group`` and write their priorities back through ``hkl_per_update_group`` (three launches each):
  an all-prioritized update is 10 (+ 4) launches, a mixed one 11 (+ 4).
* ``PopulationRing`` -- the S replay rings in one storage, filled by one ragged push per step;
  ``PopulationPrioritizedRing`` adds the device sampler's weights and block sums per member (GPU only).
* ``train_population`` -- ``hockey_amd.td3.train`` for S members side by side: one VecHockeyEnv of S x n arenas, one
  ``hkl_act`` launch per step through a PolicyBank, one OpponentMix, one grouped learner.  With ``self_play=`` the
  members keep their own self-play pools in one ``PopulationOpponentMix`` over a wide PolicyBank (``hkl_act_wide``).

What is and is not composition-independent: the LEARNER is -- its slots and target noise come from each member's own
Philox stream (seeded by the agent's seed), its arithmetic from the member's own grid slice.  COLLECTION is not: the
exploration noise, the random-phase actions and the opponent draws come from torch generators shared by the
population, and the step kernel's device draws are keyed by the global arena id, so a member's trajectory depends on
its position in the population and on who else is in it.  ``train_population(explore="device")`` takes the exploration
out of that list: hockey_amd.explore keys each member's draws by its own seed, its arenas' indices inside the member and
its own call counter.  ``train_population(collect="device")`` takes the rest: hockey_amd.collect keys the opponent
draws and the bots' phases the same way and supplies the step kernel's draws, so that member j's whole run -- its
trajectories, replay ring and weights -- is the same bits alone and inside a population of 64.
"""
import ctypes
import dataclasses

import torch

from . import learner_hip as LH
from .constants import Mode
from .learner_hip import GROUP_MAX
from .host_round import PopulationExplorer, TorchCollector, check_collect_args
from .td3 import TD3, Learner, PairRunner, PerBlocks, ReplayRing, RoundClock, reset_round, updates_for


# ---------------------------------------------------------------------------------------------------- replay
class _MemberRing(ReplayRing):
    """Member j's slice of a PopulationRing with ReplayRing's attributes (views; the fill level is a 0-d view of
    the population's [S] tensor).  Filled through PopulationRing.push only."""

    def __init__(self, pop, j):  # noqa: super().__init__ would allocate
        lo, hi = j * pop.cap, (j + 1) * pop.cap
        self.cap, self.device = pop.cap, pop.device
        self.s, self.a, self.r, self.s2, self.d = pop.s[lo:hi], pop.a[lo:hi], pop.r[lo:hi], pop.s2[lo:hi], pop.d[lo:hi]
        self.size_t = pop.size_t[j]

    size = property(lambda self: int(self.size_t))  # one host sync

    def push(self, *a):
        raise RuntimeError("a PopulationRing member is filled through PopulationRing.push")


class PopulationRing:
    """S uniform FIFO replay rings (hockey_amd.td3.ReplayRing) of ``capacity`` slots each in one storage
    [S * capacity, ...] per column; fill levels and write positions live on the device ([S] int64)."""

    def __init__(self, S, capacity, device="cuda:0", n_obs=18, n_act=4):
        self.S, self.cap = int(S), int(capacity)
        d = self.device = torch.device(device)
        n = self.S * self.cap
        self.s = torch.zeros((n, n_obs), device=d)
        self.a = torch.zeros((n, n_act), device=d)
        self.r = torch.zeros(n, device=d)
        self.s2 = torch.zeros((n, n_obs), device=d)
        self.d = torch.zeros(n, device=d)
        self.size_t = torch.zeros(self.S, dtype=torch.int64, device=d)
        self.pos_t = torch.zeros(self.S, dtype=torch.int64, device=d)
        self._members = [self._make_member(j) for j in range(self.S)]
        self._ar = torch.arange(self.S, device=d)

    def _make_member(self, j):
        return _MemberRing(self, j)

    def member(self, j):
        return self._members[j]

    def push(self, member_of_row, s, a, r, s2, d):
        """Store a ragged batch: row i goes to member ``member_of_row[i]`` ([n] int64 on the device), any number of
        rows per member (none included), at most ``capacity`` rows in all.  The contents and the wrap-around are
        those of S ``ReplayRing.push`` calls in member order (a member's rows keep their order); the number of
        launches does not depend on S and nothing is read back."""
        n = int(member_of_row.shape[0])
        if n > self.cap:
            raise ValueError(f"push of {n} transitions exceeds the ring capacity {self.cap}")
        if n == 0:
            return
        m = member_of_row.long()
        onehot = (m[:, None] == self._ar[None, :]).to(torch.int64)  # [n, S]
        rank = (torch.cumsum(onehot, 0) - 1).gather(1, m[:, None]).squeeze(1)  # the row's index among its member's
        dst = m * self.cap + (self.pos_t[m] + rank) % self.cap
        self.s[dst] = s
        self.a[dst] = a
        self.r[dst] = r.float()
        self.s2[dst] = s2
        self.d[dst] = d.float()
        counts = onehot.sum(0)
        self._before_commit(counts, n)
        self.pos_t.copy_((self.pos_t + counts) % self.cap)
        self.size_t.copy_(torch.clamp(self.size_t + counts, max=self.cap))

    def _before_commit(self, counts, n):
        """Called by push with the per-member row counts ([S] int64 on the device) and the push's rows, while pos_t
        and size_t still hold the values before the push."""


class _MemberPrioritizedRing(_MemberRing):
    """Member j of a PopulationPrioritizedRing with the attributes FusedLearner reads off a
    hockey_amd.td3.DevicePrioritizedRing: ``per`` onto the member's slices, ``w``, ``beta``, ``last``."""

    prioritized = True
    device_sampler = True

    def __init__(self, pop, j):
        super().__init__(pop, j)
        nb = pop.nblk
        self.beta = pop.beta[j]
        self.w = pop.w[j * pop.wstride:j * pop.wstride + pop.cap]
        self._bsum, self._bpre, self._bmax = (t[j * nb:(j + 1) * nb] for t in (pop.bsum, pop.bpre, pop.bmax))
        self._last, self._bown = pop.last[j * pop.cap:(j + 1) * pop.cap], pop.bown[j * nb:(j + 1) * nb]
        self.last = torch.zeros(1, dtype=torch.long, device=pop.device)
        self.per = pop.pers[j]


class PopulationPrioritizedRing(PopulationRing):
    """PopulationRing whose members carry prioritized replay's weights (hockey_amd.td3.DevicePrioritizedRing, S of
    them): one storage per array of the sampler -- ``w`` [S * wstride], ``bsum`` / ``bpre`` / ``bmax`` [S * nblk],
    ``last`` [S * capacity], ``bown`` [S * nblk] -- driven by the hkl_per_*_group kernels (include/hockey_learner.h).
    wstride is the capacity rounded up to 4 floats, so that every member's weights start 16-byte aligned (the
    kernels read a block as float4); the padding is never addressed.  GPU only.

    ``prioritized``: one bool per member (default all true); a member with False is a plain uniform member
    (``member(j).prioritized`` is False) whose weights are pushed but never read.  ``beta``: a scalar or one value
    per member.  ``push`` is PopulationRing's ragged push plus ONE hkl_per_push_group over all S members: the write
    positions, the per-member row counts and the fill levels after the push are taken on the device, nothing is read
    back, and member j's weights and block sums are those of DevicePrioritizedRing.push of its rows.  Code that
    stores to ``w`` itself calls ``refresh()`` afterwards."""

    def __init__(self, S, capacity, prioritized=None, beta=0.15, init_weight=1e8, device="cuda:0", n_obs=18, n_act=4):
        from . import _native

        if torch.device(device).type != "cuda":
            raise _native.HockeyNativeError("the device prioritized replay sampler runs on the GPU only")
        self._L = LH.lib()
        S = int(S)
        self.prioritized = [True] * S if prioritized is None else [bool(x) for x in prioritized]
        self.beta = [float(x) for x in (beta if isinstance(beta, (list, tuple)) else [beta] * S)]
        if len(self.prioritized) != S or len(self.beta) != S:
            raise ValueError("prioritized and beta take one value per member")
        if not 1 <= S <= GROUP_MAX:
            raise ValueError(f"a population has 1 to {GROUP_MAX} members, got {S}")
        cap = int(capacity)
        d = torch.device(device)
        self.wstride = -(-cap // 4) * 4
        self.w = torch.full((S * self.wstride,), float(init_weight), device=d)
        self.pers = None
        super().__init__(S, cap, device=d, n_obs=n_obs, n_act=n_act)  # builds the members through _make_member
        # the push's device arguments: fixed buffers, so that the launch reads what this push computed
        self._push_args = torch.zeros((3, S), dtype=torch.int64, device=d)
        self.refresh()

    def _make_member(self, j):
        if self.pers is None:  # the first member: the fill levels exist by now
            blk = self._blocks = PerBlocks(self.S, self.cap, self.w, self.wstride, self.size_t)
            self.nblk, self.pers = blk.nblk, blk.pers
            self.bsum, self.bpre, self.bmax, self.last, self.bown = blk.buffers
            self._pers_dev = LH.upload(self.pers, self.device)
        return _MemberPrioritizedRing(self, j) if self.prioritized[j] else _MemberRing(self, j)

    def refresh(self):
        """Recompute every member's block sums and maxima from ``w`` and the fill levels."""
        LH.check(self._L.hkl_per_refresh_group(self.pers, self._pers_dev.data_ptr(), self.S,
                                               LH.stream_ptr(self.device)), "hkl_per_refresh_group")

    def _before_commit(self, counts, n):
        # hkl_per_push per member, before the fill levels change: the pushed blocks' sums are taken against the
        # fill level after the push, which is passed (PopulationRing.push stores it next)
        a = self._push_args
        a[0].copy_(self.pos_t)
        a[1].copy_(counts)
        torch.clamp(self.size_t + counts, max=self.cap, out=a[2])
        p = a.data_ptr()
        LH.check(self._L.hkl_per_push_group(self.pers, self._pers_dev.data_ptr(), p, p + 8 * self.S, p + 16 * self.S,
                                            min(int(n), self.cap), self.S, LH.stream_ptr(self.device)),
                 "hkl_per_push_group")


# ---------------------------------------------------------------------------------------------------- learner
class PopulationLearner(PairRunner):
    """Learner updates of S = len(agents) <= 64 TD3 agents, agent j on rings[j], at batch ``batch`` in the launches
    one agent takes (module docstring).  rng is "device" only: each member's slots and target noise come from its own
    Philox stream, keyed by its agent's seed.  Members may differ in seed, lr_q, lr_pol, wd_*, gamma, tau_* and the
    target-noise scale / clip; batch_size, policy_update_freq (2) and the hidden width (256) must be equal.  A ring
    may be a prioritized member of a PopulationPrioritizedRing (the device sampler; beta per member): uniform and
    prioritized members mix freely, and any other prioritized ring raises.

    ``update(train_actor)`` is one grouped update, ``run(k)`` k of them with the (critic; critic + actor) pair
    captured as a HIP graph after ``warm_pairs`` eager pairs, as hockey_amd.td3.Learner.run does (a linear chain on
    one stream).  ``take_losses()`` returns per-member means.  On a CPU device every member gets an eager
    ``Learner(fused=False)`` instead, so that code built on this class is testable without a GPU."""

    def __init__(self, agents, rings, batch, graphs=True, warm_pairs=3):
        self.agents, self.rings, self.B = list(agents), list(rings), int(batch)
        S = self.S = len(self.agents)
        if not 1 <= S <= GROUP_MAX:
            raise ValueError(f"a population has 1 to {GROUP_MAX} members, got {S}")
        if len(self.rings) != S:
            raise ValueError("one ring per agent")
        c0 = self.agents[0].cfg
        for j, ag in enumerate(self.agents):
            c = ag.cfg
            if c.batch_size != c0.batch_size:
                raise ValueError(f"member {j}: batch_size {c.batch_size} differs from member 0's {c0.batch_size}")
            if c.policy_update_freq != 2:
                raise ValueError(f"member {j}: policy_update_freq must be 2, got {c.policy_update_freq}")
            if ag.actor.fc1.out_features != 256:
                raise ValueError(f"member {j}: hidden width must be 256, got {ag.actor.fc1.out_features}")
            if rings[j].prioritized and not getattr(rings[j], "device_sampler", False):
                raise ValueError(f"member {j}: prioritized replay is grouped on the device sampler only (a member "
                                 "of a PopulationPrioritizedRing), not on a ring with the whole-ring torch sampler")
        self.device = self.agents[0].device
        self.train_step = 0
        self.graph, self.warm_left = None, int(warm_pairs)
        self.members = None
        if self.device.type != "cuda":
            self.eager = [Learner(ag, rg, self.B, graphs=False, fused=False) for ag, rg in zip(self.agents, self.rings)]
            self.use_graph = False
            return
        self.eager = None
        self.use_graph = bool(graphs)
        self.L = LH.lib()
        self.members = [LH.FusedLearner(ag, rg, self.B, rng="device") for ag, rg in zip(self.agents, self.rings)]
        self.acc = torch.zeros((S, 4), dtype=torch.float64, device=self.device)  # per member: Learner.acc
        for j, f in enumerate(self.members):
            f.set_loss_accumulator(self.acc[j])
        self._gather()

    def _gather(self):
        """The members' io structs as host arrays (kept: the grouped calls check them) and their device copies."""
        S, ms = self.S, self.members
        h = {"cio": (LH.CriticIO * S)(*[f.cio for f in ms]),
             "aio": (LH.ActorIO * S)(*[f.aio for f in ms]), "adam_a": (LH.AdamIO * S)(*[f.adam["actor"] for f in ms])}
        # the batch's slots: hkl_sample_group over the uniform members, hkl_per_sample_group over the prioritized
        # ones, whose priorities hkl_per_update_group writes back; everything else runs over all S members
        uni = [f for f in ms if f.psio is None]
        per = [f for f in ms if f.psio is not None]
        self.n_uniform, self.n_per = len(uni), len(per)
        if uni:
            h["sio"] = (LH.SampleIO * len(uni))(*[f.sio for f in uni])
        if per:
            h["psio"] = (LH.PerSampleIO * len(per))(*[f.psio for f in per])
            h["puio"] = (LH.PerUpdateIO * len(per))(*[f.puio for f in per])
            for f in per:
                f.ring.last = f.idx  # as FusedLearner.update leaves it
        for k in ("c256", "c32", "a256", "a32"):
            n = len(ms[0].wg[k])
            h[k] = (LH.WgJob * (S * n))(*[f.wg[k][i] for f in ms for i in range(n)])
        # the critic's Adam folds its soft_update in on actor updates only: one array per value of the flag
        for flag in (0, 1):
            arr = (LH.AdamIO * S)(*[f.adam["critic"] for f in ms])
            for io in arr:
                io.polyak = flag
            h["adam_c%d" % flag] = arr
        for io in h["adam_a"]:
            io.polyak = 1
        pc, pa = (LH.PackIO * S)(), (LH.PackIO * S)()
        for j, f in enumerate(ms):
            for i, k in enumerate(("q1", "q2")):
                pc[j].net[i] = f.nets[k].net
            pc[j].step = f.step["critic"].data_ptr()
            for i, k in enumerate(("actor", "target_actor", "tq1", "tq2")):
                pa[j].net[i] = f.nets[k].net
            pa[j].step = f.step["actor"].data_ptr()
        h["pack_c"], h["pack_a"] = pc, pa
        self.host = h
        self.dev = {k: LH.upload(v, self.device) for k, v in h.items()}
        self.dptr = {k: ctypes.c_void_p(v.data_ptr()) for k, v in self.dev.items()}

    # ------------------------------------------------------------------ one update
    def update(self, train_actor):
        """FusedLearner.update(train_actor) of every member, each call in its grouped form."""
        if self.eager is not None:
            for lr in self.eager:
                lr._one(bool(train_actor))
            return
        L, S, B, h, ck = self.L, self.S, self.B, self.host, LH.check
        st = LH.stream_ptr(self.device)
        d = self.dptr
        if self.n_uniform:
            ck(L.hkl_sample_group(h["sio"], d["sio"], self.n_uniform, st), "hkl_sample_group")
        if self.n_per:  # slots, target noise and importance weights
            ck(L.hkl_per_sample_group(h["psio"], d["psio"], self.n_per, st), "hkl_per_sample_group")
        ck(L.hkl_critic_step_group(h["cio"], d["cio"], S, st), "hkl_critic_step_group")
        ck(L.hkl_wgrad_pair_group(h["c256"], d["c256"], 2, h["c32"], d["c32"], 2, B, S, st), "hkl_wgrad_pair_group")
        adam_c = "adam_c1" if train_actor else "adam_c0"
        ck(L.hkl_adam_group(h[adam_c], d[adam_c], S, st), "hkl_adam_group")
        ck(L.hkl_pack_group(h["pack_c"], d["pack_c"], 2, S, st), "hkl_pack_group")
        if self.n_per:  # the TD errors become the sampled slots' priorities, where FusedLearner.update does it
            ck(L.hkl_per_update_group(h["puio"], d["puio"], self.n_per, st), "hkl_per_update_group")
        if not train_actor:
            return
        ck(L.hkl_actor_step_group(h["aio"], d["aio"], S, st), "hkl_actor_step_group")
        ck(L.hkl_wgrad_pair_group(h["a256"], d["a256"], 1, h["a32"], d["a32"], 1, B, S, st), "hkl_wgrad_pair_group")
        ck(L.hkl_adam_group(h["adam_a"], d["adam_a"], S, st), "hkl_adam_group")
        ck(L.hkl_pack_group(h["pack_a"], d["pack_a"], 4, S, st), "hkl_pack_group")

    def _one(self):
        self.train_step += 1
        self.update(self.train_step % 2 == 0)

    def _pair(self):
        self.update(False)
        self.update(True)

    def run(self, k):
        """k updates of every member (hockey_amd.td3.Learner.run: graph replay of update pairs after the warm-up)."""
        self._run_pairs(k, self, self.device)  # the count is this learner's own, mirrored to the agents afterwards
        for ag in self.agents:
            ag.train_step = self.train_step

    def take_losses(self):
        """[(mean critic loss, mean actor loss)] per member since the last call (None without updates)."""
        if self.eager is not None:
            return [lr.take_losses() for lr in self.eager]
        rows = self.acc.cpu().tolist()  # one host sync
        self.acc.zero_()
        return [((s[0] / s[2] if s[2] else None), (s[1] / s[3] if s[3] else None)) for s in rows]


# ---------------------------------------------------------------------------------------------------- training
_SHARED = ("curriculum_name", "max_steps", "train_iters", "batch_size", "policy_update_freq", "buffer_size",
           "eval_interval")


def _check_members(members, per_ok=False, self_play_ok=False):
    from .opponents import CURRICULA

    out = []
    for m in members:
        if len(m) not in (2, 3):
            raise ValueError("members are (TD3Config, seed) or (TD3Config, seed, resume_from)")
        out.append((m[0], int(m[1]), m[2] if len(m) == 3 else None))
    if not 1 <= len(out) <= GROUP_MAX:
        raise ValueError(f"a population has 1 to {GROUP_MAX} members, got {len(out)}")
    c0 = out[0][0]
    for j, (c, _, _) in enumerate(out):
        if c.prioritized_replay and not per_ok:
            raise ValueError(f"member {j}: prioritized_replay needs the device sampler's grouped kernels, so "
                             "train_population supports it on a CUDA device only")
        if c.use_self_play and not self_play_ok and any(row[3] > 0 for row in CURRICULA[c.curriculum_name]):
            raise ValueError(f"member {j}: self-play (use_self_play with a self-play share in curriculum "
                             f"'{c.curriculum_name}') is not supported by train_population without its self_play "
                             "argument: pass self_play='arena' or 'step'")
        for k in _SHARED:
            if getattr(c, k) != getattr(c0, k):
                raise ValueError(f"member {j}: {k} = {getattr(c, k)!r} differs from member 0's {getattr(c0, k)!r}; "
                                 "the members of a population share it")
    return out


def train_population(members, n_arenas=20, rounds=10, device="cuda:0", mode=Mode.NORMAL, episode_end="max_steps",
                     updates_per_round=None, eval_fn=None, on_step=None, env=None, replay_capacity=None, graphs=True,
                     log=None, timing=False, self_play=None, explore="torch", collect="torch", poll_every=16,
                     evaluator=None):
    """``hockey_amd.td3.train`` for S = len(members) agents side by side in one process.  ``members`` is a list of
    (TD3Config, seed) or (TD3Config, seed, resume_from); member j owns arenas [j n, (j + 1) n) of one VecHockeyEnv of
    S * n_arenas arenas (``env``: a ready batch of that many arenas, e.g. the kernel source's host build in the CPU
    tests) and its own slice of a PopulationRing.  Returns (agents, stats) with stats[j] shaped like ``train``'s.

    * Player 1 acts through a PolicyBank of S slots with policy[i] = i // n: one ``hkl_act`` launch per step.  The
      bank is refreshed from the members' actors after each round's updates: actors only change there.
    * Player 2 is one OpponentMix over all arenas (seeded by member 0), so the members share ``curriculum_name``,
      ``max_steps`` and ``train_iters`` (and batch_size, policy_update_freq, buffer_size, eval_interval).
    * ``self_play``: None (the default) refuses a member with self-play (use_self_play and a self-play share in the
      curriculum): ValueError.  "arena" or "step" accepts such members: player 2 is then one
      ``hockey_amd.opponents.PopulationOpponentMix`` with a pool per self-play member -- the member's own interval,
      pool size, scores and snapshots, seeded by its seed -- mirrored in one wide PolicyBank, and ONE ``act`` call per
      step plays every self-play arena of the population ("arena": each arena draws its own snapshot per step;
      "step": one snapshot per member and step).  Members with and without use_self_play may share a population.
      ``stats[j]["opponents"]`` is then member j's own counts (with "snapshots") and ``stats[j]["pool_size"]`` its
      pool's size after each round.  On a CPU device the mix runs on the bank's torch backend.
    * ``prioritized_replay`` is per member: on a CUDA device the ring is a PopulationPrioritizedRing with member j
      prioritized as cfg_j says and beta_j = cfg_j.beta, every step's ragged push stores the new transitions'
      priorities, and prioritized and uniform members share one population.  On a CPU device such a member raises
      ValueError (the device sampler has no CPU form).
    * Resets (episode e of member j is seeded seed_j + e), ``episode_end`` ("max_steps" / "done"), the replay ratio
      and ``eval_fn(agent_j, episodes)`` follow ``train``, per member.
    * Updates start in the first round after which EVERY member's total_steps exceeds the batch -- a batched
      difference from ``train``'s per-agent guard; rounds skipped that way are counted in stats[j]["skipped_rounds"].
    * on_step(member_of_row, arena_of_row, obs, action, reward, next_obs, done, step_result) sees every stored
      transition of a step, ragged over the members (test hook).

    explore / collect: "torch" (default) or "device": where exploration and the rest of a collection step run
    (hockey_amd.host_round states both, with the collectors).  collect="device" needs explore="device", self_play None
    or "arena" and no on_step; player 2 is then always a ``PopulationOpponentMix`` (without ``self_play`` one whose
    members keep no pools) and ``stats[j]["opponents"]`` member j's own counts, taken over its running arenas.
    poll_every: collect="device"'s steps between two reads of the survivors' count.

    evaluator: a callable such as ``hockey_amd.evaluator.PopulationEval``, called once per due evaluation -- where
    ``eval_fn`` would be called once per member -- as ``evaluator(agents, bank, episodes)`` with the acting bank (slot j
    holds member j's actor, refreshed after the round's updates); its one record per member is appended to
    ``stats[j]["evals"]``.  Passing both ``eval_fn`` and ``evaluator`` raises ValueError.

    Collection randomness is shared under collect="torch" (hockey_amd.host_round); the self-play pools, their scores
    and their snapshot schedule are per member.  Only the learner is composition-independent there (module
    docstring)."""
    from .opponents import OpponentMix, PopulationOpponentMix
    from .policy_bank import PolicyBank

    dev = torch.device(device)
    if self_play not in (None, "arena", "step"):
        raise ValueError("self_play must be None, 'arena' or 'step'")
    ms = _check_members(members, per_ok=dev.type == "cuda", self_play_ok=self_play is not None)
    if episode_end not in ("max_steps", "done"):
        raise ValueError("episode_end must be 'max_steps' or 'done'")
    check_collect_args(explore, collect, self_play == "step", on_step)
    if eval_fn is not None and evaluator is not None:
        raise ValueError("pass eval_fn (one call per member) or evaluator (one call per evaluation), not both")
    S, n = len(ms), int(n_arenas)
    N = S * n
    c0, seeds = ms[0][0], [s for _, s, _ in ms]
    planned = rounds * c0.max_steps * n
    agents = []
    for cfg, seed, resume in ms:
        ag = TD3(cfg, dev, seed, max_total_steps=planned, n_envs=1)
        if resume is not None:
            ag.load(resume)
        agents.append(ag)
    own_env = env is None
    if own_env:
        from .vec_env import VecHockeyEnv

        env = VecHockeyEnv(N, mode=mode, device=dev, policies=("external", "external"), auto_reset=False,
                           seed=ms[0][1])
    if collect == "device" and self_play is None:  # the Collector's mix, with no member keeping a pool
        mix = PopulationOpponentMix([dataclasses.replace(c, use_self_play=False) for c, _, _ in ms],
                                    seeds, n, dev, sampling="arena")
    elif self_play is None:
        mix = OpponentMix(N, c0.curriculum_name, False, c0.self_play_interval, c0.self_play_pool_size, dev, ms[0][1])
    else:
        mix = PopulationOpponentMix([c for c, _, _ in ms], seeds, n, dev, sampling=self_play)
    cap = replay_capacity or max(c0.buffer_size, n * c0.max_steps)
    if any(c.prioritized_replay for c, _, _ in ms):
        ring = PopulationPrioritizedRing(S, cap, prioritized=[c.prioritized_replay for c, _, _ in ms],
                                         beta=[c.beta for c, _, _ in ms], device=dev)
    else:
        ring = PopulationRing(S, cap, device=dev)
    batch = int(c0.batch_size)
    learner = PopulationLearner(agents, [ring.member(j) for j in range(S)], batch, graphs=graphs)
    updates = updates_per_round if updates_per_round is not None else updates_for(c0, n, c0.max_steps, batch)
    bank = PolicyBank(S, dev)
    for j, ag in enumerate(agents):
        bank.replace(j, ag.actor)
    # on a GPU the kernels, and an error without the library: no quiet fall-back to the numpy laws
    backend = "hip" if dev.type == "cuda" else "torch"
    if explore == "device":
        from .explore import Explorer, Member

        explorer = Explorer(bank, [Member.from_agent(ag) for ag in agents], n,
                            policy=(torch.arange(N, device=dev) // n).to(torch.int32), backend=backend)
    else:
        explorer = PopulationExplorer(agents, bank, n)
    if collect == "device":
        from .collect import Collector

        collector = Collector(env, bank, mix, ring, explorer, seeds, n, backend=backend, episode_end=episode_end,
                              poll_every=poll_every)
    else:
        store = None
        if on_step is not None:
            all_rows = torch.arange(N, device=dev)

            def store(rows, res, *row):  # the collector's own ragged push, shown to the hook
                on_step(collector.push(rows, res, *row), all_rows if rows is None else rows, *row, res)

        collector = TorchCollector(env, bank, mix, ring, explorer, seeds, n, episode_end=episode_end, store=store)
    stats = [{"env_steps": 0, "updates": 0, "updates_per_round": updates, "batch": batch,
              "replay_ratio": updates * batch / (n * c0.max_steps), "replay_capacity": cap, "critic_loss": [],
              "actor_loss": [], "mean_reward": [], "opponents": [], "evals": [], "round_time": [],
              "skipped_rounds": 0, "noise_scale": []} for _ in range(S)]
    if self_play is not None:
        for st in stats:
            st["pool_size"] = []
    episodes = 0
    clock = RoundClock(dev, timing, c0.eval_interval)
    for rnd in range(rounds):
        clock.start()
        mix.update_schedule((episodes + 1) / (rounds * n))
        obs, obs2 = reset_round(env, "seeded", mode, rnd, n, seeds)
        explorer.reset_noise()
        collector.begin_round(obs, obs2, c0.max_steps)
        collector.run_round()
        episodes += n
        explorer.sync(agents)
        # per member; the snapshots precede the updates
        round_steps, ep_reward, opp = collector.end_round([ag.actor for ag in agents], n)
        mean_r = ep_reward.view(S, n).mean(1).tolist()
        for j in range(S):
            stats[j]["env_steps"] += round_steps[j]
            stats[j]["mean_reward"].append(mean_r[j])
            stats[j]["opponents"].append(opp[j])
            if self_play is not None:
                stats[j]["pool_size"].append(mix.pool_sizes()[j])
            stats[j]["noise_scale"].append(agents[j].current_noise_scale)
        clock.collected()
        if all(ag.total_steps > batch for ag in agents):
            learner.run(updates)
            for j, (cl, al) in enumerate(learner.take_losses()):
                stats[j]["updates"] += updates
                stats[j]["critic_loss"].append(cl)
                if al is not None:
                    stats[j]["actor_loss"].append(al)
            for j, ag in enumerate(agents):  # the actors changed: refresh the acting bank
                bank.replace(j, ag.actor)
        else:
            for st in stats:
                st["skipped_rounds"] += 1
        clock.updated(stats)
        if eval_fn is not None and clock.eval_due(episodes):
            for j, ag in enumerate(agents):
                stats[j]["evals"].append(eval_fn(ag, episodes))
        if evaluator is not None and clock.eval_due(episodes):
            for j, rec in enumerate(evaluator(agents, bank, episodes)):
                stats[j]["evals"].append(rec)
        if log:
            log(rnd, stats)
    if own_env:
        env.close()
    sizes = ring.size_t.cpu().tolist()
    for j, ag in enumerate(agents):
        stats[j]["replay_size"] = sizes[j]
        stats[j]["train_step"] = ag.train_step
    return agents, stats
